"""Fused narrow records of the tiled layout (``PML_TL_FUSE``, ops/tiled.py) on the CPU: a bf16 chunk built with the
switch on holds the same entries in the same order as one built with it off (``logical()``, the host emulations),
its record stream satisfies the position formula the kernels read it by, and fp32 / fp64 chunks do not change."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from photon_ml_amd.ops import tiled
from photon_ml_amd.ops.tiled import TLFwdChunk, TLTChunk

DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}
RBITS = 6                 # 64-row forward blocks: a few dozen units in ~1000 rows
ITEM_ENTRIES = 1536       # up to 6 rounds per transpose item (1024 would cap a unit at NW = 4 rounds)
DIM = 8000
TAIL_END = 4096           # random tail columns live in column tiles 0-3
CHUNK_ROWS = (1100, 1000)


def fused_case_matrix(seed: int = 0) -> sp.csr_matrix:
    """2100 rows x 8000 columns: row groups of 64 (one forward block of ``RBITS`` = 6 each) with ``h`` hot columns
    (columns < h, in every row of the group: full 256-entry groups of 4 columns -> narrow rounds in the forward
    copy, dense rows -> narrow rounds in the transpose copy) and ``t`` tail columns per row drawn from
    [64, TAIL_END) (about ceil(t / 4) wide rounds per forward block), plus four small designed column tiles. The
    round counts the units end up with are asserted by ``round_coverage``, not assumed; values are
    bf16-representable so every precision stores them exactly."""
    rng = np.random.default_rng(seed)
    groups = [(40, 12), (0, 4), (4, 0), (24, 20), (36, 8), (0, 28), (40, 40), (8, 2), (0, 12), (40, 28), (0, 0),
              (12, 4), (0, 40), (40, 6), (0, 1), (4, 8), (40, 0)]    # rows 1024-1087: narrow rounds only
    n = sum(CHUNK_ROWS)
    starts = np.cumsum((0,) + CHUNK_ROWS[:-1])
    rows, cols = [], []
    for r in range(n):
        h, t = groups[(r // 64) % len(groups)]
        q = r - starts[np.searchsorted(starts, r, side="right") - 1]       # row inside its chunk
        # column tiles 4-7 hold one small transpose item per chunk each: 3 narrow rounds and nothing else, 4 wide
        # rounds, 5 wide rounds, 1 narrow round
        extra = ([4096 + k for k in range(8)] if q < 96 else []) + ([5120 + q % 7] if q < 1000 else []) + \
                ([6144 + 3 * k + q % 3 for k in range(2 if q < 200 else 1)] if q < 1000 else []) + \
                ([7168 + 2 * k for k in range(8)] if q < 32 else [])
        c = np.r_[np.arange(h), 64 + rng.choice(TAIL_END - 64, size=t, replace=False), extra].astype(np.int64)
        rows.append(np.full(len(c), r))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = torch.from_numpy(rng.normal(size=len(rows))).to(torch.bfloat16).double().numpy()
    vals[vals == 0] = 1.0
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, DIM))


def _chunks(x: sp.csr_matrix, dtype, fuse: int, monkeypatch):
    monkeypatch.setattr(tiled, "FUSE", fuse)
    monkeypatch.setattr(tiled, "DEFAULT_RBITS", RBITS)
    out, lo = [], 0
    for m in CHUNK_ROWS:
        xc = x[lo:lo + m]
        rp = torch.from_numpy(xc.indptr.astype(np.int64))
        col = torch.from_numpy(xc.indices.astype(np.int64))
        val = torch.from_numpy(xc.data).to(dtype)
        out.append((TLFwdChunk(rp, col, val, DIM), TLTChunk(rp, col, val, DIM, max(CHUNK_ROWS),
                                                            item_entries=ITEM_ENTRIES), xc))
        lo += m
    return out


@pytest.mark.parametrize("precision", ["bf16", "f32", "f64"])
def test_fused_chunks_hold_the_same_entries(precision, monkeypatch):
    x = fused_case_matrix()
    on = _chunks(x, DTYPES[precision], 1, monkeypatch)
    off = _chunks(x, DTYPES[precision], 0, monkeypatch)
    rng = np.random.default_rng(1)
    for (f1, t1, xc), (f0, t0, _) in zip(on, off):
        assert f1.n_narrow_rounds > 0 and t1.n_narrow_rounds > 0
        assert f1.fused == t1.fused == (precision == "bf16") and not f0.fused and not t0.fused
        for a, b in ((f1, f0), (t1, t0)):
            assert torch.equal(a._table(), b._table())
            (pa, va), (pb, vb) = a.logical(), b.logical()
            assert pa.dtype == pb.dtype and torch.equal(pa, pb)
            assert va.dtype == vb.dtype and torch.equal(va, vb)
            assert torch.equal(a.nbase, b.nbase) and torch.equal(a.pack, b.pack) and torch.equal(a.val, b.val)
            assert a.nbytes() == b.nbytes()
            if precision != "bf16":                      # byte-identical streams
                assert a.npack.dtype == b.npack.dtype and torch.equal(a.npack, b.npack)
                assert a.nval.dtype == b.nval.dtype and torch.equal(a.nval, b.nval)
        w = torch.from_numpy(rng.normal(size=DIM))
        r = torch.from_numpy(rng.normal(size=xc.shape[0]))
        z1, z0 = f1.emulate_matvec(w), f0.emulate_matvec(w)
        assert torch.equal(z1, z0)
        np.testing.assert_allclose(z1.numpy(), xc @ w.numpy(), atol=1e-12)
        for sq in (False, True):
            g1, g0 = t1.emulate_rmatvec(r, square=sq), t0.emulate_rmatvec(r, square=sq)
            assert torch.equal(g1, g0)
            np.testing.assert_allclose(g1.numpy(), (xc.multiply(xc) if sq else xc).T @ r.numpy(), atol=1e-12)
        # every item's narrow window (what TLTMulti.emulate_rmatvec reads) is the same too
        for n_lo, n_hi in t1.items[:, 4:6].tolist():
            (pa, va), (pb, vb) = t1.narrow_window(n_lo, n_hi), t0.narrow_window(n_lo, n_hi)
            assert torch.equal(pa, pb) and torch.equal(va, vb)


def test_fused_record_positions(monkeypatch):
    """Lane L of narrow round r owns the 16 bytes at (r * 64 + L) * 16 of the record stream: 16-bit words
    {p0, p1, p2, p3, v0, v1, v2, v3} = the packs and bf16 bit patterns of logical entries L, L+64, L+128, L+192 of
    the round, i.e. words k and 4 + k of lane L are element r * 256 + 4 L + k of the two-array layout's pack and
    value streams."""
    x = fused_case_matrix()
    on = _chunks(x, torch.bfloat16, 1, monkeypatch)
    off = _chunks(x, torch.bfloat16, 0, monkeypatch)
    for (f1, t1, _), (f0, t0, _) in zip(on, off):
        for a, b in ((f1, f0), (t1, t0)):
            R = a.n_narrow_rounds
            assert R > 0 and a.nrec.dtype == torch.int16 and a.nrec.is_contiguous()
            assert a.nrec.numel() == R * 64 * 8 and b.npack.numel() == R * 256
            assert a.nar.val is None and a.nar.pack == a.nrec.data_ptr() and b.nar.val == b.nval.data_ptr()
            rec = a.nrec.view(R, 64, 8)
            assert torch.equal(rec[:, :, :4].reshape(-1), b.npack)
            assert torch.equal(rec[:, :, 4:].reshape(-1), b.nval.view(torch.int16))
            # against the logical order: word k of lane L of round r is logical entry 64 k + L of that round
            pk, vl = b.narrow_window(0, R)
            sb = a._sbits
            p16 = (((pk >> sb) - b.nbase.to(torch.int64).repeat_interleave(256)) << sb) | (pk & ((1 << sb) - 1))
            assert torch.equal(rec[:, :, :4].to(torch.int64) & 0xFFFF, p16.view(R, 4, 64).transpose(1, 2))
            assert torch.equal(rec[:, :, 4:], vl.view(torch.int16).view(R, 4, 64).transpose(1, 2))
    # the shard-wide pointer table: slot 2 = the record stream, slot 3 = null for a fused chunk
    ptrs = tiled.stream_ptr_table([c[0] for c in on] + [off[0][0]], "cpu").view(-1, 6)
    assert ptrs[0, 2] == on[0][0].nrec.data_ptr() and ptrs[0, 3] == 0 and ptrs[1, 3] == 0
    assert ptrs[2, 2] == off[0][0].npack.data_ptr() and ptrs[2, 3] == off[0][0].nval.data_ptr()


def test_case_matrix_covers_the_round_counts(monkeypatch):
    """The shared test matrix really contains the unit shapes the GPU test relies on (see ``round_coverage``)."""
    chunks = _chunks(fused_case_matrix(), torch.bfloat16, 1, monkeypatch)
    round_coverage([c[0] for c in chunks], 2)
    round_coverage([c[1] for c in chunks], 4)


def round_coverage(chunks, nw: int):
    """Assert from the unit tables that the units of ``chunks`` (one copy of every row chunk; ``nw`` waves per
    work-group) include 0, 1, 2, 3 and a larger odd and even number of wide rounds, 0, 1 and more than ``nw``
    narrow rounds, and a non-empty section with fewer rounds than waves (empty wave shares)."""
    wide, narrow = set(), set()
    for ch in chunks:
        t = ch._table().to(torch.int64)
        lo, hi = ch._ew
        wide |= set(((t[:, hi] - t[:, lo] + 255) // 256).tolist())
        narrow |= set((t[:, 5] - t[:, 4]).tolist())
    assert {0, 1, 2, 3} <= wide, sorted(wide)
    assert any(w > 3 and w % 2 for w in wide) and any(w > 3 and w % 2 == 0 for w in wide), sorted(wide)
    assert {0, 1} <= narrow and any(k > nw for k in narrow), sorted(narrow)
    assert any(0 < w < nw for w in wide) and any(0 < k < nw for k in narrow)
