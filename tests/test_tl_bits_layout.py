"""The tiled layout at every block width (``rbits``) and tile width (``cbits``) the builder accepts, on the CPU.

``bits_case`` scales one designed matrix by the widths, so that the slot mask / key shift of every stream variant,
the 64 / 32 / 16-key narrow window (``narrow_width``), the three LDS accumulator sizes and the combine grids of
tiles narrower than 64 columns all get units with the round counts the stream loops distinguish. Everything the GPU
tests (test_tl_bits_gpu.py) rely on is asserted here from the unit tables, nothing is assumed.

EXACT INPUTS. The values are in {+-0.5, +-1, +-1.5, +-2} (bf16 holds them exactly) and the test vectors ``w`` / ``r``
are non-zero multiples of 1/8 of magnitude <= 2. A product ``v w`` is a multiple of 2^-4 of magnitude <= 4 and a
product ``v^2 r`` a multiple of 2^-5 of magnitude <= 8, so a sum of at most 2^16 of them is a multiple of 2^-5 below
2^19: 24 significant bits. Every fp32 (and fp64) partial sum is exact, whatever the order, and ``X w``, ``X^T r``,
``(X.X)^T r`` of a correct kernel equal the float64 scipy products BIT FOR BIT — a comparison without a tolerance,
which one lost, duplicated or misplaced entry cannot pass (``test_one_lost_entry_...``: the project's
``atol = 2e-5 max|g|`` gradient check does not see such an entry).

THE MATRIX. Rows: two chunks; a chunk is three QUIET forward blocks of R = 2^rbits rows, then its LOUD rows (whole
blocks and a partial last block, at least 768 rows). Columns: [0, 240) forward hot region, [240, FEND) random tail,
six DESIGNED column tiles of C = 2^cbits columns, and at least 64 more columns ending in a partial tile, the last of
which are dense.

* a quiet block holds ``k`` x 256 entries filled column-major over columns < 96 (k narrow rounds: a full 256-entry
  group spans at most 12 columns) and ``T`` tail entries in random cells (ceil(T / 256) wide rounds), nothing else;
* a loud block holds two such hot groups, a 256-entry group over exactly W_r = narrow_width(rbits) columns (narrow:
  span W_r - 1) and one over W_r + 1 columns (span W_r: stays wide), 400 tail entries, and in every row the column
  ``dim - 65 + W_r`` (the last column up to 10 bits) with enough neighbours below it for 512 entries per block: a
  narrow round whose base is clamped to ``dim - 64``. At 11 / 12 bits the last column is in every loud row too,
  where it can only form wide rounds (its key is 63 above the clamped base, the window is 32 / 16 keys) — which is
  why it is NOT in the quiet blocks: a 2048-row block would carry 8 wide rounds of it and no unit with 0 to 3 wide
  rounds could exist;
* the loud rows of a chunk carry the transpose design, the same way with rows and columns swapped: four tiles with
  one item each of ``k`` dense-row narrow rounds and ``T`` wide entries (two per row), a tile with the W_c - 1 / W_c
  row-span pair, and a tile of 12 entries per row (split into several items: the two-level combine) whose last
  rows, ``m - 64 ...``, are dense (narrow rounds with the base clamped to ``m - 64``).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from photon_ml_amd.ops import tiled
from photon_ml_amd.ops.tiled import TLFwdChunk, TLTChunk, TLTMulti, narrow_width
from test_tl_fused_layout import DTYPES, round_coverage

WIDTHS = (5, 6, 8, 10, 11, 12)
MIXED = ((12, 5), (5, 12))
ITEM_ENTRIES = 3072        # 12 rounds: above every designed single-item tile, a third of the split tile
LOUD_ROWS = 768            # rows per chunk that carry the transpose design (6 wide rounds at 2 entries per row)
VALUES = np.array([-2.0, -1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0])
# (narrow rounds, tail / wide entries) of the quiet forward blocks (2 waves) and of the designed transpose items (4)
QUIET_BLOCKS = ((3, 0), (1, 200), (0, 300), (0, 700), (0, 1200), (5, 1500))
QUIET_ITEMS = ((6, 0), (0, 300), (0, 700), (0, 1200), (5, 1400), (1, 200), (2, 0), (0, 100))
SLOT_LIMIT = 1 << 16       # entries per accumulator slot up to which the exact-arithmetic argument holds


def _dyadic(rng, n: int) -> np.ndarray:
    """Non-zero multiples of 1/8 in [-2, 2]."""
    return rng.integers(1, 17, size=n) / 8.0 * rng.choice([-1.0, 1.0], size=n)


def _span_group(keys_lo: int, w: int, wide: bool):
    """(key, slot) of a 256-entry group over the ``w`` keys from ``keys_lo`` (span w - 1) or, ``wide``, over
    w + 1 keys (span w): 256 / w entries per key (slots 0, 1, ...), one moved from the first key to key w."""
    per = 256 // w
    k = np.repeat(np.arange(w), per)
    s = np.tile(np.arange(per), w)
    if wide:
        k, s = np.r_[k[1:], w], np.r_[s[1:], 0]
    return keys_lo + k, s


def bits_case(bits_r: int, bits_c: int, seed: int = 0) -> SimpleNamespace:
    """The case of block width ``bits_r`` and tile width ``bits_c`` (module docstring): ``x`` (scipy CSR, float64),
    ``chunk_rows`` (two unequal chunks; the first is the ``chunk_rows`` argument of the shard builders),
    ``item_entries``, the exact test vectors ``w`` (dim) and ``r`` (rows) and the float64 products ``z = X w``,
    ``g = X^T r``, ``g2 = (X.X)^T r``."""
    rng = np.random.default_rng(seed)
    R, C = 1 << bits_r, 1 << bits_c
    wr, wc = narrow_width(bits_r), narrow_width(bits_c)
    fend = max(512, C)                     # forward region [0, fend): a whole number of tiles
    t0 = fend // C                         # first designed tile
    dim = (t0 + 6) * C + C // 2 + 5 + (64 if C < 128 else 0)   # the last 64 columns lie beyond the designed tiles
    partial = (R // 2 + 7, R // 4 + 3)
    loud_full = max(0, -(-(LOUD_ROWS - min(partial)) // R))     # whole loud blocks before the partial one
    chunk_rows = tuple((3 + loud_full) * R + p for p in partial)
    assert chunk_rows[0] > chunk_rows[1] and dim < (1 << 16) and dim > 2 * C and dim % C
    rows, cols = [], []

    def put(r, c):
        rows.append(np.asarray(r, dtype=np.int64).reshape(-1))
        cols.append(np.asarray(c, dtype=np.int64).reshape(-1))

    def cells(n, nrows, c_lo, c_hi, r_lo):
        """``n`` distinct random cells of rows [r_lo, r_lo + nrows) x columns [c_lo, c_hi)."""
        pick = rng.choice(nrows * (c_hi - c_lo), size=n, replace=False)
        put(r_lo + pick // (c_hi - c_lo), c_lo + pick % (c_hi - c_lo))

    def hot(k, nrows, r_lo):
        rr = min(nrows, 256)
        j = np.arange(256 * k)
        put(r_lo + j % rr, j // rr)

    c_clamp = dim - 65 + wr                # the highest key of a narrow window clamped to dim - 64
    n_end = max(1, -(-512 // R))           # dense columns up to c_clamp: >= 512 entries per whole loud block
    row0 = 0
    for c, m in enumerate(chunk_rows):
        for b in range(3):                                       # quiet forward blocks
            k, t = QUIET_BLOCKS[3 * c + b]
            hot(k, R, row0 + b * R)
            cells(t, R, 240, fend, row0 + b * R)
        loud0 = row0 + 3 * R
        nloud = m - 3 * R
        for lo in range(0, nloud, R):                            # loud forward blocks
            nr = min(R, nloud - lo)
            hot(2, nr, loud0 + lo)
            for wide, c_lo in ((False, 100), (True, 100 + wr + 5)):
                kk, ss = _span_group(c_lo, wr, wide)
                put(loud0 + lo + ss, kk)
            cells(400, nr, 240, fend, loud0 + lo)
        lr = np.arange(loud0, loud0 + nloud)
        for cc in sorted(set(range(c_clamp - n_end + 1, c_clamp + 1)) | {dim - 1}):
            put(lr, np.full(nloud, cc))
        # transpose design: one item per (chunk, tile) in tiles t0 .. t0 + 3
        cw = min(C, 256)
        for i in range(4):
            k, t = QUIET_ITEMS[4 * c + i]
            base = (t0 + i) * C
            j = np.arange(256 * k)
            put(loud0 + j // cw, base + j % cw)                  # dense rows: k narrow rounds
            assert 256 * k // cw <= 64 and 64 + (t + 1) // 2 <= nloud
            for e in range(2):                                   # two wide entries per row from row 64 on
                rws = np.arange((t + 1 - e) // 2)
                put(loud0 + 64 + rws, base + (rng.integers(0, C // 2, size=len(rws)) * 2 + e))
        base = (t0 + 4) * C                                      # the row-span pair
        for wide, r_lo in ((False, 0), (True, wc + 3)):
            kk, ss = _span_group(loud0 + r_lo, wc, wide)
            put(kk, base + ss)
        base = (t0 + 5) * C                                      # the split tile and the clamped row window
        body = np.arange(loud0, row0 + m - 64)
        for e in range(12):
            put(body, base + (e * (C // 12) + (body * 5 + e) % (C // 12)))
        dens = min(C, 64)
        for q in range(m - 64, m - 64 + wc):
            put(np.full(dens, row0 + q), base + np.arange(dens))
        row0 += m
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    n = sum(chunk_rows)
    assert len(np.unique(rows * dim + cols)) == len(rows), "the designed cells overlap"
    vals = rng.choice(VALUES, size=len(rows))
    vals[cols >= dim - 64] = 2.0           # the dense last columns: one large gradient component (max |g|)
    x = sp.csr_matrix((vals, (rows, cols)), shape=(n, dim))
    x.sort_indices()
    w, r = _dyadic(rng, dim), _dyadic(rng, n)
    last = x[:, dim - 1].toarray().ravel() != 0
    r[last] = np.abs(r[last])              # ... of about 2 x the number of loud rows
    return SimpleNamespace(x=x, chunk_rows=chunk_rows, item_entries=ITEM_ENTRIES, dim=dim, w=w, r=r,
                           z=x @ w, g=x.T @ r, g2=x.multiply(x).T @ r, bits=(bits_r, bits_c))


_CASES = {}


def cached_case(bits_r: int, bits_c: int) -> SimpleNamespace:
    """``bits_case`` once per process and width pair (read-only)."""
    if (bits_r, bits_c) not in _CASES:
        _CASES[bits_r, bits_c] = bits_case(bits_r, bits_c)
    return _CASES[bits_r, bits_c]


def case_for(bits, precision: str) -> SimpleNamespace:
    """The case of a width REQUEST: fp64 chunks get at most 11 bits (``TL_MAXBITS_F64``), so a request of 12 is
    tested on the matrix designed for the 11 bits it is cut down to."""
    cap = tiled.TL_MAXBITS_F64 if precision == "f64" else tiled.TL_MAXBITS
    return cached_case(min(bits[0], cap), min(bits[1], cap))


def build_chunks(case, dtype, monkeypatch, request=None):
    """[(forward copy, transpose copy, scipy rows)] per chunk, built with the requested widths (default: the
    case's) as the builder's defaults."""
    monkeypatch.setattr(tiled, "DEFAULT_RBITS", (request or case.bits)[0])
    monkeypatch.setattr(tiled, "DEFAULT_CBITS", (request or case.bits)[1])
    out, lo = [], 0
    for m in case.chunk_rows:
        xc = case.x[lo:lo + m]
        rp = torch.from_numpy(xc.indptr.astype(np.int64))
        col = torch.from_numpy(xc.indices.astype(np.int64))
        val = torch.from_numpy(xc.data).to(dtype)
        out.append((TLFwdChunk(rp, col, val, case.dim),
                    TLTChunk(rp, col, val, case.dim, case.chunk_rows[0], item_entries=case.item_entries), xc))
        lo += m
    return out


def full_groups(ch):
    """Every full 256-entry group of every unit of ``ch`` in the unit's sorted order, as the builder cut them:
    ``[(key span, is a narrow round, its base or None)]``, reconstructed from the unit table and the streams."""
    pk, _ = ch.logical()
    pk = pk.to(torch.int64).cpu().numpy() & 0xFFFFFFFF
    t = ch._table().to(torch.int64).cpu().numpy()
    counts = ch.unit_counts().cpu().numpy()
    nbase = ch.nbase.cpu().numpy()
    out, off = [], 0
    for u in range(t.shape[0]):
        seg = pk[off:off + counts[u]]
        off += counts[u]
        nn = 256 * (t[u, 5] - t[u, 4])
        first = {int(p): int(nbase[t[u, 4] + i]) for i, p in enumerate(seg[:nn:256])}
        assert all(np.all(np.diff(seg[i:i + 256]) > 0) for i in range(0, nn, 256))      # a round is sorted
        srt = np.sort(seg)
        assert np.all(np.diff(srt) > 0)                                                # packs are unique in a unit
        unit = [(int((srt[i + 255] >> ch._sbits) - (srt[i] >> ch._sbits)), int(srt[i]) in first, first.get(int(srt[i])))
                for i in range(0, len(srt) - 255, 256)]
        assert sum(g[1] for g in unit) == t[u, 5] - t[u, 4]       # every narrow round is one of the sorted groups
        out += unit
    return out


def assert_case_layout(case, fwd, tr, precision: str):
    """What the GPU tests rely on, from the unit tables of the forward copies ``fwd`` and the transpose copies
    ``tr`` of the case's chunks (``build_chunks`` or a shard's ``csr`` / ``csc``)."""
    want_r, want_c = case.bits
    assert max(case.bits) <= (11 if precision == "f64" else 12)        # TL_MAXBITS_F64, TL_MAXBITS
    assert [f.m for f in fwd] == list(case.chunk_rows) == [t.m for t in tr]
    for f, t in zip(fwd, tr):
        assert f.rbits == want_r and t.cbits == want_c, (f.rbits, t.cbits)
        assert f.il and t.il and f.wbase is None
        assert f.n_narrow_rounds > 0 and t.n_narrow_rounds > 0
        assert f.fused == t.fused == (precision == "bf16")
        assert t.nparts > 0 and t.ncu > 0                  # some tile is split: the two-level combine runs
        assert f.nblk >= 3 and f.m % (1 << f.rbits) != 0   # two whole blocks or more and a partial one
    round_coverage(fwd, 2)
    round_coverage(tr, 4)
    for copies, bits, xlens in ((fwd, want_r, [case.dim] * len(fwd)), (tr, want_c, [t.m for t in tr])):
        w = narrow_width(bits)
        assert w == {5: 64, 6: 64, 8: 64, 10: 64, 11: 32, 12: 16}[bits]
        groups = [g + (xl,) for ch, xl in zip(copies, xlens) for g in full_groups(ch)]
        assert all(span < w for span, nar, _, _ in groups if nar)
        assert any(nar and span == w - 1 for span, nar, _, _ in groups), f"no narrow round of span {w - 1}"
        assert any(not nar and span == w for span, nar, _, _ in groups), f"no wide group of span {w}"
        assert any(nar and base == xl - 64 for _, nar, base, xl in groups), "no clamped narrow base"


@pytest.mark.parametrize("precision", ["bf16", "f32", "f64"])
@pytest.mark.parametrize("bits", [(b, b) for b in WIDTHS] + list(MIXED), ids=lambda b: f"r{b[0]}c{b[1]}")
def test_layout_at_every_width(bits, precision, monkeypatch):
    case = case_for(bits, precision)
    assert case.bits == tuple(min(b, 11 if precision == "f64" else 12) for b in bits)     # the builder's caps
    x = case.x
    assert len(case.chunk_rows) == 2 and case.chunk_rows[0] != case.chunk_rows[1]
    assert case.dim > 2 << case.bits[1] and case.dim % (1 << case.bits[1]) and case.dim < (1 << 16)
    assert np.all(np.isin(x.data, VALUES))
    assert max(int(np.diff(x.indptr).max()), int(np.bincount(x.indices).max())) <= SLOT_LIMIT
    chunks = build_chunks(case, DTYPES[precision], monkeypatch, request=bits)
    assert_case_layout(case, [c[0] for c in chunks], [c[1] for c in chunks], precision)
    w, r = torch.from_numpy(case.w), torch.from_numpy(case.r)
    lo = 0
    for f, t, xc in chunks:
        rc = r[lo:lo + f.m]
        assert np.array_equal(f.emulate_matvec(w).numpy(), case.z[lo:lo + f.m])
        assert np.array_equal(t.emulate_rmatvec(rc).numpy(), xc.T @ rc.numpy())
        assert np.array_equal(t.emulate_rmatvec(rc, square=True).numpy(), xc.multiply(xc).T @ rc.numpy())
        lo += f.m
    mt = TLTMulti([c[1] for c in chunks], [0, case.chunk_rows[0], sum(case.chunk_rows)], case.dim)
    assert mt.nparts > 0 and mt.ncu > 0
    assert np.array_equal(mt.emulate_rmatvec(r).numpy(), case.g)
    assert np.array_equal(mt.emulate_rmatvec(r, square=True).numpy(), case.g2)


def _f32_sums(index: np.ndarray, prod32: np.ndarray, size: int, rng, nparts: int = 4) -> np.ndarray:
    """Sum ``prod32`` (float32) into ``size`` slots: the entries are dealt at random to ``nparts`` partial
    accumulators, each summed sequentially IN FLOAT32 in a random order; the partials are added in float64."""
    assert prod32.dtype == np.float32
    part = rng.integers(0, nparts, size=len(index))
    total = np.zeros(size, dtype=np.float64)
    for p in range(nparts):
        sel = rng.permutation(np.flatnonzero(part == p))
        acc = np.zeros(size, dtype=np.float32)
        np.add.at(acc, index[sel], prod32[sel])
        assert acc.dtype == np.float32
        total += acc.astype(np.float64)
    return total


@pytest.mark.parametrize("bits", [(b, b) for b in WIDTHS] + list(MIXED), ids=lambda b: f"r{b[0]}c{b[1]}")
def test_float32_sums_of_the_case_are_exact(bits):
    """The premise of the tolerance-free GPU comparison: fp32 products and fp32 partial sums in any order give
    the float64 scipy products bit for bit."""
    case = cached_case(*bits)
    coo = case.x.tocoo()
    v32, w32, r32 = coo.data.astype(np.float32), case.w.astype(np.float32), case.r.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), coo.data)
    assert np.array_equal(w32.astype(np.float64), case.w) and np.array_equal(r32.astype(np.float64), case.r)
    assert np.array_equal(torch.from_numpy(coo.data).to(torch.bfloat16).double().numpy(), coo.data)
    assert np.all(case.w * 8 == np.round(case.w * 8)) and np.all(np.abs(case.w) <= 2) and np.all(case.w != 0)
    assert np.all(case.r * 8 == np.round(case.r * 8)) and np.all(np.abs(case.r) <= 2) and np.all(case.r != 0)
    n, dim = case.x.shape
    rng = np.random.default_rng(7)
    for _ in range(2):
        assert np.array_equal(_f32_sums(coo.row, v32 * w32[coo.col], n, rng), case.z)
        assert np.array_equal(_f32_sums(coo.col, v32 * r32[coo.row], dim, rng), case.g)
        assert np.array_equal(_f32_sums(coo.col, (v32 * v32) * r32[coo.row], dim, rng), case.g2)


def test_one_lost_entry_passes_the_tolerance_check_and_fails_the_exact_one():
    """Why the exact inputs exist: drop one entry of a cold column. The gradient check of the parity tests
    (``atol = 2e-5 max|g|``, test_kernels_gpu.py) accepts the result; ``torch.equal`` does not."""
    case = cached_case(11, 11)
    x = case.x.tocoo()
    cold = np.flatnonzero(np.bincount(x.col, minlength=case.dim) <= 2)
    cand = np.flatnonzero(np.isin(x.col, cold))
    e = cand[np.argmin(np.abs(x.data[cand] * case.r[x.row[cand]]))]
    keep = np.ones(len(x.data), dtype=bool)
    keep[e] = False
    y = sp.csr_matrix((x.data[keep], (x.row[keep], x.col[keep])), shape=x.shape)
    assert y.nnz == case.x.nnz - 1
    tol = 2e-5
    for g_ok, g_lost in ((case.g, y.T @ case.r), (case.g2, y.multiply(y).T @ case.r)):
        g_ok, g_lost = torch.from_numpy(g_ok), torch.from_numpy(g_lost)
        assert not torch.equal(g_lost, g_ok)
        assert int((g_lost != g_ok).sum()) == 1 and bool(g_lost[x.col[e]] != g_ok[x.col[e]])
        assert torch.allclose(g_lost, g_ok, rtol=tol, atol=tol * float(g_ok.abs().max()))
