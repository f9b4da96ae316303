"""Tall forward units of the tiled layout (ops/tiled.py, TALL FORWARD UNITS), builder only: the tall layout is forced
at small ``dim`` through the constructor argument and read back through ``logical()`` / ``emulate_matvec``."""
import numpy as np
import pytest
import torch

from photon_ml_amd.ops import tiled
from photon_ml_amd.ops.tiled import TLFwdChunk
from tl_tall_util import CASES, make_case

_CACHE = {}


def built(name, dtype):
    """(csr, tall chunk, plain chunk, expectations) of a case, built once."""
    key = (name, dtype)
    if key not in _CACHE:
        x, narrow, wide, bases = make_case(name)
        rp = torch.from_numpy(x.indptr.astype(np.int64))
        col = torch.from_numpy(x.indices.astype(np.int64))
        val = torch.from_numpy(x.data).to(dtype)
        _CACHE[key] = (x, val, TLFwdChunk(rp, col, val, x.shape[1], tall=True),
                       TLFwdChunk(rp, col, val, x.shape[1], tall=False), (narrow, wide, bases))
    return _CACHE[key]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_tall_chunk_holds_the_input(name, dtype):
    x, val, f, plain, (narrow, wide, bases) = built(name, dtype)
    m, dim = x.shape
    assert f.tbits == 12 and f.rbits == 10 and f.ubits == 12 and plain.tbits == 0
    b = f.blk.to(torch.int64)
    assert b.shape == (-(-m // 4096), tiled.TALL_COLS) and f.nblk == b.shape[0] and f.nstats == -(-m // 1024)
    # units cover the rows in order; the last one may be ragged
    assert int(b[0, 0]) == 0 and bool((b[1:, 0] == b[:-1, 0] + b[:-1, 1]).all()) and int(b[-1, 0] + b[-1, 1]) == m
    assert bool((b[:-1, 1] == 4096).all())
    # four narrow ranges per unit, consecutive in the chunk's narrow stream
    bounds = torch.stack([b[:, 4], b[:, 6], b[:, 7], b[:, 8], b[:, 5]], 1)
    assert bool((bounds[:, 1:] >= bounds[:, :-1]).all()) and int(bounds[0, 0]) == 0
    assert bool((bounds[1:, 0] == bounds[:-1, 4]).all()) and int(bounds[-1, 4]) == f.n_narrow_rounds
    # the sections the case is about
    n_wide = int((b[:, 3] - b[:, 2]).sum())
    assert (f.n_narrow_rounds > 0) == narrow and (n_wide > 0) == wide and (f.wbase is not None) == bases
    assert bool((b[:, 2] % 256 == 0).all())
    # logical(): exactly the input's (row, col, value) multiset
    pk, vl = f.logical()
    cnt = f.unit_counts()
    assert int(cnt.sum()) == x.nnz == pk.numel()
    unit = torch.repeat_interleave(torch.arange(f.nblk), cnt)
    row = (unit << 12) + (pk & 4095)
    col = pk >> 12
    got = torch.stack([row, col], 1)
    order = np.lexsort((col.numpy(), row.numpy()))
    want_row = np.repeat(np.arange(m), np.diff(x.indptr))
    assert (got.numpy()[order] == np.stack([want_row, x.indices], 1)).all()
    assert torch.equal(vl[torch.from_numpy(order)], val)          # sorted CSR, distinct columns per row: same order
    # each unit: narrow entries first (sub-block by sub-block), then ONE wide section sorted by (column, row)
    starts = np.r_[0, np.cumsum(cnt.numpy())]
    nn = 256 * (b[:, 5] - b[:, 4]).numpy()
    p = pk.numpy()
    for lo, hi, k in zip(starts[:-1], starts[1:], nn):
        assert (np.diff(p[lo + k:hi]) > 0).all()
    # the sub-blocks' narrow sections are the plain layout's own (same split rule, same rounds)
    assert f.n_narrow_rounds == plain.n_narrow_rounds and torch.equal(f.nbase, plain.nbase)
    assert torch.equal(f.npack.reshape(-1), plain.npack.reshape(-1))
    # entries are moved, not duplicated: never more bytes than the plain layout
    assert f.nbytes() <= plain.nbytes(), (f.nbytes(), plain.nbytes())


@pytest.mark.parametrize("name", CASES)
def test_tall_emulation_matches_scipy(name):
    x, val, f, _, _ = built(name, torch.float32)
    rng = np.random.default_rng(7)
    w = rng.normal(size=x.shape[1])
    xs = x.copy()
    xs.data = val.to(torch.float64).numpy()                        # the values the chunk stores
    np.testing.assert_allclose(f.emulate_matvec(torch.from_numpy(w)).numpy(), xs @ w, rtol=0, atol=1e-12)


def test_engagement_rule(monkeypatch):
    """fp64 chunks, plain-order streams and other sub-block heights never build tall units, even when asked; the
    rule itself needs a wide feature space and one full unit of rows."""
    x, _, _, _ = make_case("short")
    rp = torch.from_numpy(x.indptr.astype(np.int64))
    col = torch.from_numpy(x.indices.astype(np.int64))
    v32 = torch.from_numpy(x.data).to(torch.float32)
    assert TLFwdChunk(rp, col, v32.double(), x.shape[1], tall=True).tbits == 0
    assert TLFwdChunk(rp, col, v32, x.shape[1], tall=True, il=0).tbits == 0
    assert TLFwdChunk(rp, col, v32, x.shape[1], tall=True, rbits=9).tbits == 0
    monkeypatch.setattr(tiled, "TALL", None)
    want = tiled.TALL_DEFAULT
    assert tiled.tall_engages(None, 1 << 16, 4096, torch.bfloat16, 1, 10) == want
    assert not tiled.tall_engages(None, (1 << 16) - 1, 4096, torch.bfloat16, 1, 10)
    assert not tiled.tall_engages(None, 1 << 16, 4095, torch.float32, 1, 10)
    assert not tiled.tall_engages(None, 1 << 20, 1 << 20, torch.float64, 1, 11)
    assert tiled.shard_tall(1 << 20, 1 << 20) == want and tiled.shard_tall(5000, 1 << 20) is False
    monkeypatch.setattr(tiled, "TALL", False)
    assert not tiled.tall_engages(None, 1 << 20, 1 << 20, torch.bfloat16, 1, 10) and tiled.shard_tall(1 << 20, 1 << 20) is None
    monkeypatch.setattr(tiled, "TALL", True)
    assert tiled.tall_engages(None, 100, 10, torch.bfloat16, 1, 10)
