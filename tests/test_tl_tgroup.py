"""Tile groups of the transpose copy (``ops/tiled.py``, TILE GROUPS) on the host: the grouped chunk holds its input,
its emulated product matches scipy, and a numpy emulation that performs the fp64 additions one by one in the order
and grouping of ``tl_t_item`` (ungrouped layout) and of ``tl_t_group`` (grouped layout) gives bitwise-equal sums for
every column tile."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from photon_ml_amd.ops.tiled import IL_ROUND, TG_EMPTY, TLTChunk, TLTMulti, il_phys, tgroup_engages
from tl_tgroup_util import DIM, EMPTY_TILE, ITEM_ENTRIES, make_matrix

ROWS = 3000
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
_CH = {}


def chunks(precision, wide_exponents=False):
    """(stored matrix, grouped chunk, ungrouped chunk) of one shape; built once per precision."""
    key = (precision, wide_exponents)
    if key not in _CH:
        x = make_matrix(ROWS, wide_exponents=wide_exponents)
        val = torch.from_numpy(x.data).to(DTYPES[precision])
        x = sp.csr_matrix((val.double().numpy(), x.indices, x.indptr), shape=x.shape)    # what the chunk stores
        rp, col = torch.from_numpy(x.indptr.astype(np.int64)), torch.from_numpy(x.indices.astype(np.int64))
        mk = lambda g: TLTChunk(rp, col, val, DIM, ROWS, item_entries=ITEM_ENTRIES, tgroup=g)
        _CH[key] = (x, mk(True), mk(False))
    return _CH[key]


def test_engagement_rule(monkeypatch):
    from photon_ml_amd.ops.tiled import shard_tgroup
    monkeypatch.delenv("PML_TL_TGROUP", raising=False)
    can = lambda **k: tgroup_engages(**{**dict(tgroup=True, dim=1 << 16, chunk_rows=1 << 20, dtype=torch.bfloat16,
                                               il=1, cbits=10), **k})
    # what the layout can hold, when asked for
    assert can() and can(dtype=torch.float32) and can(dim=100)
    assert not can(dtype=torch.float64) and not can(cbits=11) and not can(il=0)
    assert not can(chunk_rows=(1 << 20) + 1)                  # bits(chunk rows) + 12 <= 32
    assert not can(tgroup=False) and not can(tgroup=None)     # a chunk on its own: only when asked for
    # the shard rule: wide feature spaces and enough chunks for the long group units to fill the device
    assert shard_tgroup(1 << 16, 96 << 20, 1 << 20) is True and shard_tgroup(1_000_000, 125_000_000, 1 << 20) is True
    assert shard_tgroup((1 << 16) - 1, 96 << 20, 1 << 20) is False
    assert shard_tgroup(1_000_000, 62_500_000, 1 << 20) is False and shard_tgroup(1 << 16, 4000, 4000) is False
    monkeypatch.setenv("PML_TL_TGROUP", "0")
    assert shard_tgroup(1 << 16, 96 << 20, 1 << 20) is None and not can(tgroup=None) and can(tgroup=True)
    monkeypatch.setenv("PML_TL_TGROUP", "1")
    assert can(tgroup=None, dim=100) and not can(tgroup=None, dtype=torch.float64)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_grouped_chunk_holds_the_input(precision):
    x, g, u = chunks(precision)
    ntiles = (DIM + 1023) // 1024
    assert ntiles == 69 and g.ngroups > 0 and u.ngroups == 0
    tiles_g = g.groups[:, 0].tolist()
    assert all(t % 4 == 0 and t + 3 < ntiles - 1 for t in tiles_g)          # the leftover / ragged tile: never grouped
    multi = set(u.mt_tiles[: u.nmt].tolist())
    assert multi and not any(t // 4 * 4 in tiles_g for t in multi)         # a multi-item tile keeps its whole quadruple
    assert set(g.items[:, 0].tolist()) == {t for t in u.items[:, 0].tolist() if t // 4 * 4 not in tiles_g}
    assert g.nparts == u.nparts and torch.equal(g.cu, u.cu) and torch.equal(g.mt_tiles, u.mt_tiles)
    # the narrow section is the ungrouped chunk's, stream and bases
    assert torch.equal(g.npack, u.npack) and torch.equal(g.nval, u.nval) and torch.equal(g.nbase, u.nbase)
    assert g.n_narrow_rounds == u.n_narrow_rounds > 0
    # every stored entry once: logical() against scipy
    row, col, val = g.coo()
    coo = x.tocoo()
    order = np.lexsort((coo.col, coo.row))
    assert np.array_equal(row.numpy(), coo.row[order]) and np.array_equal(col.numpy(), coo.col[order])
    assert np.array_equal(val.double().numpy(), coo.data[order])
    assert int(g.unit_counts().sum()) == x.nnz
    # entries are moved, not duplicated: no more bytes than the pad rounds allow
    assert g.nbytes() <= u.nbytes() + g.ngroups * (4 * 24 + 4 * IL_ROUND * (4 + val.element_size()))
    # the cases the kernels must meet
    gt = g.groups.to(torch.int64)
    assert EMPTY_TILE // 4 * 4 in tiles_g and int(gt[tiles_g.index(EMPTY_TILE // 4 * 4), 1 + EMPTY_TILE % 4]) == TG_EMPTY
    wide_rounds = (gt[:, 17:21] - gt[:, 13:17] + IL_ROUND - 1) // IL_ROUND
    assert bool((wide_rounds.sum(1) > 0).all()) and bool((wide_rounds == 0).any())   # some quarter is empty
    t = u.items.to(torch.int64)
    both = (t[:, 5] > t[:, 4]) & (t[:, 2] > t[:, 1]) & (t[:, 3] < 0)
    assert any(int(tl) // 4 * 4 in tiles_g for tl in t[both, 0])            # a grouped tile with narrow and wide rounds
    # the ungrouped twin is the chunk that tgroup=False builds
    w = g.ungrouped()
    assert torch.equal(w.pack, u.pack) and torch.equal(w.val, u.val) and torch.equal(w.items, u.items)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_emulated_rmatvec_matches_scipy(precision):
    x, g, u = chunks(precision)
    rng = np.random.default_rng(1)
    r = torch.from_numpy(rng.normal(size=ROWS))
    for sq in (False, True):
        want = (x.multiply(x) if sq else x).T @ r.numpy()
        got = g.emulate_rmatvec(r, square=sq).numpy()
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    # shard-wide tables of two chunks: the slots and combine tables of the ungrouped shard, groups cut by a bucket
    mg, mu = TLTMulti([g, g], [0, ROWS], DIM), TLTMulti([u, u], [0, ROWS], DIM)
    assert mg.ngroups == 2 * g.ngroups and mg.nitems + int((mg.groups[:, 1:5] != TG_EMPTY).sum()) == mu.nitems
    assert mg.nparts == mu.nparts and torch.equal(mg.cu, mu.cu) and torch.equal(mg.mt_tiles, mu.mt_tiles)
    assert bool((mg.groups[:, 1:5][mg.groups[:, 1:5] != TG_EMPTY] >= 0).all())      # two chunks: every tile is split
    part_u = {(c, t): p for c, t, _, _, p, *_ in mu.items.tolist()}
    for row in mg.groups.tolist():
        for k in range(4):
            if row[1 + k] != TG_EMPTY:
                assert part_u[(row[21], row[0] + k)] == row[1 + k]
    r2 = torch.cat([r, 2 * r])
    want = x.T @ (3 * r.numpy())
    assert np.allclose(mg.emulate_rmatvec(r2).numpy(), want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    t0 = g.groups[1, 0].item()
    b = TLTMulti([g, g], [0, ROWS], DIM, tile_range=(t0, t0 + 8))
    assert b.ngroups == 4
    got = b.emulate_rmatvec(r2).numpy()
    assert np.allclose(got[t0 * 1024:(t0 + 8) * 1024], want[t0 * 1024:(t0 + 8) * 1024], rtol=1e-12, atol=1e-12)
    assert not got[: t0 * 1024].any() and not got[(t0 + 8) * 1024:].any()
    with pytest.raises(ValueError):
        TLTMulti([g, g], [0, ROWS], DIM, tile_range=(t0 + 1, t0 + 8))


def _add_in_order(acc, slots, terms):
    for s, t in zip(slots.tolist(), terms.tolist()):       # one fp64 addition at a time, in the given order
        acc[s] += t


def _wide(ch, e_lo, n):
    ph = il_phys(torch.tensor([e_lo]), torch.tensor([n]))
    return ch.pack[ph].to(torch.int64).numpy() & 0xFFFFFFFF, ch.val[ph].double().numpy()


def _item_sums(ch, item, r):
    """tl_t_item<NW = 4>, fp64 accumulators: wave w adds its quarter of the narrow rounds, then its quarter of the
    wide rounds, in stored order; ((A0 + A1) + A2) + A3."""
    _, e_lo, e_hi, _, n_lo, n_hi = item
    nn, nr = n_hi - n_lo, -(-(e_hi - e_lo) // IL_ROUND)
    wp, wv = _wide(ch, e_lo, e_hi - e_lo)
    A = []
    for w in range(4):
        acc = np.zeros(1024)
        npk, nvl = ch.narrow_window(n_lo + nn * w // 4, n_lo + nn * (w + 1) // 4)
        npk = npk.numpy()
        _add_in_order(acc, npk & 1023, nvl.double().numpy() * r[npk >> 10])
        lo, hi = IL_ROUND * (nr * w // 4), min(IL_ROUND * (nr * (w + 1) // 4), len(wp))
        _add_in_order(acc, wp[lo:hi] & 1023, wv[lo:hi] * r[wp[lo:hi] >> 10])
        A.append(acc)
    return ((A[0] + A[1]) + A[2]) + A[3]


def _group_sums(ch, g, r):
    """tl_t_group: for q = 0..3, wave k adds quarter q of tile k's narrow rounds into slots [1024 k, 1024 k + 1024),
    one wave adds sub-window q in stored order; tot = q ? tot + acc : acc."""
    tot = None
    for q in range(4):
        acc = np.zeros(4096)
        for k in range(4):
            n_lo, nn = g[5 + k], g[9 + k] - g[5 + k]
            npk, nvl = ch.narrow_window(n_lo + nn * q // 4, n_lo + nn * (q + 1) // 4)
            npk = npk.numpy()
            _add_in_order(acc, 1024 * k + (npk & 1023), nvl.double().numpy() * r[npk >> 10])
        wp, wv = _wide(ch, g[13 + q], g[17 + q] - g[13 + q])
        _add_in_order(acc, wp & 4095, wv * r[wp >> 12])
        tot = acc if q == 0 else tot + acc
    return tot


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_order_of_additions_is_the_ungrouped_layout_s(precision):
    """Values over 2^-20 .. 2^20 times a per-row vector over 2^-10 .. 2^10: a column's fp64 sum depends on the order
    and the grouping of its additions (checked below), and the grouped layout reproduces every tile's bits."""
    _, g, u = chunks(precision, wide_exponents=True)
    rng = np.random.default_rng(2)
    r = (rng.normal(size=ROWS) * 2.0 ** rng.integers(-10, 11, ROWS)).astype(np.float32).astype(np.float64)
    want = {it[0]: _item_sums(u, it, r) for it in u.items.tolist() if it[3] < 0}     # the single-item tiles
    checked, order_matters = 0, False
    for row in g.groups.tolist():
        tot = _group_sums(g, row, r)
        for k in range(4):
            if row[1 + k] == TG_EMPTY:
                assert row[0] + k not in want and not tot[1024 * k:1024 * (k + 1)].any()
                continue
            assert np.array_equal(tot[1024 * k:1024 * (k + 1)], want[row[0] + k]), f"tile {row[0] + k}"
            checked += 1
    assert checked == int((g.groups[:, 1:5] != TG_EMPTY).sum()) > 40
    # the same entries summed in plain (row, column) order give other bits somewhere: the test can fail
    x_r, x_c, x_v = g.coo()
    plain = np.zeros(DIM)
    _add_in_order(plain, x_c.numpy(), x_v.double().numpy() * r[x_r.numpy()])
    for t, s in want.items():
        order_matters |= not np.array_equal(plain[t * 1024:(t + 1) * 1024][: len(s)], s[: DIM - t * 1024])
    assert order_matters
