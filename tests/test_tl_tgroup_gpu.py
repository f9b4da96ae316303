"""Tile groups of the transpose copy on the GPU (``tl_tg_kernel`` / ``tl_tg_multi_kernel``): the same shard with the
groups on and off must agree BIT FOR BIT (the group kernel performs the additions of ``tl_t_item`` in its order and
grouping), both agree with the fp64 CPU reference at the tolerance of tests/test_tl_tall_gpu.py, and repeated
passes are bitwise equal. Shapes: tests/tl_tgroup_util.py (69 tiles: groups, multi-item tiles, an empty tile inside
a group, a leftover and a ragged tile), 4000 rows per chunk."""
import numpy as np
import pytest
import torch

from photon_ml_amd.data.matrix import LabeledData
from photon_ml_amd.function.losses import LOGISTIC, POISSON, SQUARED
from photon_ml_amd.ops.reference import TorchGLMData
from photon_ml_amd.ops.tiled import IL_ROUND, TG_EMPTY
from tl_tgroup_util import DIM, EMPTY_TILE, ITEM_ENTRIES, make_matrix

pytestmark = pytest.mark.gpu

TOL = {"f32": 2e-5, "bf16": 2e-5}          # tests/test_tl_tall_gpu.py TOL
CHUNK_ROWS = 4000
LOSSES = (LOGISTIC, POISSON, SQUARED)
_DATA, _REF, _DEV = {}, {}, {}


def labeled(precision, chunks):
    key = (precision, chunks)
    if key not in _DATA:
        x = make_matrix(CHUNK_ROWS * chunks, seed=chunks)
        if precision == "bf16":
            x.data = torch.from_numpy(x.data).to(torch.bfloat16).double().numpy()
        else:
            x.data = x.data.astype(np.float32).astype(np.float64)
        rng = np.random.default_rng(11)
        n = x.shape[0]
        y = (rng.random(n) < 0.4).astype(float)
        _DATA[key] = LabeledData(x, y, offsets=rng.normal(size=n) * 0.1, weights=rng.random(n) + 0.5)
    return _DATA[key]


def vectors():
    """Coefficients and a direction on a 2^-10 grid (exact in fp32, which the kernels gather)."""
    rng = np.random.default_rng(5)
    return (torch.from_numpy(rng.integers(-60, 61, DIM) / 1024.0), torch.from_numpy(rng.integers(-60, 61, DIM) / 1024.0))


def reference(precision, chunks):
    key = (precision, chunks)
    if key not in _REF:
        ref = TorchGLMData(labeled(precision, chunks), "cpu")
        w, v = vectors()
        _REF[key] = {"vg": {l.loss_id: ref.value_grad_sums(l, w, 0.03) for l in LOSSES},
                     "hv": ref.hv_sums(LOGISTIC, w, 0.01, v, 0.2), "hd": ref.hdiag_sums(LOGISTIC, w)}
    return _REF[key]


def device_shard(precision, chunks, tgroup):
    from photon_ml_amd.ops.device import DeviceGLMData
    key = (precision, chunks, tgroup)
    if key not in _DEV:
        data = labeled(precision, chunks)
        x = data.x
        dev = DeviceGLMData.from_device_csr(
            torch.from_numpy(x.indptr.astype(np.int64)), torch.from_numpy(x.indices.astype(np.int64)),
            torch.from_numpy(x.data), torch.from_numpy(data.y), torch.from_numpy(data.offsets),
            torch.from_numpy(data.weights), DIM, "cuda", precision, chunk_rows=CHUNK_ROWS, item_entries=ITEM_ENTRIES,
            tgroup=tgroup)
        assert len(dev.csc) == chunks and all((ch.ngroups > 0) == tgroup and ch.cbits == 10 for ch in dev.csc)
        dev.track_hessian = True
        _DEV[key] = dev
    return _DEV[key]


def close(got, want, tol):
    want = torch.as_tensor(want)
    return torch.allclose(torch.as_tensor(got).cpu(), want, rtol=tol, atol=tol * max(1.0, float(want.abs().max())))


def test_shapes_hold_every_case():
    """What the kernels must meet occurs in the shards of the tests below."""
    one, three = device_shard("bf16", 1, True), device_shard("bf16", 3, True)
    ch = one.csc[0]
    g = ch.groups.cpu().to(torch.int64)
    tiles = g[:, 0].tolist()
    assert ch.nmt > 0 and ch.nitems > 0                                       # multi-item tiles next to the groups
    assert int(g[tiles.index(EMPTY_TILE // 4 * 4), 1 + EMPTY_TILE % 4]) == TG_EMPTY   # an empty tile inside a group
    rounds = (g[:, 17:21] - g[:, 13:17] + IL_ROUND - 1) // IL_ROUND
    assert bool(((rounds == 0).any(1) & (rounds.sum(1) > 0)).any())          # fewer than 4 wide rounds: empty quarters
    k12 = g[tiles.index(12), :]
    assert int(k12[9] - k12[5]) > 0 and int((k12[17:21] - k12[13:17]).sum()) > 0   # tile 12: narrow and wide rounds
    assert (DIM + 1023) // 1024 == 69 and max(tiles) + 4 <= 68                # leftover + ragged tile stay items
    assert 68 in ch.items[:, 0].tolist()
    one._build_multi_t()
    three._build_multi_t()
    p1, p3 = one._multi_t.groups[:, 1:5], three._multi_t.groups[:, 1:5]
    assert bool((p1[p1 != TG_EMPTY] == -1).all()) and bool((p3[p3 != TG_EMPTY] >= 0).all())   # part < 0 / part >= 0
    assert one._multi_t.ngroups == ch.ngroups and three._multi_t.ngroups == sum(c.ngroups for c in three.csc)


@pytest.mark.parametrize("multi", [0, 1])
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_grouped_equals_ungrouped_bit_for_bit(precision, chunks, multi):
    """Gradient (three losses), Hessian-vector product and Hessian diagonal (the squared transpose): groups on vs
    off with torch.equal, per-chunk and shard-wide launches, one and three chunks; both against the fp64 reference;
    a second pass is bitwise equal."""
    from photon_ml_amd.ops.native import configure
    want = reference(precision, chunks)
    on, off = device_shard(precision, chunks, True), device_shard(precision, chunks, False)
    assert on.validate() is not False and off.validate() is not False
    w, v = vectors()
    w, v = w.cuda(), v.cuda()
    tol = TOL[precision]
    try:
        configure(tl_multi=multi)
        for loss in LOSSES:
            f0, s0, g0 = want["vg"][loss.loss_id]
            f1, s1, g1 = on.value_grad_sums(loss, w, 0.03)
            fu, su, gu = off.value_grad_sums(loss, w, 0.03)
            assert f1 == fu and s1 == su and torch.equal(g1, gu), loss
            assert abs(f1 - f0) <= tol * max(1.0, abs(f0)) and abs(s1 - s0) <= tol * max(1.0, abs(s0))
            assert torch.allclose(g1.cpu(), g0, rtol=tol, atol=tol * float(g0.abs().max()))
            f2, s2, g2 = on.value_grad_sums(loss, w, 0.03)
            assert f2 == f1 and s2 == s1 and torch.equal(g2, g1)
        hv = []
        for dev in (on, off):
            dev.value_grad_sums(LOGISTIC, w, 0.01)
            hv.append(dev.hv_sums(LOGISTIC, w, 0.01, v, 0.2))
        assert hv[0][1] == hv[1][1] and torch.equal(hv[0][0], hv[1][0])
        h0, p0 = want["hv"]
        assert abs(hv[0][1] - p0) <= 10 * tol * max(1.0, abs(p0)) and close(hv[0][0], h0, 10 * tol)
        hd1, hd0 = on.hdiag_sums(LOGISTIC, w), off.hdiag_sums(LOGISTIC, w)
        assert torch.equal(hd1, hd0) and close(hd1, want["hd"], 10 * tol)
        assert torch.equal(on.hdiag_sums(LOGISTIC, w), hd1)
    finally:
        configure(tl_multi=1)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_bucketed_launches(precision):
    """Gradient buckets (``tile_range`` launches) of a grouped shard: cuts on group boundaries, some bucket holds
    groups, and the result is the one-launch pass's and the ungrouped shard's, bit for bit."""
    on, off = device_shard(precision, 3, True), device_shard(precision, 3, False)
    w, _ = vectors()
    w = w.cuda()
    buckets = on.grad_buckets(3)
    assert buckets and len(buckets) >= 2 and all(c0 % 4096 == 0 for _, c0, _ in buckets)
    assert sum(mt.ngroups for mt, _, _ in buckets) == sum(ch.ngroups for ch in on.csc) > 0
    got = on.value_grad_packed_overlap(LOGISTIC, w, 0.03, lambda s: None, nb=3)
    assert torch.equal(got, off.value_grad_packed_overlap(LOGISTIC, w, 0.03, lambda s: None, nb=3))
    assert torch.equal(got, on.value_grad_packed(LOGISTIC, w, 0.03))


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_live_mask_path(precision):
    """Entity-masked transpose (per-chunk launches with live flags): a group runs iff one of its four tiles holds a
    column of an active entity; the active entities' columns equal the ungrouped shard's bit for bit and the
    unmasked product's, and a dead group writes nothing."""
    on, off = device_shard(precision, 3, True), device_shard(precision, 3, False)
    n = on.n_rows
    row_entity = torch.zeros(n, dtype=torch.int64, device="cuda")            # every row: entity 0 (always active)
    col_entity = torch.arange(DIM, device="cuda") // 6000                      # 12 entities cut across tiles and groups
    active = torch.zeros(12, dtype=torch.bool, device="cuda")
    active[[0, 3, 4, 9]] = True
    r = torch.from_numpy(np.random.default_rng(7).integers(-60, 61, n) / 1024.0).cuda()
    full = on.rmatvec(r)
    out = []
    for dev in (on, off):
        geo = dev.entity_mask_geometry(row_entity, col_entity)
        assert geo
        try:
            dev.set_entity_mask(active, geo)
            out.append(dev.rmatvec(r))
            out.append(dev.rmatvec(r))
        finally:
            dev.set_entity_mask(None)
    cols = active[col_entity]
    assert torch.equal(out[0][cols], out[2][cols]) and torch.equal(out[0][cols], full[cols])
    assert torch.equal(out[0], out[1])
    # a group without an active column did not run: its (non-empty) columns stay zero
    dead = torch.zeros(DIM, dtype=torch.bool, device="cuda")
    for t0 in on.csc[0].groups[:, 0].tolist():
        lo, hi = t0 * 1024, min((t0 + 4) * 1024, DIM)
        if not bool(cols[lo:hi].any()):
            dead[lo:hi] = True
    assert bool(dead.any()) and bool((full[dead] != 0).any()) and bool((out[0][dead] == 0).all())


def test_row_sampled_copy_and_column_stats_of_a_grouped_shard():
    """The readers that walk items get the chunks' ungrouped twins: the row-sampled copy of a grouped shard and its
    column statistics equal the ungrouped shard's bit for bit."""
    on, off = device_shard("bf16", 3, True), device_shard("bf16", 3, False)
    keep = torch.from_numpy(np.random.default_rng(3).random(on.n_rows) < 0.5).cuda()
    w, _ = vectors()
    w = w.cuda()
    views = [dev.row_sampled(keep) for dev in (on, off)]
    assert all(v is not None and v.validate() is not False for v in views)
    assert all(ch.ngroups == 0 for ch in views[0].csc)
    saved = on.wt.clone(), off.wt.clone()
    try:
        res = []
        for dev, view in zip((on, off), views):
            dev.wt.mul_(keep.to(dev.wt.dtype))
            dev.mark_weights_changed()
            res.append(view.value_grad_sums(LOGISTIC, w, 0.03))
    finally:
        for dev, s in zip((on, off), saved):
            dev.wt.copy_(s)
            dev.mark_weights_changed()
    assert res[0][0] == res[1][0] and torch.equal(res[0][2], res[1][2])
    for a, b in zip(on.column_stats(), off.column_stats()):
        assert torch.equal(a, b)
