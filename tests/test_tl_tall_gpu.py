"""Tall forward units on the GPU (``tl_fwd_tall_kernel`` / ``tl_fwd_tall_multi_kernel``): the shapes of
tests/test_tl_tall.py with the tall layout forced, against the fp64 CPU reference with the tolerances of
tests/test_kernels_gpu.py, against the same shard with the tall layout off (a pure fp64 re-ordering), run to run,
and through the row-sampled copies and the live block masks."""
import numpy as np
import pytest
import torch

from photon_ml_amd.data.matrix import LabeledData
from photon_ml_amd.function.losses import LOGISTIC, POISSON
from photon_ml_amd.ops.reference import TorchGLMData
from tl_tall_util import CASES, make_case

pytestmark = pytest.mark.gpu

TOL = {"f32": 2e-5, "bf16": 2e-5}          # tests/test_kernels_gpu.py TOL
_DATA, _REF, _DEV = {}, {}, {}


def labeled(name, precision):
    """The case as LabeledData (bf16: values rounded first, so the reference sees what the shard stores)."""
    key = (name, precision)
    if key not in _DATA:
        x, *_ = make_case(name)
        rng = np.random.default_rng(11)
        n = x.shape[0]
        if precision == "bf16":
            x.data = torch.from_numpy(x.data).to(torch.bfloat16).double().numpy()
        y = (rng.random(n) < 0.4).astype(float)
        _DATA[key] = LabeledData(x, y, offsets=rng.normal(size=n) * 0.1, weights=rng.random(n) + 0.5)
    return _DATA[key]


def vectors(dim):
    """Coefficients and a direction on a 2^-10 grid: w, d and w + d / 2 are exact in fp32 (the kernels gather fp32)."""
    rng = np.random.default_rng(5)
    w = torch.from_numpy(rng.integers(-60, 61, dim) / 1024.0)
    d = torch.from_numpy(rng.integers(-60, 61, dim) / 1024.0)
    return w, d


def reference(name, precision):
    key = (name, precision)
    if key not in _REF:
        data = labeled(name, precision)
        ref = TorchGLMData(data, "cpu")
        w, v = vectors(data.n_features)
        out = {"vg": {l.loss_id: ref.value_grad_sums(l, w, 0.03) for l in (LOGISTIC, POISSON)},
               "z": ref.margins(w), "hv": ref.hv_sums(LOGISTIC, w, 0.01, v, 0.2), "hd": ref.hdiag_sums(LOGISTIC, w),
               "z_half": ref.margins(w + 0.5 * v)}
        _REF[key] = (ref, out)
    return _REF[key]


def device_shard(name, precision, chunks, tall=True):
    from photon_ml_amd.ops.device import DeviceGLMData
    key = (name, precision, chunks, tall)
    if key not in _DEV:
        data = labeled(name, precision)
        x = data.x
        n = x.shape[0]
        dev = DeviceGLMData.from_device_csr(
            torch.from_numpy(x.indptr.astype(np.int64)), torch.from_numpy(x.indices.astype(np.int64)),
            torch.from_numpy(x.data), torch.from_numpy(data.y), torch.from_numpy(data.offsets),
            torch.from_numpy(data.weights), x.shape[1], "cuda", precision, chunk_rows=-(-n // chunks), tall=tall)
        assert len(dev.csr) == chunks and all(ch.tbits == (12 if tall else 0) for ch in dev.csr)
        dev.track_hessian = True
        _DEV[key] = dev
    return _DEV[key]


def close(got, want, tol):
    want = torch.as_tensor(want)
    return torch.allclose(torch.as_tensor(got).cpu(), want, rtol=tol, atol=tol * max(1.0, float(want.abs().max())))


@pytest.mark.parametrize("chunks,multi", [(1, 1), (2, 0), (2, 1)])
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_tall_parity_and_determinism(name, precision, chunks, multi):
    """Value / gradient (logistic, Poisson), margins, Hessian-vector and Hessian diagonal vs the fp64 reference,
    through the per-chunk and the shard-wide launch, one and two chunks per shard; two passes are bitwise equal."""
    from photon_ml_amd.ops.native import configure
    ref, want = reference(name, precision)
    dev = device_shard(name, precision, chunks)
    assert dev.validate() is not False
    w, v = vectors(dev.dim)
    w, v = w.cuda(), v.cuda()
    tol = TOL[precision]
    try:
        configure(tl_multi=multi)
        for loss in (LOGISTIC, POISSON):
            f0, s0, g0 = want["vg"][loss.loss_id]
            f1, s1, g1 = dev.value_grad_sums(loss, w, 0.03)
            assert abs(f1 - f0) <= tol * max(1.0, abs(f0)) and abs(s1 - s0) <= tol * max(1.0, abs(s0))
            assert torch.allclose(g1.cpu(), g0, rtol=tol, atol=tol * float(g0.abs().max()))
            f2, s2, g2 = dev.value_grad_sums(loss, w, 0.03)
            assert f2 == f1 and s2 == s1 and torch.equal(g2, g1)
        z = dev.margins(w).clone()
        assert close(z, want["z"], tol) and torch.equal(dev.margins(w), z)
        dev.value_grad_sums(LOGISTIC, w, 0.01)
        h1, p1 = dev.hv_sums(LOGISTIC, w, 0.01, v, 0.2)
        h0, p0 = want["hv"]
        assert abs(p1 - p0) <= 10 * tol * max(1.0, abs(p0)) and close(h1, h0, 10 * tol)
        assert close(dev.hdiag_sums(LOGISTIC, w), want["hd"], 10 * tol)
    finally:
        configure(tl_multi=1)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_tall_on_matches_tall_off(name, precision):
    """The same shard with tall units on and off: a pure fp64 re-ordering of each row's sum."""
    on, off = device_shard(name, precision, 2), device_shard(name, precision, 2, tall=False)
    w, _ = vectors(on.dim)
    w = w.cuda()
    z1, z0 = on.margins(w), off.margins(w)
    assert torch.allclose(z1, z0, rtol=1e-12, atol=1e-12 * float(z0.abs().max()))
    g1, g0 = on.value_grad_sums(LOGISTIC, w, 0.0)[2], off.value_grad_sums(LOGISTIC, w, 0.0)[2]
    assert torch.allclose(g1, g0, rtol=1e-12, atol=1e-12 * float(g0.abs().max()))


@pytest.mark.parametrize("multi", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_tall_loss_sums_are_the_row_block_layout_s(name, multi):
    """bf16 values (8 significant bits) times coefficients on the 2^-10 grid (6 bits) are sums of at most 12 terms
    whose exponents span far less than 53 bits: every row sum is exact in fp64, in any order, so the margins of the
    tall and the row-block layout are bitwise equal. The loss and sum l' must then be bitwise equal too: the tall
    kernel writes one stats pair per 1024-row sub-block, summed as the row-block kernel sums a block's."""
    from photon_ml_amd.ops.native import configure
    on, off = device_shard(name, "bf16", 2), device_shard(name, "bf16", 2, tall=False)
    assert all(ch.rbits == 10 for ch in off.csr) and [c.nstats for c in on.csr] == [c.nstats for c in off.csr]
    w, _ = vectors(on.dim)
    w = w.cuda()
    try:
        configure(tl_multi=multi)
        assert torch.equal(on.margins(w), off.margins(w))
        for loss in (LOGISTIC, POISSON):
            f1, s1, g1 = on.value_grad_sums(loss, w, 0.03)
            f0, s0, g0 = off.value_grad_sums(loss, w, 0.03)
            assert f1 == f0 and s1 == s0 and torch.equal(g1, g0)
    finally:
        configure(tl_multi=1)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("name", ["zipf", "short", "widedim"])
def test_tall_line_search_forward_mode(name, precision):
    """The margin-space line search's direction pass (FWD_LS) over tall units: the cached margins z0 + t zd equal
    the reference's margins at w + t d (both exact in fp32), with no further forward pass."""
    from photon_ml_amd.ops.device import DeviceGLMData
    _, want = reference(name, precision)
    data = labeled(name, precision)
    x = data.x
    dev = DeviceGLMData.from_device_csr(
        torch.from_numpy(x.indptr.astype(np.int64)), torch.from_numpy(x.indices.astype(np.int64)),
        torch.from_numpy(x.data), torch.from_numpy(data.y), torch.from_numpy(data.offsets),
        torch.from_numpy(data.weights), x.shape[1], "cuda", precision, chunk_rows=-(-x.shape[0] // 2), tall=True)
    w, d = vectors(dev.dim)
    w, d = w.cuda(), d.cuda()
    dev.enable_margin_cache()
    dev.value_grad_packed(LOGISTIC, w, 0.0)
    assert dev.ls_begin(w, 0.0, d, 0.0, 1.0, LOGISTIC)
    w1 = w + 0.5 * d
    dev.ls_finish_packed(LOGISTIC, 0.5, w1, 0.0)
    n0 = dev.n_passes
    cached = dev.margins(w1)
    assert dev.n_passes == n0 and close(cached, want["z_half"], TOL[precision])


@pytest.mark.parametrize("rate", [0.1, 0.3, 0.95])
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("name", ["zipf", "short", "uniform", "hot"])
def test_tall_row_sampled_copy(name, precision, rate):
    """``RowCompaction`` of tall chunks (0.1: the narrow rounds are filtered too; 0.3 and 0.95: shared): the copy
    passes the kernel-input validation and matches the reference with the dropped rows at zero weight."""
    data = labeled(name, precision)
    dev = device_shard(name, precision, 2)
    keep = torch.from_numpy(np.random.default_rng(3).random(data.x.shape[0]) < rate)
    keep[100:400] = False
    view = dev.row_sampled(keep.cuda())
    assert view is not None and view.validate() is not False
    assert all(ch.tbits == 12 for ch in view.csr) and view._multi is not None
    from photon_ml_amd.ops.device import NARROW_FILTER_BELOW
    filt = float(keep.double().mean()) < NARROW_FILTER_BELOW          # few rows kept: the narrow rounds are filtered too
    if name != "short":                                                # (short: 300 of its 700 rows dropped outright)
        assert filt == (rate < 0.2)
    assert sum(ch.n_narrow_rounds for ch in view.csr) == (0 if filt else sum(ch.n_narrow_rounds for ch in dev.csr))
    for full, samp in zip(dev.csr, view.csr):
        assert samp.nnz <= full.nnz
    ref = TorchGLMData(LabeledData(data.x, data.y, offsets=data.offsets, weights=data.weights * keep.numpy()), "cpu")
    w, _ = vectors(dev.dim)
    tol = TOL[precision]
    f0, s0, g0 = ref.value_grad_sums(LOGISTIC, w, 0.03)
    saved = dev.wt.clone()
    try:
        dev.wt.mul_(keep.cuda().to(dev.wt.dtype))       # the copy shares the row vectors of the full shard
        dev.mark_weights_changed()
        f1, s1, g1 = view.value_grad_sums(LOGISTIC, w.cuda(), 0.03)
        z1 = view.margins(w.cuda()).cpu()
    finally:
        dev.wt.copy_(saved)
        dev.mark_weights_changed()
    assert abs(f1 - f0) <= tol * max(1.0, abs(f0)) and abs(s1 - s0) <= tol * max(1.0, abs(s0))
    assert torch.allclose(g1.cpu(), g0, rtol=tol, atol=tol * float(g0.abs().max()))
    z0 = ref.margins(w)
    assert torch.allclose(z1[keep], z0[keep], rtol=tol, atol=tol * max(1.0, float(z0.abs().max())))


def test_tall_row_sampled_copy_needs_absolute_keys():
    """Per-round key bases do not survive compaction (entries move across rounds): no copy, as for row blocks."""
    dev = device_shard("widedim", "bf16", 2)
    assert all(ch.wbase is not None for ch in dev.csr)
    assert dev.row_sampled(torch.ones(dev.n_rows, dtype=torch.bool, device="cuda")) is None


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_tall_live_block_mask(precision):
    """Entity-masked forward over tall units: a unit runs iff one of its rows belongs to an active entity; the
    active entities' margins match the reference, skipped units stay zero."""
    _, want = reference("zipf", precision)
    dev = device_shard("zipf", precision, 2)
    n = dev.n_rows
    row_entity = (1 + torch.arange(n, device="cuda") // 1500)           # entities cut across units and chunks
    col_entity = torch.zeros(dev.dim, dtype=torch.int64, device="cuda")  # every column: entity 0 (always active)
    active = torch.tensor([True, False, True, False, False, False, True, False], device="cuda")
    assert int(row_entity.max()) < active.numel()
    geo = dev.entity_mask_geometry(row_entity, col_entity)
    assert geo
    w, _ = vectors(dev.dim)
    try:
        dev.set_entity_mask(active, geo)
        z = dev.margins(w.cuda()).cpu()
    finally:
        dev.set_entity_mask(None)
    rows = active[row_entity].cpu()
    tol = TOL[precision]
    assert torch.allclose(z[rows], want["z"][rows], rtol=tol, atol=tol * max(1.0, float(want["z"].abs().max())))
    blk = dev._multi_blk.cpu().to(torch.int64)
    ran = torch.zeros(n, dtype=torch.bool)
    for lo, cnt in zip(blk[:, 1].tolist(), blk[:, 2].tolist()):
        ran[lo:lo + cnt] = bool(rows[lo:lo + cnt].any())
    assert bool((~ran).any()) and bool((z[~ran] == 0).all())
