"""The tiled kernels at the block widths (``rbits``) and tile widths (``cbits``) the layout builder accepts, on the
GPU: 5 bits (tiles narrower than a combine work-group's 64 columns), 8, 11 (2048 LDS slots, 32-key narrow window),
12 (4096 slots, 16-key window; an fp64 shard is cut down to 11) and both mixed pairs (a forward / transpose width
mix-up), for bf16, fp32 and fp64 shards, through the shard-wide (``tl_multi=1``) and the per-chunk kernels.

EXACT: ``X w``, ``X^T r`` and ``(X.X)^T r`` of the case's dyadic vectors are ``torch.equal`` to the float64 scipy
products — no tolerance; test_tl_bits_layout.py shows that every fp32 / fp64 summation order gives these bits and
that the tolerance check of the parity tests would not notice a lost entry. PARITY with the fp64 CPU reference to
the tolerances of test_kernels_gpu.py, bitwise repeatability, and bit-equal forward outputs of the two launch
paths. Row-sampled copies at 11 and 12 bits.

Shapes: test_tl_bits_layout.bits_case (27.7K rows x 30.7K columns, 61K non-zeros at 12 bits; 1.8K rows x 789
columns, 132K non-zeros at 5)."""
import numpy as np
import pytest
import torch

from photon_ml_amd.data.matrix import LabeledData
from photon_ml_amd.function.losses import LOGISTIC
from photon_ml_amd.ops.reference import TorchGLMData
from test_kernels_gpu import TOL
from test_tl_bits_layout import assert_case_layout, case_for

pytestmark = pytest.mark.gpu

BITS = ((5, 5), (8, 8), (11, 11), (12, 12), (12, 5), (5, 12))
PRECISIONS = ("bf16", "f32", "f64")


def _build(bits, precision):
    from photon_ml_amd.ops import tiled
    from photon_ml_amd.ops.device import DeviceGLMData
    case = case_for(bits, precision)
    rng = np.random.default_rng(4)
    n = case.x.shape[0]
    data = LabeledData(case.x, (rng.random(n) < 0.5).astype(float), offsets=rng.normal(size=n) * 0.1,
                       weights=rng.random(n) + 0.5)
    saved = tiled.DEFAULT_RBITS, tiled.DEFAULT_CBITS
    try:
        tiled.DEFAULT_RBITS, tiled.DEFAULT_CBITS = bits          # the REQUEST (an fp64 shard gets at most 11)
        dev = DeviceGLMData.from_labeled(data, "cuda", precision, chunk_rows=case.chunk_rows[0], relabel=False,
                                         layout="tiled", item_entries=case.item_entries)
    finally:
        tiled.DEFAULT_RBITS, tiled.DEFAULT_CBITS = saved
    dev.track_hessian = True
    rng = np.random.default_rng(1)
    w = torch.from_numpy(rng.normal(size=case.dim) * 0.05).float().double()     # the kernels gather w in fp32
    v = torch.from_numpy(rng.normal(size=case.dim)).float().double()
    return case, data, dev, w, v


@pytest.fixture(scope="module", params=[(b, p) for b in BITS for p in PRECISIONS],
                ids=lambda bp: f"r{bp[0][0]}c{bp[0][1]}-{bp[1]}")
def shard(request):
    """(bits, precision, case, labeled data, shard, w, v): one shard per parameter set, built once."""
    bits, precision = request.param
    return (bits, precision) + _build(bits, precision)


def test_shard_has_the_widths_and_unit_shapes(shard):
    bits, precision, case, _, dev, _, _ = shard
    cap = 11 if precision == "f64" else 12
    assert len(dev.csr) == len(dev.csc) == 2 and dev.layout == "tiled"
    assert all(f.rbits == min(bits[0], cap) for f in dev.csr) and all(t.cbits == min(bits[1], cap) for t in dev.csc)
    assert dev.validate()
    assert_case_layout(case, dev.csr, dev.csc, precision)


@pytest.mark.parametrize("multi", [1, 0])
def test_products_equal_scipy_bit_for_bit(shard, multi):
    from photon_ml_amd.ops.native import configure
    _, _, case, _, dev, _, _ = shard
    w, r = torch.from_numpy(case.w).cuda(), torch.from_numpy(case.r).cuda()
    try:
        configure(tl_multi=multi)
        for _ in range(2):
            z = dev.matvec(w).cpu()
            g = dev.rmatvec(r).cpu()
            g2 = dev.rmatvec(r, square=True).cpu()
            if multi:
                assert dev._multi is not None and dev._multi_t is not None     # the one-launch kernels really ran
            for name, got, want in (("X w", z, case.z), ("X^T r", g, case.g), ("(X.X)^T r", g2, case.g2)):
                want = torch.from_numpy(want)
                bad = torch.nonzero(got != want).reshape(-1)
                assert got.dtype == torch.float64 and got.shape == want.shape
                assert torch.equal(got, want), (f"{name}: {bad.numel()} of {want.numel()} differ, first at "
                                                f"{bad[:5].tolist()}: {got[bad[:5]].tolist()} != "
                                                f"{want[bad[:5]].tolist()}")
    finally:
        configure(tl_multi=1)


def _passes(dev, w, v):
    f, s, g = dev.value_grad_sums(LOGISTIC, w.cuda(), 0.01)
    h, p = dev.hv_sums(LOGISTIC, w.cuda(), 0.01, v.cuda(), 0.2)
    d = dev.hdiag_sums(LOGISTIC, w.cuda())
    z = dev.margins(w.cuda() * 0.5, 0.0, True)
    return f, s, p, g.clone(), h.clone(), d.clone(), z.clone()


def _same(a, b):
    return a[:3] == b[:3] and all(torch.equal(x, y) for x, y in zip(a[3:], b[3:]))


def test_parity_with_the_cpu_reference_and_bitwise_repeatability(shard):
    """Value, gradient, Hessian-vector product, Hessian diagonal and margins with offsets against ``TorchGLMData``
    in fp64 (tolerances: ``TOL`` of test_kernels_gpu.py, x 10 for the Hessian quantities, in the form of
    test_tl_fused_gpu.py); every quantity identical on a second run; F, S and the margins bit-equal between the
    shard-wide and the per-chunk launches."""
    from photon_ml_amd.ops.native import configure
    _, precision, _, data, dev, w, v = shard
    tol = TOL[precision]
    ref = TorchGLMData(data, "cpu")
    f0, s0, g0 = ref.value_grad_sums(LOGISTIC, w, 0.01)
    h0, p0 = ref.hv_sums(LOGISTIC, w, 0.01, v, 0.2)
    d0 = ref.hdiag_sums(LOGISTIC, w)
    z0 = ref.margins(w * 0.5, 0.0, True)
    out = {}
    try:
        for multi in (1, 0):
            configure(tl_multi=multi)
            dev._dzz_key = None
            out[multi] = _passes(dev, w, v)
            dev._dzz_key = None
            assert _same(_passes(dev, w, v), out[multi]), f"tl_multi={multi}: two passes differ"
            if multi:
                assert dev._multi is not None and dev._multi_t is not None
            f1, s1, p1, g1, h1, d1, z1 = out[multi]
            assert abs(f1 - f0) <= tol * max(1.0, abs(f0)) and abs(s1 - s0) <= tol * max(1.0, abs(s0))
            assert torch.allclose(g1.cpu(), g0, rtol=tol, atol=tol * float(g0.abs().max()))
            assert abs(p1 - p0) <= tol * max(1, abs(p0)) * 10
            assert torch.allclose(h1.cpu(), h0, rtol=tol * 10, atol=tol * 10 * float(h0.abs().max()))
            assert torch.allclose(d1.cpu(), d0, rtol=tol * 10, atol=tol * 10 * float(d0.abs().max()))
            assert torch.allclose(z1.cpu(), z0, rtol=tol, atol=tol * 10)
    finally:
        configure(tl_multi=1)
    assert out[1][:2] == out[0][:2] and torch.equal(out[1][6], out[0][6])     # F, S, margins: the same blocks


@pytest.fixture(scope="module", params=[(11, 11), (12, 12)], ids=lambda b: f"r{b[0]}c{b[1]}-bf16")
def bf16_shard(request):
    return (request.param, "bf16") + _build(request.param, "bf16")


@pytest.mark.parametrize("filt", [0.0, 1.0])
def test_row_sampled_copy(bf16_shard, filt, monkeypatch):
    """``row_sampled`` at the 32-key and the 16-key narrow window (narrow rounds shared: 0.0, filtered: 1.0): the
    copy's products equal those of the row-masked matrix bit for bit (``X w`` on the kept rows: a dropped row may
    keep partial margins by design)."""
    from photon_ml_amd.ops import device
    _, _, case, _, dev, _, _ = bf16_shard
    monkeypatch.setattr(device, "NARROW_FILTER_BELOW", filt)
    n = case.x.shape[0]
    keep = torch.rand(n, generator=torch.Generator().manual_seed(3)) < 0.4
    lo = case.chunk_rows[0] - 300                # a dropped 200-row span among the loud rows of chunk 0
    keep[lo:lo + 200] = False
    view = dev.row_sampled(keep.cuda())
    assert view is not None and view.validate()
    assert all((c.n_narrow_rounds == 0) == bool(filt) for c in view.csr + view.csc)
    k = keep.numpy()
    xm = case.x.multiply(k[:, None].astype(np.float64)).tocsr()
    r = np.where(k, case.r, 0.0)
    assert torch.equal(view.rmatvec(torch.from_numpy(r).cuda()).cpu(), torch.from_numpy(xm.T @ r))
    assert torch.equal(view.rmatvec(torch.from_numpy(r).cuda(), square=True).cpu(),
                       torch.from_numpy(xm.multiply(xm).T @ r))
    z = view.matvec(torch.from_numpy(case.w).cuda()).cpu()
    assert torch.equal(z[keep], torch.from_numpy(case.z)[keep])
