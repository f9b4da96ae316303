"""Fused narrow records (``PML_TL_FUSE``) on the GPU: a bf16 shard built with the switch on gives bit for bit what
the same shard built with it off gives — value, gradient, Hessian-vector product and Hessian diagonal (the squared
transpose), through the shard-wide and the per-chunk kernels, and for row-sampled copies — and both agree with the
fp64 CPU reference to the bf16 tolerances of test_kernels_gpu.py.

Small shapes (test_tl_fused_layout.fused_case_matrix): 2100 rows in two chunks (1100 + 1000), 8000 columns, 64-row
forward blocks and transpose items of at most 1536 entries, so a few dozen units per copy cover every round count
the stream loops distinguish (asserted from the unit tables, not assumed)."""
import numpy as np
import pytest
import torch

from photon_ml_amd.data.matrix import LabeledData
from photon_ml_amd.function.losses import LOGISTIC
from photon_ml_amd.ops.reference import TorchGLMData
from test_tl_fused_layout import CHUNK_ROWS, DIM, ITEM_ENTRIES, RBITS, fused_case_matrix, round_coverage

pytestmark = pytest.mark.gpu

TOL = 2e-5            # bf16 storage, fp32 coefficient gathers: tests/test_kernels_gpu.py TOL["bf16"] (x 10 for Hessians)


def _labeled() -> LabeledData:
    x = fused_case_matrix()
    rng = np.random.default_rng(4)
    n = x.shape[0]
    return LabeledData(x, (rng.random(n) < 0.5).astype(float), offsets=rng.normal(size=n) * 0.1,
                       weights=rng.random(n) + 0.5)


@pytest.fixture(scope="module")
def case():
    """{fuse: shard} for fuse in (0, 1), the fp64 reference and the test vectors; built once."""
    from photon_ml_amd.ops import tiled
    from photon_ml_amd.ops.device import DeviceGLMData
    data = _labeled()
    saved = tiled.FUSE, tiled.DEFAULT_RBITS
    shards = {}
    try:
        tiled.DEFAULT_RBITS = RBITS
        for fuse in (0, 1):
            tiled.FUSE = fuse
            shards[fuse] = DeviceGLMData.from_labeled(data, "cuda", "bf16", chunk_rows=CHUNK_ROWS[0], relabel=False,
                                                      layout="tiled", item_entries=ITEM_ENTRIES)
            shards[fuse].track_hessian = True
    finally:
        tiled.FUSE, tiled.DEFAULT_RBITS = saved
    rng = np.random.default_rng(1)
    w = torch.from_numpy(rng.normal(size=DIM) * 0.05).float().double()      # the kernels gather w in fp32
    v = torch.from_numpy(rng.normal(size=DIM)).float().double()
    return shards, TorchGLMData(data, "cpu"), w, v


def _passes(dev, w, v):
    f, s, g = dev.value_grad_sums(LOGISTIC, w.cuda(), 0.01)
    h, p = dev.hv_sums(LOGISTIC, w.cuda(), 0.01, v.cuda(), 0.2)
    d = dev.hdiag_sums(LOGISTIC, w.cuda())
    z = dev.margins(w.cuda() * 0.5)
    return f, s, p, g.clone(), h.clone(), d.clone(), z.clone()


def _same(a, b):
    return a[:3] == b[:3] and all(torch.equal(x, y) for x, y in zip(a[3:], b[3:]))


def test_shards_hold_the_unit_shapes(case):
    shards = case[0]
    for fuse, dev in shards.items():
        assert len(dev.csr) == 2 and [c.m for c in dev.csr] == list(CHUNK_ROWS) and dev.validate()
        assert all(c.fused == bool(fuse) and c.n_narrow_rounds > 0 for c in dev.csr + dev.csc)
        round_coverage(dev.csr, 2)              # forward work-groups: 2 waves
        round_coverage(dev.csc, 4)              # transpose work-groups: 4 waves
        assert all(c.nparts > 0 and c.ncu > 0 for c in dev.csc)      # split tiles: the two-level combine runs
    for a, b in zip(shards[0].csr + shards[0].csc, shards[1].csr + shards[1].csc):
        assert torch.equal(a._table(), b._table()) and a.nbytes() == b.nbytes()


@pytest.mark.parametrize("multi", [1, 0])
def test_fused_equals_two_array_layout_bitwise(case, multi):
    """Switch on == switch off, bit for bit, through the shard-wide (``multi``) and the per-chunk kernels; each is
    bitwise repeatable; both match the fp64 reference."""
    from photon_ml_amd.ops.native import configure
    shards, ref, w, v = case
    out = {}
    try:
        configure(tl_multi=multi)
        for fuse, dev in shards.items():
            dev._dzz_key = None
            out[fuse] = _passes(dev, w, v)
            dev._dzz_key = None
            assert _same(_passes(dev, w, v), out[fuse]), f"fuse={fuse}: two passes differ"
            if multi:
                assert dev._multi is not None and dev._multi_t is not None     # the one-launch paths really ran
    finally:
        configure(tl_multi=1)
    assert _same(out[1], out[0])
    f0, s0, g0 = ref.value_grad_sums(LOGISTIC, w, 0.01)
    h0, p0 = ref.hv_sums(LOGISTIC, w, 0.01, v, 0.2)
    d0 = ref.hdiag_sums(LOGISTIC, w)
    f1, s1, p1, g1, h1, d1, z1 = out[1]
    assert abs(f1 - f0) <= TOL * max(1.0, abs(f0)) and abs(s1 - s0) <= TOL * max(1.0, abs(s0))
    assert torch.allclose(g1.cpu(), g0, rtol=TOL, atol=TOL * float(g0.abs().max()))
    assert abs(p1 - p0) <= TOL * max(1, abs(p0)) * 10
    assert torch.allclose(h1.cpu(), h0, rtol=TOL * 10, atol=TOL * 10 * float(h0.abs().max()))
    assert torch.allclose(d1.cpu(), d0, rtol=TOL * 10, atol=TOL * 10 * float(d0.abs().max()))
    assert torch.allclose(z1.cpu(), ref.margins(w * 0.5), rtol=TOL, atol=TOL * 10)


@pytest.mark.parametrize("filt", [False, True])
def test_row_sampled_copy_of_a_fused_shard(case, filt, monkeypatch):
    """``row_sampled`` reads the narrow entries through the same position function (``filt``: narrow rounds
    filtered too, else shared): streams, tables and passes equal those of the two-array shard's copy."""
    from photon_ml_amd.ops import device
    shards, _, w, v = case
    monkeypatch.setattr(device, "NARROW_FILTER_BELOW", 1.0 if filt else 0.0)
    keep = torch.rand(sum(CHUNK_ROWS), generator=torch.Generator().manual_seed(3)) < 0.4
    keep[300:500] = False
    views = {fuse: dev.row_sampled(keep.cuda()) for fuse, dev in shards.items()}
    for a, b in zip(views[0].csr + views[0].csc, views[1].csr + views[1].csc):
        assert b.fused == (not filt) and not a.fused
        assert b.n_narrow_rounds == a.n_narrow_rounds and (a.n_narrow_rounds == 0) == filt
        assert torch.equal(a._table(), b._table()) and torch.equal(a.pack, b.pack) and torch.equal(a.val, b.val)
        (pa, va), (pb, vb) = a.logical(), b.logical()
        assert torch.equal(pa, pb) and torch.equal(va, vb)
    assert views[1].validate()
    for view in views.values():
        view.track_hessian = True
    assert _same(_passes(views[1], w, v), _passes(views[0], w, v))
