"""The blocked FULL-variance route on the GPU (``128 < m = min(n_e, d_e) <= 1024``): ``var_blk_normal_kernel`` /
``var_blk_gram_kernel`` / ``blocked_chol_kernel`` / ``blocked_trinv_kernel`` / ``var_blk_colnorm_kernel`` through
``SegmentedFullVariance(blocked_mmax=VAR_BLOCKED_MMAX)``, the wrappers alone and the coordinate end to end.

Tolerance and yardstick are those of test_full_variance_gpu.py: 1e-9 relative against ``numpy.linalg.inv`` of the
dense fp64 Hessian, with cond(H_e) <= 1e6 asserted on the CPU (the shapes here stay below 1e4). The panels and MFMA
tiles are 16 wide, so the orders sit on both sides of multiples of 16, of the class bounds (160, 192, 256, 512) and at
the cap.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import full_variance_util
from full_variance_util import BlockProblem, relative_error

pytestmark = pytest.mark.gpu

RTOL = 1e-9
COND_MAX = 1e6


def _plan(p: BlockProblem, **kw):
    from photon_ml_amd.ops.native import VAR_BLOCKED_MMAX
    from photon_ml_amd.optimization.variance import SegmentedFullVariance
    rp, cp, csr, c = p.tensors("cuda")
    kw.setdefault("blocked_mmax", VAR_BLOCKED_MMAX)
    return SegmentedFullVariance(rp, cp, csr, **kw), c


def _check(p: BlockProblem, lam: float, **kw):
    want = p.numpy_variances(lam, cond_max=COND_MAX)
    plan, c = _plan(p, **kw)
    got, stats = plan.compute(c, lam)
    torch.cuda.synchronize()
    err = relative_error(got.cpu().numpy(), want)
    print(f"shapes {p.shapes} lambda {lam}: max relative error {err:.3e}, routes {stats}")
    assert err <= RTOL
    return stats


@pytest.mark.parametrize("d", [129, 144, 145, 160, 161, 191, 192, 193, 256, 257, 511, 512, 513, 1024])
def test_blocked_primal_route(d):
    shapes = [(d, d), (d + 76, d)] + ([(3 * 129 + 1, 129)] if d == 129 else [])
    stats = _check(BlockProblem(shapes, seed=300 + d), 0.1 if d % 2 else 1.0)
    assert stats["blocked_primal"] == len(shapes) and stats["torch"] == 0 and stats["failed_factors"] == 0
    assert stats["blocked_row_space"] == 0 and stats["primal"] == 0


@pytest.mark.parametrize("n,d", [(129, 130), (129, 700), (193, 600), (257, 1001), (320, 1001), (513, 2048),
                                 (1023, 1024), (1024, 2048)])
def test_blocked_row_space_route(n, d):
    stats = _check(BlockProblem([(n, d)], seed=400 + n), 0.1 if n % 2 else 1.0)
    assert stats["blocked_row_space"] == 1 and stats["torch"] == 0 and stats["failed_factors"] == 0


def test_long_primal_entity():
    """4100 rows of 129 coefficients: every wave of the work-group walks the rows and owns a share of the output."""
    stats = _check(BlockProblem([(4100, 129)], seed=21), 0.1)
    assert stats["blocked_primal"] == 1 and stats["torch"] == 0


def test_rows_with_up_to_d_entries(monkeypatch):
    monkeypatch.setattr(full_variance_util, "MAX_ROW_NNZ", 10 ** 6)
    p = BlockProblem([(300, 200), (150, 200)], seed=22)
    assert int(np.diff(p.indptr).max()) > 150
    stats = _check(p, 1.0)
    assert stats["blocked_primal"] == 1 and stats["blocked_row_space"] == 1 and stats["torch"] == 0


def test_singular_gram_and_zero_weights():
    p = BlockProblem([(200, 400)], seed=7, duplicate_rows=(0,))
    assert np.linalg.matrix_rank(p.entity_dense(0) @ p.entity_dense(0).T) == 2
    stats = _check(p, 0.1)
    assert stats["blocked_row_space"] == 1 and stats["failed_factors"] == 0
    q = BlockProblem([(300, 1001)], seed=8, zero_weight_fraction=0.34)
    assert (q.c == 0).sum() >= 100
    stats = _check(q, 1.0)
    assert stats["blocked_row_space"] == 1 and stats["failed_factors"] == 0


def test_every_route_in_one_coordinate():
    shapes = [(40, 40), (10, 30), (129, 129), (129, 200), (200, 129), (0, 7), (1025, 1025), (1025, 1100)]
    p = BlockProblem(shapes, seed=11)
    lam = 0.1
    stats = _check(p, lam)
    assert stats == {"primal": 1, "row_space": 1, "blocked_primal": 2, "blocked_row_space": 1, "torch": 2, "empty": 1,
                     "failed_factors": 0}
    plan, c = _plan(p)
    got = plan.compute(c, lam)[0].cpu().numpy()
    assert np.array_equal(got[p.col_ptr[5]:p.col_ptr[6]], np.full(7, 1.0 / lam))
    from photon_ml_amd.optimization.variance import SegmentedFullVariance
    rp, cp, csr, c = p.tensors("cuda")
    got0, stats0 = SegmentedFullVariance(rp, cp, csr).compute(c, lam)
    assert stats0 == {"primal": 1, "row_space": 1, "torch": 5, "empty": 1, "failed_factors": 0}
    assert relative_error(got0.cpu().numpy(), p.numpy_variances(lam)) <= RTOL


CHUNK_SHAPES = [(140, 135), (150, 129), (160, 160), (135, 131), (200, 150), (131, 131), (170, 145),
                (130, 300), (135, 140), (150, 700), (129, 131), (160, 161), (144, 500), (131, 999)]


def test_chunking_is_bitwise_neutral():
    """Two classes (primal and row space, orders up to 160) of 7 entities each; a workspace of three slabs forces
    three chunks per class and gives bitwise what one chunk gives."""
    from photon_ml_amd.optimization.variance import blocked_chunk_entities
    p = BlockProblem(CHUNK_SHAPES, seed=23)
    plan, c = _plan(p)
    assert sorted(int(e.numel()) for _, _, e, _, _ in plan.blocked_classes) == [7, 7]
    one, stats = plan.compute(c, 0.1)
    one = one.clone()
    assert stats["blocked_primal"] == 7 and stats["blocked_row_space"] == 7 and stats["torch"] == 0
    small = 3 * 8 * 160 * 160
    for _, n, e, _, _ in plan.blocked_classes:
        step = blocked_chunk_entities(n, small)
        assert (int(e.numel()) + step - 1) // step >= 3
    assert torch.equal(one, plan.compute(c, 0.1, workspace_bytes=small)[0])
    assert torch.equal(one, plan.compute(c, 0.1, workspace_bytes=1)[0])
    plan_small, _ = _plan(p, blocked_workspace_bytes=small)
    assert torch.equal(one, plan_small.compute(c, 0.1)[0])
    assert relative_error(one.cpu().numpy(), p.numpy_variances(0.1, cond_max=COND_MAX)) <= RTOL


def test_deterministic():
    p = BlockProblem([(129, 129), (300, 140), (150, 400), (200, 1001), (40, 40), (10, 30), (1000, 130)], seed=24)
    plan, c = _plan(p)
    a = plan.compute(c, 0.1)[0].clone()
    b = plan.compute(c, 0.1)[0]
    assert torch.equal(a, b)
    plan2, _ = _plan(p)
    assert torch.equal(a, plan2.compute(c, 0.1)[0])


@pytest.mark.parametrize("n,nv", [(129, 129), (192, 192), (193, 180), (513, 513), (1024, 1024)])
def test_blocked_cholesky_alone(n, nv):
    """Against numpy.linalg.cholesky: max |L - L_ref| <= 1e-12 max |L_ref| on matrices with cond ~ 10. The rows and
    columns beyond ``nv`` hold NaN on entry (they are not read) and the identity on return; the strict upper triangle
    is zero; the slabs before and after the problem's own keep their sentinel."""
    from photon_ml_amd.ops import native
    rng = np.random.default_rng(n)
    M = rng.standard_normal((nv, nv))
    A = M @ M.T / nv + np.eye(nv)
    K = torch.full((3, n, n), 7.25, dtype=torch.float64, device="cuda")
    K[1] = float("nan")
    K[1, :nv, :nv] = torch.from_numpy(A).cuda()
    L, info = native.blocked_cholesky(K[1:2], torch.tensor([nv], device="cuda"))
    torch.cuda.synchronize()
    assert int(info[0]) == 0
    assert bool((K[0] == 7.25).all()) and bool((K[2] == 7.25).all())
    got = L[0].cpu().numpy()
    want = np.eye(n)
    want[:nv, :nv] = np.linalg.cholesky(A)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"blocked_cholesky n={n} nv={nv}: max error {err:.3e} of max |L|")
    assert err <= 1e-12
    assert np.array_equal(np.triu(got, 1), np.zeros((n, n)))
    assert np.array_equal(got[nv:, :], np.eye(n)[nv:, :]) and np.array_equal(got[:, nv:], np.eye(n)[:, nv:])


def test_blocked_cholesky_bad_pivots():
    from photon_ml_amd.ops import native
    K = torch.full((4, 200, 200), 7.25, dtype=torch.float64, device="cuda")
    K[1] = torch.eye(200, dtype=torch.float64, device="cuda")
    K[2] = torch.eye(200, dtype=torch.float64, device="cuda")
    K[1, 150, 150] = -1.0
    K[2, 37, 37] = float("nan")
    _, info = native.blocked_cholesky(K[1:3], torch.tensor([200, 200], device="cuda"))
    torch.cuda.synchronize()
    assert info.tolist() == [151, 38]
    assert bool((K[0] == 7.25).all()) and bool((K[3] == 7.25).all())


def test_validation_raises_before_any_launch():
    from photon_ml_amd.ops import native
    p = BlockProblem([(140, 130), (130, 150), (20, 20)], seed=3)
    rp, cp, csr, c = p.tensors("cuda")
    out = torch.full((int(cp[-1]),), -1.0, dtype=torch.float64, device="cuda")
    work = torch.full((2 * 130 * 130,), -2.0, dtype=torch.float64, device="cuda")
    e0 = torch.tensor([0], device="cuda")
    nv = torch.tensor([130], device="cuda")
    for order in (native.VAR_MMAX, native.VAR_BLOCKED_MMAX + 1):
        big = torch.zeros(order * order, dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError, match="class order"):
            native.var_blocked_assemble(native.VAR_PRIMAL, torch.tensor([2], device="cuda"), order, rp, cp, csr, c, 0.1,
                                        big)
        with pytest.raises(ValueError, match="class order"):
            native.var_blocked_colnorm(native.VAR_PRIMAL, big.view(1, order, order), torch.tensor([20], device="cuda"),
                                       torch.tensor([2], device="cuda"), rp, cp, out)
        assert bool((big == 0).all())
    with pytest.raises(ValueError, match="order"):
        native.blocked_cholesky(torch.zeros(1, 1025, 1025, dtype=torch.float64, device="cuda"), nv)
    for bad in ([3], [-1], [1 << 40]):
        ents = torch.tensor(bad, device="cuda")
        with pytest.raises(ValueError, match="entity index"):
            native.var_blocked_assemble(native.VAR_PRIMAL, ents, 130, rp, cp, csr, c, 0.1, work)
        with pytest.raises(ValueError, match="entity index"):
            native.var_blocked_colnorm(native.VAR_PRIMAL, work[:130 * 130].view(1, 130, 130), nv, ents, rp, cp, out)
    with pytest.raises(ValueError, match="workspace"):
        native.var_blocked_assemble(native.VAR_PRIMAL, e0, 130, rp, cp, csr, c, 0.1, work[:130 * 130 - 1])
    with pytest.raises(ValueError, match="workspace"):
        native.var_blocked_assemble(native.VAR_PRIMAL, e0, 130, rp, cp, csr, c, 0.1, work.cpu())
    with pytest.raises(ValueError, match="variance vector"):
        native.var_blocked_colnorm(native.VAR_PRIMAL, work[:130 * 130].view(1, 130, 130), nv, e0, rp, cp,
                                   out[:100].contiguous())
    # an entity wider than its primal class, a factor order above the entity, a row-space entity wider than its image
    with pytest.raises(ValueError, match="coefficients"):
        native.var_blocked_assemble(native.VAR_PRIMAL, torch.tensor([1], device="cuda"), 130, rp, cp, csr, c, 0.1, work)
    with pytest.raises(ValueError, match="factor orders"):
        native.var_blocked_colnorm(native.VAR_PRIMAL, work[:130 * 130].view(1, 130, 130),
                                   torch.tensor([131], device="cuda"), e0, rp, cp, out)
    with pytest.raises(ValueError, match="coefficients"):
        native.var_blocked_assemble(native.VAR_ROW_SPACE, torch.tensor([1], device="cuda"), 130, rp, cp, csr, c, 0.1,
                                    work, dcap=128)
    with pytest.raises(ValueError, match="image width"):
        native.var_blocked_assemble(native.VAR_ROW_SPACE, torch.tensor([1], device="cuda"), 130, rp, cp, csr, c, 0.1,
                                    work, dcap=native.VAR_BLOCKED_DMAX + 64)
    with pytest.raises(ValueError, match="row-space route needs"):
        native.var_blocked_colnorm(native.VAR_ROW_SPACE, work[:130 * 130].view(1, 130, 130), nv,
                                   torch.tensor([1], device="cuda"), rp, cp, out, 0.0, csr, c, dcap=192)
    lib = native.require_game_lib()
    assert lib.pml_var_blocked_mmax() == native.VAR_BLOCKED_MMAX == 1024
    assert lib.pml_var_blocked_dmax() == native.VAR_BLOCKED_DMAX
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()) and bool((work == -2.0).all())


def test_non_canonical_rows_raise_under_the_input_check(monkeypatch):
    from photon_ml_amd.ops import native
    monkeypatch.setenv("PML_CHECK_KERNEL_INPUTS", "1")
    p = BlockProblem([(140, 130)], seed=4)
    k0 = int(p.indptr[5])
    assert p.indptr[6] - k0 >= 2
    p.cols[[k0, k0 + 1]] = p.cols[[k0 + 1, k0]]
    rp, cp, csr, c = p.tensors("cuda")
    work = torch.full((130 * 130,), -2.0, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="strictly increasing"):
        native.var_blocked_assemble(native.VAR_PRIMAL, torch.tensor([0], device="cuda"), 130, rp, cp, csr, c, 0.1, work)
    torch.cuda.synchronize()
    assert bool((work == -2.0).all())


def test_estimator_on_device_end_to_end(monkeypatch):
    """GameEstimator on the device with FULL over users of 160 coefficients: users with 129 .. 159 rows take the
    blocked row-space route, users with at least 160 rows the blocked primal route; variances against the CPU
    definition at the device run's own coefficients. With PML_VAR_BLOCKED=0 the same entities are counted under torch."""
    from photon_ml_amd.data.game_data import generate_game_data
    from photon_ml_amd.data.random_effect import FixedEffectDataConfiguration, RandomEffectDataConfiguration
    from photon_ml_amd.estimators.game_estimator import GameEstimator
    from photon_ml_amd.function.losses import loss_for_task
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    from photon_ml_amd.optimization.variance import segmented_full_variance
    task, lam = "LOGISTIC_REGRESSION", 1.0
    data, _ = generate_game_data(n_rows=8000, n_users=60, d_user=160, seed=28, task=task)
    cfg = GLMOptimizationConfiguration(OptimizerConfig("TRON", 30, 1e-10), RegularizationContext("L2"), lam)
    loss = loss_for_task(task)

    def fit():
        est = (GameEstimator(device="cuda").set_training_task(task)
               .set_coordinate_data_configurations({"global": FixedEffectDataConfiguration("global"),
                                                    "per-user": RandomEffectDataConfiguration("userId", "user")})
               .set_coordinate_update_sequence(["global", "per-user"]))
        est.set_variance_computation_type("FULL")
        return est, est.fit(data, None, [{"global": cfg, "per-user": cfg}])[0]

    est, res = fit()
    co = est.coordinates["per-user"]
    routes = co.last_variance_routes
    print(f"device estimator, blocked route: routes {routes}")
    assert routes["blocked_primal"] > 0 and routes["blocked_row_space"] > 0 and routes["failed_factors"] == 0, routes
    re = res.model.get("per-user")
    seg = co.dataset.seg
    nip, pos, val = (t.cpu() for t in co.dataset._seg_csr)
    W = torch.from_numpy(re.values)
    X = sp.csr_matrix((val.numpy(), pos.numpy(), nip.numpy()), shape=(seg.y.numel(), W.numel()))
    z = torch.from_numpy(X @ W.numpy()) + seg.o.cpu()
    c = seg.w.cpu() * loss.dzz(z, seg.y.cpu())
    want, _ = segmented_full_variance(seg.row_ptr.cpu(), seg.col_ptr.cpu(), (nip, pos, val), c, lam)
    err = relative_error(re.variances, want.numpy())
    print(f"device estimator, random effect: max relative error {err:.3e}")
    assert err <= RTOL
    monkeypatch.setenv("PML_VAR_BLOCKED", "0")
    est0, res0 = fit()
    routes0 = est0.coordinates["per-user"].last_variance_routes
    assert "blocked_primal" not in routes0 and "blocked_row_space" not in routes0
    assert routes0["torch"] == routes["torch"] + routes["blocked_primal"] + routes["blocked_row_space"]
    assert relative_error(res0.model.get("per-user").variances, want.numpy()) <= RTOL
