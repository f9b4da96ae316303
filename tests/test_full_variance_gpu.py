"""FULL coefficient variances on the GPU: ``var_normal_kernel`` / ``var_scale_gram_kernel`` / ``chol_colnorm_kernel``
(through ``optimization.variance.SegmentedFullVariance`` and ``dense_full_variance_device``) against the CPU fp64
definition.

Tolerance: 1e-9 relative, the project's tolerance for random-effect kernel parity (tests/test_re_parity_gpu.py). Every
generated entity has cond(H_e) <= 1e6 (asserted on the CPU by ``BlockProblem.numpy_variances``), so the yardstick's own
error (~cond * 2^-53 ~ 1e-10) stays inside it. Inputs: at most 51 entries per row, lambda in {0.1, 1}, values N(0, 1).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from full_variance_util import BlockProblem, relative_error
from photon_ml_amd.constants import EPSILON

pytestmark = pytest.mark.gpu

RTOL = 1e-9
COND_MAX = 1e6


def _plan(p: BlockProblem):
    from photon_ml_amd.optimization.variance import SegmentedFullVariance
    rp, cp, csr, c = p.tensors("cuda")
    return SegmentedFullVariance(rp, cp, csr), c


def _check(p: BlockProblem, lam: float):
    want = p.numpy_variances(lam, cond_max=COND_MAX)
    plan, c = _plan(p)
    got, stats = plan.compute(c, lam)
    torch.cuda.synchronize()
    err = relative_error(got.cpu().numpy(), want)
    print(f"shapes {p.shapes} lambda {lam}: max relative error {err:.3e}, routes {stats}")
    assert err <= RTOL
    return stats


@pytest.mark.parametrize("d", [1, 2, 16, 17, 63, 64, 65, 127, 128])
def test_primal_route(d):
    """d_e <= n_e: n_e = d_e and n_e ~ 3 d_e."""
    p = BlockProblem([(d, d), (3 * d, d), (3 * d + 1, d)], seed=100 + d)
    stats = _check(p, 0.1 if d % 2 else 1.0)
    assert stats["primal"] == 3 and stats["row_space"] == 0 and stats["torch"] == 0


@pytest.mark.parametrize("n,d", [(1, 5), (2, 3), (16, 64), (17, 65), (63, 129), (64, 300), (128, 129), (128, 700)])
def test_row_space_route(n, d):
    p = BlockProblem([(n, d), (n, d)], seed=200 + n)
    stats = _check(p, 0.1 if n % 2 else 1.0)
    assert stats["row_space"] == 2 and stats["primal"] == 0 and stats["torch"] == 0


def test_row_space_duplicated_rows_and_zero_weights():
    """K_e singular (every row a copy of the first two) while A = lam I + B B^T is not; a third of the rows at
    weight 0 (c_i = 0: the Woodbury form holds no 1 / c_i)."""
    p = BlockProblem([(12, 40), (20, 90)], seed=7, duplicate_rows=(0, 1))
    assert np.linalg.matrix_rank(p.entity_dense(0) @ p.entity_dense(0).T) == 2
    assert _check(p, 0.1)["row_space"] == 2
    q = BlockProblem([(30, 100), (9, 31), (48, 49)], seed=8, zero_weight_fraction=0.34)
    assert (q.c == 0).sum() >= 10 + 3 + 16
    stats = _check(q, 1.0)
    assert stats["row_space"] == 3 and stats["failed_factors"] == 0


def test_other_paths():
    """The dispatch boundary n_e = d_e (primal), m = 129 (torch fallback), an entity without rows (1 / lambda), all
    in one coordinate with both HIP routes."""
    shapes = [(40, 40), (129, 129), (0, 7), (129, 200), (10, 30), (200, 129), (50, 20)]
    p = BlockProblem(shapes, seed=11)
    lam = 0.1
    stats = _check(p, lam)
    assert stats == {"primal": 2, "row_space": 1, "torch": 3, "empty": 1, "failed_factors": 0}
    # nearly square row-space entities (more than 96 rows, at most 128 coefficients) were measured slower on the HIP
    # path than in the torch fallback and are routed there; one row fewer, or a wider entity, stays on the HIP path
    stats = _check(BlockProblem([(100, 120), (96, 120), (100, 129)], seed=12), lam)
    assert stats == {"primal": 0, "row_space": 2, "torch": 1, "empty": 0, "failed_factors": 0}
    plan, c = _plan(p)
    got = plan.compute(c, lam)[0].cpu().numpy()
    assert np.array_equal(got[p.col_ptr[2]:p.col_ptr[3]], np.full(7, 1.0 / lam))


@pytest.mark.parametrize("d", [8, 64, 128, 160])
def test_dense_bucket(d):
    """A dense bucket (RANDOM / IDENTITY projections): torch.bmm normal matrix, HIP factor and column norms up to the
    cap, the torch definition beyond it (d = 160)."""
    from photon_ml_amd.optimization.variance import dense_full_variance_device
    rng = np.random.default_rng(d)
    B, n, lam = 5, d + 9, 0.1
    X = rng.standard_normal((B, n, d)) * (rng.random((B, n, d)) < min(1.0, 51.0 / d))
    X[1, d // 2:] = 0.0                  # a wide problem: fewer rows than coefficients
    c = rng.uniform(0.05, 0.25, size=(B, n)) * rng.choice([0.0, 0.5, 1.0, 2.0], size=(B, n))
    want = np.empty((B, d))
    for b in range(B):
        H = X[b].T @ (c[b][:, None] * X[b]) + lam * np.eye(d)
        assert np.linalg.cond(H) <= COND_MAX
        want[b] = np.diag(np.linalg.inv(H))
    got, n_torch = dense_full_variance_device(torch.from_numpy(X).cuda(), torch.from_numpy(c).cuda(), lam)
    err = relative_error(got.cpu().numpy(), want)
    print(f"dense bucket d={d}: max relative error {err:.3e}, torch path {n_torch}")
    assert err <= RTOL
    assert n_torch == (B if d > 128 else 0)


def test_deterministic():
    """The same call twice in one process: bitwise equal (no atomics, fixed summation order)."""
    p = BlockProblem([(64, 300), (100, 30), (128, 128), (17, 65), (5, 5), (33, 90)], seed=13)
    plan, c = _plan(p)
    a = plan.compute(c, 0.1)[0].clone()
    b = plan.compute(c, 0.1)[0]
    assert torch.equal(a, b)
    plan2, _ = _plan(p)
    assert torch.equal(a, plan2.compute(c, 0.1)[0])


def test_validation_raises_before_any_launch():
    """An out-of-range ``ents`` value and a class above the cap raise on the host; nothing is launched (the output
    vector keeps its fill value)."""
    from photon_ml_amd.ops import native
    p = BlockProblem([(20, 20), (6, 25)], seed=3)
    rp, cp, csr, c = p.tensors("cuda")
    out = torch.full((int(cp[-1]),), -1.0, dtype=torch.float64, device="cuda")
    L = torch.eye(20, dtype=torch.float64, device="cuda").repeat(1, 1, 1).contiguous()
    nv = torch.tensor([20], device="cuda")
    for bad in ([2], [-1], [1 << 40]):
        ents = torch.tensor(bad, device="cuda")
        with pytest.raises(ValueError, match="entity index"):
            native.chol_colnorm(native.VAR_PRIMAL, L, nv, ents, rp, cp, out)
        with pytest.raises(ValueError, match="entity index"):
            native.var_normal(ents, 20, rp, cp, csr, c, 0.1)
        with pytest.raises(ValueError, match="entity index"):
            native.var_scale_gram(L.clone(), ents, rp, c, 0.1)
    big = native.VAR_MMAX + 1
    Lb = torch.eye(big, dtype=torch.float64, device="cuda").unsqueeze(0).contiguous()
    e0 = torch.tensor([0], device="cuda")
    with pytest.raises(ValueError, match="class order"):
        native.chol_colnorm(native.VAR_PRIMAL, Lb, nv, e0, rp, cp, out)
    with pytest.raises(ValueError, match="class order"):
        native.var_normal(e0, big, rp, cp, csr, c, 0.1)
    # an entity wider than its primal class, a factor order above the class, a short output vector
    with pytest.raises(ValueError, match="coefficients"):
        native.var_normal(e0, 16, rp, cp, csr, c, 0.1)
    with pytest.raises(ValueError, match="factor orders"):
        native.chol_colnorm(native.VAR_PRIMAL, L, torch.tensor([21], device="cuda"), e0, rp, cp, out)
    with pytest.raises(ValueError, match="variance vector"):
        native.chol_colnorm(native.VAR_PRIMAL, L, nv, e0, rp, cp, out[:10].contiguous())
    with pytest.raises(ValueError, match="row-space route needs"):
        native.chol_colnorm(native.VAR_ROW_SPACE, L, nv, e0, rp, cp, out, 0.0, csr, c)
    assert native.chol_colnorm_lds_bytes(native.VAR_ROW_SPACE, native.VAR_MMAX) <= native.VAR_LDS_MAX
    assert native.chol_colnorm_lds_bytes(native.VAR_ROW_SPACE, native.VAR_MMAX) == \
        native.require_game_lib().pml_chol_colnorm_lds(1, native.VAR_MMAX)
    assert native.require_game_lib().pml_var_mmax() == native.VAR_MMAX
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())


def test_estimator_on_device_end_to_end(monkeypatch):
    """GameEstimator on the device with FULL over a GAME problem whose random effect runs the row-space, fused and
    pass-path solver components together; variances against the CPU definition at the device run's own coefficients.
    Then ``compute_variance=True``: bitwise today's SIMPLE values 1 / (hdiag + EPSILON)."""
    import photon_ml_amd.optimization.entity_tron as et
    from photon_ml_amd.data.game_data import generate_game_data
    from photon_ml_amd.data.random_effect import FixedEffectDataConfiguration, RandomEffectDataConfiguration
    from photon_ml_amd.estimators.game_estimator import GameEstimator
    from photon_ml_amd.function.losses import loss_for_task
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    from photon_ml_amd.optimization.variance import segmented_full_variance
    task, lam = "LOGISTIC_REGRESSION", 1.0
    monkeypatch.setenv("PML_RE_FUSED", "1")
    monkeypatch.setattr(et, "FUSED_MAX_ROWS", 200)
    data, _ = generate_game_data(n_rows=6000, n_users=150, d_user=12, seed=26, task=task)
    cfg = GLMOptimizationConfiguration(OptimizerConfig("TRON", 30, 1e-10), RegularizationContext("L2"), lam)
    loss = loss_for_task(task)

    def fit(setter):
        est = (GameEstimator(device="cuda").set_training_task(task)
               .set_coordinate_data_configurations({"global": FixedEffectDataConfiguration("global"),
                                                    "per-user": RandomEffectDataConfiguration("userId", "user")})
               .set_coordinate_update_sequence(["global", "per-user"]))
        setter(est)
        return est, est.fit(data, None, [{"global": cfg, "per-user": cfg}])[0]

    est, res = fit(lambda e: e.set_variance_computation_type("FULL"))
    co = est.coordinates["per-user"]
    routing = co.solver_routing()
    assert routing["row_space"] > 0 and routing["fused"] > 0 and routing["pass_path"] > 0, routing
    routes = co.last_variance_routes
    assert routes["primal"] > 0 and routes["row_space"] > 0 and routes["failed_factors"] == 0, routes
    re = res.model.get("per-user")
    seg = co.dataset.seg
    nip, pos, val = (t.cpu() for t in co.dataset._seg_csr)
    W = torch.from_numpy(re.values)
    X = sp.csr_matrix((val.numpy(), pos.numpy(), nip.numpy()), shape=(seg.y.numel(), W.numel()))
    z = torch.from_numpy(X @ W.numpy()) + seg.o.cpu()
    c = seg.w.cpu() * loss.dzz(z, seg.y.cpu())
    want, _ = segmented_full_variance(seg.row_ptr.cpu(), seg.col_ptr.cpu(), (nip, pos, val), c, lam)
    err = relative_error(re.variances, want.numpy())
    print(f"device estimator, random effect: max relative error {err:.3e}, routes {routes}")
    assert err <= RTOL
    # fixed effect (trained first, against zero random-effect scores)
    fe = res.model.get("global").glm.coefficients
    Xg = np.asarray(data.shards["global"].todense())
    w = fe.means.cpu().numpy()
    dzz = loss.dzz(torch.from_numpy(Xg @ w + data.offsets), torch.from_numpy(data.response)).numpy()
    H = Xg.T @ ((data.weights * dzz)[:, None] * Xg) + lam * np.eye(Xg.shape[1])
    err = relative_error(fe.variances.cpu().numpy(), np.diag(np.linalg.inv(H)))
    print(f"device estimator, fixed effect: max relative error {err:.3e}")
    assert err <= RTOL
    # the unchanged path
    est_s, res_s = fit(lambda e: e.set_compute_variance(True))
    co_s = est_s.coordinates["per-user"]
    re_s = res_s.model.get("per-user")
    assert np.array_equal(re_s.values, re.values)
    Ws = torch.from_numpy(re_s.values).cuda()
    today = 1.0 / (co_s.dataset.seg.hdiag(loss, Ws, lam) + EPSILON)
    assert np.array_equal(re_s.variances, today.cpu().numpy())
    assert (re.variances >= re_s.variances).all() and not np.allclose(re.variances, re_s.variances, rtol=1e-3)
