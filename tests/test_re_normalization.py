"""Normalization for random-effect coordinates (``GameEstimator.set_random_effect_normalization``), CPU tier.

Every numeric check compares against the independent oracle of ``re_norm_util`` (per entity the dense ``X' = (X -
s) f`` solved with normalization off, mapped with ``T``), in the two regimes of ``test_re_parity_gpu.py``:
iteration-limited (tolerance 0, a few iterations: identical iteration counts, W to 1e-9 relative) and converged
(tolerance 1e-8: identical iteration counts and stop reasons, W to 1e-6 relative).
"""
import numpy as np
import pytest
import torch

import re_norm_util as U

TASK = "LOGISTIC_REGRESSION"
SHAPES = [(12, 5), (30, 9), (7, 3), (20, 14), (1, 1), (3, 2), (25, 6)]
SOLVERS = {"tron_l2": ("TRON", "L2"), "lbfgs_l2": ("LBFGS", "L2"), "lbfgs_en": ("LBFGS", "ELASTIC_NET")}
REGIMES = {"limited": (0.0, 4, 1e-9), "converged": (1e-8, 200, 1e-6)}

_DATA = {}


def data_for(intercept="last", task=TASK):
    key = (intercept, task)
    if key not in _DATA:
        _DATA[key] = U.make_data(SHAPES, intercept, seed=3, task=task)
    return _DATA[key]


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("layout", ["segmented", "dense"])
@pytest.mark.parametrize("norm_type", U.NORM_TYPES)
def test_matches_dense_oracle(norm_type, layout, solver, regime):
    data, icpt = data_for()
    ctx = U.build_context(data, norm_type, icpt)
    opt, reg = SOLVERS[solver]
    tol, iters, bound = REGIMES[regime]
    cfg = U.opt_config(opt, reg, 1.5, tol, iters)
    W_ref, _, it_ref, rc_ref = U.oracle(data, ctx, icpt, cfg, TASK, layout)
    c = U.coordinate(data, cfg, TASK, layout=layout, normalization=ctx)
    assert (c.dataset.norm is not None) and c.dataset.norm.has_shift == (norm_type == "STANDARDIZATION")
    W, it, rc, _ = U.run(c)
    err = U.rel_err(W, W_ref)
    print(f"{norm_type} {layout} {solver} {regime}: rel err {err:.3e}")
    if layout == "segmented":
        assert np.array_equal(it, it_ref) and np.array_equal(rc, rc_ref)
    assert err <= bound


def test_identity_projection_dense_buckets():
    """IDENTITY projection: every entity holds all features, X' materialised in the bucket."""
    data, icpt = U.make_data([(14, 5)] * 4 + [(9, 5)] * 2, "middle", seed=5, shared=4)
    ctx = U.build_context(data, "STANDARDIZATION", icpt)
    cfg = U.opt_config("TRON", "L2", 0.7, 0.0, 4)
    # the oracle over ALL features of every entity: (X - s) f is dense under the IDENTITY projection
    x = np.asarray(data.shards["user"].todense())
    xp = (x - ctx.shifts.numpy()) * ctx.factors.numpy()
    import scipy.sparse as sp
    from photon_ml_amd.data.game_data import GameData
    td = GameData(data.response, {"user": sp.csr_matrix(xp)}, dict(data.id_tags), data.offsets, data.weights)
    Wp, _, _, _ = U.run(U.coordinate(td, cfg, TASK, layout="dense", projector="IDENTITY"))
    W, _, _, _ = U.run(U.coordinate(data, cfg, TASK, layout="dense", projector="IDENTITY", normalization=ctx))
    assert U.rel_err(W, U.to_original(Wp, ctx, icpt)) <= 1e-9


def _estimator(data, icpt, norm=None, flag=None, iterations=1, variance=None):
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration
    from photon_ml_amd.estimators.game_estimator import GameEstimator
    est = (GameEstimator(device="cpu").set_training_task(TASK)
           .set_coordinate_data_configurations({"u": RandomEffectDataConfiguration("userId", "user")})
           .set_coordinate_update_sequence(["u"]).set_coordinate_descent_iterations(iterations))
    if norm is not None:
        est.set_normalization(norm, {"user": icpt})
    if flag is not None:
        est.set_random_effect_normalization(flag)
    if variance is not None:
        est.set_variance_computation_type(variance)
    return est


def test_estimator_fit_matches_oracle_and_scores():
    data, icpt = data_for()
    cfg = U.opt_config("TRON", "L2", 1.5, 1e-8, 200)
    est = _estimator(data, icpt, "STANDARDIZATION", True)
    res = est.fit(data, None, [{"u": cfg}])
    m = res[0].model.get("u")
    ctx = U.build_context(data, "STANDARDIZATION", icpt)          # per shard, over all rows
    W_ref, _, _, _ = U.oracle(data, ctx, icpt, cfg, TASK, est.coordinates["u"].dataset.layout)
    W = U.model_dense(m, data.shards["user"].shape[1])
    assert U.rel_err(W, W_ref) <= 1e-6
    # training scores are X w of the returned (original-space) model
    xw = np.asarray(data.shards["user"] @ W.T)[np.arange(data.n_rows), data.id_tags["userId"]]
    s = est.coordinates["u"].score(m).numpy()
    assert np.abs(s - xw).max() <= 1e-9 * max(1.0, np.abs(xw).max())
    assert np.abs(m.score(data, "cpu").numpy() - xw).max() <= 1e-9 * max(1.0, np.abs(xw).max())


@pytest.mark.parametrize("layout", ["segmented", "dense"])
def test_second_iteration_warm_start(layout):
    """A second update (cached solver state) and a foreign warm start (through T^-1) both reproduce the oracle's
    solve from the same w, to the iteration-limited bound."""
    data, icpt = data_for()
    ctx = U.build_context(data, "STANDARDIZATION", icpt)
    # two iterations per update: the second update still takes real steps (an entity already converged to rounding
    # accepts or rejects its steps by rounding alone, and its iteration count means nothing)
    cfg = U.opt_config("TRON", "L2", 1.5, 0.0, 2)
    c = U.coordinate(data, cfg, TASK, layout=layout, normalization=ctx)
    W1, _, _, m1 = U.run(c)
    W2, it2, _, _ = U.run(c, start=m1)
    W_ref, _, it_ref, _ = U.oracle(data, ctx, icpt, cfg, TASK, layout, start_w=W1)
    assert U.rel_err(W2, W_ref) <= 1e-9
    fresh = U.coordinate(data, cfg, TASK, layout=layout, normalization=ctx)
    W3, it3, _, _ = U.run(fresh, start=U.dense_model(fresh, W1))
    assert U.rel_err(W3, W_ref) <= 1e-9
    if layout == "segmented":
        assert np.array_equal(it2, it_ref) and np.array_equal(it3, it_ref)


def test_flag_off_is_bitwise_unchanged():
    data, icpt = data_for()
    cfg = U.opt_config("TRON", "L2", 1.5, 1e-8, 50)
    D = data.shards["user"].shape[1]
    plain = _estimator(data, icpt).fit(data, None, [{"u": cfg}])[0].model.get("u")
    for flag in (None, False):
        off = _estimator(data, icpt, "STANDARDIZATION", flag).fit(data, None, [{"u": cfg}])[0].model.get("u")
        assert np.array_equal(U.model_dense(off, D), U.model_dense(plain, D))
    on = _estimator(data, icpt, "STANDARDIZATION", True).fit(data, None, [{"u": cfg}])[0].model.get("u")
    assert not np.array_equal(U.model_dense(on, D), U.model_dense(plain, D))


def test_explicit_context_wins_over_type():
    data, icpt = data_for()
    cfg = U.opt_config("TRON", "L2", 1.5, 0.0, 3)
    ctx = U.build_context(data, "SCALE_WITH_MAX_MAGNITUDE", icpt)
    est = _estimator(data, icpt, "STANDARDIZATION", True).set_coordinate_normalization_contexts({"u": ctx})
    m = est.fit(data, None, [{"u": cfg}])[0].model.get("u")
    W_ref, _, _, _ = U.oracle(data, ctx, icpt, cfg, TASK, est.coordinates["u"].dataset.layout)
    assert U.rel_err(U.model_dense(m, data.shards["user"].shape[1]), W_ref) <= 1e-9


@pytest.mark.parametrize("layout", ["segmented", "dense"])
@pytest.mark.parametrize("solver", ["tron_l2", "lbfgs_en"])
def test_regularization_term_value(layout, solver):
    data, icpt = data_for()
    ctx = U.build_context(data, "STANDARDIZATION", icpt)
    opt, reg = SOLVERS[solver]
    lam = 1.5
    cfg = U.opt_config(opt, reg, lam, 1e-8, 100)
    c = U.coordinate(data, cfg, TASK, layout=layout, normalization=ctx)
    W, _, _, m = U.run(c)
    Wp = U.to_transformed(W, ctx, icpt)
    l1 = cfg.regularization_context.l1_weight(lam)
    l2 = cfg.regularization_context.l2_weight(lam)
    want = 0.5 * l2 * float((Wp ** 2).sum()) + l1 * float(np.abs(Wp).sum())
    assert c.regularization_term_value(m) == pytest.approx(want, rel=1e-10)
    # a model the coordinate did not return: mapped from its coefficients
    assert c.regularization_term_value(U.dense_model(c, W)) == pytest.approx(want, rel=1e-10)


def test_scale_only_variances():
    """Scale-only types support variances: var_w = f^2 var_w' (SIMPLE)."""
    data, icpt = data_for()
    ctx = U.build_context(data, "SCALE_WITH_STANDARD_DEVIATION", icpt)
    cfg = U.opt_config("TRON", "L2", 1.5, 1e-8, 100)
    D = data.shards["user"].shape[1]
    for layout in ("segmented", "dense"):
        c = U.coordinate(data, cfg, TASK, layout=layout, normalization=ctx, compute_variance="SIMPLE")
        m = c.update_model(c.initialize_model())
        o = U.coordinate(U.transformed_data(data, ctx), cfg, TASK, layout=layout, compute_variance="SIMPLE")
        mo = o.update_model(o.initialize_model())
        k, _ = m.tensors("cpu")
        ko, _ = mo.tensors("cpu")
        assert torch.equal(k, ko)
        f2 = ctx.factors[k % D].square()
        got, ref = m.variance_tensor("cpu"), mo.variance_tensor("cpu") * f2
        assert float(((got - ref).abs() / ref.abs()).max()) <= 1e-6


# ---- what normalization of a random effect cannot be combined with: ValueError naming the coordinate, before training
def test_error_prior_model():
    data, icpt = data_for()
    cfg = U.opt_config("TRON", "L2", 1.5, 1e-8, 10)
    ctx = U.build_context(data, "SCALE_WITH_STANDARD_DEVIATION", icpt)
    prior = U.coordinate(data, cfg, TASK).initialize_model()
    with pytest.raises(ValueError, match="coordinate u.*prior model"):
        U.coordinate(data, cfg, TASK, normalization=ctx, prior=prior)


def test_error_random_projector():
    data, icpt = data_for()
    cfg = U.opt_config("TRON", "L2", 1.5, 1e-8, 10)
    ctx = U.build_context(data, "SCALE_WITH_STANDARD_DEVIATION", icpt)
    with pytest.raises(ValueError, match="coordinate u.*RANDOM"):
        U.coordinate(data, cfg, TASK, layout="dense", projector="RANDOM=4", normalization=ctx)


def test_error_process_group():
    from photon_ml_amd.algorithm.coordinates import ShardedRandomEffectCoordinate
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration
    data, icpt = data_for()
    cfg = U.opt_config("TRON", "L2", 1.5, 1e-8, 10)
    ctx = U.build_context(data, "SCALE_WITH_STANDARD_DEVIATION", icpt)
    with pytest.raises(ValueError, match="coordinate u.*process group"):
        ShardedRandomEffectCoordinate("u", data, RandomEffectDataConfiguration("userId", "user"), cfg, TASK,
                                      device="cpu", normalization=ctx)


@pytest.mark.parametrize("layout", ["segmented", "dense"])
def test_error_entity_without_intercept(layout):
    import scipy.sparse as sp
    from photon_ml_amd.data.game_data import GameData
    data, icpt = data_for()
    x = data.shards["user"].tolil()
    ids = data.id_tags["userId"]
    for e in (1, 3):                                   # two entities lose their intercept
        for r in np.nonzero(ids == e)[0]:
            x[r, icpt] = 0.0
    x = sp.csr_matrix(x)
    x.eliminate_zeros()
    bad = GameData(data.response, {"user": x}, dict(data.id_tags), data.offsets, data.weights)
    cfg = U.opt_config("TRON", "L2", 1.5, 1e-8, 10)
    ctx = U.build_context(data, "STANDARDIZATION", icpt)
    with pytest.raises(ValueError, match=r"coordinate u.*intercept.* 2 of 7 trained entities"):
        U.coordinate(bad, cfg, TASK, layout=layout, normalization=ctx)
    # scale-only needs no intercept
    U.coordinate(bad, cfg, TASK, layout=layout, normalization=U.build_context(data, "SCALE_WITH_STANDARD_DEVIATION",
                                                                             icpt))


@pytest.mark.parametrize("variance", ["SIMPLE", "FULL"])
def test_error_standardization_with_variances(variance):
    data, icpt = data_for()
    cfg = U.opt_config("TRON", "L2", 1.5, 1e-8, 10)
    ctx = U.build_context(data, "STANDARDIZATION", icpt)
    with pytest.raises(ValueError, match="coordinate u.*variances"):
        U.coordinate(data, cfg, TASK, normalization=ctx, compute_variance=variance)
    with pytest.raises(ValueError, match="coordinate u.*variances"):
        _estimator(data, icpt, "STANDARDIZATION", True, variance=variance).fit(data, None, [{"u": cfg}])


# ---- PML_CHECK_KERNEL_INPUTS: the shifted fused kernel's host-side input check (nothing is launched)
def _shift_inputs():
    order = torch.tensor([1, 0], dtype=torch.int32)
    col_ptr = torch.tensor([0, 3, 5], dtype=torch.int64)
    c = torch.tensor([0.5, 0.0, -1.0, 0.0, 2.0], dtype=torch.float64)
    i0 = torch.tensor([1, 0], dtype=torch.int32)
    return order, col_ptr, c, i0


def test_shift_input_check_accepts_valid():
    from photon_ml_amd.ops.native import check_re_shift_inputs
    check_re_shift_inputs(*_shift_inputs())


@pytest.mark.parametrize("bad_i0", [-1, 2, 7])
def test_shift_input_check_rejects_i0_out_of_range(bad_i0, monkeypatch):
    from photon_ml_amd.ops.native import check_re_shift_inputs, re_tron_csr
    order, col_ptr, c, i0 = _shift_inputs()
    i0[1] = bad_i0                                     # entity 1 has 2 coefficients
    with pytest.raises(ValueError, match="intercept column"):
        check_re_shift_inputs(order, col_ptr, c, i0)
    # through the launcher: rejected on the host before anything else is touched
    monkeypatch.setenv("PML_CHECK_KERNEL_INPUTS", "1")
    z = torch.zeros(0)
    with pytest.raises(ValueError, match="intercept column"):
        re_tron_csr(order, z, col_ptr, z, z, z, z, z, z, z, z, z, z, z, z, 0, 1.0, 1e-6, 5, 5, 20, 256,
                    shift=(c, i0))


def test_shift_input_check_rejects_shifted_intercept_and_nonfinite():
    from photon_ml_amd.ops.native import check_re_shift_inputs
    order, col_ptr, c, i0 = _shift_inputs()
    c2 = c.clone()
    c2[1] = 0.25                                       # c[i0] of entity 0
    with pytest.raises(ValueError, match="must be 0"):
        check_re_shift_inputs(order, col_ptr, c2, i0)
    c3 = c.clone()
    c3[4] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        check_re_shift_inputs(order, col_ptr, c3, i0)
    # an entity that is not launched is not checked
    check_re_shift_inputs(torch.tensor([1], dtype=torch.int32), col_ptr, c2, i0)
