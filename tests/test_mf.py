"""Matrix-factorization coordinate on the CPU (the definition): half-updates against the per-entity float64 TRON,
monotone objective, determinism, GAME integration, model I/O, checkpoint / resume and the refused configurations."""
import logging
from collections import OrderedDict

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from mf_util import LOSSES, TASKS, half_case, half_mismatches, make_mf_data, mf_coordinate, objective, \
    start_factors, with_config
from photon_ml_amd.data.game_data import GameData
from photon_ml_amd.data.random_effect import FixedEffectDataConfiguration, MatrixFactorizationDataConfiguration
from photon_ml_amd.estimators.game_estimator import GameEstimator, GameTransformer
from photon_ml_amd.models.game import GameModel, MatrixFactorizationModel
from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig, RegularizationContext)

SIZES = [1, 2, 3, 5, 9, 16, 17, 33, 40, 7]


@pytest.mark.parametrize("loss", LOSSES)
def test_half_updates_match_per_entity_tron(loss):
    """Every entity's factors after a row half and after a column half equal the per-entity ``TRON`` over the
    materialised features from the same start, offsets and weights: identical iteration counts and reasons, W and the
    margins equal to rounding (1e-9 iteration-limited, 1e-6 converged; ``mf_util.REGIMES``). Rows at weight 0, a
    non-zero partial score, ids that arrive unsorted."""
    data, partial, ref = half_case(5, loss, seed=1)
    assert (data.weights == 0).any() and not np.all(np.sort(data.id_tags["userId"]) == data.id_tags["userId"])
    assert half_mismatches(mf_coordinate(data, loss, 5, "cpu"), partial, ref) == []


@pytest.mark.parametrize("loss", LOSSES)
def test_objective_never_increases(loss):
    """loss + regularization term after each half of 6 alternations is non-increasing (1e-12 relative slack); the
    tolerance is tight enough that every solve converges."""
    from photon_ml_amd.optimization.batched import REASON_CODES
    data = make_mf_data(SIZES, 9, 3, seed=8, loss=loss)
    c = mf_coordinate(data, loss, 4, "cpu", l2=0.5, tol=1e-10, max_iter=200)
    m = c.initialize_model()
    U, V = m.U, m.V
    f = objective(c, U, V, loss, 0.5)
    for alt in range(6):
        for s in (0, 1):
            W, _, it, rs = c.solve_half(s, U, V)
            assert all(REASON_CODES[int(r)] is not None and int(r) != 1 for r in rs), (alt, s, rs)
            U, V = (W, V) if s == 0 else (U, W)
            f_new = objective(c, U, V, loss, 0.5)
            assert f_new <= f + 1e-12 * abs(f), (loss, alt, s, f_new, f)
            f = f_new
    assert f < objective(c, m.U, m.V, loss, 0.5)


def test_update_is_deterministic_and_seeded():
    data = make_mf_data(SIZES, 9, 3, seed=2, loss="LOGISTIC")
    fit = lambda seed: mf_coordinate(data, "LOGISTIC", 4, "cpu", seed=seed, alternations=2)
    c = fit(7)
    m1 = c.update_model(c.initialize_model(), None)
    c2 = fit(7)
    m2 = c2.update_model(c2.initialize_model(), None)
    assert torch.equal(m1.U, m2.U) and torch.equal(m1.V, m2.V)
    assert torch.equal(c.score(m1), c2.score(m2))
    c3 = fit(8)
    m3 = c3.update_model(c3.initialize_model(), None)
    assert not torch.equal(m1.V, m3.V)
    # the start: U = 0, V ~ N(0, init_std^2) from default_rng(seed) over the sorted column ids
    m0 = c.initialize_model()
    assert not m0.U.any()
    assert np.array_equal(m0.V.numpy(), np.random.default_rng(7).normal(0.0, 0.1, size=(len(c.col_ids), 4)))
    assert list(c.col_ids) == sorted(c.col_ids)
    # another lambda and back: the layout is not rebuilt, the first result comes back from the same start
    sides = c.sides
    with_config(c, 5.0, 1e-8, 60)
    m5 = c.update_model(c.initialize_model(), None)
    assert not torch.equal(m5.U, m1.U)
    assert c.regularization_term_value(m5) == pytest.approx(2.5 * float(m5.U.square().sum() + m5.V.square().sum()))
    with_config(c, 1.0, 1e-8, 60)
    m1b = c.update_model(c.initialize_model(), None)
    assert c.sides is sides and torch.equal(m1b.U, m1.U) and torch.equal(m1b.V, m1.V)


def test_foreign_model_is_mapped_by_entity_id():
    data = make_mf_data(SIZES, 9, 3, seed=2, loss="SQUARED")
    c = mf_coordinate(data, "SQUARED", 3, "cpu", seed=4)
    U, V = start_factors(c, 1)
    keep_r, keep_c = np.arange(len(c.row_ids))[::2], np.arange(len(c.col_ids))[1:]
    foreign = MatrixFactorizationModel("userId", "itemId", TASKS["SQUARED"], c.row_ids[keep_r].copy(),
                                       c.col_ids[keep_c].copy(), U[keep_r], V[keep_c])
    U0, V0 = c._factors_of(foreign)
    exp_u = torch.zeros_like(U)
    exp_u[keep_r] = U[keep_r]
    exp_v = c.initialize_model().V.clone()
    exp_v[keep_c] = V[keep_c]
    assert torch.equal(U0, exp_u) and torch.equal(V0, exp_v)
    # scoring a foreign model: rows of an entity it does not hold score 0
    s = c.score(foreign)
    a, b = c.codes[0].long(), c.codes[1].long()
    seen = torch.from_numpy(np.isin(a.numpy(), keep_r) & np.isin(b.numpy(), keep_c))
    assert torch.equal(s[~seen], torch.zeros(int((~seen).sum()), dtype=torch.float64)) and bool(seen.any())
    assert torch.allclose(s[seen], (U[a] * V[b]).sum(1)[seen], rtol=0, atol=1e-15)


def _planted(n=3000, users=40, items=30, seed=0):
    rng = np.random.default_rng(seed)
    u, it = rng.integers(0, users, n), rng.integers(0, items, n)
    x = np.hstack([rng.normal(size=(n, 3)), np.ones((n, 1))])
    Ut, Vt = rng.normal(size=(users, 2)), rng.normal(size=(items, 2))
    y = x @ np.array([0.5, -1.0, 0.3, 0.2]) + (Ut[u] * Vt[it]).sum(1) + 0.05 * rng.normal(size=n)
    ids = {"userId": np.array([f"u{k}" for k in u], dtype=object), "itemId": np.array([f"i{k}" for k in it], dtype=object)}
    return GameData(y, {"global": sp.csr_matrix(x)}, ids)


def _cfg(opt="TRON", reg="L2", lam=0.1, max_iter=30, tol=1e-8, **kw):
    return GLMOptimizationConfiguration(OptimizerConfig(opt, max_iter, tol, **kw.pop("oc", {})),
                                        RegularizationContext(reg), lam, **kw)


def _estimator(cfgs, iterations=2):
    return (GameEstimator(device="cpu").set_training_task("LINEAR_REGRESSION")
            .set_coordinate_data_configurations(cfgs).set_coordinate_descent_iterations(iterations))


MF_DC = MatrixFactorizationDataConfiguration("userId", "itemId", 2, alternations=2, seed=7)


@pytest.fixture(scope="module")
def planted_fit():
    data = _planted()
    est = _estimator(OrderedDict(fixed=FixedEffectDataConfiguration("global"), mf=MF_DC))
    res = est.fit(data, None, [{"fixed": _cfg("LBFGS", lam=0.01), "mf": _cfg()}])[0]
    return data, est, res


def test_game_with_planted_interaction_beats_fixed_effect_alone(planted_fit):
    data, est, res = planted_fit
    alone = _estimator(OrderedDict(fixed=FixedEffectDataConfiguration("global")))
    alone.fit(data, None, [{"fixed": _cfg("LBFGS", lam=0.01)}])
    assert isinstance(res.model.get("mf"), MatrixFactorizationModel)
    assert est.history[0][-1]["training_loss"] < 0.5 * alone.history[0][-1]["training_loss"]
    # the objective over the coordinate updates never increases
    obj = [r["objective"] for r in est.history[0]]
    assert all(b <= a + 1e-9 * abs(a) for a, b in zip(obj, obj[1:])), obj


def test_save_load_transform(planted_fit, tmp_path):
    from photon_ml_amd.io.index_map import DefaultIndexMap
    from photon_ml_amd.io.model_io import load_game_model, save_game_model
    data, est, res = planted_fit
    maps = {"global": DefaultIndexMap.from_keys([f"f{j}\u0001t" for j in range(4)])}
    save_game_model(res.model, str(tmp_path / "m"), maps, "LINEAR_REGRESSION")
    d = tmp_path / "m" / "matrix-factorization" / "mf"
    assert (d / "id-info").read_text().split("\n")[:3] == ["userId", "itemId", "2"]
    assert (d / "row-latent-factors" / "part-00000.avro").exists()
    assert (d / "col-latent-factors" / "part-00000.avro").exists()
    back = load_game_model(str(tmp_path / "m"), maps)
    m, b = res.model.get("mf"), back.get("mf")
    assert list(b.row_ids) == list(m.row_ids) and list(b.col_ids) == list(m.col_ids)
    assert torch.equal(b.U, m.U.cpu()) and torch.equal(b.V, m.V.cpu())          # Avro doubles are exact
    # a scoring set with an unseen user and an unseen item
    n = 50
    ids = {"userId": data.id_tags["userId"][:n].copy(), "itemId": data.id_tags["itemId"][:n].copy()}
    ids["userId"][3] = "nobody"
    ids["itemId"][5] = "nothing"
    sdata = GameData(data.response[:n], {"global": data.shards["global"][:n]}, ids)
    scores, _ = GameTransformer(back, device="cpu").transform(sdata)
    assert torch.allclose(scores, res.model.score(sdata, "cpu"), rtol=0, atol=1e-12)
    mf_scores = b.score(sdata, "cpu")
    assert mf_scores[3] == 0 and mf_scores[5] == 0 and int((mf_scores != 0).sum()) == n - 2
    assert torch.equal(mf_scores, m.score(sdata, "cpu"))


def test_checkpoint_resume_reproduces_uninterrupted_run(planted_fit, tmp_path):
    """Coordinate descent interrupted after the first sweep and resumed ends at the uninterrupted run's model."""
    data, est, res = planted_fit
    cfgs = OrderedDict(fixed=FixedEffectDataConfiguration("global"), mf=MF_DC)
    conf = [{"fixed": _cfg("LBFGS", lam=0.01), "mf": _cfg()}]
    first = _estimator(cfgs, iterations=1).set_checkpoint_directory(str(tmp_path / "ck"))
    first.fit(data, None, conf)
    # the state on disk says "iteration 1, coordinate 0 next": a run of two sweeps resumes there
    second = _estimator(cfgs, iterations=2).set_checkpoint_directory(str(tmp_path / "ck"), resume=True)
    out = second.fit(data, None, conf)[0]
    assert [r["iteration"] for r in second.history[0]] == [0, 0, 1, 1]
    a, b = res.model.get("mf"), out.model.get("mf")
    assert torch.equal(a.U, b.U) and torch.equal(a.V, b.V)
    assert torch.equal(res.model.get("fixed").glm.coefficients.means.cpu(),
                       out.model.get("fixed").glm.coefficients.means.cpu())


def test_refused_configurations_name_the_coordinate():
    data = _planted(200, 8, 6)
    fe = FixedEffectDataConfiguration("global")

    def fit(dc=MF_DC, cfg=None, task="LINEAR_REGRESSION", prior=None):
        est = (GameEstimator(device="cpu").set_training_task(task)
               .set_coordinate_data_configurations(OrderedDict(fixed=fe, inter=dc)))
        if prior is not None:
            est.set_prior_model(prior)
        touched = []
        est.event_callback = touched.append
        with pytest.raises(ValueError, match="inter"):
            est.fit(data, None, [{"fixed": _cfg("LBFGS"), "inter": cfg or _cfg()}])
        assert not touched                     # before any training

    for k in (0, 33):
        fit(MatrixFactorizationDataConfiguration("userId", "itemId", k))
    fit(cfg=_cfg("LBFGS"))
    fit(cfg=_cfg(reg="L1"))
    fit(cfg=GLMOptimizationConfiguration(OptimizerConfig("TRON", 10, 1e-6), RegularizationContext("ELASTIC_NET", 0.5),
                                         1.0))
    fit(task="SMOOTHED_HINGE_LOSS_LINEAR_SVM")
    fit(cfg=GLMOptimizationConfiguration(OptimizerConfig("TRON", 10, 1e-6, {0: (-1.0, 1.0)}),
                                         RegularizationContext("L2"), 1.0))
    fit(cfg=GLMOptimizationConfiguration(OptimizerConfig("TRON", 10, 1e-6), RegularizationContext("L2"), 1.0, 0.5))
    fit(MatrixFactorizationDataConfiguration("userId", "songId", 2))
    c = mf_coordinate(make_mf_data([3, 4], 3, 2, 1, "SQUARED"), "SQUARED", 2, "cpu")
    m = c.initialize_model()
    fit(prior=GameModel(OrderedDict(inter=m)))


def test_process_group_is_refused(monkeypatch):
    import photon_ml_amd.algorithm.matrix_factorization as mfm
    monkeypatch.setattr(mfm, "is_dist", lambda: True)
    with pytest.raises(ValueError, match="mf.*process group"):
        mf_coordinate(make_mf_data([3, 4], 3, 2, 1, "SQUARED"), "SQUARED", 2, "cpu")


def test_normalization_and_variance_settings_are_logged_and_ignored():
    data = _planted(200, 8, 6)
    est = _estimator(OrderedDict(mf=MF_DC), 1).set_variance_computation_type("SIMPLE")
    seen = []

    class Collect(logging.Handler):
        def emit(self, record):
            seen.append(record.getMessage())
    lg, handler = logging.getLogger("photon_ml_amd.estimators.game_estimator"), Collect()
    level = lg.level
    lg.addHandler(handler)
    lg.setLevel(logging.INFO)
    try:
        res = est.fit(data, None, [{"mf": _cfg()}])[0]
    finally:
        lg.removeHandler(handler)
        lg.setLevel(level)
    assert sum("do not apply to matrix factorization" in m for m in seen) == 1
    assert isinstance(res.model.get("mf"), MatrixFactorizationModel)


def test_half_statistics_per_half():
    data = make_mf_data(SIZES, 9, 3, seed=2, loss="LOGISTIC")
    c = mf_coordinate(data, "LOGISTIC", 3, "cpu", alternations=2)
    c.update_model(c.initialize_model(), None)
    st = c.half_stats
    assert [s["entities"] for s in st] == [len(SIZES), 9, len(SIZES), 9]
    assert c.last_stats == st[-1] and st[0]["convergence_reasons"]
