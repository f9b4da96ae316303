"""Incremental training on the CPU: a saved model's means and variances as a Gaussian prior.

Each coordinate's L2 term ``lambda/2 sum w_j^2`` becomes ``lambda/2 sum_j (w_j - mu_j)^2 / sigma_j^2`` (``mu = 0,
sigma^2 = 1`` where the prior model has no coefficient). The implementation folds the prior into the data once
(``w = mu + sigma v``: column-scaled data, shifted offsets, plain L2 on ``v``); these tests check the DEFINITION on the
unscaled data: the closed form of squared loss, the gradient of the explicit-prior objective, the derived quantities
(regularization term, SIMPLE / FULL variances, scores), and the wiring (estimator, errors, CLI, process group).

Closed-form tolerance (profiles/incremental_training.md): on the same data with no prior, the fits below are within
``RIDGE_ERR`` of plain ridge regression (measured on the commit before this feature); with a prior the bound is 10 x
that, because ``sigma in [0.5, 2]`` moves the conditioning of the folded problem by up to 16 x.
"""
import os
import socket
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from photon_ml_amd.algorithm.coordinates import FixedEffectCoordinate, RandomEffectCoordinate
from photon_ml_amd.constants import EPSILON
from photon_ml_amd.data.game_data import GameData, generate_game_data
from photon_ml_amd.data.random_effect import FixedEffectDataConfiguration, RandomEffectDataConfiguration
from photon_ml_amd.estimators.game_estimator import GameEstimator
from photon_ml_amd.models.game import FixedEffectModel, GameModel, RandomEffectModel
from photon_ml_amd.models.glm import Coefficients, model_for_task
from photon_ml_amd.optimization.config import GLMOptimizationConfiguration, OptimizerConfig, RegularizationContext

HERE = os.path.dirname(os.path.abspath(__file__))
LAM = 2.0
TOL = 1e-9
# max |w - ridge| of the no-prior fits of this file's data on the commit before the feature (TRON, tolerance TOL; one
# update stops on "function values converged", which pins w to ~sqrt(TOL)): fixed effect 3.744e-6, random effect
# 1.061e-6 (both layouts), rounded up; see profiles/incremental_training.md
RIDGE_ERR = {"fixed": 3.8e-6, "random": 1.1e-6}
E, D, DG = 6, 7, 9


def cfg(opt="TRON", reg="L2", lam=LAM, tol=TOL, iters=200, constraints=None):
    return GLMOptimizationConfiguration(OptimizerConfig(opt, iters, tol, constraints), RegularizationContext(reg), lam)


def make_data():
    """420 rows, 6 entities. Random-effect shard: 7 features; entity 0 never has feature 4 (its prior for it meets no
    data), feature 5 has no prior anywhere, entity 5 has no prior at all."""
    rng = np.random.default_rng(5)
    n = 420
    ids = rng.integers(0, E, n)
    xu = rng.normal(size=(n, D)) * (rng.random((n, D)) < 0.7)
    xu[:, D - 1] = 1.0
    xu[ids == 0, 4] = 0.0
    xg = rng.normal(size=(n, DG)) * (rng.random((n, DG)) < 0.6)
    xg[:, DG - 1] = 1.0
    wu, wg = rng.normal(size=(E, D)), rng.normal(size=DG)
    y = xg @ wg + np.einsum("ij,ij->i", xu, wu[ids]) + 0.1 * rng.normal(size=n)
    off = 0.3 * np.sin(np.arange(n))
    wts = rng.uniform(0.5, 2.0, n)
    return GameData(y, {"g": sp.csr_matrix(xg), "u": sp.csr_matrix(xu)}, {"uid": ids}, off, wts)


def make_priors():
    """(fixed-effect prior model, random-effect prior model, dense mu / sigma^2 tables [E, D] of the latter)."""
    rng = np.random.default_rng(9)
    fe = FixedEffectModel(model_for_task("LINEAR_REGRESSION", Coefficients(
        torch.from_numpy(rng.normal(size=DG)), torch.from_numpy(rng.uniform(0.25, 4.0, DG)))), "g")
    mu, s2 = np.zeros((E, D)), np.ones((E, D))
    keys, vals, var = [], [], []
    for e in range(E - 1):                       # entity 5: no prior
        for f in (0, 1, 2, 3, 4, 6):             # feature 5: no prior
            mu[e, f], s2[e, f] = rng.normal(), rng.uniform(0.25, 4.0)
            keys.append(e * D + f), vals.append(mu[e, f]), var.append(s2[e, f])
    re = RandomEffectModel("uid", "u", "LINEAR_REGRESSION", np.arange(E - 1), D, np.array(keys), np.array(vals),
                           np.array(var))
    return fe, re, mu, s2


def make_logistic(data):
    y = (data.response > np.median(data.response)).astype(float)
    return GameData(y, data.shards, data.id_tags, data.offsets, data.weights)


@pytest.fixture(scope="module")
def data():
    return make_data()


@pytest.fixture(scope="module")
def priors():
    return make_priors()


@pytest.fixture(scope="module")
def logistic(data):
    return make_logistic(data)


def identity_prior(model):
    if isinstance(model, FixedEffectModel):
        d = model.glm.coefficients.dim
        return FixedEffectModel(model_for_task(model.task, Coefficients(
            torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64))), model.feature_shard_id)
    k = model.keys
    return RandomEffectModel(model.random_effect_type, model.feature_shard_id, model.task, model.entity_ids, model.dim,
                             k, np.zeros(len(k)), np.ones(len(k)))


def fe_coord(data, prior=None, variance="NONE", c=None, task="LINEAR_REGRESSION", **kw):
    return FixedEffectCoordinate("fixed", data, FixedEffectDataConfiguration("g"), c or cfg(), task,
                                 compute_variance=variance, device="cpu", prior=prior, **kw)


def re_coord(data, layout, prior=None, variance="NONE", c=None, task="LINEAR_REGRESSION", dc=None):
    return RandomEffectCoordinate("per-user", data, dc or RandomEffectDataConfiguration("uid", "u"), c or cfg(), task,
                                  compute_variance=variance, device="cpu", layout=layout, prior=prior)


def entity_problem(data, e, mu=None, s2=None):
    """Entity ``e``: (rows, present features, X over them, prior mu, prior sigma^2)."""
    ids = data.id_tags["uid"]
    r = np.nonzero(ids == e)[0]
    xe = data.shards["u"][r].toarray()
    feats = np.nonzero((xe != 0).any(axis=0))[0]
    m = np.zeros(len(feats)) if mu is None else mu[e, feats]
    s = np.ones(len(feats)) if s2 is None else s2[e, feats]
    return r, feats, xe[:, feats], m, s


def closed_form(X, y, off, wts, lam, mu, s2):
    P = np.diag(1.0 / s2)
    return np.linalg.solve(X.T @ (wts[:, None] * X) + lam * P, X.T @ (wts * (y - off)) + lam * P @ mu)


# ---------------------------------------------------------------------------------------------------------------
# identity prior: bitwise the plain-L2 model
# ---------------------------------------------------------------------------------------------------------------
def test_identity_prior_is_bitwise_no_prior_fixed_effect(data):
    c0 = fe_coord(data, variance="SIMPLE")
    m0 = c0.update_model(c0.initialize_model())
    c1 = fe_coord(data, prior=identity_prior(m0), variance="SIMPLE")
    m1 = c1.update_model(c1.initialize_model())
    assert torch.equal(m0.glm.coefficients.means, m1.glm.coefficients.means)
    assert torch.equal(m0.glm.coefficients.variances, m1.glm.coefficients.variances)


@pytest.mark.parametrize("layout", ["dense", "segmented"])
def test_identity_prior_is_bitwise_no_prior_random_effect(data, layout):
    c0 = re_coord(data, layout, variance="SIMPLE")
    m0 = c0.update_model(c0.initialize_model())
    c1 = re_coord(data, layout, prior=identity_prior(m0), variance="SIMPLE")
    m1 = c1.update_model(c1.initialize_model())
    assert np.array_equal(m0.keys, m1.keys) and np.array_equal(m0.values, m1.values)
    assert np.array_equal(m0.variances, m1.variances)
    assert torch.equal(c0.score(m0), c1.score(m1))


# ---------------------------------------------------------------------------------------------------------------
# closed form (squared loss)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prior", [False, True])
def test_fixed_effect_matches_closed_form(data, priors, with_prior):
    fe = priors[0] if with_prior else None
    c = fe_coord(data, prior=fe)
    m = c.update_model(c.initialize_model())
    X = data.shards["g"].toarray()
    mu = fe.glm.coefficients.means.numpy() if with_prior else np.zeros(DG)
    s2 = fe.glm.coefficients.variances.numpy() if with_prior else np.ones(DG)
    w = closed_form(X, data.response, data.offsets, data.weights, LAM, mu, s2)
    err = np.abs(m.glm.coefficients.means.numpy() - w).max()
    print("fixed effect, prior =", with_prior, "max |w - closed form| =", err)
    assert err <= RIDGE_ERR["fixed"] * (10 if with_prior else 1)


@pytest.mark.parametrize("layout", ["dense", "segmented"])
@pytest.mark.parametrize("with_prior", [False, True])
def test_random_effect_matches_closed_form(data, priors, layout, with_prior):
    _, re, mu, s2 = priors
    c = re_coord(data, layout, prior=re if with_prior else None)
    m = c.update_model(c.initialize_model())
    worst = 0.0
    for e in range(E):
        r, feats, X, pm, ps = entity_problem(data, e, *((mu, s2) if with_prior else (None, None)))
        w = closed_form(X, data.response[r], data.offsets[r], data.weights[r], LAM, pm, ps)
        got = m.coefficients_of(e).means.numpy()
        worst = max(worst, np.abs(got[feats] - w).max())
        absent = np.setdiff1d(np.arange(D), feats)
        assert not got[absent].any()             # a prior feature the entity's data never has is not in the model
    print("random effect", layout, "prior =", with_prior, "max |w - closed form| =", worst)
    assert worst <= RIDGE_ERR["random"] * (10 if with_prior else 1)


# ---------------------------------------------------------------------------------------------------------------
# gradient of the explicit-prior objective on the unscaled data (logistic loss)
# ---------------------------------------------------------------------------------------------------------------
UPDATES = 6


def _explicit_gradient(X, y, off, wts, w, lam, mu, s2):
    Xt, wt = torch.from_numpy(X), torch.from_numpy(w).clone().requires_grad_(True)
    z = Xt @ wt + torch.from_numpy(off)
    yt = torch.from_numpy(y)
    f = (torch.from_numpy(wts) * (torch.nn.functional.softplus(z) - yt * z)).sum() \
        + 0.5 * lam * (((wt - torch.from_numpy(mu)) ** 2) / torch.from_numpy(s2)).sum()
    f.backward()
    return wt.grad.numpy()


def test_gradient_of_explicit_prior_objective_fixed_effect(logistic, priors):
    """The project's convergence rule: ||g|| <= tolerance x the gradient norm at the optimizer's zero point (v = 0,
    i.e. w = mu). Formed in torch fp64 autograd on the unscaled data with the prior written out.

    The rule has two halves with one tolerance: |f - f_prev| <= tol f(0) or ||g|| <= tol ||g(0)||. A single update
    always stops on the first half here (with or without a prior; TRON's truncated CG gains ~10 x per iteration), at
    ||g|| / ||g(0)|| ~ 1e-5 for tol = 1e-7. So the fit is UPDATES warm-started updates, each from the model the last
    one returned, as coordinate descent runs them: each adds at least one iteration from the previous point (through
    the original-space model for the fixed effect, i.e. the v0 = (w0 - mu) / sigma map)."""
    tol = 1e-7
    fe = priors[0]
    c = fe_coord(logistic, prior=fe, c=cfg(tol=tol), task="LOGISTIC_REGRESSION")
    m = c.initialize_model()
    for _ in range(UPDATES):
        m = c.update_model(m)
    X = logistic.shards["g"].toarray()
    mu, s2 = fe.glm.coefficients.means.numpy(), fe.glm.coefficients.variances.numpy()
    args = (X, logistic.response, logistic.offsets, logistic.weights)
    g = np.linalg.norm(_explicit_gradient(*args, m.glm.coefficients.means.numpy(), LAM, mu, s2))
    g0 = np.linalg.norm(_explicit_gradient(*args, mu, LAM, mu, s2))
    print("fixed effect: ||g|| =", g, "tolerance x ||g(start)|| =", tol * g0)
    assert g <= tol * g0


@pytest.mark.parametrize("layout", ["dense", "segmented"])
def test_gradient_of_explicit_prior_objective_random_effect(logistic, priors, layout):
    tol = 1e-7
    _, re, mu, s2 = priors
    c = re_coord(logistic, layout, prior=re, c=cfg(tol=tol), task="LOGISTIC_REGRESSION")
    m = c.initialize_model()
    for _ in range(UPDATES):                      # see the fixed-effect test
        m = c.update_model(m)
    for e in range(E):
        r, feats, X, pm, ps = entity_problem(logistic, e, mu, s2)
        args = (X, logistic.response[r], logistic.offsets[r], logistic.weights[r])
        g = np.linalg.norm(_explicit_gradient(*args, m.coefficients_of(e).means.numpy()[feats], LAM, pm, ps))
        g0 = np.linalg.norm(_explicit_gradient(*args, pm, LAM, pm, ps))
        print("entity", e, layout, "||g|| =", g, "tolerance x ||g(start)|| =", tol * g0)
        assert g <= tol * g0


# ---------------------------------------------------------------------------------------------------------------
# derived quantities
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "segmented"])
def test_random_effect_derived_quantities(logistic, priors, layout):
    _, re, mu, s2 = priors
    c = re_coord(logistic, layout, prior=re, variance="SIMPLE", task="LOGISTIC_REGRESSION")
    m = c.update_model(c.initialize_model())
    reg, ids = 0.0, logistic.id_tags["uid"]
    xw = np.zeros(logistic.n_rows)
    for e in range(E):
        r, feats, X, pm, ps = entity_problem(logistic, e, mu, s2)
        co = m.coefficients_of(e)
        w = co.means.numpy()[feats]
        reg += 0.5 * LAM * (((w - pm) ** 2) / ps).sum()
        xw[r] = X @ w
        z = xw[r] + logistic.offsets[r]
        p = 1 / (1 + np.exp(-z))
        h = (X * X).T @ (logistic.weights[r] * p * (1 - p))
        np.testing.assert_allclose(co.variances.numpy()[feats], ps / (ps * h + LAM + EPSILON), rtol=1e-12)
    assert c.regularization_term_value(m) == pytest.approx(reg, rel=1e-12)
    # ... also for a model the coordinate did not return itself (mapped from its coefficients)
    copy = RandomEffectModel("uid", "u", m.task, m.entity_ids, m.dim, m.keys.copy(), m.values.copy())
    assert c.regularization_term_value(copy) == pytest.approx(reg, rel=1e-12)
    np.testing.assert_allclose(c.score(m).numpy(), xw, rtol=0, atol=1e-12 * np.abs(xw).max())


def test_random_effect_full_variances_on_a_12_coefficient_entity(priors):
    """FULL variances = diag((X^T C X + lambda P)^-1), 1e-9 relative, one entity of 12 coefficients."""
    rng = np.random.default_rng(2)
    n, d = 40, 12
    X = rng.normal(size=(n, d))
    y = (rng.random(n) < 0.5).astype(float)
    gd = GameData(y, {"u": sp.csr_matrix(X)}, {"uid": np.zeros(n, dtype=np.int64)})
    mu, s2 = rng.normal(size=d), rng.uniform(0.25, 4.0, d)
    prior = RandomEffectModel("uid", "u", "LOGISTIC_REGRESSION", np.array([0]), d, np.arange(d), mu, s2)
    for layout in ("dense", "segmented"):
        c = re_coord(gd, layout, prior=prior, variance="FULL", task="LOGISTIC_REGRESSION")
        m = c.update_model(c.initialize_model())
        w = m.coefficients_of(0).means.numpy()
        p = 1 / (1 + np.exp(-(X @ w)))
        H = X.T @ ((p * (1 - p))[:, None] * X) + LAM * np.diag(1 / s2)
        np.testing.assert_allclose(m.coefficients_of(0).variances.numpy(), np.diag(np.linalg.inv(H)), rtol=1e-9)


def test_fixed_effect_derived_quantities(logistic, priors):
    fe = priors[0]
    mu, s2 = fe.glm.coefficients.means.numpy(), fe.glm.coefficients.variances.numpy()
    X = logistic.shards["g"].toarray()
    for variance in ("SIMPLE", "FULL"):
        c = fe_coord(logistic, prior=fe, variance=variance, task="LOGISTIC_REGRESSION")
        m = c.update_model(c.initialize_model())
        w = m.glm.coefficients.means.numpy()
        assert c.regularization_term_value(m) == pytest.approx(0.5 * LAM * (((w - mu) ** 2) / s2).sum(), rel=1e-12)
        p = 1 / (1 + np.exp(-(X @ w + logistic.offsets)))
        cw = logistic.weights * p * (1 - p)
        if variance == "SIMPLE":
            want = s2 / (s2 * ((X * X).T @ cw) + LAM + EPSILON)
        else:
            want = np.diag(np.linalg.inv(X.T @ (cw[:, None] * X) + LAM * np.diag(1 / s2)))
        np.testing.assert_allclose(m.glm.coefficients.variances.numpy(), want, rtol=1e-9)
        np.testing.assert_allclose(c.score(m).numpy(), X @ w, rtol=0, atol=1e-12 * np.abs(X @ w).max())


def test_large_lambda_returns_the_prior_means(data, priors):
    """lambda = 1e8: w within 1e-6 of mu. The exact minimiser sits sigma^2 X^T W r / lambda from mu (r the prior
    model's residuals), so the 40 rows used here have residuals of 0.02 at the prior means: at most 40 x 0.02 x 2
    (weight) x ~3 (|x|) x 4 (sigma^2) / 1e8 = 2e-7."""
    fe, re, mu, s2 = priors
    big = cfg(lam=1e8)
    sub = data.subset(np.arange(40))
    ids = sub.id_tags["uid"]
    small = 0.02 * np.cos(np.arange(40))
    y_fe = sub.offsets + sub.shards["g"] @ fe.glm.coefficients.means.numpy() + small
    y_re = sub.offsets + np.einsum("ij,ij->i", sub.shards["u"].toarray(), mu[ids]) + small
    d_fe = GameData(y_fe, sub.shards, sub.id_tags, sub.offsets, sub.weights)
    d_re = GameData(y_re, sub.shards, sub.id_tags, sub.offsets, sub.weights)
    c = fe_coord(d_fe, prior=fe, c=big)
    w = c.update_model(c.initialize_model()).glm.coefficients.means.numpy()
    assert np.abs(w - fe.glm.coefficients.means.numpy()).max() < 1e-6
    for layout in ("dense", "segmented"):
        c = re_coord(d_re, layout, prior=re, c=big)
        m = c.update_model(c.initialize_model())
        for e in np.unique(ids):
            _, feats, _, pm, _ = entity_problem(d_re, e, mu, s2)
            assert np.abs(m.coefficients_of(e).means.numpy()[feats] - pm).max() < 1e-6


# ---------------------------------------------------------------------------------------------------------------
# errors: each names the coordinate and is raised before any training
# ---------------------------------------------------------------------------------------------------------------
def test_prior_errors(data, priors):
    from photon_ml_amd.normalization.context import NormalizationContext
    from photon_ml_amd.optimization.problem import GLMOptimizationProblem
    fe, re, _, _ = priors
    for reg, opt in (("L1", "LBFGS"), ("ELASTIC_NET", "LBFGS")):
        with pytest.raises(ValueError, match="per-user"):
            re_coord(data, "dense", prior=re, c=cfg(opt=opt, reg=reg))
        with pytest.raises(ValueError, match="fixed"):
            fe_coord(data, prior=fe, c=cfg(opt=opt, reg=reg))
    with pytest.raises(ValueError, match="per-user.*RANDOM"):
        re_coord(data, "dense", prior=re, dc=RandomEffectDataConfiguration("uid", "u", projector_type="RANDOM=4"))
    norm = NormalizationContext(torch.full((DG,), 0.5, dtype=torch.float64), None, None)
    with pytest.raises(ValueError, match="fixed.*normalization"):
        fe_coord(data, prior=fe, normalization=norm)
    mu_sigma = (fe.glm.coefficients.means, fe.glm.coefficients.variances.sqrt())
    with pytest.raises(ValueError, match="fixed.*feature-sharded"):
        GLMOptimizationProblem(cfg(), "LINEAR_REGRESSION", feature_sharded=True, prior=mu_sigma, name="fixed")
    box = {0: (-1.0, 1.0)}
    with pytest.raises(ValueError, match="fixed.*constraints"):
        fe_coord(data, prior=fe, c=cfg(opt="LBFGS", constraints=box))
    with pytest.raises(ValueError, match="per-user.*constraints"):
        re_coord(data, "dense", prior=re, c=cfg(opt="LBFGS", constraints=box))
    # a later configuration (a lambda path through set_config) is checked the same way
    c = re_coord(data, "dense", prior=re)
    with pytest.raises(ValueError, match="per-user"):
        c.set_config(cfg(opt="LBFGS", reg="L1"))
    # the estimator: normalization by type on a fixed-effect coordinate with a prior
    est = estimator().set_prior_model(GameModel(OrderedDict(fixed=fe))).set_normalization(
        "SCALE_WITH_STANDARD_DEVIATION", {"g": DG - 1})
    with pytest.raises(ValueError, match="fixed.*normalization"):
        est.fit(data, None, [{"fixed": cfg(), "per-user": cfg()}])
    bad = RandomEffectModel("uid", "u", "LINEAR_REGRESSION", np.arange(2), D, np.array([0, 1]), np.array([1.0, np.nan]))
    with pytest.raises(ValueError, match="non-finite"):
        re_coord(data, "dense", prior=bad)


def estimator():
    return (GameEstimator(device="cpu").set_training_task("LINEAR_REGRESSION")
            .set_coordinate_data_configurations({"fixed": FixedEffectDataConfiguration("g"),
                                                 "per-user": RandomEffectDataConfiguration("uid", "u")})
            .set_coordinate_update_sequence(["fixed", "per-user"]).set_coordinate_descent_iterations(2))


def test_estimator_prior_model(data, priors):
    """``set_prior_model``: each coordinate gets its own sub-model; a coordinate absent from the prior model trains
    with plain L2 (bitwise the no-prior coordinate on the same residuals is covered above: here, the fit differs
    from the plain fit exactly where a prior exists)."""
    fe, re, _, _ = priors
    confs = [{"fixed": cfg(), "per-user": cfg()}]
    plain = estimator().fit(data, None, confs)[0].model
    only_fe = estimator().set_prior_model(GameModel(OrderedDict(fixed=fe))).fit(data, None, confs)[0].model
    est = estimator().set_prior_model(GameModel(OrderedDict([("fixed", fe), ("per-user", re)])))
    both = est.fit(data, None, confs)[0].model
    assert est.coordinates["fixed"].prior is not None and est.coordinates["per-user"].has_prior
    w = lambda m: m.get("fixed").glm.coefficients.means.numpy()
    assert np.abs(w(plain) - w(only_fe)).max() > 1e-3 and np.abs(w(both) - w(only_fe)).max() > 1e-6
    assert np.abs(both.get("per-user").values - only_fe.get("per-user").values).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------
SHARDS = ["--feature-shard-configurations", "name=global,feature.bags=features",
          "--feature-shard-configurations", "name=user,feature.bags=userFeatures,intercept=true"]
FIXED = "name=fixed,feature.shard=global,optimizer=TRON,max.iter=50,tolerance=1e-9,regularization=L2,reg.weights=1"
RANDOM = ("name=per-user,feature.shard=user,random.effect.type=userId,optimizer=TRON,max.iter=50,tolerance=1e-9,"
          "regularization=L2,reg.weights=1")


def _train(inp, out, *extra):
    from photon_ml_amd.cli import game_training
    args = ["--input-data-directories", str(inp), "--root-output-directory", str(out), "--training-task",
            "LOGISTIC_REGRESSION", *SHARDS, "--coordinate-configurations", FIXED, "--coordinate-configurations",
            RANDOM, "--coordinate-update-sequence", "fixed,per-user", "--coordinate-descent-iterations", "2",
            "--device", "cpu", *extra]
    return game_training.GameTrainingDriver(game_training.build_parser().parse_args(args)).run()


def test_cli_incremental_training(tmp_path):
    from photon_ml_amd.cli import game_training
    from photon_ml_amd.cli.params import load_config_file, parse_args_with_config
    from photon_ml_amd.io.data_writer import write_game_avro
    data, _ = generate_game_data(n_rows=1200, n_users=15, seed=4, task="LOGISTIC_REGRESSION")
    bags = {"global": "features", "user": "userFeatures"}
    users = data.id_tags["userId"]
    quiet = sorted(set(users))[3]                       # an entity whose new rows carry no weight: no active signal
    half = data.subset(np.arange(0, 1200, 2))
    half.weights = np.where(half.id_tags["userId"] == quiet, 0.0, half.weights)
    write_game_avro(str(tmp_path / "day1"), data, bags)
    write_game_avro(str(tmp_path / "day2"), half, bags)
    _train(tmp_path / "day1", tmp_path / "m1", "--variance-computation-type", "SIMPLE")
    prior_dir = str(tmp_path / "m1" / "best")
    warm = _train(tmp_path / "day2", tmp_path / "m2", "--model-input-directory", prior_dir)
    inc = _train(tmp_path / "day2", tmp_path / "m3", "--model-input-directory", prior_dir, "--incremental-training",
                 "true")
    wm, im = warm["best"].model, inc["best"].model
    f = lambda m: m.get("fixed").glm.coefficients.means.numpy()
    assert np.abs(f(wm) - f(im)).max() > 1e-3            # the prior changes the result; a warm start alone does not
    # the quiet entity keeps yesterday's coefficients wherever it appears in today's model
    from photon_ml_amd.io.model_io import load_game_model
    old = load_game_model(prior_dir, inc["index_maps"]).get("per-user")
    new = im.get("per-user")
    co_new, co_old = new.coefficients_of(quiet).means.numpy(), old.coefficients_of(quiet).means.numpy()
    present = co_new != 0
    assert present.any() and np.array_equal(co_new[present], co_old[present])
    assert np.abs(wm.get("per-user").coefficients_of(quiet).means.numpy()).max() < 1e-6    # plain L2 forgets it
    # the flag round-trips through --write-config / --config-file
    args = ["--input-data-directories", "x", "--root-output-directory", "y", "--training-task", "LOGISTIC_REGRESSION",
            *SHARDS, "--coordinate-configurations", FIXED, "--coordinate-update-sequence", "fixed",
            "--coordinate-descent-iterations", "1"]
    inc_args = args + ["--model-input-directory", prior_dir, "--incremental-training", "true"]
    parse_args_with_config(game_training.build_parser(), inc_args + ["--write-config", str(tmp_path / "inc.yaml")])
    assert load_config_file(str(tmp_path / "inc.yaml"))["incremental-training"] is True
    ns = parse_args_with_config(game_training.build_parser(), ["--config-file", str(tmp_path / "inc.yaml")])
    assert ns.incremental_training is True and ns.model_input_directory == prior_dir
    assert game_training.build_parser().parse_args(args).incremental_training is False
    # without a model directory the flag fails at parse time
    with pytest.raises(SystemExit):
        game_training.build_parser().parse_args(args + ["--incremental-training", "true"])


# ---------------------------------------------------------------------------------------------------------------
# process group: entity-sharded random effects with a prior
# ---------------------------------------------------------------------------------------------------------------
def test_entity_sharded_fit_with_prior_matches_single_process(tmp_path):
    import incremental_worker as iw
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PML_BACKEND="torch", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "incremental_worker.py"), str(r), "2", str(port),
                               str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=600)[0].decode(errors="replace") for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    data, prior = iw.problem()
    ref = iw.estimator(prior).fit(data, None, [iw.configuration()])[0].model
    fe = ref.get("global").glm.coefficients.means.numpy()
    users = ref.get("per-user")
    seen = 0
    for r in range(2):
        assert np.abs(np.load(tmp_path / f"fe_r{r}.npy") - fe).max() <= 1e-8
        part = np.load(tmp_path / f"re_r{r}.npz", allow_pickle=True)
        for e, w in zip(part["ids"], part["W"]):
            if np.any(w):                                             # entities this rank owns
                assert np.abs(w - users.coefficients_of(e).means.numpy()).max() <= 1e-8
                seen += 1
    assert seen == users.n_entities
