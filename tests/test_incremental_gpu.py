"""Incremental training on the GPU: the production random-effect solvers on prior-folded data.

The prior fold (``prior_fold_kernel``) rewrites the entity-sorted CSR once; every solver route then runs unchanged on
the folded data and the coordinate maps ``v <-> w`` at its boundary. Per route (row space, lean fused, ``rs_big``,
tall-narrow exact-Hessian, pass path) the model is compared with the CPU float64 TRON of tests/test_re_parity_gpu.py,
entity by entity, on data folded ON THE HOST (``X_e diag(sigma)``, offsets ``+ X_e mu``, ``w = mu + sigma v``), in the
project's two regimes: iteration-limited (tolerance 0, 4 iterations) W to 1e-9 relative; converged at 1e-8 identical
iteration counts, W to 1e-6. The helpers are copies of that file's.
"""
from collections import OrderedDict

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from photon_ml_amd.constants import EPSILON
from photon_ml_amd.data.game_data import GameData, generate_game_data
from photon_ml_amd.models.game import FixedEffectModel, GameModel, RandomEffectModel

pytestmark = pytest.mark.gpu
TASK = "LOGISTIC_REGRESSION"


def make_entities(sizes, d_pool, nnz_row, seed, dense_pool=False):
    """One random-effect shard: entity k has ``sizes[k]`` rows, ``nnz_row`` features per row from its own pool of
    ``d_pool`` global features (+ an intercept column); logistic labels from a per-entity ground truth."""
    rng = np.random.default_rng(seed)
    D = len(sizes) * d_pool + 1
    rows, cols, vals, ids, z = [], [], [], [], []
    r = 0
    for k, n in enumerate(sizes):
        wt = rng.normal(size=d_pool) * 0.5
        for _ in range(n):
            f = np.arange(d_pool) if dense_pool else np.sort(rng.choice(d_pool, size=nnz_row, replace=False))
            v = rng.normal(size=f.size)
            rows += [r] * (f.size + 1)
            cols += list(k * d_pool + f) + [D - 1]
            vals += list(v) + [1.0]
            z.append(float(v @ wt[f]) + 0.2 * np.sin(k))
            ids.append(k)
            r += 1
    x = sp.csr_matrix((vals, (rows, cols)), shape=(r, D))
    y = (rng.random(r) < 1 / (1 + np.exp(-np.array(z)))).astype(float)
    return GameData(y, {"user": x}, {"userId": np.array(ids)})


def make_prior(data, seed, identity=False):
    """A prior over the entities' present features: means 0.3 N(0, 1), variances in [0.25, 4]; the LAST entity has no
    prior, every entity lacks one for its first present feature, and has one for a feature its data never shows (the
    column before its first feature, where there is one). Returns (model, {e: mu over D}, {e: sigma^2 over D})."""
    rng = np.random.default_rng(seed)
    x = data.shards["user"].tocsr()
    ids = data.id_tags["userId"]
    D = x.shape[1]
    ents = np.unique(ids)
    keys, vals, var, mu, s2 = [], [], [], {}, {}
    for i, e in enumerate(ents):
        mu[e], s2[e] = np.zeros(D), np.ones(D)
        if i == len(ents) - 1:
            continue
        feats = np.unique(x[np.nonzero(ids == e)[0]].indices)
        have = feats[1:]
        if feats[0] > 0 and not identity:
            have = np.concatenate([[feats[0] - 1], have])
        m = np.zeros(len(have)) if identity else 0.3 * rng.normal(size=len(have))
        v = np.ones(len(have)) if identity else rng.uniform(0.25, 4.0, size=len(have))
        mu[e][have], s2[e][have] = m, v
        keys.append(i * D + have), vals.append(m), var.append(v)
    model = RandomEffectModel("userId", "user", TASK, ents[:-1], D, np.concatenate(keys), np.concatenate(vals),
                              np.concatenate(var))
    return model, mu, s2


def cpu_tron(data, l2, tol, max_iter, mu, s2, offsets=None, w0=None):
    """Per entity, the CPU float64 TRON on the entity's rows restricted to its features, with the prior folded on the
    host: ``X_e diag(sigma)``, offsets ``+ X_e mu``, start ``(w0 - mu) / sigma``, result ``w = mu + sigma v``.
    {entity id: (w over the global features, iterations, convergence reason)}."""
    from photon_ml_amd.data.matrix import LabeledData
    from photon_ml_amd.function.losses import LOGISTIC
    from photon_ml_amd.function.objective import GLMObjective
    from photon_ml_amd.ops.reference import TorchGLMData
    from photon_ml_amd.optimization.tron import TRON
    x = data.shards["user"].tocsr()
    ids = data.id_tags["userId"]
    off = np.zeros(data.n_rows) if offsets is None else offsets
    out = {}
    for e in np.unique(ids):
        r = np.nonzero(ids == e)[0]
        xe = x[r]
        feats = np.unique(xe.indices)
        m, s = mu[e][feats], np.sqrt(s2[e][feats])
        xl = xe[:, feats]
        folded = sp.csr_matrix(xl.multiply(s[None, :]))
        gd = TorchGLMData(LabeledData(folded, data.response[r], off[r] + xl @ m, np.ones(len(r))), torch.device("cpu"))
        opt = TRON(tolerance=tol, max_iterations=max_iter, track_state=False)
        start = torch.zeros(len(feats), dtype=torch.float64) if w0 is None else \
            torch.from_numpy(np.ascontiguousarray((w0[e][feats] - m) / s))
        v, _ = opt.optimize(GLMObjective(LOGISTIC, l2_weight=l2), gd, start)
        full = np.zeros(x.shape[1])
        full[feats] = m + s * v.numpy()
        out[e] = (full, int(opt.current.iter), opt.convergence_reason())
    return out


def coordinate(data, l2, tol, max_iter, prior, opt="TRON", variance="NONE", dc=None, device="cuda"):
    from photon_ml_amd.algorithm.coordinates import RandomEffectCoordinate
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    cfg = GLMOptimizationConfiguration(OptimizerConfig(opt, max_iter, tol), RegularizationContext("L2"), l2)
    return RandomEffectCoordinate("u", data, dc or RandomEffectDataConfiguration("userId", "user"), cfg, TASK,
                                  compute_variance=variance, device=device, layout="segmented", prior=prior)


def gpu_fit(data, l2, tol, max_iter, prior, opt="TRON", start=None, device="cuda"):
    """The production coordinate on the GPU; returns ({entity: w}, {entity: iterations}, coordinate, model)."""
    c = coordinate(data, l2, tol, max_iter, prior, opt, device=device)
    got = {}
    c._defer_stats = lambda it, rc, act, sec: got.update(it=it.cpu().numpy(), rc=rc.cpu().numpy())
    m = c.update_model(start if start is not None else c.initialize_model(), None)
    m.materialize()
    W = {e: np.asarray(m.coefficients_of(e).means, dtype=np.float64) for e in m.entity_ids}
    its = {e: int(got["it"][i]) for i, e in enumerate(c.dataset.entity_ids)}
    return W, its, c, m


CASES = {
    # name: (sizes, d_pool, nnz_row, dense_pool, env, expected component)
    "rs_20": ([20] * 40 + [17] * 10, 120, 12, False, {}, "rs"),
    "lean_quad": ([90, 120, 150, 200, 260, 75] * 4, 300, 16, False, {"PML_RE_ROW_SPACE": "0"}, "lean"),
    "rs_big": ([80] * 10 + [100] * 6 + [128] * 4, 150, 0, True, {}, "rs_big"),
    "tall": ([150, 90, 200, 120, 65] * 3, 40, 0, True, {}, "tall"),          # d_e = 41 <= 64 < n_e
}


def _check_routing(c, kind):
    rs, fused, sub = c._comps
    assert sub is None
    if kind == "lean":
        assert rs is None and fused is not None and fused.quad and fused.res is None
        assert all(not h and dm <= 1024 for dm, _, h in fused.launches)
    elif kind == "tall":
        assert rs is None and fused is not None and fused.res is None and all(h for _, _, h in fused.launches)
    else:
        assert fused is None and rs is not None
        ns = [cl.n for cl in rs.classes]
        assert (max(ns) > 64) == (kind == "rs_big"), ns


def _rel(w, w_ref):
    return np.abs(w - w_ref).max() / max(np.abs(w_ref).max(), 1e-300)


@pytest.mark.parametrize("case", list(CASES))
def test_production_re_kernel_on_folded_data_matches_cpu_tron_fp64(case, monkeypatch):
    import photon_ml_amd.optimization.entity_tron as et
    sizes, dp, nnz, dense, env, kind = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(et, "RESIDENT", "0")
    data = make_entities(sizes, dp, nnz, seed=len(case), dense_pool=dense)
    prior, mu, s2 = make_prior(data, seed=7)
    # (1) iteration-limited: tolerance 0, every entity runs exactly 4 TRON iterations on both sides
    W, its, c, _ = gpu_fit(data, 1.0, 0.0, 4, prior)
    _check_routing(c, kind)
    ref = cpu_tron(data, 1.0, 0.0, 4, mu, s2)
    worst = 0.0
    for e, (w_ref, it_ref, _) in ref.items():
        assert its[e] == it_ref == 4, (e, its[e], it_ref)
        worst = max(worst, _rel(W[e], w_ref))
    print(case, "iteration-limited: max relative error", worst)
    assert worst < 1e-9, (case, worst)
    # (2) converged: the same iteration count per entity
    W, its, c, m = gpu_fit(data, 1.0, 1e-8, 60, prior)
    ref = cpu_tron(data, 1.0, 1e-8, 60, mu, s2)
    worst = 0.0
    for e, (w_ref, it_ref, _) in ref.items():
        assert its[e] == it_ref, (case, e, its[e], it_ref)
        worst = max(worst, _rel(W[e], w_ref))
    print(case, "converged: max relative error", worst)
    assert worst < 1e-6, (case, worst)
    # (3) a FOREIGN warm start maps through v0 = (w0 - mu) / sigma. The start is halfway between the prior means and
    # the converged model, i.e. half the converged v: like the plain-L2 test's half model it lies in the row space of
    # the (folded) data, which is all a row-space warm start can represent (beta = L^-1 X v0)
    w_half = {e: np.where(W[e] != 0, mu[e] + 0.5 * (W[e] - mu[e]), 0.0) for e in W}
    keys = np.concatenate([int(i) * m.dim + np.nonzero(w_half[e])[0] for i, e in enumerate(m.entity_ids)])
    vals = np.concatenate([w_half[e][np.nonzero(w_half[e])[0]] for e in m.entity_ids])
    foreign = RandomEffectModel(m.random_effect_type, m.feature_shard_id, TASK, m.entity_ids, m.dim, keys, vals)
    W2, its2, _, _ = gpu_fit(data, 1.0, 0.0, 4, prior, start=foreign)
    ref2 = cpu_tron(data, 1.0, 0.0, 4, mu, s2, w0=w_half)
    worst = 0.0
    for e, (w_ref, it_ref, _) in ref2.items():
        assert its2[e] == it_ref
        worst = max(worst, _rel(W2[e], w_ref))
    print(case, "foreign warm start: max relative error", worst)
    assert worst < 1e-9, (case, worst)


def folded_on_host(data, mu, s2):
    """The plain-L2 problem the fold defines, built on the host from scipy: values ``x_ij sigma_{e(i) j}``, offsets
    ``x_i . mu_{e(i)}``."""
    x = data.shards["user"].tocoo()
    ids = data.id_tags["userId"]
    sg = np.array([np.sqrt(s2[ids[r]][c]) for r, c in zip(x.row, x.col)])
    m = np.array([mu[ids[r]][c] for r, c in zip(x.row, x.col)])
    off = np.bincount(x.row, weights=x.data * m, minlength=data.n_rows)
    xs = sp.csr_matrix((x.data * sg, (x.row, x.col)), shape=x.shape)
    return GameData(data.response, {"user": xs}, data.id_tags, off, np.ones(data.n_rows))


def test_pass_path_lbfgs_on_folded_data(monkeypatch):
    """An L-BFGS configuration takes no fused solver: the block-diagonal passes over the tiled layout (built from the
    folded CSR) solve every entity. Reference: the CPU coordinate WITHOUT a prior on data folded on the host, the same
    batched L-BFGS, so only rounding separates them: iteration-limited (tolerance 0, 4 iterations) to 1e-9 relative;
    converged at 1e-8 with the same iteration counts, W to 1e-6."""
    monkeypatch.setenv("PML_RE_ROW_SPACE", "0")
    data = make_entities([70, 90, 120, 65] * 3, 40, 10, seed=4)
    prior, mu, s2 = make_prior(data, seed=8)
    host = folded_on_host(data, mu, s2)
    for tol, iters, bound in ((0.0, 4, 1e-9), (1e-8, 100, 1e-6)):
        W, its, c, _ = gpu_fit(data, 1.0, tol, iters, prior, opt="LBFGS")
        assert getattr(c, "_comps", None) is None and c.dataset.seg.glm.built       # the pass layout ran
        V, its_ref, _, _ = gpu_fit(host, 1.0, tol, iters, None, opt="LBFGS", device="cpu")
        worst = 0.0
        for e in W:
            assert its[e] == its_ref[e], (tol, e, its[e], its_ref[e])
            # w = mu + sigma v on the entity's projected coefficients (v != 0), nothing elsewhere
            worst = max(worst, _rel(W[e], np.where(V[e] != 0, mu[e] + np.sqrt(s2[e]) * V[e], 0.0)))
        print("pass path, tolerance", tol, ": max relative error", worst)
        assert worst < bound, (tol, worst)


# ---------------------------------------------------------------------------------------------------------------
# the coordinate boundary on the device
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    data = make_entities([20] * 12 + [17] * 5 + [90, 75, 130], 60, 12, seed=11)
    return (data,) + make_prior(data, seed=12)


def test_identity_prior_is_bitwise_no_prior_on_the_device(small):
    data = small[0]
    ident, _, _ = make_prior(data, seed=0, identity=True)
    for variance in ("NONE", "SIMPLE"):
        out = []
        for prior in (None, ident):
            c = coordinate(data, 1.0, 1e-8, 30, prior, variance=variance)
            m = c.update_model(c.initialize_model(), None)
            out.append((m.keys, m.values, m.variances, c.score(m).cpu(), c.regularization_term_value(m)))
        a, b = out
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and torch.equal(a[3], b[3])
        assert (a[2] is None and b[2] is None) or np.array_equal(a[2], b[2])
        assert a[4] == pytest.approx(b[4], rel=1e-14)


def _xw(data, model):
    """``x_i . w_{e(i)}`` from scipy and the model's coefficients."""
    x = data.shards["user"].tocsr()
    ids = data.id_tags["userId"]
    out = np.zeros(data.n_rows)
    for e in np.unique(ids):
        r = np.nonzero(ids == e)[0]
        out[r] = x[r] @ model.coefficients_of(e).means.numpy()
    return out


def test_score_matches_original_space_on_active_and_passive_rows(small):
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration
    data, prior, mu, s2 = small
    dc = RandomEffectDataConfiguration("userId", "user", active_data_upper_bound=40, passive_data_lower_bound=5)
    c = coordinate(data, 1.0, 1e-8, 30, prior, dc=dc)
    assert len(c.dataset.passive_rows) > 0 and len(c.dataset.active_rows) < data.n_rows
    m = c.update_model(c.initialize_model(), torch.from_numpy(0.2 * np.cos(np.arange(data.n_rows))))
    got = c.score(m).cpu().numpy()
    m.materialize()
    want = np.where(c.dataset.score_mask, _xw(data, m), 0.0)
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


def test_warm_start_from_the_prior_model_starts_at_v_zero(small):
    """The solvers' budget is at least one iteration (``OptimizerConfig`` refuses 0, and the fused kernels test the
    budget after a step), so the zero-iteration statement is checked on what the solvers are handed: the prior model
    mapped as a foreign warm start is v = 0 exactly, and v = 0 maps back to w = mu exactly."""
    data, prior, mu, s2 = small
    c = coordinate(data, 1.0, 1e-8, 30, prior)
    v0 = c._warm_start_segmented(prior)
    assert v0.numel() == c.dataset.d_total and not bool(v0.any())
    w = c._to_original_segmented(v0)[0]
    assert torch.equal(w, c.dataset.prior.mu)
    back = RandomEffectModel("userId", "user", TASK, c.dataset.entity_ids, c.dataset.dim, c.dataset.projection_keys_t, w)
    for e in np.unique(data.id_tags["userId"])[:-1]:
        feats = np.nonzero(back.coefficients_of(e).means.numpy())[0]
        assert len(feats) and np.array_equal(back.coefficients_of(e).means.numpy()[feats], mu[e][feats])


@pytest.mark.parametrize("variance", ["SIMPLE", "FULL"])
def test_variances_on_the_device_match_the_host_definitions(small, variance):
    """SIMPLE = sigma^2 / (sigma^2 h_jj + lambda + eps), FULL = diag((X^T C X + lambda P)^-1), per entity in numpy at
    the returned w; 1e-9 relative, the tolerance of tests/test_full_variance_gpu.py."""
    data, prior, mu, s2 = small
    lam = 1.0
    c = coordinate(data, lam, 1e-8, 30, prior, variance=variance)
    m = c.update_model(c.initialize_model(), None)
    x = data.shards["user"].tocsr()
    ids = data.id_tags["userId"]
    worst = 0.0
    for e in np.unique(ids):
        r = np.nonzero(ids == e)[0]
        feats = np.unique(x[r].indices)
        X = x[r][:, feats].toarray()
        co = m.coefficients_of(e)
        p = 1 / (1 + np.exp(-(X @ co.means.numpy()[feats])))
        cw = p * (1 - p)
        v = s2[e][feats]
        if variance == "SIMPLE":
            want = v / (v * ((X * X).T @ cw) + lam + EPSILON)
        else:
            want = np.diag(np.linalg.inv(X.T @ (cw[:, None] * X) + lam * np.diag(1 / v)))
        worst = max(worst, (np.abs(co.variances.numpy()[feats] - want) / want).max())
    print(variance, "variances: max relative error", worst)
    assert worst <= 1e-9


# ---------------------------------------------------------------------------------------------------------------
# fixed effect + random effect through the estimator
# ---------------------------------------------------------------------------------------------------------------
# max |GPU - CPU| over all coefficients of the no-prior fit below (the shapes and configuration of
# tests/test_game_gpu.py::test_game_fit_gpu_matches_cpu, which holds rtol 1e-5 / atol 1e-6), measured on an MI355X:
# see profiles/incremental_training.md. With a prior the bound is 10 x that.
GAME_GPU_CPU = {"global": 4.5e-16, "per-user": 4.5e-16}      # measured 4.44e-16 both (2 ulp at |w| ~ 1)


def _game_fit(device, data, prior):
    from photon_ml_amd.data.random_effect import FixedEffectDataConfiguration, RandomEffectDataConfiguration
    from photon_ml_amd.estimators.game_estimator import GameEstimator
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    cfg = GLMOptimizationConfiguration(OptimizerConfig("LBFGS", 100, 1e-10), RegularizationContext("L2"), 1.0)
    est = (GameEstimator(device=device).set_training_task(TASK)
           .set_coordinate_data_configurations({"global": FixedEffectDataConfiguration("global"),
                                                "per-user": RandomEffectDataConfiguration("userId", "user")})
           .set_coordinate_update_sequence(["global", "per-user"]).set_coordinate_descent_iterations(2)
           .set_prior_model(prior))
    return est.fit(data, None, [{"global": cfg, "per-user": cfg}])[0].model


def test_game_fit_with_prior_gpu_matches_cpu():
    from photon_ml_amd.models.glm import Coefficients, model_for_task
    data, _ = generate_game_data(n_rows=4000, n_users=40, n_items=25, seed=21, task=TASK)
    rng = np.random.default_rng(6)
    dg, du = data.shards["global"].shape[1], data.shards["user"].shape[1]
    fe = FixedEffectModel(model_for_task(TASK, Coefficients(torch.from_numpy(0.3 * rng.normal(size=dg)),
                                                            torch.from_numpy(rng.uniform(0.25, 4.0, dg)))), "global")
    ents = np.array(sorted(set(data.id_tags["userId"].astype(str)))[:30])
    keys = (np.arange(30)[:, None] * du + np.arange(du - 1)[None, :]).reshape(-1)
    re = RandomEffectModel("userId", "user", TASK, ents, du, keys, 0.3 * rng.normal(size=keys.size),
                           rng.uniform(0.25, 4.0, keys.size))
    prior = GameModel(OrderedDict([("global", fe), ("per-user", re)]))
    diffs = {}
    for name, pm in (("no prior", None), ("prior", prior)):
        mc, mg = _game_fit("cpu", data, pm), _game_fit("cuda", data, pm)
        d_fe = float((mc.get("global").glm.coefficients.means.cpu()
                      - mg.get("global").glm.coefficients.means.cpu()).abs().max())
        assert np.array_equal(mc.get("per-user").keys, mg.get("per-user").keys)
        d_re = float(np.abs(mc.get("per-user").values - mg.get("per-user").values).max())
        diffs[name] = {"global": d_fe, "per-user": d_re}
        print("GAME fit GPU vs CPU,", name, ": max |difference| fixed", d_fe, "random", d_re)
    for cid in ("global", "per-user"):
        assert diffs["prior"][cid] <= 10 * GAME_GPU_CPU[cid], diffs
