"""Shared pieces of the random-effect normalization tests: generated data, contexts, and the independent oracle.

The oracle uses none of the shift code: per entity it builds ``X' = (X - s) f`` DENSELY with numpy over the entity's
active features, solves that data with normalization off by the existing CPU float64 solvers (a CPU
``RandomEffectCoordinate`` without a context: ``batched_tron`` / ``batched_lbfgs`` over plain data) and maps the
solution with ``T``: ``w_j = f_j w'_j``, ``w_i0 = w'_i0 - sum_j f_j s_j w'_j``.
"""
import numpy as np
import scipy.sparse as sp
import torch

from photon_ml_amd.data.game_data import GameData
from photon_ml_amd.normalization.context import NormalizationContext

TASKS = {"LOGISTIC_REGRESSION": "logistic", "POISSON_REGRESSION": "poisson", "LINEAR_REGRESSION": "squared"}
NORM_TYPES = ("SCALE_WITH_MAX_MAGNITUDE", "SCALE_WITH_STANDARD_DEVIATION", "STANDARDIZATION")


def make_data(shapes, intercept="last", seed=0, task="LOGISTIC_REGRESSION", nnz_frac=0.6, zero_weight=True,
              offsets=True, shared=4):
    """One random-effect shard. ``shapes``: (rows, coefficients incl. the intercept) per entity; entity k draws its
    non-intercept features from ``shared`` features common to all entities and a pool of its own (every feature of
    the entity appears in at least one row, so d_e is exact). The intercept (value 1 in every row) has feature id 0,
    D - 1 or D // 2 (``intercept`` = first / last / middle). Feature means are non-zero and variances O(1)."""
    rng = np.random.default_rng(seed)
    own = [max(d - 1 - shared, 0) for _, d in shapes]
    D = shared + sum(own) + 1
    icpt = {"first": 0, "last": D - 1, "middle": D // 2}[intercept]
    ids_free = np.array([j for j in range(D) if j != icpt])
    mean = rng.normal(size=D) * 0.7
    scale = rng.uniform(0.6, 1.6, size=D)
    rows, cols, vals, ent, z = [], [], [], [], []
    r = 0
    lo = shared
    for k, (n, d) in enumerate(shapes):
        feats = np.concatenate([np.arange(min(shared, d - 1)), np.arange(lo, lo + own[k])])[: d - 1]
        lo += own[k]
        gf = ids_free[feats]
        wt = rng.normal(size=gf.size) * 0.4
        for i in range(n):
            keep = rng.random(gf.size) < nnz_frac
            if i == 0:
                keep[:] = True                      # every feature of the entity is active
            f = gf[keep]
            v = mean[f] + scale[f] * rng.normal(size=f.size)
            rows += [r] * (f.size + 1)
            cols += list(f) + [icpt]
            vals += list(v) + [1.0]
            z.append(float((v - mean[f]) @ wt[keep]) * 0.5 + 0.1 * np.cos(k))
            ent.append(k)
            r += 1
    x = sp.csr_matrix((vals, (rows, cols)), shape=(r, D))
    z = np.array(z)
    if task == "LOGISTIC_REGRESSION":
        y = (rng.random(r) < 1 / (1 + np.exp(-z))).astype(float)
    elif task == "POISSON_REGRESSION":
        y = rng.poisson(np.exp(np.clip(z, -2, 2))).astype(float)
    else:
        y = z + 0.3 * rng.normal(size=r)
    w = rng.uniform(0.5, 2.0, size=r)
    if zero_weight:
        w[rng.random(r) < 0.1] = 0.0
    off = 0.2 * rng.normal(size=r) if offsets else np.zeros(r)
    return GameData(y, {"user": x}, {"userId": np.array(ent)}, off, w), icpt


def build_context(data, norm_type, icpt):
    from photon_ml_amd.stat.summary import BasicStatisticalSummary
    return NormalizationContext.build(norm_type, BasicStatisticalSummary.compute(data.shards["user"]), icpt)


def opt_config(optimizer, reg, lam, tol, max_iter, alpha=0.5):
    from photon_ml_amd.optimization.config import GLMOptimizationConfiguration, OptimizerConfig, RegularizationContext
    rc = RegularizationContext(reg, alpha) if reg == "ELASTIC_NET" else RegularizationContext(reg)
    return GLMOptimizationConfiguration(OptimizerConfig(optimizer, max_iter, tol), rc, lam)


def coordinate(data, cfg, task, device="cpu", layout="segmented", normalization=None, projector=None, **kw):
    from photon_ml_amd.algorithm.coordinates import RandomEffectCoordinate
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration
    dc = RandomEffectDataConfiguration("userId", "user") if projector is None else \
        RandomEffectDataConfiguration("userId", "user", projector_type=projector)
    return RandomEffectCoordinate("u", data, dc, cfg, task, device=device, layout=layout,
                                  normalization=normalization, **kw)


def run(coord, start=None, partial=None):
    """One update; ({entity: w over the global features}, iterations, reason codes, model)."""
    got = {}
    if coord.dataset.layout == "segmented":
        coord._defer_stats = lambda it, rc, act, sec: got.update(it=it.cpu().numpy().copy(), rc=rc.cpu().numpy().copy())
    m = coord.update_model(start if start is not None else coord.initialize_model(), partial)
    if hasattr(m, "materialize"):
        m.materialize()
    W = model_dense(m, coord.dataset.dim)
    return W, got.get("it"), got.get("rc"), m


def model_dense(m, D):
    """[entities, D] dense coefficients of a RandomEffectModel (rows in the model's entity order)."""
    keys, vals = m.tensors("cpu")
    out = np.zeros((len(m.entity_ids), D))
    k = keys.numpy()
    out[k // D, k % D] = vals.numpy()
    return out


def transformed_data(data, ctx):
    """The oracle's data: per entity ``X' = (X - s) f`` densely over the entity's active features (numpy)."""
    x = data.shards["user"].tocsr()
    D = x.shape[1]
    f = np.ones(D) if ctx.factors is None else ctx.factors.numpy()
    s = np.zeros(D) if ctx.shifts is None else ctx.shifts.numpy()
    ids = data.id_tags["userId"]
    xd = np.asarray(x.todense())
    out = np.zeros_like(xd)
    for e in np.unique(ids):
        r = np.nonzero(ids == e)[0]
        feats = np.unique(x[r].indices)
        out[np.ix_(r, feats)] = (xd[np.ix_(r, feats)] - s[feats]) * f[feats]
    xp = sp.csr_matrix(out)
    # an exact zero of X' must not drop a feature from an entity's model
    for e in np.unique(ids):
        r = np.nonzero(ids == e)[0]
        assert np.array_equal(np.unique(xp[r].indices), np.unique(x[r].indices))
    return GameData(data.response, {"user": xp}, {"userId": ids}, data.offsets, data.weights)


def to_original(Wp, ctx, icpt):
    """``T`` per entity row of the dense [entities, D] transformed-space coefficients (numpy)."""
    D = Wp.shape[1]
    f = np.ones(D) if ctx.factors is None else ctx.factors.numpy()
    W = Wp * f
    if ctx.shifts is not None:
        W[:, icpt] -= (Wp * f * ctx.shifts.numpy()).sum(1)
    return W


def to_transformed(W, ctx, icpt):
    """``T^-1`` per entity row (numpy)."""
    D = W.shape[1]
    f = np.ones(D) if ctx.factors is None else ctx.factors.numpy()
    Wp = W.copy()
    if ctx.shifts is not None:
        Wp[:, icpt] += (W * ctx.shifts.numpy()).sum(1)
    return Wp / f


def oracle(data, ctx, icpt, cfg, task, layout="segmented", start_w=None, partial=None):
    """(W in original space, W' in transformed space, iterations, reasons) of the independent oracle; ``start_w``:
    dense original-space warm start [entities, D]."""
    from photon_ml_amd.models.game import RandomEffectModel
    td = transformed_data(data, ctx)
    c = coordinate(td, cfg, task, device="cpu", layout=layout)
    start = None
    if start_w is not None:
        sp_ = to_transformed(start_w, ctx, icpt)
        D = sp_.shape[1]
        e, j = np.nonzero(sp_)
        keys = e.astype(np.int64) * D + j
        start = RandomEffectModel("userId", "user", c.task, c.dataset.entity_ids, D, keys, sp_[e, j])
    Wp, it, rc, _ = run(c, start, partial)
    return to_original(Wp, ctx, icpt), Wp, it, rc


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def dense_model(coord, W):
    """A RandomEffectModel holding the dense [entities, D] coefficients ``W`` (a foreign warm start)."""
    from photon_ml_amd.models.game import RandomEffectModel
    D = W.shape[1]
    e, j = np.nonzero(W)
    return RandomEffectModel("userId", "user", coord.task, coord.dataset.entity_ids, D, e.astype(np.int64) * D + j,
                             W[e, j])
