"""Shared helpers of the random-effect parity tests (not a test file): weighted per-entity data for the three fused
losses, the CPU float64 TRON oracle per entity, the production coordinate on the GPU, and the rounding floor of the
oracle itself.

The oracle is ``optimization/tron.py`` (the LIBLINEAR-semantics TRON of the reference, ``TRON.scala:80-340``) on
``TorchGLMData`` in float64, one entity at a time on its own projected rows
(``SingleNodeOptimizationProblem.scala:85-103``). ``tests/test_re_reference_weights.py`` shows that it treats row
weights as row multiplicities. For L-BFGS / OWL-QN the oracle is ``batched.batched_lbfgs`` in float64 on the CPU over
the segmented coordinate (:func:`cpu_owlqn`), with the rows of the data permuted for its floor.
"""
import numpy as np
import scipy.sparse as sp
import torch

from photon_ml_amd.data.game_data import GameData

TASKS = {"LOGISTIC": "LOGISTIC_REGRESSION", "POISSON": "POISSON_REGRESSION", "SQUARED": "LINEAR_REGRESSION"}


def loss_of(loss):
    """The pointwise loss object of a loss name (LOGISTIC / POISSON / SQUARED)."""
    from photon_ml_amd.function.losses import loss_for_task
    return loss_for_task(TASKS[loss])


def make_entities(sizes, d_pool, nnz_row, seed, dense_pool=False, loss="LOGISTIC", weighted=True):
    """One random-effect shard: entity k has ``sizes[k]`` rows, ``nnz_row`` features per row from its own pool of
    ``d_pool`` global features (+ an intercept column); labels of ``loss`` from a per-entity ground truth (with
    ``dense_pool`` scaled by ``1 / sqrt(d_pool / 16)``, so Poisson margins stay inside the clip).

    Row weights ``integers(1, 17) / 4`` (in [0.25, 4], exact in binary) with about 15 % of the rows at exactly 0.0
    (``weighted=False``: all 1.0); base offsets ``0.3 sin(arange(n))``."""
    rng = np.random.default_rng(seed)
    D = len(sizes) * d_pool + 1
    scale = 1.0 / np.sqrt(d_pool / 16.0) if dense_pool else 1.0
    rows, cols, vals, ids, z = [], [], [], [], []
    r = 0
    for k, n in enumerate(sizes):
        wt = rng.normal(size=d_pool) * 0.5 * scale
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
    z = np.array(z)
    if loss == "LOGISTIC":
        y = (rng.random(r) < 1 / (1 + np.exp(-z))).astype(float)
    elif loss == "POISSON":
        y = rng.poisson(np.exp(np.clip(z, -3, 2))).astype(float)
    elif loss == "SQUARED":
        y = z + 0.3 * rng.normal(size=r)
    else:
        raise ValueError(loss)
    w = rng.integers(1, 17, size=r) / 4.0
    w[rng.random(r) < 0.15] = 0.0
    if not weighted:
        w = np.ones(r)
    return GameData(y, {"user": x}, {"userId": np.array(ids)}, offsets=0.3 * np.sin(np.arange(r)), weights=w)


def make_ragged_entities(spec, seed, loss="LOGISTIC", weighted=True, duplicate_rows=None):
    """One random-effect shard of ragged rows. ``spec``: per entity ``(n_rows, d_e, row_lengths)``; row i of the
    entity holds ``min(row_lengths[i % len(row_lengths)], d_e)`` distinct columns of the entity's own block of ``d_e``
    global columns, and every one of the ``d_e`` columns occurs in some row (the projected width is exactly ``d_e``;
    ValueError when the rows are too short for that). The columns are spread deterministically first -- the rows take
    consecutive runs of the block until it is covered -- and the rest is drawn at random. There is NO intercept
    column: a row of length 0 has no entry at all (it adds a loss term through its offset only), and an entity
    with ``d_e = 0`` has none in any row.

    Values are normal; the per-entity ground truth is scaled by ``1 / sqrt(max(1, max_len / 16))`` (``max_len``: the
    entity's longest row), so Poisson margins stay inside the clip as in :func:`make_entities`. Weights and base
    offsets as there: ``integers(1, 17) / 4`` with about 15 % of the rows at exactly 0.0 (``weighted=False``: all
    1.0), offsets ``0.3 sin(arange(n))``.

    ``duplicate_rows``: ``{entity index: ((row, earlier row), ...)}`` -- the row becomes a copy (columns and values)
    of that earlier row of the same entity, which makes the entity's Gram matrix singular."""
    rng = np.random.default_rng(seed)
    duplicate_rows = duplicate_rows or {}
    indptr, cols, vals, ids, z = [0], [], [], [], []
    base = 0
    for k, (n, d, lengths) in enumerate(spec):
        lens = [min(int(lengths[i % len(lengths)]), d) for i in range(n)]
        wt = rng.normal(size=d) * 0.5 / np.sqrt(max(1.0, max(lens, default=0) / 16.0))
        dup = {int(i): int(j) for i, j in duplicate_rows.get(k, ())}
        mine, cursor = [], 0
        for i, ln in enumerate(lens):
            if i in dup:
                assert dup[i] < i, (k, i, dup[i])
                f, v = mine[dup[i]]
            else:
                first = np.arange(cursor, min(cursor + ln, d))
                cursor += first.size
                more = rng.choice(np.setdiff1d(np.arange(d), first), size=ln - first.size, replace=False)
                f = np.sort(np.concatenate([first, more])).astype(np.int64)
                v = rng.normal(size=ln)
            mine.append((f, v))
            cols.append(base + f)
            vals.append(v)
            indptr.append(indptr[-1] + f.size)
            z.append(float(v @ wt[f]) + 0.2 * np.sin(k))
            ids.append(k)
        if cursor < d:
            raise ValueError(f"entity {k}: rows of {sum(lens)} entries cannot cover {d} columns")
        base += d
    r = len(ids)
    x = sp.csr_matrix((np.concatenate(vals) if vals else np.zeros(0), np.concatenate(cols) if cols else
                       np.zeros(0, np.int64), np.array(indptr)), shape=(r, max(base, 1)))
    z = np.array(z)
    if loss == "LOGISTIC":
        y = (rng.random(r) < 1 / (1 + np.exp(-z))).astype(float)
    elif loss == "POISSON":
        y = rng.poisson(np.exp(np.clip(z, -3, 2))).astype(float)
    elif loss == "SQUARED":
        y = z + 0.3 * rng.normal(size=r)
    else:
        raise ValueError(loss)
    w = rng.integers(1, 17, size=r) / 4.0
    w[rng.random(r) < 0.15] = 0.0
    if not weighted:
        w = np.ones(r)
    return GameData(y, {"user": x}, {"userId": np.array(ids)}, offsets=0.3 * np.sin(np.arange(r)), weights=w)


def entity_problems(data, partial=None, rows=None, mult=None, perm_seed=None):
    """Per entity, its problem as the oracle sees it: ``(entity id, global feature ids, TorchGLMData in float64 on the
    CPU)`` over the entity's rows (of ``rows`` only, when given) restricted to the features those rows hold (the
    INDEX_MAP projection), with weights ``data.weights * mult`` and offsets ``data.offsets + partial``.
    ``perm_seed`` shuffles each entity's rows: the same problem, summed in another order."""
    from photon_ml_amd.data.matrix import LabeledData
    from photon_ml_amd.ops.reference import TorchGLMData
    x = data.shards["user"].tocsr()
    ids = data.id_tags["userId"]
    n = data.n_rows
    off = data.offsets if partial is None else data.offsets + np.asarray(partial, dtype=np.float64)
    wts = data.weights if mult is None else data.weights * np.asarray(mult, dtype=np.float64)
    keep = np.ones(n, dtype=bool)
    if rows is not None:
        keep[:] = False
        keep[np.asarray(rows, dtype=np.int64)] = True
    rng = None if perm_seed is None else np.random.default_rng(perm_seed)
    for e in np.unique(ids):
        r = np.nonzero((ids == e) & keep)[0]
        if rng is not None:
            r = r[rng.permutation(len(r))]
        xe = x[r]
        feats = np.unique(xe.indices)
        yield e, feats, TorchGLMData(LabeledData(xe[:, feats], data.response[r], off[r], wts[r]), torch.device("cpu"))


def cpu_tron(data, loss, l2, tol, max_iter, partial=None, w0=None, rows=None, mult=None, perm_seed=None):
    """The oracle: per entity the CPU float64 TRON on :func:`entity_problems`, from ``w0[entity]`` (over the global
    features; zeros without). ``{entity id: (w over the global features, iterations, convergence reason)}``."""
    from photon_ml_amd.function.objective import GLMObjective
    from photon_ml_amd.optimization.tron import TRON
    D = data.shards["user"].shape[1]
    out = {}
    for e, feats, gd in entity_problems(data, partial, rows, mult, perm_seed):
        opt = TRON(tolerance=tol, max_iterations=max_iter, track_state=False)
        start = torch.zeros(len(feats), dtype=torch.float64) if w0 is None else \
            torch.from_numpy(np.ascontiguousarray(w0[e][feats]))
        w, _ = opt.optimize(GLMObjective(loss_of(loss), l2_weight=l2), gd, start)
        full = np.zeros(D)
        full[feats] = w.numpy()
        out[e] = (full, int(opt.current.iter), opt.convergence_reason())
    return out


LBFGS_TASKS = dict(TASKS, HINGE="SMOOTHED_HINGE_LOSS_LINEAR_SVM")


def permuted_rows(data, perm_seed):
    """``data`` with its rows in another order (labels, offsets, weights and ids move with them): every entity's
    problem is the same, its sums run in another order."""
    p = np.random.default_rng(perm_seed).permutation(data.n_rows)
    return GameData(data.response[p], {"user": data.shards["user"].tocsr()[p]}, {"userId": data.id_tags["userId"][p]},
                    offsets=data.offsets[p], weights=data.weights[p])


def lbfgs_coordinate(data, loss, device, l1_weight=0.5, tol=0.0, max_iter=5):
    """A segmented random-effect coordinate under L-BFGS with an L1 weight (the configuration that routes to the
    fused OWL-QN on the GPU), over the rows of ``data``."""
    from photon_ml_amd.algorithm.coordinates import RandomEffectCoordinate
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    cfg = GLMOptimizationConfiguration(OptimizerConfig("LBFGS", max_iter, tol), RegularizationContext("L1"), l1_weight)
    return RandomEffectCoordinate("u", data, RandomEffectDataConfiguration("userId", "user"), cfg, LBFGS_TASKS[loss],
                                  device=device, layout="segmented")


def segmented_offsets(c, data):
    """The base offsets of ``data`` per segmented row of the coordinate ``c`` (what an update without a partial
    score puts into ``seg.o``)."""
    off = torch.from_numpy(np.asarray(data.offsets, dtype=np.float64))
    return off[c.dataset.seg_rows.cpu()].to(c.dataset.seg.y.device)


def entity_coefficients(ds, W):
    """``{entity id: coefficients over the global features}`` of a vector packed like the dataset's segmented
    coefficients (``projection_keys_t``: entity * dim + feature)."""
    keys = ds.projection_keys_t.cpu().numpy()
    ptr = ds.seg.col_ptr.cpu().numpy()
    W = W.detach().cpu().numpy()
    out = {}
    for i, e in enumerate(ds.entity_ids):
        full = np.zeros(ds.dim)
        full[keys[ptr[i]:ptr[i + 1]] % ds.dim] = W[ptr[i]:ptr[i + 1]]
        out[e] = full
    return out


def cpu_owlqn(data, loss, l2, l1, tol, max_iter, m=10, perm_seed=None):
    """The OWL-QN / L-BFGS oracle: ``batched.batched_lbfgs`` in float64 on the CPU over the segmented coordinate of
    ``data`` (what ``RandomEffectCoordinate(device="cpu", layout="segmented")`` runs), cold, with ``m`` history
    pairs. ``perm_seed`` permutes the rows of the data first (:func:`permuted_rows`): the same problems, summed in
    another order. ``{entity id: (w over the global features, iterations, reason code)}``."""
    from photon_ml_amd.optimization.batched import batched_lbfgs
    if perm_seed is not None:
        data = permuted_rows(data, perm_seed)
    c = lbfgs_coordinate(data, loss, "cpu")
    ds = c.dataset
    seg = ds.seg
    seg.o = segmented_offsets(c, data)
    seg._dzz_key = None
    res = batched_lbfgs(seg, c.loss, l2, torch.zeros(int(seg.col_ptr[-1]), dtype=torch.float64), tol, max_iter, m=m,
                        l1=l1)
    W = entity_coefficients(ds, res.W)
    return {e: (W[e], int(res.iters[i]), int(res.reason[i])) for i, e in enumerate(ds.entity_ids)}


def cpu_objective(data, loss, l2, W, partial=None, rows=None, mult=None):
    """``{entity id: f_e(W[entity])}``: the float64 CPU objective of each entity's weighted rows (``GLMObjective
    .value``) at coefficients ``W[entity]`` over the global features."""
    from photon_ml_amd.function.objective import GLMObjective
    obj = GLMObjective(loss_of(loss), l2_weight=l2)
    return {e: float(obj.value(gd, torch.from_numpy(np.ascontiguousarray(np.asarray(W[e], dtype=np.float64)[feats]))))
            for e, feats, gd in entity_problems(data, partial, rows, mult)}


def rel_err(w, w_ref):
    """Largest coefficient difference relative to the reference's largest coefficient."""
    return float(np.abs(np.asarray(w) - np.asarray(w_ref)).max() / max(np.abs(w_ref).max(), 1e-300))


def reference_floor(a, b):
    """The oracle's own rounding floor: the maximum over entities of the relative W difference between two oracle
    runs (results of :func:`cpu_tron`, e.g. with and without ``perm_seed``)."""
    return max(rel_err(b[e][0], a[e][0]) for e in a)


def foreign_model(m, W, loss):
    """``W`` ({entity id: coefficients over the global features}) as a ``RandomEffectModel`` the coordinate has never
    seen (its warm start is then mapped from the model's coefficients), with the entities and shape of ``m``."""
    from photon_ml_amd.models.game import RandomEffectModel
    nz = [np.nonzero(W[e])[0] for e in m.entity_ids]
    keys = np.concatenate([int(i) * m.dim + j for i, j in enumerate(nz)])
    vals = np.concatenate([np.asarray(W[e])[j] for e, j in zip(m.entity_ids, nz)])
    return RandomEffectModel(m.random_effect_type, m.feature_shard_id, TASKS[loss], m.entity_ids, m.dim, keys, vals)


def gpu_fit(data, loss, l2, tol, max_iter, monkeypatch, partial=None, start=None, layout="segmented", config=None):
    """The production coordinate on the GPU: ``({entity: w}, {entity: iterations}, {entity: convergence reason},
    coordinate, model)``. The reasons are the per-entity codes the coordinate hands to its tracker statistics, mapped
    through ``batched.REASON_CODES``. ``partial``: the partial score (added to the data's base offsets);
    ``config``: the ``RandomEffectDataConfiguration`` (default: every row active)."""
    import photon_ml_amd.algorithm.coordinates as co
    from photon_ml_amd.algorithm.coordinates import RandomEffectCoordinate
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration
    from photon_ml_amd.optimization.batched import REASON_CODES
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    cfg = GLMOptimizationConfiguration(OptimizerConfig("TRON", max_iter, tol), RegularizationContext("L2"), l2)
    c = RandomEffectCoordinate("u", data, config or RandomEffectDataConfiguration("userId", "user"), cfg, TASKS[loss],
                               device="cuda", layout=layout)
    got = {}
    if c.dataset.layout == "segmented":
        # per entity of the dataset, in its entity order
        c._defer_stats = lambda it, rc, act, sec: got.update(it=it.cpu().numpy(), rc=rc.cpu().numpy())
        order = np.arange(len(c.dataset.entity_ids))
    else:
        # dense buckets: the statistics arrive bucket after bucket
        real = co.random_effect_tracker_stats

        def spy(it, rc, sec):
            got.update(it=it.cpu().numpy(), rc=rc.cpu().numpy())
            return real(it, rc, sec)
        monkeypatch.setattr(co, "random_effect_tracker_stats", spy)
        order = np.concatenate([bk.entities for bk in c.dataset.buckets])
    ps = None if partial is None else torch.from_numpy(np.asarray(partial, dtype=np.float64))
    m = c.update_model(start if start is not None else c.initialize_model(), ps)
    if hasattr(m, "materialize"):
        m.materialize()
    if c.dataset.layout != "segmented":
        monkeypatch.setattr(co, "random_effect_tracker_stats", real)
    ids = c.dataset.entity_ids
    W = {e: np.asarray(m.coefficients_of(e).means, dtype=np.float64) for e in m.entity_ids}
    its = {ids[k]: int(got["it"][i]) for i, k in enumerate(order)}
    reasons = {ids[k]: REASON_CODES[int(got["rc"][i])] for i, k in enumerate(order)}
    return W, its, reasons, c, m


# The shapes and routes of the fused random-effect solvers (test_re_weighted_parity_gpu.py describes each route).
SHAPES = {
    # name: (sizes, d_pool, nnz_row, dense_pool, seed)
    "rs": ([20] * 3 + [17] * 2 + [32] * 2 + [25] + [48] * 2 + [41] + [64] * 2 + [57], 120, 12, False, 2),
    "rs_big": ([80] * 2 + [100] * 2 + [128] * 2, 150, 0, True, 3),
    "lean": ([90, 120, 150, 75] * 2, 300, 16, False, 9),
    "lean_scalar": ([90, 120, 150, 75] * 2, 300, 6, False, 14),
    "tall": ([150, 90, 200, 65] * 2, 40, 0, True, 7),
    "csr": ([90, 110] * 2, 1800, 24, False, 3),
    "dense_wide": ([80, 95, 70] * 2, 100, 0, True, 4),
    "dense_hess": ([80, 95] * 2, 30, 0, True, 10),
}
ROUTES = {
    # name: (shape, environment, RESIDENT policy, layout)
    "rs": ("rs", {}, "0", "segmented"),
    "rs_big": ("rs_big", {}, "0", "segmented"),
    "lean_quad": ("lean", {"PML_RE_ROW_SPACE": "0"}, "0", "segmented"),
    "lean_scalar": ("lean_scalar", {"PML_RE_ROW_SPACE": "0"}, "0", "segmented"),
    "resident": ("lean", {"PML_RE_ROW_SPACE": "0"}, "force", "segmented"),
    "tall": ("tall", {}, "0", "segmented"),
    "csr": ("csr", {"PML_RE_ROW_SPACE": "0"}, "0", "segmented"),
    "dense_wide": ("dense_wide", {}, "0", "dense"),
    "dense_hess": ("dense_hess", {}, "0", "dense"),
    "pass": ("lean", {"PML_RE_FUSED": "0", "PML_RE_ROW_SPACE": "0"}, "0", "segmented"),
}


def _set_route(route, monkeypatch):
    import photon_ml_amd.optimization.entity_tron as et
    shape, env, resident, layout = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(et, "RESIDENT", resident)
    return shape, layout


def _check_routing(route, c, data):
    """The case reached the kernel it is named after (a case that routes elsewhere fails)."""
    if route in ("dense_wide", "dense_hess"):
        assert c.dataset.layout == "dense" and len(c.dataset.buckets)
        fz = [c._dense_fused(b, bk, 0.0) for b, bk in enumerate(c.dataset.buckets)]
        assert all(f is not None for f in fz)
        if route == "dense_wide":
            assert all(f.quad and f.d > 64 for f in fz)
        else:
            assert all(f.d <= 64 and f.launch[2] for f in fz)
        return
    assert c.dataset.layout == "segmented"
    if route == "pass":
        # the fused solvers are off: no components at all, the block-diagonal passes under batched_tron
        assert getattr(c, "_comps", None) is None and getattr(c, "_rs", None) is None
        return
    rs, fused, sub = c._comps
    assert sub is None
    if route in ("rs", "rs_big"):
        assert fused is None and rs is not None and rs.B == len(c.dataset.entity_ids)
        ns = {cl.n for cl in rs.classes}
        if route == "rs":
            assert ns >= {20, 32, 48, 64} and max(ns) <= 64, ns
        else:
            assert max(ns) > 64, ns
        return
    assert rs is None and fused is not None and fused.B == len(c.dataset.entity_ids)
    if route == "resident":
        assert fused.res is not None and fused.res["n"] > 0
        return
    assert fused.res is None and fused.launches
    if route == "lean_quad":
        assert fused.quad and all(not h and dm <= 1024 for dm, _, h in fused.launches)
    elif route == "lean_scalar":
        assert not fused.quad and all(not h and dm <= 1024 for dm, _, h in fused.launches)
    elif route == "tall":
        assert all(h for _, _, h in fused.launches)
    elif route == "csr":
        x, ids = data.shards["user"].tocsr(), data.id_tags["userId"]
        d_e = [len(np.unique(x[ids == e].indices)) for e in np.unique(ids)]
        assert all(1024 < d <= 2048 for d in d_e), d_e
        assert all(dm > 1024 and not h for dm, _, h in fused.launches)
    else:
        raise AssertionError(route)
