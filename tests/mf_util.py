"""Shared helpers of the matrix-factorization tests (not a test file): two-id data for the three TRON losses, the
coordinate under test, and the per-entity CPU float64 TRON oracle of one half-update.

The oracle is ``optimization/tron.py`` on ``TorchGLMData`` in float64, one entity at a time over the MATERIALISED
features ``Other[code of the row's other-side entity]`` -- the TRON the fused random-effect kernels are tested
against (``tests/re_parity_util.py``)."""
import numpy as np
import scipy.sparse as sp
import torch

from photon_ml_amd.data.game_data import GameData

TASKS = {"LOGISTIC": "LOGISTIC_REGRESSION", "POISSON": "POISSON_REGRESSION", "SQUARED": "LINEAR_REGRESSION"}
LOSSES = tuple(TASKS)


def make_mf_data(sizes, n_cols, k_true, seed, loss="LOGISTIC", weighted=True, shared_col_entities=(), shuffle=True,
                 string_ids=True):
    """Row entity i has ``sizes[i]`` rows; every row's column entity is drawn from ``n_cols`` (each column entity
    occurs at least once when there are enough rows), except that the row entities listed in ``shared_col_entities``
    meet ONE column entity in all their rows. Labels of ``loss`` from a planted rank-``k_true`` interaction scaled so
    that the margins stay inside the Poisson clip (as ``re_parity_util.make_entities``); weights ``integers(1, 17) /
    4`` with about 15 % of the rows at exactly 0 (``weighted=False``: all 1), base offsets ``0.3 sin(arange(n))``.
    ``shuffle``: the rows (and with them the ids) arrive in random order."""
    rng = np.random.default_rng(seed)
    a = np.repeat(np.arange(len(sizes)), sizes)
    n = len(a)
    b = rng.integers(0, n_cols, size=n)
    b[rng.permutation(n)[:min(n, n_cols)]] = np.arange(min(n, n_cols))     # every column entity occurs
    for i in shared_col_entities:
        b[a == i] = i % n_cols
    s = np.sqrt(0.6 / np.sqrt(k_true))
    Ut, Vt = rng.normal(size=(len(sizes), k_true)) * s, rng.normal(size=(n_cols, k_true)) * s
    z = (Ut[a] * Vt[b]).sum(1)
    if loss == "LOGISTIC":
        y = (rng.random(n) < 1 / (1 + np.exp(-3 * z))).astype(float)
    elif loss == "POISSON":
        y = rng.poisson(np.exp(np.clip(z, -3, 2))).astype(float)
    elif loss == "SQUARED":
        y = z + 0.1 * rng.normal(size=n)
    else:
        raise ValueError(loss)
    w = rng.integers(1, 17, size=n) / 4.0
    w[rng.random(n) < 0.15] = 0.0
    if not weighted:
        w = np.ones(n)
    off = 0.3 * np.sin(np.arange(n))
    if shuffle:
        p = rng.permutation(n)
        a, b, y, w = a[p], b[p], y[p], w[p]
    if string_ids:
        ids = {"userId": np.array([f"u{i:05d}" for i in a], dtype=object),
               "itemId": np.array([f"i{j:05d}" for j in b], dtype=object)}
    else:
        ids = {"userId": a, "itemId": b}
    return GameData(y, {"global": sp.csr_matrix(np.ones((n, 1)))}, ids, offsets=off, weights=w)


def mf_coordinate(data, loss, K, device, l2=1.0, tol=1e-8, max_iter=60, **kw):
    from photon_ml_amd.algorithm.matrix_factorization import MatrixFactorizationCoordinate
    from photon_ml_amd.data.random_effect import MatrixFactorizationDataConfiguration
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    cfg = GLMOptimizationConfiguration(OptimizerConfig("TRON", max_iter, tol), RegularizationContext("L2"), l2)
    return MatrixFactorizationCoordinate("mf", data, MatrixFactorizationDataConfiguration("userId", "itemId", K, **kw),
                                         cfg, TASKS[loss], device=device)


def with_config(c, l2, tol, max_iter):
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    c.set_config(GLMOptimizationConfiguration(OptimizerConfig("TRON", max_iter, tol), RegularizationContext("L2"), l2))
    return c


def start_factors(c, seed, scale=0.3):
    """Non-trivial factors (U, V) for a coordinate's entity tables, fp64 on the CPU."""
    rng = np.random.default_rng(seed)
    s = scale / np.sqrt(np.sqrt(c.K))
    return (torch.from_numpy(rng.normal(size=(len(c.row_ids), c.K)) * s),
            torch.from_numpy(rng.normal(size=(len(c.col_ids), c.K)) * s))


def oracle_half(c, side, U, V, loss, l2, tol, max_iter, partial=None, entities=None, perm_seed=None):
    """Per entity of ``side`` (0: rows given V, 1: columns given U) the CPU float64 TRON over the materialised
    features, from the entity's current factors: ``(W [E, K], iterations [E], reason codes [E], margins per row in the
    data's order)``. ``entities``: solve only these (the others keep their start, iterations -1). ``perm_seed`` shuffles
    each entity's rows: the same problem, summed in another order."""
    from photon_ml_amd.data.matrix import LabeledData
    from photon_ml_amd.function.losses import loss_for_task
    from photon_ml_amd.function.objective import GLMObjective
    from photon_ml_amd.ops.reference import TorchGLMData
    from photon_ml_amd.optimization.batched import REASON_CODES
    from photon_ml_amd.optimization.tron import TRON
    data = c.data
    code = {v: k for k, v in REASON_CODES.items()}
    mine, theirs = (c.codes[0], c.codes[1]) if side == 0 else (c.codes[1], c.codes[0])
    mine, theirs = mine.cpu().numpy(), theirs.cpu().numpy()
    W0, other = ((U, V) if side == 0 else (V, U))
    W0, other = W0.detach().cpu().numpy().copy(), other.detach().cpu().numpy()
    off = data.offsets if partial is None else data.offsets + np.asarray(partial, dtype=np.float64)
    W = W0.copy()
    its = np.full(len(W0), -1)
    reasons = np.full(len(W0), -1)
    z = np.zeros(data.n_rows)
    for e in (range(len(W0)) if entities is None else entities):
        r = np.nonzero(mine == e)[0]
        if perm_seed is not None:
            r = r[np.random.default_rng(perm_seed + e).permutation(len(r))]
        F = other[theirs[r]]
        gd = TorchGLMData(LabeledData(sp.csr_matrix(F), data.response[r], off[r], data.weights[r]),
                          torch.device("cpu"))
        opt = TRON(tolerance=tol, max_iterations=max_iter, track_state=False)
        w, _ = opt.optimize(GLMObjective(loss_for_task(TASKS[loss]), l2_weight=l2), gd,
                            torch.from_numpy(np.ascontiguousarray(W0[e])))
        W[e] = w.numpy()
        its[e] = int(opt.current.iter)
        reasons[e] = code[opt.convergence_reason()]
        z[r] = F @ W[e]
    return W, its, reasons, z


def objective(c, U, V, loss, l2, partial=None):
    """sum_r wt_r l(y_r, o_r + u.v) + l2/2 (||U||^2 + ||V||^2) in float64 on the CPU."""
    from photon_ml_amd.function.losses import loss_for_task, weighted
    data = c.data
    U, V = U.detach().cpu(), V.detach().cpu()
    a, b = c.codes[0].cpu().long(), c.codes[1].cpu().long()
    off = data.offsets if partial is None else data.offsets + np.asarray(partial, dtype=np.float64)
    zz = (U[a] * V[b]).sum(1) + torch.from_numpy(off)
    l, _ = loss_for_task(TASKS[loss]).loss_and_dz(zz, torch.from_numpy(data.response))
    return float(weighted(torch.from_numpy(data.weights), l).sum()) + 0.5 * l2 * float(U.square().sum() +
                                                                                         V.square().sum())


def rel_err(w, w_ref):
    """Largest difference relative to the reference's largest magnitude."""
    return float(np.abs(np.asarray(w) - np.asarray(w_ref)).max() / max(np.abs(np.asarray(w_ref)).max(), 1e-300))


# ---- the half-update parity cases shared by the CPU and GPU tests ------------------------------------------------
# Row entities of 1, 15, 16, 17, 32, 33 and 70 rows (the staging block of 16 and the two-block pipeline of
# mf_tron_kernel) and one of 24 rows that meets a single column entity in all of them (every gather hits one address).
HALF_SIZES = [1, 15, 16, 17, 32, 33, 70, 24]
HALF_SHARED = (7,)
HALF_COLS = 12
# Two regimes, as tests/test_re_parity_gpu.py. ITERATION-LIMITED (tolerance 0, 4 iterations): only rounding may
# separate two implementations, so the problems must not reach their rounding floor within the 4 iterations -- once
# an entity sits at its optimum to machine precision, whether a further step is "accepted" is decided by the last bit
# of f and two correct implementations (the CPU batched TRON and the per-entity TRON already) disagree. With K <= 32
# coefficients and entities of one row that happens at once at unit scale (a one-row squared-loss entity is solved
# exactly by the first Newton step), so this regime runs on features of scale 0.02 with lambda = 0.005: every
# entity's curvature stays below 1/85, the Newton step lies outside the trust region (delta_0 = ||g||, growing at most
# 4 x per iteration: 1 + 4 + 16 + 64 = 85) and all 4 iterations are full trust-region steps on both sides.
# CONVERGED (1e-8, 60) runs at unit scale with lambda = 1.
LIMITED = dict(scale=0.02, l2=0.005, tol=0.0, max_iter=4, bound=1e-9)
CONVERGED = dict(scale=0.3, l2=1.0, tol=1e-8, max_iter=60, bound=1e-6)
REGIMES = {"limited": LIMITED, "converged": CONVERGED}


def half_case(K, loss, seed):
    """The data of one parity case and, per regime, its reference: the start (U, V), the partial score and the
    oracle's row half and column half, each from that start (the column half of the limited regime from the row half's
    result would see features grown by four trust-region steps, no longer of small curvature)."""
    data = make_mf_data(HALF_SIZES, HALF_COLS, 3, seed=seed, loss=loss, shared_col_entities=HALF_SHARED)
    c = mf_coordinate(data, loss, K, "cpu")
    partial = 0.3 * np.cos(np.arange(data.n_rows))
    ref = {}
    for name, r in REGIMES.items():
        U, V = start_factors(c, seed + 1, r["scale"])
        row = oracle_half(c, 0, U, V, loss, r["l2"], r["tol"], r["max_iter"], partial)
        col = oracle_half(c, 1, U, V, loss, r["l2"], r["tol"], r["max_iter"], partial)
        ref[name] = (U, V, row, col)
    return data, partial, ref


def half_mismatches(c, partial, ref, loss=None, floor_seed=None):
    """Run both halves of both regimes on coordinate ``c`` from the reference's inputs; the list of disagreements with
    the oracle (empty: parity). ``floor_seed``: compare the oracle with ITSELF on permuted rows instead (how stable
    the reference's own counts are)."""
    out = []
    ps = torch.from_numpy(partial)
    for name, r in REGIMES.items():
        U, V, row, col = ref[name]
        with_config(c, r["l2"], r["tol"], r["max_iter"])
        for side, (u, want) in enumerate(((U, row), (U, col))):
            if floor_seed is None:
                W, z, it, rs = c.solve_half(side, u, V, ps)
                W, z, it, rs = W.cpu().numpy(), z.cpu().numpy(), it.cpu().numpy(), rs.cpu().numpy()
            else:
                W, it, rs, z = oracle_half(c, side, u, V, loss, r["l2"], r["tol"], r["max_iter"], partial,
                                           perm_seed=floor_seed)
            W_ref, it_ref, rs_ref, z_ref = want
            tag = (name, "row" if side == 0 else "column")
            if not np.array_equal(it, it_ref):
                out.append(tag + ("iterations", it.tolist(), it_ref.tolist()))
            if not np.array_equal(rs, rs_ref):
                out.append(tag + ("reasons", rs.tolist(), rs_ref.tolist()))
            if name == "limited" and not np.all(it_ref == r["max_iter"]):
                out.append(tag + ("the oracle did not run all iterations", it_ref.tolist()))
            if not rel_err(W, W_ref) < r["bound"]:
                out.append(tag + ("W", rel_err(W, W_ref)))
            if not rel_err(z, z_ref) < r["bound"]:
                out.append(tag + ("margins", rel_err(z, z_ref)))
    return out
