"""One random-effect update under STANDARDIZATION with ``shift_routes="csr"`` against ``"auto"``, next to the same
coordinate without normalization (``profiles/re_shift_routes.md``).

Two synthetic coordinates: ``wide`` (game5pl-like: many entities of 20 rows x ``--wide-d`` coefficients) and ``tall``
(game5tall-like: entities of ``--tall-n`` rows x 32 coefficients). Every entity draws its features from one common
pool, so a STANDARDIZATION context built from the shard is well conditioned. The three settings are timed alternately
(``--rounds`` rounds of one warm-up update and ``--reps`` timed updates each, from a fresh start model every time);
the median update time per setting and the routing dictionaries are printed as one JSON line per workload."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def make(n_ent, n, d, nnz_row, seed):
    """``n_ent`` entities of ``n`` rows over the SAME ``d - 1`` features plus an intercept (feature d - 1)."""
    rng = np.random.default_rng(seed)
    N = n_ent * n
    step = max(1, (d - 1) // (nnz_row - 1) - 1)                  # (nnz_row - 1) step < d - 1: distinct columns per row
    cols = (rng.integers(0, d - 1, size=(N, 1)) + np.arange(nnz_row - 1)[None, :] * step) % (d - 1)
    mean, scale = rng.normal(size=d - 1) * 0.7, rng.uniform(0.6, 1.6, size=d - 1)
    vals = mean[cols] + scale[cols] * rng.normal(size=cols.shape)
    cols = np.concatenate([cols, np.full((N, 1), d - 1)], 1)
    vals = np.concatenate([vals, np.ones((N, 1))], 1)
    x = sp.csr_matrix((vals.ravel(), cols.ravel(), np.arange(N + 1) * nnz_row), shape=(N, d))
    x.sort_indices()
    ent = np.repeat(np.arange(n_ent), n)
    z = 0.3 * rng.normal(size=N)
    y = (rng.random(N) < 1 / (1 + np.exp(-z))).astype(float)
    from photon_ml_amd.data.game_data import GameData
    return GameData(y, {"user": x}, {"userId": ent}, np.zeros(N), np.ones(N)), d - 1


def coordinate(data, ctx, routes, device):
    from photon_ml_amd.algorithm.coordinates import RandomEffectCoordinate
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration
    from photon_ml_amd.optimization.config import GLMOptimizationConfiguration, OptimizerConfig, RegularizationContext
    cfg = GLMOptimizationConfiguration(OptimizerConfig("TRON", 20, 1e-5), RegularizationContext("L2"), 1.0)
    kw = {} if ctx is None else {"normalization": ctx, "shift_routes": routes}
    return RandomEffectCoordinate("u", data, RandomEffectDataConfiguration("userId", "user"), cfg,
                                  "LOGISTIC_REGRESSION", device=device, layout="segmented", **kw)


def update_ms(c):
    sync = torch.cuda.synchronize if c.device.type == "cuda" else (lambda: None)
    sync()
    t = time.perf_counter()
    m = c.update_model(c.initialize_model(), None)
    c.score(m)
    sync()
    return (time.perf_counter() - t) * 1e3


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--wide-entities", type=int, default=20000)
    p.add_argument("--wide-d", type=int, default=1001)
    p.add_argument("--tall-entities", type=int, default=4000)
    p.add_argument("--tall-n", type=int, default=300)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--device", default="cuda")
    a = p.parse_args()
    from photon_ml_amd.normalization.context import NormalizationContext
    from photon_ml_amd.stat.summary import BasicStatisticalSummary
    for name, (n_ent, n, d, nnz) in {"wide": (a.wide_entities, 20, a.wide_d, 51),
                                     "tall": (a.tall_entities, a.tall_n, 32, 20)}.items():
        data, icpt = make(n_ent, n, d, nnz, seed=7)
        ctx = NormalizationContext.build("STANDARDIZATION", BasicStatisticalSummary.compute(data.shards["user"]), icpt)
        coords = {"none": coordinate(data, None, None, a.device), "csr": coordinate(data, ctx, "csr", a.device),
                  "auto": coordinate(data, ctx, "auto", a.device)}
        ms = {k: [] for k in coords}
        for _ in range(a.rounds):                         # alternated: none, csr, auto, none, csr, auto, ...
            for k, c in coords.items():
                update_ms(c)                              # warm-up of this setting's launches
                ms[k] += [update_ms(c) for _ in range(a.reps)]
        print(json.dumps({"workload": name, "entities": n_ent, "rows": n, "coefficients": d,
                          "update_ms_median": {k: round(float(np.median(v)), 3) for k, v in ms.items()},
                          "update_ms_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                          "routing": {k: c.solver_routing() for k, c in coords.items()}}), flush=True)


if __name__ == "__main__":
    main()
