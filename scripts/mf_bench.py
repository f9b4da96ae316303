"""A/B of the two device routes of a matrix-factorization coordinate update (``profiles/mf_fused.md``).

``python scripts/mf_bench.py [ROW_ENTITIES COL_ENTITIES MEAN_ROWS ROUNDS OUT.json]`` on one GPU: power-law row entities
(Pareto 1.3 sizes capped at 20000 rows, as ``bench_game.py --config game5pl`` draws them; default 200,000 row entities
x 20,000 column entities, mean 50 rows = 10M rows), logistic labels from a planted rank-4 interaction, K = 16 and
K = 32. One timed call is one ``update_model`` with ``alternations=1`` (a row half and a column half) from the seeded
start, with a device synchronisation on both sides. The fused route (``PML_MF_FUSED=1``: ``mf_tron_kernel``) and the
materialised route (``PML_MF_FUSED=0``: ``re_tron_tall_kernel`` over a copy of the gathered rows) alternate inside every
round; one untimed round first. Row passes and TRON iterations per entity are recorded for both routes, so a time
difference can be told from an iteration difference. Needs a GPU: there is no CPU fall-back."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def power_law_sizes(n_entities: int, mean_rows: float, rng, alpha: float = 1.3, max_rows: int = 20000):
    u = rng.random(n_entities)
    target = n_entities * mean_rows
    xm = float(mean_rows) * (alpha - 1) / alpha
    for _ in range(30):          # scale so that the capped Pareto sizes have the requested mean
        cnt = np.minimum(np.ceil(xm * u ** (-1.0 / alpha)), max_rows).astype(np.int64)
        tot = int(cnt.sum())
        if abs(tot - target) <= 0.001 * target:
            break
        xm *= target / tot
    return cnt


def make_data(n_row_ent: int, n_col_ent: int, mean_rows: float, seed: int = 1):
    from photon_ml_amd.data.game_data import GameData
    rng = np.random.default_rng(seed)
    cnt = power_law_sizes(n_row_ent, mean_rows, rng)
    a = rng.permutation(np.repeat(np.arange(n_row_ent, dtype=np.int64), cnt))
    b = rng.integers(0, n_col_ent, size=len(a))
    s = np.sqrt(1.0 / 2.0)
    z = ((rng.normal(size=(n_row_ent, 4)) * s)[a] * (rng.normal(size=(n_col_ent, 4)) * s)[b]).sum(1)
    y = (rng.random(len(a)) < 1 / (1 + np.exp(-z))).astype(np.float64)
    return GameData(y, {}, {"rowId": a, "colId": b}), cnt


def main(argv):
    n_row_ent = int(argv[1]) if len(argv) > 1 else 200_000
    n_col_ent = int(argv[2]) if len(argv) > 2 else 20_000
    mean_rows = float(argv[3]) if len(argv) > 3 else 50.0
    rounds = int(argv[4]) if len(argv) > 4 else 5
    out_path = argv[5] if len(argv) > 5 else None
    if not torch.cuda.is_available():
        raise SystemExit("mf_bench needs a GPU")
    from photon_ml_amd.algorithm.matrix_factorization import MatrixFactorizationCoordinate
    from photon_ml_amd.data.random_effect import MatrixFactorizationDataConfiguration
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    t0 = time.time()
    data, cnt = make_data(n_row_ent, n_col_ent, mean_rows)
    print(f"data: {data.n_rows} rows, {n_row_ent} x {n_col_ent} entities, row sizes {cnt.min()} .. {cnt.max()} "
          f"({time.time() - t0:.1f} s)", flush=True)
    cfg = GLMOptimizationConfiguration(OptimizerConfig("TRON", 10, 1e-6), RegularizationContext("L2"), 1.0)
    results = []
    for K in (16, 32):
        t0 = time.time()
        c = MatrixFactorizationCoordinate("mf", data, MatrixFactorizationDataConfiguration("rowId", "colId", K), cfg,
                                          "LOGISTIC_REGRESSION", device="cuda")
        start = c.initialize_model()
        print(f"K={K}: layout built in {time.time() - t0:.1f} s", flush=True)
        n_ent = n_row_ent + n_col_ent
        times = {"1": [], "0": []}
        stats, models = {}, {}
        for r in range(rounds + 1):
            for route in ("1", "0"):
                os.environ["PML_MF_FUSED"] = route
                torch.cuda.synchronize()
                t = time.perf_counter()
                m = c.update_model(start, None)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t) * 1e3
                if r == 0:
                    p, it = c.last_passes
                    stats[route] = (float(p) / n_ent, float(it) / n_ent)
                    models[route] = (m.U.clone(), m.V.clone(), [h[0].clone() for h in c._half_raw])
                else:
                    times[route].append(dt)
        fu, fv, fit = models["1"]
        mu, mv, mit = models["0"]
        same = float(sum((a == b).sum() for a, b in zip(fit, mit))) / n_ent
        diff = max(float((fu - mu).abs().max()), float((fv - mv).abs().max()))
        scale = max(float(mu.abs().max()), float(mv.abs().max()))
        for route, name in (("1", "fused"), ("0", "materialised")):
            ts = times[route]
            results.append({"K": K, "route": name, "median_ms": statistics.median(ts), "min_ms": min(ts),
                            "max_ms": max(ts), "row_passes_per_entity": stats[route][0],
                            "tron_iterations_per_entity": stats[route][1], "rows": data.n_rows,
                            "row_entities": n_row_ent, "col_entities": n_col_ent, "rounds": rounds,
                            "equal_iteration_share": same, "max_abs_factor_diff": diff, "max_abs_factor": scale})
            print(json.dumps(results[-1]), flush=True)
        del c, models
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main(sys.argv)
