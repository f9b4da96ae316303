"""Benchmark of the FULL coefficient variances diag(H_e^-1) of a segmented random-effect coordinate
(``optimization/variance.py``: ``SegmentedFullVariance`` = the HIP routes + the batched torch fallback).

Samples (seeded, generated on the device; 1000- or 100-feature pools + intercept per entity, 51 entries per row with
distinct sorted columns and N(0,1) values, curvature of a logistic loss):

* ``wide``   game5pl-like wide entities: 5 .. 64 rows (Pareto 1.3), d_e = 1001 -> the row-space route;
* ``fused``  the entity sizes of ``scripts/re_fused_bench.py`` (65 .. 20000 rows, Pareto 1.3) with d_e = 1001: rows
             <= 128 take the row-space route, 129 .. 1000 rows the blocked row-space route and more rows the blocked
             primal route (with ``--no-blocked`` all of m = min(n_e, d_e) > 128 takes the torch fallback);
* ``tall``   the same sizes with 100-feature pools (d_e = 101 <= n_e) -> the primal route.

For every sample: the FULL variance (all routes, as the coordinate runs it), the same entities through the batched
torch fallback alone, and the SIMPLE pass ``1 / (hdiag + EPSILON)`` (one squared transpose pass of the GLM kernels);
per size class the HIP time (device events inside one ``compute``) against the torch fallback on the same entities.
Times are medians over ``--reps`` runs after a warm-up, each ending in a device synchronise; the HIP and torch
results are compared before anything is timed.

usage: python scripts/full_variance_bench.py [--wide N] [--fused N] [--tall N] [--reps R] [--class-cap N]
                                             [--no-blocked] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

NNZ = 51


def make_sample(n_e: torch.Tensor, pool: int, seed: int, dev):
    """Block-diagonal CSR of entities with ``n_e`` rows each over ``pool`` features + intercept."""
    g = torch.Generator(device=dev).manual_seed(seed)
    E, d = int(n_e.numel()), pool + 1
    N = int(n_e.sum())
    row_ptr = torch.zeros(E + 1, dtype=torch.int64, device=dev)
    torch.cumsum(n_e, 0, out=row_ptr[1:])
    col_ptr = torch.arange(E + 1, dtype=torch.int64, device=dev) * d
    # 50 distinct pool features per row: a + k s mod pool with s coprime to the pool size (1000 or 100)
    strides = torch.tensor([s for s in range(1, pool // 5) if s % 2 and s % 5], device=dev)
    a = torch.randint(0, pool, (N, 1), generator=g, device=dev)
    s_ = strides[torch.randint(0, strides.numel(), (N, 1), generator=g, device=dev)]
    cols = (a + torch.arange(NNZ - 1, device=dev)[None, :] * s_) % pool
    cols, _ = torch.sort(cols, dim=1)
    cols = torch.cat([cols, torch.full((N, 1), pool, device=dev)], 1)
    ent = torch.repeat_interleave(torch.arange(E, device=dev), n_e, output_size=N)
    pos = (cols + col_ptr[ent][:, None]).reshape(-1)
    val = torch.randn(N * NNZ, generator=g, device=dev, dtype=torch.float64)
    val.view(N, NNZ)[:, -1] = 1.0
    nip = torch.arange(N + 1, dtype=torch.int64, device=dev) * NNZ
    z = torch.randn(N, generator=g, device=dev, dtype=torch.float64)
    p = torch.sigmoid(z)
    c = p * (1 - p)                                       # unit weights x logistic l''
    return row_ptr, col_ptr, (nip, pos, val), c


def pareto_sizes(E: int, lo: float, hi: int, seed: int, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    u = torch.rand(E, generator=g, device=dev, dtype=torch.float64)
    return torch.clamp(torch.ceil(lo * u ** (-1.0 / 1.3)), max=hi).to(torch.int64)


def timed(fn, reps: int):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def bench_sample(name: str, n_e: torch.Tensor, pool: int, lam: float, reps: int, class_cap: int, dev,
                 blocked: bool = True) -> dict:
    from photon_ml_amd.constants import EPSILON
    from photon_ml_amd.ops.device import DeviceGLMData
    from photon_ml_amd.ops.native import VAR_BLOCKED_MMAX, VAR_MMAX, VAR_PRIMAL
    from photon_ml_amd.optimization.variance import SegmentedFullVariance, segmented_full_variance
    row_ptr, col_ptr, csr, c = make_sample(n_e, pool, 1, dev)
    E, N = int(n_e.numel()), int(n_e.sum())
    print(f"[{name}] {E} entities, {N} rows, {N * NNZ / 1e6:.1f}M non-zeros, n_e {int(n_e.min())}..{int(n_e.max())}, "
          f"d_e {pool + 1}", flush=True)
    t0 = time.perf_counter()
    plan = SegmentedFullVariance(row_ptr, col_ptr, csr, blocked_mmax=VAR_BLOCKED_MMAX if blocked else 0)
    torch.cuda.synchronize()
    out = {"sample": name, "entities": E, "rows": N, "d_e": pool + 1, "lambda": lam, "routes": plan.counts,
           "plan_build_ms": (time.perf_counter() - t0) * 1e3}
    var, stats = plan.compute(c, lam)
    out["routes"] = stats
    # correctness first: the HIP routes against the torch definition on (a sample of) their entities
    # (the LDS-resident classes and the blocked classes each on up to 256 of their entities)
    for key, cls in (("max_rel_err_vs_torch", plan.classes), ("blocked_max_rel_err_vs_torch", plan.blocked_classes)):
        hip_ents = torch.cat([e for _, _, e, *_ in cls]) if cls else torch.zeros(0, dtype=torch.int64, device=dev)
        chk = hip_ents[torch.linspace(0, max(hip_ents.numel() - 1, 0), min(hip_ents.numel(), 256), device=dev).long()]
        if chk.numel():
            ref, _ = segmented_full_variance(row_ptr, col_ptr, csr, c, lam, ents=chk)
            m = ref != 0
            out[key] = float(((var[m] - ref[m]).abs() / ref[m].abs()).max())
    out["full_ms"], out["full_min_ms"] = timed(lambda: plan.compute(c, lam), reps)
    # per class: HIP (events inside one compute; median over reps) vs torch on the same entities (capped)
    per = {}
    for _ in range(reps):
        tm = []
        plan.compute(c, lam, timings=tm)
        torch.cuda.synchronize()
        for route, n, b, e0, e1 in tm:
            per.setdefault((route, n, b), []).append(e0.elapsed_time(e1))
    classes = []
    for (route, n, e, *_) in plan.classes + plan.blocked_classes:
        hip_ms = statistics.median(per[(route, n, int(e.numel()))])
        sub = e[:class_cap]
        t_ms, _ = timed(lambda: segmented_full_variance(row_ptr, col_ptr, csr, c, lam, ents=sub), max(1, reps // 2))
        label = ("blocked_" if n > VAR_MMAX else "") + ("primal" if route == VAR_PRIMAL else "row_space")
        classes.append({"route": label, "n": n, "entities": int(e.numel()),
                        "hip_ms": hip_ms, "hip_us_per_entity": 1e3 * hip_ms / e.numel(),
                        "torch_entities": int(sub.numel()), "torch_ms": t_ms,
                        "torch_us_per_entity": 1e3 * t_ms / sub.numel()})
        print(f"[{name}] {classes[-1]}", flush=True)
    out["classes"] = classes
    # the whole sample through the torch fallback alone (entities capped per call for the time budget)
    live = torch.nonzero(n_e > 0).squeeze(1)
    fb = live if live.numel() <= 4 * class_cap else live[torch.randperm(live.numel(), device=dev)[:4 * class_cap]]
    t_ms, _ = timed(lambda: segmented_full_variance(row_ptr, col_ptr, csr, c, lam, ents=fb), 1)
    out["torch_all_entities"] = int(fb.numel())
    out["torch_all_ms"] = t_ms
    out["torch_all_ms_scaled_to_sample"] = t_ms * live.numel() / max(fb.numel(), 1)
    # SIMPLE: one squared transpose pass of the GLM kernels + the reciprocal
    y = torch.zeros(N, dtype=torch.float64, device=dev)
    glm = DeviceGLMData.from_device_csr(csr[0], csr[1], csr[2], y, y.clone(), torch.ones_like(y), int(col_ptr[-1]), dev,
                                        "f64", col_windows=True)
    out["simple_ms"], _ = timed(lambda: 1.0 / (glm.rmatvec(c, square=True) + lam + EPSILON), reps)
    print(f"[{name}] FULL {out['full_ms']:.2f} ms (routes {stats}); torch alone {out['torch_all_ms']:.1f} ms on "
          f"{fb.numel()} entities; SIMPLE {out['simple_ms']:.2f} ms", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--wide", type=int, default=20000)
    ap.add_argument("--fused", type=int, default=43000)
    ap.add_argument("--tall", type=int, default=43000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--class-cap", type=int, default=512, help="entities per class timed through the torch fallback")
    ap.add_argument("--lam", type=float, default=1.0)
    ap.add_argument("--no-blocked", action="store_true",
                    help="leave the blocked route (128 < m <= 1024) off: those entities take the torch fallback")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("full_variance_bench needs a GPU: nothing here is measured on the host")
    dev = torch.device("cuda")
    res = []
    if a.wide:
        res.append(bench_sample("wide", pareto_sizes(a.wide, 5.0, 64, 2, dev), 1000, a.lam, a.reps, a.class_cap, dev,
                                not a.no_blocked))
    if a.fused:
        res.append(bench_sample("fused", pareto_sizes(a.fused, 65.0, 20000, 1, dev), 1000, a.lam, a.reps,
                                a.class_cap, dev, not a.no_blocked))
    if a.tall:
        res.append(bench_sample("tall", pareto_sizes(a.tall, 65.0, 20000, 1, dev), 100, a.lam, a.reps, a.class_cap,
                                dev, not a.no_blocked))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
