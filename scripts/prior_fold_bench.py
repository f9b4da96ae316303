"""Cost of the prior fold (incremental training) in the random-effect dataset build, on a game5pl-like shard.

Generates the random-effect shard of ``bench_game.py --config game5pl`` at ``--entities`` entities (power-law entity
sizes of mean 20 rows, 1000-feature pools + intercept, 50 entries per row; the full config has 1.25M entities per GPU),
builds the segmented device dataset without a prior and with a prior that covers EVERY projected coefficient (the most
lookups the fold can meet), and prints the build phases of both (device-complete: ``PML_SYNC_TIMED=1``) plus the fold
kernel alone (``prior_fold_kernel``, device events, median of ``--reps`` launches on a fresh copy of the values).

usage: python scripts/prior_fold_bench.py [--entities N] [--reps R] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("PML_SYNC_TIMED", "1")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch


def build(data, prior):
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration, RandomEffectDataset
    from photon_ml_amd.utils.timing import TIMELINE
    TIMELINE.clear()
    torch.cuda.synchronize()
    ds = RandomEffectDataset(data, RandomEffectDataConfiguration("entityId", "entity"), "cuda", prior=prior)
    torch.cuda.synchronize()
    return ds, {k: round(sum(v), 4) for k, v in TIMELINE.items() if k.startswith("RE ")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=250_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    from photon_ml_amd.data.synthetic import generate_game_bench_data_device
    from photon_ml_amd.models.game import RandomEffectModel
    from photon_ml_amd.ops.native import prior_fold
    data = generate_game_bench_data_device(a.entities, 20, re_dim=1000, re_nnz=50, fe_dim=1000, fe_nnz=2,
                                           int_ids=True, sizes="powerlaw")
    build(data, None)                                                 # warm-up: first launches, allocator
    ds, plain = build(data, None)
    g = torch.Generator(device="cuda").manual_seed(1)
    keys = ds.projection_keys_t
    mu = torch.randn(keys.numel(), generator=g, device="cuda", dtype=torch.float64)
    var = torch.rand(keys.numel(), generator=g, device="cuda", dtype=torch.float64) * 3.75 + 0.25
    prior = RandomEffectModel("entityId", "entity", "LOGISTIC_REGRESSION", ds.entity_ids, ds.dim, keys, mu, var)
    nip, pos, val = ds._seg_csr
    nnz, rows, d_total = int(val.numel()), int(nip.numel()) - 1, int(ds.d_total)
    del ds
    ds, folded = build(data, prior)
    nip, pos, val = ds._seg_csr
    sigma = ds.prior.sigma
    ms = []
    for _ in range(a.reps):
        v = val.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        prior_fold(nip, pos, v, mu, sigma)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    kernel_ms = statistics.median(ms)
    traffic = nnz * (8 + 8 + 8 + 8 + 8) + rows * 16          # pos, val read, mu + sigma gathers, val write; nip, m
    out = {"entities": a.entities, "rows": rows, "nnz": nnz, "coefficients": d_total,
           "build_phases_s": {"no_prior": plain, "prior": folded},
           "fold_kernel_ms": round(kernel_ms, 3), "fold_kernel_GBps": round(traffic / kernel_ms / 1e6, 1)}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=2)


if __name__ == "__main__":
    main()
