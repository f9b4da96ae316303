"""Per-feature statistics on the device, measured (profiles/colstats_device.md).

For each precision: a synthetic tiled shard (data/synthetic.py, the bench generator) and
  * ``DeviceGLMData.column_stats`` — the HIP column-statistics pass (4 sum launches + combine, 1 max/min launch
    per chunk), median of ``--reps`` calls, and whether two calls give the same bits;
  * one ``rmatvec`` (the transpose pass of a training step) on the same shard, for scale;
and ``BasicStatisticalSummary.compute`` (scipy, host) on a ``--host-nnz`` matrix. One JSON line per measurement.
The torch scatter-reduction path that ``from_device`` ran on a GPU before the kernels existed is NOT timed here:
on the generator's shards (an intercept in every row) it did not finish (profiles/colstats_device.md).

    python scripts/colstats_bench.py --rows 16000000 --features 1000000 --nnz 100 --precisions f64,bf16
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    """Median / min / max wall time in ms of ``fn`` (device-synchronised), after one untimed call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": reps}


def emit(rec):
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--features", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=100)
    ap.add_argument("--precisions", default="f64,bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-nnz", type=int, default=30_000_000)
    a = ap.parse_args()
    from photon_ml_amd.data.synthetic import generate_device_shard
    from photon_ml_amd.stat.summary import BasicStatisticalSummary
    dev = torch.device("cuda")
    for prec in a.precisions.split(","):
        data, _ = generate_device_shard(a.rows, a.features, a.nnz, dev, prec)
        torch.cuda.synchronize()
        shape = {"precision": prec, "rows": a.rows, "features": a.features, "nnz": a.rows * a.nnz,
                 "chunks": len(data.csc), "cbits": data.csc[0].cbits}
        first = data.column_stats()
        again = data.column_stats()
        emit({**shape, "what": "column_stats", **timed(data.column_stats, a.reps),
              "bitwise_repeatable": all(torch.equal(x, y) for x, y in zip(first, again))})
        r = torch.ones(a.rows, dtype=torch.float64, device=dev)
        emit({**shape, "what": "rmatvec", **timed(lambda: data.rmatvec(r), a.reps)})
        del data, first, again, r
        torch.cuda.empty_cache()
    if a.host_nnz:
        rng = np.random.default_rng(0)
        n = a.host_nnz // a.nnz
        x = sp.csr_matrix((rng.random(n * a.nnz) + 0.5, rng.integers(0, a.features, size=n * a.nnz),
                           np.arange(n + 1) * a.nnz), shape=(n, a.features))
        t = time.perf_counter()
        BasicStatisticalSummary.compute(x)
        s = time.perf_counter() - t
        emit({"what": "BasicStatisticalSummary.compute (host)", "rows": n, "features": a.features, "nnz": x.nnz,
              "s": s, "ns_per_nnz": s / x.nnz * 1e9})


if __name__ == "__main__":
    main()
