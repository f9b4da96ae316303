"""Microbenchmark of the fused per-entity OWL-QN (``re_lbfgs_csr_kernel``) against the block-diagonal pass path
(``batched_lbfgs`` over the tiled GLM kernels: the route of an L1 random effect with ``PML_RE_FUSED=0``) on the
game5pl-like entity set of ``scripts/re_fused_bench.py``: power-law sizes (Pareto 1.3, 65 .. 20000 rows),
1000-feature pools + intercept, 50 distinct pool features per row, logistic labels.

One L1 (lambda = 1) update, both routes in the same process on the same data from the same warm start (a 3-iteration
OWL-QN solve from zero), 20 iterations at tolerance 1e-7. Prints the median of 5 timed runs after 2 warm-ups per
route, the iteration histogram, the row passes per entity, the resident workgroups per LDS class and how far the
two routes' solutions are apart.

usage: python scripts/re_owlqn_bench.py [n_entities=43000] [routes, e.g. fused,pass]
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from photon_ml_amd.function.losses import LOGISTIC
from photon_ml_amd.ops.native import RE_LBFGS_M, re_lbfgs_csr, re_lbfgs_grid

E = int(sys.argv[1]) if len(sys.argv) > 1 else 43_000
ROUTES = sys.argv[2].split(",") if len(sys.argv) > 2 else ["fused", "pass"]
L1, L2, TOL, MAX_ITER, DMAX = 1.0, 0.0, 1e-7, 20, 1024
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(1)
u = torch.rand(E, generator=g, device=dev, dtype=torch.float64)
n_e = torch.clamp(torch.ceil(65.0 * u ** (-1.0 / 1.3)), max=20000).to(torch.int64)
N = int(n_e.sum())
NNZ = 51
d = 1001
row_ptr = torch.zeros(E + 1, dtype=torch.int64, device=dev)
torch.cumsum(n_e, 0, out=row_ptr[1:])
col_ptr = torch.arange(E + 1, dtype=torch.int64, device=dev) * d
# 50 distinct pool features per row: a + k s mod 1000 with s coprime to 1000
strides = torch.tensor([s for s in range(1, 200) if s % 2 and s % 5], device=dev)
a = torch.randint(0, d - 1, (N, 1), generator=g, device=dev)
s_ = strides[torch.randint(0, strides.numel(), (N, 1), generator=g, device=dev)]
cols = (a + torch.arange(NNZ - 1, device=dev)[None, :] * s_) % (d - 1)
cols, _ = torch.sort(cols, dim=1)
lcol = torch.cat([cols, torch.full((N, 1), d - 1, device=dev)], 1).reshape(-1).to(torch.int16)
del cols, a, s_
val = torch.randn(N * NNZ, generator=g, device=dev, dtype=torch.float64)
val.view(N, NNZ)[:, -1] = 1.0
nip = torch.arange(N + 1, dtype=torch.int64, device=dev) * NNZ
y = (torch.rand(N, generator=g, device=dev) < 0.4).double()
off = torch.zeros(N, dtype=torch.float64, device=dev)
wt = torch.ones(N, dtype=torch.float64, device=dev)
print(f"{E} entities, {N} rows, {N * NNZ / 1e6:.0f}M non-zeros, max n_e {int(n_e.max())}", flush=True)

order = torch.argsort(n_e, descending=True).to(torch.int32)
grids = {dm: re_lbfgs_grid(dm) for dm in (256, 512, 1024, 2048)}
grid = min(grids[DMAX], E)
scr = torch.empty(4 * N, dtype=torch.float64, device=dev)
hist = torch.empty(grid * 2 * RE_LBFGS_M * DMAX, dtype=torch.float64, device=dev)
ticket = torch.zeros(1, dtype=torch.int32, device=dev)
f = torch.empty(E, dtype=torch.float64, device=dev)
it = torch.empty(E, dtype=torch.int32, device=dev)
rc = torch.empty(E, dtype=torch.int32, device=dev)
z = torch.empty(N, dtype=torch.float64, device=dev)
npass = torch.zeros(E, dtype=torch.int32, device=dev)


def fused(W0, max_iter, np_=None):
    W = W0.clone()
    re_lbfgs_csr(order, row_ptr, col_ptr, nip, lcol, val, y, off, wt, scr, W, f, it, rc, z, 0, L2, L1, TOL, max_iter,
                 DMAX, hist, ticket, grid, npass=np_)
    return W


W_warm = fused(torch.zeros(E * d, dtype=torch.float64, device=dev), 3)
torch.cuda.synchronize()


def timed(call, warmups=2, reps=5):
    out, ts = None, []
    for k in range(warmups + reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        if k >= warmups:
            ts.append((time.perf_counter() - t) * 1e3)
    return out, statistics.median(ts), ts


res = {"entities": E, "rows": N, "nnz": N * NNZ, "resident_workgroups": grids, "grid": grid}
sol = {}
if "fused" in ROUTES:
    W, ms, ts = timed(lambda: fused(W_warm, MAX_ITER))
    fused(W_warm, MAX_ITER, npass)
    torch.cuda.synchronize()
    sol["fused"] = (W, it.to(torch.int64).clone())
    res["fused_ms"] = ms
    res["fused_ms_runs"] = ts
    res["fused_iterations_hist"] = torch.bincount(it.to(torch.int64), minlength=MAX_ITER + 1).tolist()
    res["fused_reasons_hist"] = torch.bincount(rc.to(torch.int64), minlength=5).tolist()
    npd = npass.double()
    res["npass"] = {"mean": float(npd.mean()), "median": float(npd.median()), "max": int(npass.max()),
                    "per_iteration": float(npd.sum() / it.double().sum().clamp(min=1))}
    # bytes per row pass: 10 per non-zero (int16 column + fp64 value) + ~40 per row (pointer, y, off, wt, D, z)
    res["fused_row_pass_gb"] = float((npd * (n_e * (NNZ * 10 + 40)).double()).sum()) / 1e9
    # two-loop history traffic: per iteration up to 4 m reads + 2 writes of d doubles
    res["fused_history_gb_bound"] = float((it.double() * (4 * RE_LBFGS_M + 2) * d * 8).sum()) / 1e9
    print(f"fused: {ms:.2f} ms (runs {', '.join(f'{t:.2f}' for t in ts)})", flush=True)
if "pass" in ROUTES:
    from photon_ml_amd.ops.device import DeviceGLMData
    from photon_ml_amd.optimization.batched import SegmentedGLMData, batched_lbfgs
    row_ent = torch.repeat_interleave(torch.arange(E, device=dev), n_e, output_size=N)
    pos = lcol.to(torch.int64) + torch.repeat_interleave(col_ptr[row_ent], NNZ, output_size=N * NNZ)
    glm = DeviceGLMData.from_device_csr(nip, pos, val, y, torch.zeros_like(y), wt, E * d, dev, "f64",
                                        col_windows=True)
    del pos
    col_ent = torch.repeat_interleave(torch.arange(E, device=dev), d, output_size=E * d)
    seg = SegmentedGLMData(glm, row_ent, col_ent, E, y, wt, off)
    r, ms, ts = timed(lambda: batched_lbfgs(seg, LOGISTIC, L2, W_warm, TOL, MAX_ITER, l1=L1))
    sol["pass"] = (r.W, r.iters.to(torch.int64))
    res["pass_ms"] = ms
    res["pass_ms_runs"] = ts
    res["pass_iterations_hist"] = torch.bincount(r.iters.to(torch.int64), minlength=MAX_ITER + 1).tolist()
    print(f"pass path: {ms:.2f} ms (runs {', '.join(f'{t:.2f}' for t in ts)})", flush=True)
if len(sol) == 2:
    (Wa, ia), (Wb, ib) = sol["fused"], sol["pass"]
    res["speedup"] = res["pass_ms"] / res["fused_ms"]
    res["max_abs_w_diff"] = float((Wa - Wb).abs().max())
    res["zero_pattern_mismatches"] = int(((Wa == 0) != (Wb == 0)).sum())
    res["iterations_equal_share"] = float((ia == ib).double().mean())
print(json.dumps(res), flush=True)
