"""One L2 TRON update over game5pl-like random-effect entities under normalization (``profiles/re_normalization.md``).

The entities are those of ``scripts/re_fused_bench.py`` (power-law sizes, Pareto 1.3, 65 .. 20000 rows; a
1000-feature pool + intercept, d_e = 1001; 50 pool features per row with N(0,1) values; logistic labels). Four cases,
every solve from zero with the same TRON settings (l2 = 1, tolerance 1e-12, <= 10 iterations, <= 20 CG steps):

  a  NONE as routed today: ``re_tron_lean_kernel`` on quad-padded rows
  b  a scale-only context: the same launches on the folded values (val *= f[col])
  c  STANDARDIZATION: ``re_tron_csr_kernel<LOSS, true>`` on the folded values with (c, i0)
  d  the same problem as c on the pass path (``batched_tron`` over ``SegmentedGLMData`` with a shift)

The cases alternate inside every round (a b c [d], ROUNDS times); per case the median and the spread over the rounds
are printed, with the row passes per entity, since b / c solve other problems than a and take other iteration counts.

usage: python scripts/re_norm_bench.py [n_entities=43000] [rounds=5] [pass_path=1]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from photon_ml_amd.ops.native import re_tron_csr
from photon_ml_amd.optimization.entity_tron import pad_rows_to_quads

E = int(sys.argv[1]) if len(sys.argv) > 1 else 43_000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
PASS_PATH = (sys.argv[3] if len(sys.argv) > 3 else "1") != "0"
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
strides = torch.tensor([s for s in range(1, 200) if s % 2 and s % 5], device=dev)
a_ = torch.randint(0, d - 1, (N, 1), generator=g, device=dev)
s_ = strides[torch.randint(0, strides.numel(), (N, 1), generator=g, device=dev)]
cols = (a_ + torch.arange(NNZ - 1, device=dev)[None, :] * s_) % (d - 1)
cols, _ = torch.sort(cols, dim=1)
lcol = torch.cat([cols, torch.full((N, 1), d - 1, device=dev)], 1).reshape(-1).to(torch.int16)
del cols, a_, s_
val = torch.randn(N * NNZ, generator=g, device=dev, dtype=torch.float64)
val.view(N, NNZ)[:, -1] = 1.0
nip = torch.arange(N + 1, dtype=torch.int64, device=dev) * NNZ
y = (torch.rand(N, generator=g, device=dev) < 0.4).double()
off = torch.zeros(N, dtype=torch.float64, device=dev)
wt = torch.ones(N, dtype=torch.float64, device=dev)
scr = torch.empty(4 * N, dtype=torch.float64, device=dev)
# one context for the shard: factors in [0.5, 2], shifts N(0, 0.3^2); the intercept (local column d - 1) untouched
f_sh = 0.5 + 1.5 * torch.rand(d, generator=g, device=dev, dtype=torch.float64)
s_sh = 0.3 * torch.randn(d, generator=g, device=dev, dtype=torch.float64)
f_sh[d - 1], s_sh[d - 1] = 1.0, 0.0
val_f = val * f_sh[lcol.to(torch.int64)]                       # the fold
c_pack = (f_sh * s_sh).repeat(E).contiguous()
i0 = torch.full((E,), d - 1, dtype=torch.int32, device=dev)
nip_q, lcol_q, val_q = pad_rows_to_quads(nip, lcol, val)
_, _, valf_q = pad_rows_to_quads(nip, lcol, val_f)
order = torch.argsort(n_e, descending=True).to(torch.int32).contiguous()
print(f"{E} entities, {N} rows, {N * NNZ / 1e6:.0f}M non-zeros, max n_e {int(n_e.max())}", flush=True)

L2, TOL, ITERS, FAILS, CG = 1.0, 1e-12, 10, 5, 20
W = torch.zeros(E * d, dtype=torch.float64, device=dev)
fv = torch.empty(E, dtype=torch.float64, device=dev)
it = torch.empty(E, dtype=torch.int32, device=dev)
rc = torch.empty(E, dtype=torch.int32, device=dev)
z = torch.empty(N, dtype=torch.float64, device=dev)
npass = torch.zeros(E, dtype=torch.int32, device=dev)
gsc = torch.empty_like(W)


def lean(values_q, np_=None):
    re_tron_csr(order, row_ptr, col_ptr, nip_q, lcol_q, values_q, y, off, wt, scr, W, fv, it, rc, z, 0, L2, TOL, ITERS,
                FAILS, CG, 1008, npass=np_, lean=True, quad=True, gsc=gsc)


def shifted(np_=None):
    re_tron_csr(order, row_ptr, col_ptr, nip, lcol, val_f, y, off, wt, scr, W, fv, it, rc, z, 0, L2, TOL, ITERS, FAILS,
                CG, 1024, npass=np_, lean=False, shift=(c_pack, i0))


cases = {"a": lambda np_=None: lean(val_q, np_), "b": lambda np_=None: lean(valf_q, np_), "c": shifted}
seg = None
if PASS_PATH:
    from photon_ml_amd.function.losses import LOGISTIC
    from photon_ml_amd.ops.device import DeviceGLMData
    from photon_ml_amd.optimization.batched import SegmentedGLMData, batched_tron
    row_ent = torch.repeat_interleave(torch.arange(E, device=dev), n_e, output_size=N)
    pos = (lcol.to(torch.int64).view(N, NNZ) + (row_ent * d)[:, None]).reshape(-1).contiguous()
    t0 = time.perf_counter()
    glm = DeviceGLMData.from_device_csr(nip, pos, val_f, y, torch.zeros_like(y), wt, E * d, dev, "f64", col_windows=True)
    col_ent = torch.repeat_interleave(torch.arange(E, device=dev), d, output_size=E * d)
    seg = SegmentedGLMData(glm, row_ent, col_ent, E, y, wt, off, shift=(c_pack, i0.to(torch.int64)))
    torch.cuda.synchronize()
    print(f"pass-path layout built in {time.perf_counter() - t0:.1f} s", flush=True)
    del pos
    res_d = {}

    def pass_path(np_=None):
        res_d["r"] = batched_tron(seg, LOGISTIC, L2, torch.zeros(E * d, dtype=torch.float64, device=dev), TOL, ITERS,
                                  FAILS, CG)

    cases["d"] = pass_path

stats, models = {}, {}
for k, fn in cases.items():                 # warm-up + pass counts + models
    W.zero_()
    npass.zero_()
    fn(npass)
    torch.cuda.synchronize()
    if k == "d":
        models[k] = (res_d["r"].W.clone(), res_d["r"].iters.clone())
        stats[k] = (float("nan"), float(res_d["r"].iters.double().mean()))
    else:
        models[k] = (W.clone(), it.clone().to(torch.int64))
        stats[k] = (float(npass.double().mean()), float(it.double().mean()))
times = {k: [] for k in cases}
for _ in range(ROUNDS):
    for k, fn in cases.items():
        W.zero_()
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t) * 1e3)
for k, ts in times.items():
    print(f"case {k}: median {statistics.median(ts):.2f} ms, min {min(ts):.2f}, max {max(ts):.2f} over {len(ts)} rounds "
          f"| mean row passes / entity {stats[k][0]:.1f} | mean TRON iterations {stats[k][1]:.3f}", flush=True)


def compare(name, ma, mb):
    """Agreement of two solvers' models: entities with equal iteration counts apart from the others."""
    (Wa, ia), (Wb, ib) = ma, mb
    diff = (Wa - Wb).abs().view(E, d).amax(1)
    same = ia == ib
    worst = lambda m: float(diff[m].max()) if bool(m.any()) else 0.0
    print(f"{name}: iteration counts equal for {float(same.double().mean()) * 100:.2f} % of entities; max |W diff| "
          f"{worst(same):.3e} among those, {worst(~same):.3e} among the other {int((~same).sum())} (max |W| "
          f"{float(Wa.abs().max()):.3e})", flush=True)


if "d" in models:
    compare("c (shifted fused kernel) vs d (pass path with shifts)", models["c"], models["d"])
    # the same comparison without any normalization: lean kernel vs pass path on the original values
    del seg, glm
    pos = (lcol.to(torch.int64).view(N, NNZ) + (row_ent * d)[:, None]).reshape(-1).contiguous()
    glm0 = DeviceGLMData.from_device_csr(nip, pos, val, y, torch.zeros_like(y), wt, E * d, dev, "f64", col_windows=True)
    seg0 = SegmentedGLMData(glm0, row_ent, col_ent, E, y, wt, off)
    r0 = batched_tron(seg0, LOGISTIC, L2, torch.zeros(E * d, dtype=torch.float64, device=dev), TOL, ITERS, FAILS, CG)
    compare("a (lean kernel) vs the pass path, no normalization", models["a"], (r0.W, r0.iters))
