"""Time one ``AUC:tag`` and one ``PRECISION@5:tag`` evaluation on the device (``GroupedRanking`` + the per-group
ranking kernels of ``ops/csrc/game_kernels.hip``), with device events after a warm-up.

Group sizes follow the ``game5pl`` law of ``bench_game.py``: Pareto(1.3), 5 .. 20000 rows (mean about 21). Variants:

* ``fused``      the size classes (C16 / C64 in registers, CWG sorted in LDS, LONG pre-sorted), ``wg_max = 4096``;
* ``presorted``  ``wg_max = 0``: every group through the pre-sorted streaming kernel, i.e. two stable torch sorts
  over all rows + one scan kernel -- the alternative that justifies or refutes the in-LDS / in-register sorts;
* ``host loop``  the per-group Python loop of ``MultiEvaluator`` (what every evaluation cost before), timed at
  ``--loop-groups`` groups only; larger figures in the table are extrapolations per group and labelled so.

One evaluation = per-group values + ``mean_finite`` (the scalar ``MultiEvaluator`` reports), the NaN-flag readback
included. Prints one JSON line per measurement and a markdown table (``--out`` writes it to a file).

    python scripts/multi_eval_bench.py --groups 100000 1250000 --out profiles/multi_eval_device.md
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from photon_ml_amd.evaluation.evaluators import AUCMultiEvaluator, PrecisionAtKMultiEvaluator  # noqa: E402
from photon_ml_amd.evaluation.segmented import GroupedRanking  # noqa: E402


def make_rows(n_groups: int, seed: int, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    u = torch.rand(n_groups, generator=gen, device=dev, dtype=torch.float64)
    cnt = torch.clamp(torch.ceil(5.0 * u ** (-1.0 / 1.3)), max=20000).to(torch.int64)
    n = int(cnt.sum())
    codes = torch.repeat_interleave(torch.arange(n_groups, device=dev), cnt, output_size=n)
    codes = codes[torch.randperm(n, generator=gen, device=dev)]
    y = (torch.rand(n, generator=gen, device=dev) < 0.3).to(torch.float64)
    w = torch.rand(n, generator=gen, device=dev, dtype=torch.float64) + 0.5
    s = torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
    return codes, y, w, s


def time_ms(fn, warmup: int, reps: int):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, nargs="+", default=[100_000, 1_250_000])
    ap.add_argument("--loop-groups", type=int, default=20_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rows = []
    for ng in a.groups:
        codes, y, w, s = make_rows(ng, a.seed, dev)
        for variant, wg in (("fused", 4096), ("presorted", 0)):
            lay = GroupedRanking(codes, y, w, device=dev, wg_max=wg)
            launches = sum(1 for v in lay.class_counts.values() if v)
            for metric, fn in (("AUC", lambda: lay.mean_finite(lay.auc(s))),
                               ("PRECISION@5", lambda: lay.mean_finite(lay.precision_at_k(s, 5)))):
                med, best = time_ms(fn, a.warmup, a.reps)
                rec = {"groups": ng, "rows": int(codes.numel()), "variant": variant, "metric": metric,
                       "ms_median": round(med, 3), "ms_min": round(best, 3), "value": fn(),
                       "classes": lay.class_counts, "ranking_kernel_launches": launches}
                rows.append(rec)
                print(json.dumps(rec), flush=True)
            del lay
        del codes, y, w, s
        torch.cuda.empty_cache()
    # the host loop (labels on the CPU: exactly the path every evaluation took before)
    codes, y, w, s = (t.cpu().numpy() for t in make_rows(a.loop_groups, a.seed, dev))
    loop = {}
    for metric, ev in (("AUC", AUCMultiEvaluator("tag", codes, y, None, w)),
                       ("PRECISION@5", PrecisionAtKMultiEvaluator(5, "tag", codes, y, None, w))):
        t0 = time.perf_counter()
        v = ev.evaluate(s)
        sec = time.perf_counter() - t0
        loop[metric] = sec / a.loop_groups
        rec = {"groups": a.loop_groups, "rows": int(codes.size), "variant": "host loop", "metric": metric,
               "ms_median": round(sec * 1e3, 1), "value": v, "us_per_group": round(sec / a.loop_groups * 1e6, 1)}
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    lines = ["| groups | rows | variant | metric | ms / evaluation (median) | min | classes C16 / C64 / CWG / LONG | "
             "ranking kernel launches |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["variant"] == "host loop":
            lines.append(f"| {r['groups']} | {r['rows']} | host loop (measured) | {r['metric']} | {r['ms_median']} | | "
                         f"| 0 ({r['us_per_group']} us per group) |")
        else:
            c = r["classes"]
            lines.append(f"| {r['groups']} | {r['rows']} | {r['variant']} | {r['metric']} | {r['ms_median']} | "
                         f"{r['ms_min']} | {c['C16']} / {c['C64']} / {c['CWG']} / {c['LONG']} | "
                         f"{r['ranking_kernel_launches']} |")
    for ng in a.groups:
        for metric, per in loop.items():
            lines.append(f"| {ng} | | host loop (EXTRAPOLATED per group from {a.loop_groups}) | {metric} | "
                         f"{per * ng * 1e3:.0f} | | | |")
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
