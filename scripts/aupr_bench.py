"""Time one ``AUPR:tag`` evaluation next to one ``AUC:tag`` evaluation on the device: the same ``GroupedRanking``
layout, the same process, the two metrics ALTERNATING evaluation by evaluation (device events after a warm-up of
both), so that whatever else the machine does falls on both alike. Rows and variants are those of
``scripts/multi_eval_bench.py`` (``game5pl`` group sizes; ``fused``: the size classes, ``presorted``: ``wg_max = 0``).

One evaluation = per-group values + ``mean_finite`` (the scalar ``MultiEvaluator`` reports), the NaN-flag readback
included. The whole measurement is repeated ``--rounds`` times to show its spread. Prints one JSON line per
measurement and a markdown table (``--out`` writes it to a file): the table of ``profiles/aupr_device.md``.

    python scripts/aupr_bench.py --groups 1250000 --out aupr_table.md
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from multi_eval_bench import make_rows  # noqa: E402

from photon_ml_amd.evaluation.segmented import GroupedRanking  # noqa: E402


def alternate_ms(fns: dict, warmup: int, reps: int) -> dict:
    """Median and minimum ms of every function of ``fns``, timed in turn ``reps`` times."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, nargs="+", default=[1_250_000])
    ap.add_argument("--variants", nargs="+", default=["fused", "presorted"], choices=["fused", "presorted"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aupr_bench.py measures on a GPU; none is visible")
    dev = torch.device("cuda")
    rows = []
    for ng in a.groups:
        codes, y, w, s = make_rows(ng, a.seed, dev)
        for variant in a.variants:
            lay = GroupedRanking(codes, y, w, device=dev, wg_max=4096 if variant == "fused" else 0)
            fns = {"AUC": lambda: lay.mean_finite(lay.auc(s)), "AUPR": lambda: lay.mean_finite(lay.aupr(s))}
            for rnd in range(a.rounds):
                res = alternate_ms(fns, a.warmup, a.reps)
                rec = {"groups": ng, "rows": int(codes.numel()), "variant": variant, "round": rnd,
                       "classes": lay.class_counts, "reps": a.reps,
                       **{f"{k}_ms_median": round(v[0], 3) for k, v in res.items()},
                       **{f"{k}_ms_min": round(v[1], 3) for k, v in res.items()},
                       "ratio_median": round(res["AUPR"][0] / res["AUC"][0], 3),
                       **{f"{k}_value": fn() for k, fn in fns.items()}}
                rows.append(rec)
                print(json.dumps(rec), flush=True)
            del lay
        del codes, y, w, s
        torch.cuda.empty_cache()
    lines = ["| groups | rows | variant | round | AUC:tag ms / evaluation (median) | min | AUPR:tag ms / evaluation "
             "(median) | min | AUPR / AUC | classes C16 / C64 / CWG / LONG |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        c = r["classes"]
        lines.append(f"| {r['groups']} | {r['rows']} | {r['variant']} | {r['round']} | {r['AUC_ms_median']} | "
                     f"{r['AUC_ms_min']} | {r['AUPR_ms_median']} | {r['AUPR_ms_min']} | {r['ratio_median']} | "
                     f"{c['C16']} / {c['C64']} / {c['CWG']} / {c['LONG']} |")
    lines.append("")
    for r in rows:
        if r["round"] == 0:
            lines.append(f"Mean over the finite groups, {r['groups']} groups, {r['variant']}: AUC:tag "
                         f"{r['AUC_value']!r}, AUPR:tag {r['AUPR_value']!r}.")
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
