"""Time the validation metrics under a process group on one GPU: ``AUC``, ``AUC:tag`` and ``PRECISION@5:tag`` built
through ``build_evaluator`` in a fresh child process with a one-rank RCCL group (``PML_FORCE_DIST=1``), on rows of
the ``game5pl`` group law (as ``scripts/multi_eval_bench.py``: Pareto(1.3), 5 .. 20000 rows per group).

* One evaluation each: median of ``--reps`` after ``--warmup``, host clock around a device synchronise.
* Phases, where the tree has them: route / rank kernels / reduce of the per-group metrics; local sort / exchange /
  bucket sort / ``auc_counts`` of plain AUC.
* ``auc_counts`` alone against the torch expression chain of ``auc_weighted`` (tie groups, index_add, cumsum) on
  pre-sorted device rows, ``--count-rows`` rows.

The evaluations use the public API only, so the script runs unchanged against another checkout (``--repo PATH``, e.g.
a ``git worktree`` of the parent commit). A tree whose per-group metrics gather their rows and take the per-group
Python loop under a group (its evaluators have no ``router``) is timed at ``--loop-groups`` groups only and its figures at the larger sizes are
extrapolated per group and labelled so. One rank on one GPU: the collectives run through RCCL but move nothing
between devices; runs on more than one physical GPU are not covered.

    python scripts/dist_eval_bench.py --groups 100000 1250000 --out profiles/dist_eval_device.md --label this
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time


def make_rows(torch, n_groups: int, seed: int, dev):
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


def child(a):
    sys.path.insert(0, os.path.abspath(a.repo))
    import torch
    from photon_ml_amd.evaluation import evaluators
    from photon_ml_amd.evaluation.evaluators import build_evaluator
    from photon_ml_amd.parallel.dist import init_distributed, is_dist
    dev = torch.device(a.device)
    init_distributed("nccl" if dev.type == "cuda" else "gloo")
    assert is_dist(), "the child needs PML_FORCE_DIST=1"
    if dev.type != "cuda":
        print("NOTE: not on a GPU -- a rehearsal of the script, the times mean nothing", flush=True)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)

    def timed(fn, warmup=a.warmup, reps=a.reps):
        for _ in range(warmup):
            fn()
        out = []
        for _ in range(reps):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out), min(out)

    def emit(**rec):
        rec["label"] = a.label
        print("REC " + json.dumps(rec), flush=True)

    names = ["AUC", "AUC:tag", "PRECISION@5:tag"]

    def build(codes, y, w):
        ids = codes.cpu().numpy()
        t0 = time.perf_counter()
        evs = {n: build_evaluator(n, y.cpu().numpy(), None, w.cpu().numpy(), {"tag": ids}, device=dev) for n in names}
        sync()
        return evs, time.perf_counter() - t0

    # which path do the per-group metrics take under a group in this tree?
    codes, y, w, s = make_rows(torch, a.loop_groups, a.seed, dev)
    evs, _ = build(codes, y, w)
    evs["AUC:tag"].evaluate(s)
    loops = not hasattr(evs["AUC:tag"], "router")          # a tree that gathers rows and loops over the groups
    per_group = {}
    if loops:
        for n in names[1:]:
            sync()
            t0 = time.perf_counter()
            v = evs[n].evaluate(s)
            sec = time.perf_counter() - t0
            per_group[n] = sec / a.loop_groups
            emit(kind="evaluation", groups=a.loop_groups, rows=int(s.numel()), metric=n, path="host loop (measured once)",
                 ms_median=round(sec * 1e3, 1), value=v, us_per_group=round(sec / a.loop_groups * 1e6, 1))
    del evs

    for ng in a.groups:
        codes, y, w, s = make_rows(torch, ng, a.seed, dev)
        n = int(s.numel())
        if loops:
            # the constructor and every evaluation gather all rows and loop over all groups on the host: only plain
            # AUC is measured at this size, the per-group figures are extrapolated per group
            ev = build_evaluator("AUC", y.cpu().numpy(), None, w.cpu().numpy(), device=None)
            med, best = timed(lambda: ev.evaluate(s), 1, 3)
            emit(kind="evaluation", groups=ng, rows=n, metric="AUC", path="gather + sort of all rows (labels on host)",
                 ms_median=round(med, 3), ms_min=round(best, 3), value=ev.evaluate(s))
            for m, per in per_group.items():
                emit(kind="evaluation", groups=ng, rows=n, metric=m,
                     path=f"host loop (EXTRAPOLATED per group from {a.loop_groups})", ms_median=round(per * ng * 1e3))
            continue
        evs, build_s = build(codes, y, w)
        emit(kind="build", groups=ng, rows=n, seconds=round(build_s, 3))
        for m in names:
            med, best = timed(lambda: evs[m].evaluate(s))
            path = evs[m].last_info.get("path") if m == "AUC" else evs[m].last_path
            emit(kind="evaluation", groups=ng, rows=n, metric=m, path=path, ms_median=round(med, 3),
                 ms_min=round(best, 3), value=evs[m].evaluate(s))
        # phases of the per-group metrics
        ev = evs["AUC:tag"]
        rs = ev.router.forward(s)
        vals = ev.ranking.auc(rs) if ev.ranking is not None else None
        phases = [("route scores", lambda: ev.router.forward(s))]
        if vals is not None:
            phases += [("rank kernels AUC", lambda: ev.ranking.auc(rs)),
                       ("rank kernels PRECISION@5", lambda: ev.ranking.precision_at_k(rs, 5)),
                       ("finite sums + all-reduce",
                        lambda: evaluators._allsum(*ev.ranking.finite_sums(vals).tolist()))]
        for phase, fn in phases:
            med, best = timed(fn)
            emit(kind="phase", groups=ng, rows=n, metric="per-group", phase=phase, ms_median=round(med, 3),
                 ms_min=round(best, 3))
        # phases of plain AUC
        from photon_ml_amd.ops import native
        from photon_ml_amd.parallel.sharding import RowRouter
        f = evs["AUC"].flags
        ss, order = torch.sort(s + 0.0, descending=True)
        fs = f[order]
        router = RowRouter.from_counts([n])

        def sort_local():
            t, o = torch.sort(s + 0.0, descending=True)
            return t, f[o]

        def exchange():
            r = RowRouter.from_counts([n])
            return r.exchange(ss), r.exchange(fs)

        def exchange_scores_only():
            return RowRouter.from_counts([n]).exchange(ss)

        for phase, fn in (("local sort", sort_local), ("exchange (counts + 2 all-to-all)", exchange),
                          ("exchange, scores only", exchange_scores_only),
                          ("bucket sort (world > 1 only)", sort_local), ("auc_counts", lambda: native.auc_counts(ss, fs))):
            med, best = timed(fn)
            emit(kind="phase", groups=ng, rows=n, metric="AUC", phase=phase, ms_median=round(med, 3),
                 ms_min=round(best, 3))
        del evs, ev, rs, vals, ss, fs, router
        if dev.type == "cuda":
            torch.cuda.empty_cache()

    # auc_counts alone against the torch chain of auc_weighted after its sort
    try:
        from photon_ml_amd.ops.native import auc_counts
    except ImportError:
        auc_counts = None
    n = a.count_rows
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    ss = torch.sort(torch.randn(n, generator=gen, device=dev, dtype=torch.float64), descending=True).values
    fl = (torch.rand(n, generator=gen, device=dev) < 0.3)
    fs, yy = fl.to(torch.uint8), fl.to(torch.float64)

    def chain():
        w_ = torch.ones_like(ss)
        pos = torch.where(yy > 0.5, w_, torch.zeros_like(w_))
        neg = w_ - pos
        new = torch.ones_like(ss, dtype=torch.bool)
        new[1:] = ss[1:] != ss[:-1]
        gid = torch.cumsum(new.to(torch.int64), 0) - 1
        ng_ = int(gid[-1].item()) + 1
        gp = torch.zeros(ng_, dtype=torch.float64, device=dev).index_add_(0, gid, pos)
        gn = torch.zeros(ng_, dtype=torch.float64, device=dev).index_add_(0, gid, neg)
        before = torch.cumsum(gp, 0) - gp
        raw = torch.sum(before * gn + gp * gn / 2.0)
        return float(raw / (gp.sum() * gn.sum()))

    med, best = timed(chain)
    emit(kind="counts", rows=n, variant="torch chain of auc_weighted (pre-sorted input)", ms_median=round(med, 3),
         ms_min=round(best, 3), value=chain())
    if auc_counts is not None:
        def counts():
            c = auc_counts(ss, fs).tolist()
            return (c[0] / 2.0) / (float(c[1]) * float(c[2]))
        med, best = timed(counts)
        emit(kind="counts", rows=n, variant="auc_counts (HIP, incl. 3-integer readback)", ms_median=round(med, 3),
             ms_min=round(best, 3), value=counts(), gb_per_s=round(n * 9 / (best * 1e-3) / 1e9, 1))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()
    print("CHILD OK", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, nargs="+", default=[100_000, 1_250_000])
    ap.add_argument("--loop-groups", type=int, default=20_000)
    ap.add_argument("--count-rows", type=int, default=1 << 24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               PML_FORCE_DIST="1", PML_DIST_BACKEND="nccl" if a.device == "cuda" else "gloo")
    p = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--child"] + sys.argv[1:], env=env,
                       capture_output=True, text=True, timeout=a.timeout)
    sys.stderr.write(p.stderr[-4000:])
    if p.returncode != 0 or "CHILD OK" not in p.stdout:
        sys.stdout.write(p.stdout[-4000:])
        raise SystemExit(f"child failed with exit status {p.returncode}")
    recs = [json.loads(ln[4:]) for ln in p.stdout.splitlines() if ln.startswith("REC ")]
    for r in recs:
        print(json.dumps(r))
    lines = [f"### {a.label}", "", "| what | groups | rows | metric / phase | path | ms (median) | ms (min) | value |",
             "|---|---|---|---|---|---|---|---|"]
    for r in recs:
        what = r["kind"]
        mp = r.get("metric", "") + (" / " + r["phase"] if "phase" in r else "") + r.get("variant", "")
        ms = r.get("ms_median", round(r.get("seconds", 0) * 1e3, 1))
        extra = f" ({r['us_per_group']} us per group)" if "us_per_group" in r else ""
        extra += f" ({r['gb_per_s']} GB/s of 9 B per row)" if "gb_per_s" in r else ""
        lines.append(f"| {what} | {r.get('groups', '')} | {r['rows']} | {mp} | {r.get('path', '')}{extra} | {ms} | "
                     f"{r.get('ms_min', '')} | {r.get('value', '')} |")
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(table + "\n\n")


if __name__ == "__main__":
    main()
