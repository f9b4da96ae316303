"""Worker of tests/test_dist_eval.py (gloo, CPU) and tests/test_dist_eval_gpu.py (evaluators on the GPU): one rank
of a process group evaluates ``AUC``, ``AUC:tag`` and ``PRECISION@k:tag`` on its rows of a case of
:func:`case_rows` and saves what it got; the test compares with the oracle on the concatenated rows.

    python dist_eval_worker.py CASE RANK WORLD PORT OUT DEVICE BACKEND
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

KS = (0, 1, 5, 100)                  # 0: AUC:tag, k > 0: PRECISION@k:tag
NAMES = ["AUC:tag"] + [f"PRECISION@{k}:tag" for k in KS[1:]]
BALANCE_ROWS = 20000                 # rows of the largest shard of the continuous-score balance check


def case_rows(case: str, world: int):
    """``(columns, owner)``: the rows of a case (dict of numpy arrays: codes, labels, weights, scores) and the rank
    every row is dealt to. The expected values are those of the concatenation rank 0, rank 1, ..."""
    from multi_eval_cases import boundary_case
    c = boundary_case()
    c.pop("lengths")
    n = c["codes"].size
    if case == "two_groups":         # a 255-row and a 4097-row group with both classes: most ranks own no group
        lens = np.bincount(c["codes"])
        g = [int(np.nonzero(lens == L)[0][0]) for L in (255, 4097)]
        keep = np.isin(c["codes"], g)
        c = {k: v[keep] for k, v in c.items()}
        n = c["codes"].size
    owner = np.arange(n) % world
    if case == "empty_rank":         # the last rank holds no row
        owner = np.arange(n) % (world - 1)
    if case == "all_equal":
        c["scores"] = np.full(n, 0.75)
    if case == "nan":                # one NaN score, on the last rank
        c["scores"] = c["scores"].copy()
        c["scores"][np.nonzero(owner == world - 1)[0][7]] = np.nan
    return c, owner


def concat_order(owner: np.ndarray, world: int) -> np.ndarray:
    return np.concatenate([np.nonzero(owner == r)[0] for r in range(world)])


def balance_rows(rank: int, world: int):
    """Continuous scores, uneven shards (rank r holds BALANCE_ROWS // (r + 1) rows), rank 0's shard shifted."""
    rng = np.random.default_rng(100 + rank)
    n = BALANCE_ROWS // (rank + 1)
    s = rng.normal(size=n) + (1.5 if rank == 0 else 0.0)
    return s, (rng.random(n) < 0.3).astype(np.float64)


def main(case, rank, world, port, out, device, backend):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                       "WORLD_SIZE": str(world), "LOCAL_RANK": "0", "PML_BACKEND": "torch"})
    from photon_ml_amd.parallel.dist import init_distributed, is_dist
    init_distributed(backend)
    assert is_dist()
    import torch.distributed as dist
    from photon_ml_amd.evaluation import evaluators
    from photon_ml_amd.evaluation.evaluators import build_evaluator
    from photon_ml_amd.parallel import sharding

    # recorders of the row gathers, installed BEFORE the evaluators are built
    calls = []
    phase = ["build"]

    def recording(fn, what):
        def wrapped(t, *a, **kw):
            calls.append((phase[0], what, int(t.numel())))
            return fn(t, *a, **kw)
        return wrapped

    evaluators._gather = recording(evaluators._gather, "_gather")
    sharding.all_gather_varlen = recording(sharding.all_gather_varlen, "all_gather_varlen")

    cols, owner = case_rows(case, world)
    mine = np.nonzero(owner == rank)[0]
    y, w, s, ids = (cols[k][mine] for k in ("labels", "weights", "scores", "codes"))
    shard_rows = np.bincount(owner, minlength=world)
    evs = {"AUC": build_evaluator("AUC", y, None, w, device=device)}
    for name in NAMES:
        evs[name] = build_evaluator(name, y, None, w, {"tag": ids}, device=device)
    res = {"labels_cuda": np.array([e.labels.is_cuda for e in evs.values()])}

    phase[0] = "eval"
    scores = torch.from_numpy(s).to(device)
    res["scalars"] = np.array([evs[n].evaluate(scores) for n in ["AUC"] + NAMES])
    res["paths"] = np.array([evs[n].last_path for n in NAMES])
    res["auc_path"] = np.array([evs["AUC"].last_info["path"]])
    for k, name in zip(KS, NAMES):
        keys, vals = evs[name].evaluate_groups(scores)
        res[f"keys_{k}"], res[f"vals_{k}"] = np.asarray(keys), vals.cpu().numpy()
    # no collective of an evaluation carries a column of rows: everything gathered is far shorter than a shard
    limit = int(shard_rows[shard_rows > 0].min())
    long_calls = [c for c in calls if c[0] == "eval" and c[2] >= limit
                  and not (case == "nan" and c[1] in ("_gather", "all_gather_varlen"))]
    assert not long_calls, f"row-length gathers during an evaluation: {long_calls[:6]}"
    if case == "nan":                # the per-group evaluators never gather, NaN or not; plain AUC did, on purpose
        assert res["auc_path"][0] == "gather"
        assert len([c for c in calls if c[0] == "eval" and c[1] == "_gather"]) == 2, calls

    if case == "boundary":           # bucket balance of the global AUC on continuous scores
        bs, by = balance_rows(rank, world)
        ev = build_evaluator("AUC", by, device=device)
        res["balance_auc"] = np.array([ev.evaluate(torch.from_numpy(bs).to(device))])
        res["balance_bucket_rows"] = np.array([ev.last_info["bucket_rows"]])
    np.savez(os.path.join(out, f"{case}_r{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()
    print(f"{case} rank {rank} ok", flush=True)


if __name__ == "__main__":
    a = sys.argv
    main(a[1], int(a[2]), int(a[3]), int(a[4]), a[5], a[6], a[7])
