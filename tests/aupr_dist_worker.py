"""Worker of tests/test_aupr_dist.py (gloo, CPU) and tests/test_aupr_dist_gpu.py (evaluators on the GPU): one rank of
a process group evaluates ``AUPR`` and ``AUPR:tag`` on its rows of a case of ``dist_eval_worker.case_rows`` and saves
what it got; the test compares with the oracle on the concatenated rows.

    python aupr_dist_worker.py CASE RANK WORLD PORT OUT DEVICE BACKEND
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from dist_eval_worker import case_rows  # noqa: E402

NAMES = ["AUPR", "AUPR:tag"]


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
    evs = {n: build_evaluator(n, y, None, w, {"tag": ids}, device=device) for n in NAMES}
    res = {"labels_cuda": np.array([e.labels.is_cuda for e in evs.values()])}

    phase[0] = "eval"
    scores = torch.from_numpy(s).to(device)
    res["scalars"] = np.array([evs[n].evaluate(scores) for n in NAMES])
    res["multi_path"] = np.array([evs["AUPR:tag"].last_path])
    res["aupr_path"] = np.array([evs["AUPR"].last_info["path"]])
    res["bucket_rows"] = np.array([evs["AUPR"].last_info["bucket_rows"]])
    keys, vals = evs["AUPR:tag"].evaluate_groups(scores)
    res["keys"], res["vals"] = np.asarray(keys), vals.cpu().numpy()
    # no collective of an evaluation carries a column of rows: everything gathered is far shorter than a shard
    limit = int(shard_rows[shard_rows > 0].min())
    long_calls = [c for c in calls if c[0] == "eval" and c[2] >= limit
                  and not (case == "nan" and c[1] in ("_gather", "all_gather_varlen"))]
    assert not long_calls, f"row-length gathers during an evaluation: {long_calls[:6]}"
    gathers = [c for c in calls if c[0] == "eval" and c[1] == "_gather"]
    if case == "nan":                # AUPR:tag never gathers, NaN or not; plain AUPR did, on purpose (scores, flags)
        assert res["aupr_path"][0] == "gather" and len(gathers) == 2, calls
    else:
        assert res["aupr_path"][0] == "buckets" and not gathers, calls
    np.savez(os.path.join(out, f"{case}_r{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()
    print(f"{case} rank {rank} ok", flush=True)


if __name__ == "__main__":
    a = sys.argv
    main(a[1], int(a[2]), int(a[3]), int(a[4]), a[5], a[6], a[7])
