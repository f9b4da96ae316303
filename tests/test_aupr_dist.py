"""``AUPR`` / ``AUPR:tag`` under a process group without row gathers (gloo on the CPU; tests/aupr_dist_worker.py).

``AUPR:tag`` routes every row to the rank that owns its group and evaluates the owned groups there; plain ``AUPR``
exchanges the score buckets of plain ``AUC``, all-gathers two integer counts per bucket and adds the ranks' partial
sums in rank order. Data: the cases of ``dist_eval_worker.case_rows`` (row i on rank ``i % world``). Expected:
``aupr_weighted`` on the concatenation rank 0, rank 1, ... -- of all rows for ``AUPR``, per group for ``AUPR:tag``.

Bound 1e-12: a value is a sum of G < 64 non-negative terms over P (scores on a grid of 1/4 within about +-6; one term
per tie group), each term a few roundings, and the distributed sum only associates the terms differently (per bucket,
then over the ranks): at most (G + 4) 2^-53 apart for plain ``AUPR`` (integer prefixes, exact in fp64). The per-group
values are computed by the same host function on the same rows in the same order; the ``AUPR:tag`` scalar is a mean
of at most 58 values in [0, 1] summed in another order."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from dist_eval_worker import case_rows, concat_order
from multi_eval_cases import same_bits
from test_aupr import host_group_aupr

from photon_ml_amd.evaluation.evaluators import aupr_weighted, build_evaluator
from photon_ml_amd.parallel.sharding import stable_hash64

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(case, out, world, device="cpu", backend="gloo", timeout=240, **env_extra):
    """One worker process per rank, each with a timeout; returns the per-rank results."""
    port = _free_port()
    env = dict(os.environ, PML_BACKEND="torch", OMP_NUM_THREADS="2", **env_extra)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "aupr_dist_worker.py"), case, str(r), str(world),
                               str(port), str(out), device, backend], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(world)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o.decode(errors="replace"))
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    return [np.load(os.path.join(out, f"{case}_r{r}.npz")) for r in range(world)]


_ORACLE = {}


def oracle(case, world):
    """Expected values on the concatenated rows; computed once per (case, row order)."""
    cols, owner = case_rows(case, world)
    order = concat_order(owner, world)
    key = (case, order.tobytes())
    if key not in _ORACLE:
        c = {k: v[order] for k, v in cols.items()}
        codes = np.unique(c["codes"], return_inverse=True)[1]
        _ORACLE[key] = {
            "keys": stable_hash64(np.unique(c["codes"])),
            "groups": host_group_aupr(codes, c["labels"], c["weights"], c["scores"]),
            "aupr": aupr_weighted(torch.from_numpy(c["scores"]), torch.from_numpy(c["labels"]), None),
            "cols": c,
        }
    return _ORACLE[key]


def close(a, b, tol=1e-12):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and (na.all() or float(np.abs(a[~na] - b[~nb]).max()) <= tol)


def check_case(case, world, res):
    """The equalities every case must satisfy (also used by the GPU tests)."""
    o = oracle(case, world)
    for r in res[1:]:
        assert same_bits(r["scalars"], res[0]["scalars"]), (r["scalars"], res[0]["scalars"])
    got_aupr, got_tag = res[0]["scalars"]
    print(f"{case} world {world}: AUPR {got_aupr!r} (oracle {o['aupr']!r}), AUPR:tag {got_tag!r}")
    assert close(got_aupr, o["aupr"]), (got_aupr, o["aupr"])
    want = dict(zip(o["keys"].tolist(), o["groups"].tolist()))
    keys = np.concatenate([r["keys"] for r in res])
    vals = np.concatenate([r["vals"] for r in res])
    assert keys.size == len(want) and np.unique(keys).size == keys.size, keys.size       # one owner each
    for r in res:
        assert np.all(r["keys"][1:] > r["keys"][:-1])                                     # sorted
    assert close(vals, np.array([want[int(x)] for x in keys]))
    assert sum(int(r["bucket_rows"][0]) for r in res) == (0 if case == "nan" else o["cols"]["scores"].size)
    return o, got_tag


def check_paths(res, path="buckets", multi="host"):
    for r in res:
        assert r["aupr_path"][0] == path and r["multi_path"][0] == multi, (r["aupr_path"], r["multi_path"])


@pytest.mark.parametrize("world", [2, 4])
def test_boundary_case_matches_the_oracle_without_row_gathers(tmp_path, world):
    res = launch("boundary", tmp_path, world)
    o, got_tag = check_case("boundary", world, res)
    fin = o["groups"][np.isfinite(o["groups"])]
    assert fin.size == 28 and abs(got_tag - fin.mean()) <= 1e-12, (got_tag, fin.mean())
    assert np.isfinite(o["aupr"])
    check_paths(res)
    assert min(int(r["bucket_rows"][0]) for r in res) > 0                 # every rank evaluated a bucket


def test_a_rank_without_rows(tmp_path):
    res = launch("empty_rank", tmp_path, 3)
    o, got_tag = check_case("empty_rank", 3, res)
    fin = o["groups"][np.isfinite(o["groups"])]
    assert abs(got_tag - fin.mean()) <= 1e-12
    check_paths(res)


def test_all_scores_equal_is_one_bucket(tmp_path):
    """One tie group: AUPR = P / (P + N), all rows in one bucket, the other rank adds 0."""
    res = launch("all_equal", tmp_path, 2)
    o, got_tag = check_case("all_equal", 2, res)
    y = o["cols"]["labels"]
    assert abs(res[0]["scalars"][0] - (y > 0.5).mean()) <= 1e-12
    fin = o["groups"][np.isfinite(o["groups"])]
    assert abs(got_tag - fin.mean()) <= 1e-12
    check_paths(res)
    assert sorted(int(r["bucket_rows"][0]) for r in res) == [0, y.size]


def test_a_nan_score_takes_the_gather_path_on_every_rank(tmp_path):
    world = 2
    res = launch("nan", tmp_path, world)
    o, got_tag = check_case("nan", world, res)
    check_paths(res, path="gather")
    c = o["cols"]
    single = build_evaluator("AUPR:tag", c["labels"], None, c["weights"], {"tag": c["codes"]}, device="cpu")
    assert close(got_tag, single.evaluate(torch.from_numpy(c["scores"])))
