"""Validation metrics under a process group without row gathers (gloo on the CPU; tests/dist_eval_worker.py).

``AUC:tag`` / ``PRECISION@k:tag`` route every row to the rank that owns its group and evaluate the owned groups
there; plain ``AUC`` exchanges score buckets and combines integer counts. Data: ``boundary_case()`` with row i on
rank ``i % world``. Expected: ``host_group_values`` / ``auc_weighted`` on the concatenation rank 0, rank 1, ...
(the order routed rows arrive in, so ties at position k of precision@k resolve alike). The dyadic weights make
every AUC sum exact, so per-group values and the global AUC must agree bitwise; the scalar per-group metrics are
means of G <= 4096 values in [0, 1] summed in another order, which differ by at most G * 2^-53 < 1e-12.

The worker replaces ``evaluators._gather`` and ``sharding.all_gather_varlen`` by recorders before it builds the
evaluators and fails when a call during an evaluation carries a tensor as long as a shard."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from dist_eval_worker import BALANCE_ROWS, KS, NAMES, balance_rows, case_rows, concat_order
from multi_eval_cases import host_group_values, same_bits

from photon_ml_amd.evaluation.evaluators import AUC_SAMPLES, auc_weighted, build_evaluator
from photon_ml_amd.parallel.sharding import stable_hash64

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(case, out, world, device="cpu", backend="gloo", timeout=300, **env_extra):
    """One worker process per rank; returns the per-rank results."""
    port = _free_port()
    env = dict(os.environ, PML_BACKEND="torch", OMP_NUM_THREADS="2", **env_extra)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dist_eval_worker.py"), case, str(r), str(world),
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
        o = {"keys": stable_hash64(np.unique(c["codes"]))}
        codes = np.unique(c["codes"], return_inverse=True)[1]
        for k in KS:
            o[k] = host_group_values(codes, c["labels"], c["weights"], c["scores"], k)
        o["auc"] = auc_weighted(torch.from_numpy(c["scores"]), torch.from_numpy(c["labels"]), None)
        o["cols"] = c
        _ORACLE[key] = o
    return _ORACLE[key]


def check_case(case, world, res, exact_auc=True):
    """The equalities every case must satisfy (also used by the GPU tests)."""
    o = oracle(case, world)
    for r in res[1:]:
        assert same_bits(r["scalars"], res[0]["scalars"]), (r["scalars"], res[0]["scalars"])
    if exact_auc:
        assert same_bits(res[0]["scalars"][:1], np.array([o["auc"]])), (res[0]["scalars"][0], o["auc"])
    want = dict()
    for k, name, got in zip(KS, NAMES, res[0]["scalars"][1:]):
        want[k] = dict(zip(o["keys"].tolist(), o[k].tolist()))
        keys = np.concatenate([r[f"keys_{k}"] for r in res])
        vals = np.concatenate([r[f"vals_{k}"] for r in res])
        assert keys.size == len(want[k]) and np.unique(keys).size == keys.size, (name, keys.size)   # one owner each
        for r in res:
            assert np.all(r[f"keys_{k}"][1:] > r[f"keys_{k}"][:-1]), name                          # sorted
        assert same_bits(vals, np.array([want[k][int(x)] for x in keys])), name
        fin = o[k][np.isfinite(o[k])]
        assert abs(got - fin.mean()) <= 1e-12, (name, got, fin.mean())


@pytest.mark.parametrize("world", [2, 4, 8])
def test_boundary_case_matches_the_oracle_without_row_gathers(tmp_path, world):
    res = launch("boundary", tmp_path, world)
    check_case("boundary", world, res)
    assert all(r["auc_path"][0] == "buckets" for r in res)
    # bucket balance on continuous scores: regular sampling bounds the largest bucket
    shards = [balance_rows(r, world) for r in range(world)]
    want = auc_weighted(torch.from_numpy(np.concatenate([s for s, _ in shards])),
                        torch.from_numpy(np.concatenate([y for _, y in shards])), None)
    rows = [int(r["balance_bucket_rows"][0]) for r in res]
    assert sum(rows) == sum(s.size for s, _ in shards)
    for r in res:
        assert same_bits(r["balance_auc"], np.array([want]))
    S, P = AUC_SAMPLES, world
    assert max(rows) <= (S + P) * BALANCE_ROWS / S + P, (rows, (S + P) * BALANCE_ROWS / S + P)


def test_a_rank_without_rows(tmp_path):
    res = launch("empty_rank", tmp_path, 3)
    check_case("empty_rank", 3, res)


def test_two_groups_over_four_ranks(tmp_path):
    res = launch("two_groups", tmp_path, 4)
    check_case("two_groups", 4, res)
    assert sorted(r["keys_0"].size for r in res)[:2] == [0, 0]          # at least two ranks own no group


def test_all_scores_equal_is_one_bucket(tmp_path):
    res = launch("all_equal", tmp_path, 2)
    check_case("all_equal", 2, res)


def test_a_nan_score_takes_the_gather_path_on_every_rank(tmp_path):
    world = 2
    res = launch("nan", tmp_path, world)
    o = oracle("nan", world)
    c = o["cols"]
    # plain AUC: today's value on the gathered rows; per-group scalars: the single-process value on the same scores
    for r in res:
        assert same_bits(r["scalars"][:1], np.array([o["auc"]]))
        assert same_bits(r["scalars"], res[0]["scalars"])
    for name, got in zip(NAMES, res[0]["scalars"][1:]):
        single = build_evaluator(name, c["labels"], None, c["weights"], {"tag": c["codes"]}, device="cpu")
        want = single.evaluate(torch.from_numpy(c["scores"]))
        assert abs(got - want) <= 1e-12, (name, got, want)
