"""Validation metrics under a process group with the evaluators on the GPU (tests/dist_eval_worker.py,
tests/dist_eval_gpu_worker.py): a one-rank RCCL group (``PML_FORCE_DIST=1``, device collectives), two and three
gloo ranks sharing the one GPU (rehearsals: the collectives stage through the host, the ranking and count kernels run
on the device), and a GAME fit under a forced one-rank RCCL group against the same fit without a group.

Same data and equalities as tests/test_dist_eval.py: per-group values and the global AUC bitwise the host oracle's on
the concatenated rows, the scalar per-group metrics within 1e-12 (a mean of at most 4096 values in [0, 1] summed in
another order). Every worker is its own child process with a timeout; nothing is launched after a failure."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from test_dist_eval import check_case, launch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _on_device(res):
    for r in res:
        assert all(p == "device" for p in r["paths"]), r["paths"]
        assert r["labels_cuda"].all()                       # AUC, AUC:tag and PRECISION@k:tag hold GPU labels
        assert r["auc_path"][0] == "buckets"


def test_one_rank_rccl_group(tmp_path):
    res = launch("boundary", tmp_path, 1, device="cuda", backend="nccl", timeout=240, PML_FORCE_DIST="1",
                 PML_DIST_BACKEND="nccl")
    check_case("boundary", 1, res)
    _on_device(res)


def test_two_gloo_ranks_on_one_gpu(tmp_path):
    res = launch("boundary", tmp_path, 2, device="cuda", backend="gloo", timeout=240)
    check_case("boundary", 2, res)
    _on_device(res)


def test_three_gloo_ranks_one_without_rows(tmp_path):
    res = launch("empty_rank", tmp_path, 3, device="cuda", backend="gloo", timeout=240)
    check_case("empty_rank", 3, res)
    _on_device(res)


def test_three_gloo_ranks_one_owning_no_group(tmp_path):
    res = launch("two_groups", tmp_path, 3, device="cuda", backend="gloo", timeout=240)
    check_case("two_groups", 3, res)
    _on_device(res)
    assert min(r["keys_0"].size for r in res) == 0


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _fit(mode, out, env_extra):
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(_port()), **env_extra)
    p = subprocess.run([sys.executable, "-u", os.path.join(HERE, "dist_eval_gpu_worker.py"), mode, str(out)], env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert f"{mode} ok" in p.stdout


def test_game_fit_under_a_one_rank_rccl_group_reports_what_the_plain_fit_does(tmp_path):
    """The workers check every plain-AUC evaluation of the fit and of ``GameTransformer`` against ``auc_weighted``
    on the scores it was given (bitwise), the placements, and that nothing was gathered; here the per-group scalars
    the two runs report are compared (they depend on the scores through ranks only)."""
    _fit("forced", tmp_path, {"PML_FORCE_DIST": "1", "PML_DIST_BACKEND": "nccl"})
    _fit("plain", tmp_path, {"PML_FORCE_DIST": "0"})
    for part in ("fit", "transform"):
        a, b = np.load(tmp_path / f"forced_{part}.npy"), np.load(tmp_path / f"plain_{part}.npy")
        assert np.abs(a[1:] - b[1:]).max() <= 1e-12, (part, a, b)
