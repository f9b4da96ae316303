"""``AUPR`` / ``AUPR:tag`` under a process group with the evaluators on the GPU (tests/aupr_dist_worker.py): a
one-rank RCCL group (``PML_FORCE_DIST=1``, device collectives) and two gloo ranks sharing the one GPU (a rehearsal:
the collectives stage through the host, the ranking kernels and the bucket pass run on the device).

Same data, equalities and bound as tests/test_aupr_dist.py; the per-group values now come from the HIP kernels, at
most (G + 4) 2^-53 from the host's with the dyadic weights of ``boundary_case``. Every worker is its own child process
with a timeout of 240 s; the ranks of a group start together and nothing is launched after a failure."""
import numpy as np
import pytest

from test_aupr_dist import check_case, check_paths, launch

pytestmark = pytest.mark.gpu


def _on_device(res, o, got_tag):
    check_paths(res, path="buckets", multi="device")
    for r in res:
        assert r["labels_cuda"].all()                       # AUPR and AUPR:tag hold GPU labels under a group
    fin = o["groups"][np.isfinite(o["groups"])]
    assert fin.size == 28 and abs(got_tag - fin.mean()) <= 1e-12, (got_tag, fin.mean())


def test_one_rank_rccl_group(tmp_path):
    res = launch("boundary", tmp_path, 1, device="cuda", backend="nccl", timeout=240, PML_FORCE_DIST="1",
                 PML_DIST_BACKEND="nccl")
    _on_device(res, *check_case("boundary", 1, res))


def test_two_gloo_ranks_on_one_gpu(tmp_path):
    res = launch("boundary", tmp_path, 2, device="cuda", backend="gloo", timeout=240)
    _on_device(res, *check_case("boundary", 2, res))
