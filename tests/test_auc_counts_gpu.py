"""``auc_count_kernel`` / ``auc_count_combine_kernel`` (``ops/native.py::auc_counts``) on the GPU: lengths around the
rows of one workgroup (``native.AUC_COUNT_BLOCK_ROWS``), tie groups inside a workgroup's run, across two runs and
across a whole run. The three integers must equal a numpy count model exactly, the AUC they give must equal
``auc_weighted`` on the CPU bitwise (all sums are integers), and a second call must give the same bits."""
import pytest
import torch

from auc_count_cases import PATTERNS, R, check_pattern, check_validation

from photon_ml_amd.ops import native

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pattern", PATTERNS)
def test_counts_match_the_model_and_auc_weighted(pattern):
    check_pattern(pattern, "cuda")


def test_unaligned_views_give_the_same_counts():
    """A view that starts inside an allocation (not 16-byte aligned) is copied before the 16-byte loads."""
    from auc_count_cases import count_model, make_case
    s, f = make_case("quarter_grid", 2 * R + 3)
    ts, tf = torch.from_numpy(s).cuda(), torch.from_numpy(f).cuda()
    got = native.auc_counts(ts[1:], tf[1:])
    assert tuple(got.tolist()) == count_model(s[1:], f[1:])


def test_input_validation_raises_before_launch(monkeypatch):
    monkeypatch.setenv("PML_CHECK_KERNEL_INPUTS", "1")
    check_validation("cuda")
