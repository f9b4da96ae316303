"""``ops/native.py::auc_counts`` off the GPU (the torch implementation): the integer counts of the unweighted
tie-grouped AUC of one sorted stream against a numpy count model, and the AUC they give against ``auc_weighted``
bitwise. The same cases run on the HIP kernels in tests/test_auc_counts_gpu.py."""
import pytest

from auc_count_cases import PATTERNS, check_pattern, check_validation


@pytest.mark.parametrize("pattern", PATTERNS)
def test_counts_match_the_model_and_auc_weighted(pattern):
    check_pattern(pattern, "cpu")


def test_input_validation_raises(monkeypatch):
    monkeypatch.setenv("PML_CHECK_KERNEL_INPUTS", "1")
    check_validation("cpu")
