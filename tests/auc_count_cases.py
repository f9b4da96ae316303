"""Shared inputs and checks of the sorted-stream AUC count tests (tests/test_auc_counts.py on the torch
implementation, tests/test_auc_counts_gpu.py on the HIP kernels)."""
import numpy as np
import torch

from multi_eval_cases import same_bits
from photon_ml_amd.evaluation.evaluators import auc_weighted
from photon_ml_amd.ops import native

R = native.AUC_COUNT_BLOCK_ROWS
# one run and its neighbours, several runs, a partial last run
LENGTHS = (0, 1, 2, R - 1, R, R + 1, 2 * R, 3 * R + 1, 8 * R + 5)
PATTERNS = ("distinct", "quarter_grid", "three_values", "all_equal", "spanning_tie", "all_positive", "all_negative")


def make_case(pattern: str, n: int, seed: int = 3):
    """(scores sorted non-increasing fp64, flags uint8) of ``n`` rows."""
    rng = np.random.default_rng(seed + n)
    if pattern == "distinct":
        s = rng.permutation(n).astype(np.float64) / 8.0 - n / 16.0
    elif pattern == "three_values":
        s = rng.integers(0, 3, size=n).astype(np.float64) - 1.0
    elif pattern == "all_equal":
        s = np.full(n, 0.75)
    elif pattern == "spanning_tie":
        # distinct scores, then one tie group from the last row of the first run to the first row of the third
        s = -np.arange(n, dtype=np.float64)
        s[R - 1:2 * R + 1] = -(R - 1.0)
    else:
        s = np.round(4.0 * rng.normal(size=n)) / 4.0            # heavy ties
        zero = np.nonzero(s == 0.0)[0]
        s[zero[::2]] = -0.0                                     # both zeros, interleaved
    order = np.argsort(-s, kind="stable")
    s = s[order]
    if pattern == "quarter_grid" and n >= R:
        assert np.any((s == 0.0) & np.signbit(s)) and np.any((s == 0.0) & ~np.signbit(s))
    f = (rng.random(n) < 0.4).astype(np.uint8)
    if pattern == "all_positive":
        f[:] = 1
    if pattern == "all_negative":
        f[:] = 0
    return np.ascontiguousarray(s), f


def count_model(s: np.ndarray, f: np.ndarray):
    """(2 raw, P, N): every negative row counts the positives with a greater score plus those with a greater or
    equal score (binary searches in the positives' scores)."""
    pos = np.sort(s[f != 0])
    neg = s[f == 0]
    gt = pos.size - np.searchsorted(pos, neg, side="right")
    ge = pos.size - np.searchsorted(pos, neg, side="left")
    return int(gt.sum() + ge.sum()), int(pos.size), int(neg.size)


def ratio(c) -> float:
    raw2, p, n = (int(x) for x in c)
    return (raw2 / 2.0) / (float(p) * float(n)) if p and n else float("nan")


def check_pattern(pattern: str, device: str):
    """Every length of one pattern: exact counts, the AUC bitwise, and the same bits from a second call."""
    for n in LENGTHS:
        s, f = make_case(pattern, n)
        ts, tf = torch.from_numpy(s).to(device), torch.from_numpy(f).to(device)
        got = native.auc_counts(ts, tf)
        assert got.dtype == torch.int64 and got.device.type == device and tuple(got.shape) == (3,)
        want = count_model(s, f)
        assert tuple(got.tolist()) == want, (pattern, n, got.tolist(), want)
        ref = auc_weighted(torch.from_numpy(s), torch.from_numpy(f.astype(np.float64)), None)
        assert same_bits(np.array([ratio(got.tolist())]), np.array([ref])), (pattern, n, ratio(got.tolist()), ref)
        again = native.auc_counts(ts, tf)
        assert torch.equal(got, again), (pattern, n)


def check_validation(device: str):
    """Under PML_CHECK_KERNEL_INPUTS=1 (set by the caller) malformed inputs raise before any launch."""
    import pytest
    s, f = make_case("quarter_grid", R + 7)
    ts, tf = torch.from_numpy(s).to(device), torch.from_numpy(f).to(device)
    native.auc_counts(ts, tf)
    with pytest.raises((ValueError, AssertionError)):
        native.auc_counts(ts.flip(0).contiguous(), tf)                  # increasing
    with pytest.raises((ValueError, AssertionError)):
        native.auc_counts(ts, tf[:-1].contiguous())
    with pytest.raises((ValueError, AssertionError)):
        native.auc_counts(ts.to(torch.float32), tf)
