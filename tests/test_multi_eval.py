"""Per-group ranking evaluators off the GPU: the group layout of ``GroupedRanking`` (built on any device; the
metrics themselves are HIP kernels) and the host path of ``MultiEvaluator``, which must keep returning exactly what
the per-group functions give (``MultiEvaluator.scala:49-64``)."""
import math

import numpy as np
import pytest
import torch

from multi_eval_cases import boundary_case, host_group_values

from photon_ml_amd.evaluation.evaluators import (AUCMultiEvaluator, PrecisionAtKMultiEvaluator, auc_weighted,
                                                 build_evaluator, precision_at_k)
from photon_ml_amd.evaluation.segmented import GroupedRanking


@pytest.fixture(scope="module")
def case():
    return boundary_case()


def _numpy_layout(codes, wg_max):
    perm = np.argsort(codes, kind="stable")
    lens = np.bincount(codes)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    c16, c64 = min(16, wg_max), min(64, wg_max)
    lists = {"C16": np.nonzero((lens >= 1) & (lens <= c16))[0],
             "C64": np.nonzero((lens > c16) & (lens <= c64))[0],
             "CWG": np.nonzero((lens > c64) & (lens <= wg_max))[0],
             "LONG": np.nonzero(lens > wg_max)[0]}
    return perm, ptr, lists


@pytest.mark.parametrize("wg_max", [4096, 64, 0])
def test_layout_matches_numpy_construction(case, wg_max):
    lay = GroupedRanking(case["codes"], case["labels"], case["weights"], device="cpu", wg_max=wg_max)
    perm, ptr, lists = _numpy_layout(case["codes"], wg_max)
    assert lay.n == case["codes"].size and lay.n_groups == len(ptr) - 1
    assert lay.perm.dtype == torch.int64 and lay.seg_ptr.dtype == torch.int64
    assert np.array_equal(lay.perm.numpy(), perm)
    assert np.array_equal(lay.seg_ptr.numpy(), ptr)
    assert np.array_equal(lay.wts.numpy(), case["weights"][perm])
    assert np.array_equal(lay.flag.numpy(), (case["labels"][perm] > 0.5).astype(np.uint8))
    for c in ("C16", "C64", "CWG", "LONG"):
        assert np.array_equal(lay.lists[c].numpy(), lists[c]), c
    assert lay.class_counts == {c: len(v) for c, v in lists.items()}
    if wg_max == 4096:
        # lengths 1, 2, 15, 16 | 17, 63, 64 | 65 .. 4096 | 4097, 10000; four groups each, two of length 1
        assert lay.class_counts == {"C16": 14, "C64": 12, "CWG": 24, "LONG": 8}
        assert lay.cwg_pad == 4096
    # LONG row tables: the group-ordered slots of every LONG group, in group order
    rows = np.concatenate([np.arange(ptr[g], ptr[g + 1]) for g in lists["LONG"]] or [np.zeros(0, np.int64)])
    assert np.array_equal(lay.long_rows.numpy(), rows)
    assert np.array_equal(lay.long_ptr.numpy(), np.concatenate([[0], np.cumsum(np.diff(ptr)[lists["LONG"]])]))
    assert np.array_equal(lay.long_gid.numpy(), np.repeat(np.arange(len(lists["LONG"])), np.diff(ptr)[lists["LONG"]]))


def test_layout_on_cpu_refuses_to_evaluate(case):
    lay = GroupedRanking(case["codes"], case["labels"], case["weights"], device="cpu")
    s = torch.from_numpy(case["scores"])
    with pytest.raises(RuntimeError, match="GPU"):
        lay.auc(s)
    with pytest.raises(RuntimeError, match="GPU"):
        lay.precision_at_k(s, 3)


def test_wg_max_above_cap_rejected(case):
    with pytest.raises(ValueError, match="wg_max"):
        GroupedRanking(case["codes"], case["labels"], case["weights"], device="cpu", wg_max=4097)


def test_mean_finite():
    assert GroupedRanking.mean_finite(torch.tensor([0.25, float("nan"), 0.75, float("inf")],
                                                   dtype=torch.float64)) == 0.5
    assert math.isnan(GroupedRanking.mean_finite(torch.tensor([float("nan")], dtype=torch.float64)))
    assert math.isnan(GroupedRanking.mean_finite(torch.zeros(0, dtype=torch.float64)))


def _small(seed=3, n=400, n_groups=23):
    rng = np.random.default_rng(seed)
    ids = np.array([f"q{v}" for v in rng.integers(0, n_groups, size=n)], dtype=object)
    y = (rng.random(n) < 0.45).astype(np.float64)
    w = rng.random(n) + 0.5
    off = rng.normal(size=n) * 0.1
    s = np.round(rng.normal(size=n), 1)
    return ids, y, w, off, s


def _per_group_mean(ids, y, w, z, fn):
    vals = []
    for key in np.unique(ids.astype(str)):
        m = np.nonzero(ids.astype(str) == key)[0]
        v = fn(torch.from_numpy(z[m]), torch.from_numpy(y[m]), torch.from_numpy(w[m]))
        if math.isfinite(v):
            vals.append(v)
    return float(np.mean(vals))


def test_multi_evaluator_cpu_values_are_the_per_group_functions():
    """Three pinned values, each computed here with the per-group functions (not literals)."""
    ids, y, w, off, s = _small()
    z = s + off
    pins = [(AUCMultiEvaluator("queryId", ids, y, off, w), lambda a, b, c: auc_weighted(a, b, c)),
            (PrecisionAtKMultiEvaluator(1, "queryId", ids, y, off, w), lambda a, b, c: precision_at_k(a, b, 1)),
            (PrecisionAtKMultiEvaluator(5, "queryId", ids, y, off, w), lambda a, b, c: precision_at_k(a, b, 5))]
    for ev, fn in pins:
        got = ev.evaluate(s)
        assert got == _per_group_mean(ids, y, w, z, fn), ev.name          # bit for bit
        assert ev.last_path == "host" and ev.ranking is None


def test_evaluate_groups_on_cpu_agrees_with_per_group_calls():
    ids, y, w, off, s = _small(seed=4)
    z = s + off
    uniq, inv = np.unique(ids.astype(str), return_inverse=True)
    for name, k in (("AUC:queryId", 0), ("PRECISION@3:queryId", 3)):
        ev = build_evaluator(name, y, off, w, {"queryId": ids})
        keys, vals = ev.evaluate_groups(s)
        assert np.array_equal(np.asarray(keys), uniq)
        assert vals.dtype == torch.float64 and vals.shape == (len(uniq),)
        want = host_group_values(inv, y, w, z, k)
        assert np.array_equal(vals.numpy(), want, equal_nan=True)
        fin = want[np.isfinite(want)]
        assert ev.evaluate(s) == float(np.mean(fin))
        assert ev.last_path == "host"
