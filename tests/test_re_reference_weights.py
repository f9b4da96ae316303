"""The CPU float64 TRON oracle of the random-effect parity tests (``re_parity_util.cpu_tron``) handles row weights
correctly: an integer weight is a row multiplicity, a zero weight removes the row, and an entity without any weight
stays at zero. The GPU tests compare the fused kernels with this oracle on weighted rows; these tests are what makes
it a reference for that.

A weight w on a row and the row repeated w times with unit weight give the same sums ``sum wt l``, ``sum wt l' x``
and ``sum wt l'' (x.v) x`` up to the order of the additions, so both runs take the same TRON iterations and end at
the same point up to rounding: bound 1e-10 relative (measured for POISSON on [40, 70] rows: 1.9e-12 after 4
iterations at tolerance 0, 5.5e-13 converged at tolerance 1e-8).
"""
import dataclasses

import numpy as np
import pytest

from photon_ml_amd.data.game_data import GameData
from photon_ml_amd.optimization.optimizer import ConvergenceReason
from re_parity_util import cpu_tron, make_entities, reference_floor

BOUND = 1e-10
SIZES = [40, 70]


def _with_weights(data, w):
    return dataclasses.replace(data, weights=np.asarray(w, dtype=np.float64))


def _repeat_rows(data, times):
    """Row i of ``data`` repeated ``times[i]`` times (0: dropped), every copy with unit weight."""
    idx = np.repeat(np.arange(data.n_rows), times)
    sub = data.subset(idx)
    return GameData(sub.response, sub.shards, sub.id_tags, sub.offsets, np.ones(len(idx)))


def _same(a, b, check_w=True):
    for e in a:
        assert a[e][1] == b[e][1], (e, a[e][1], b[e][1])
        assert a[e][2] == b[e][2], (e, a[e][2], b[e][2])
    if check_w:
        err = reference_floor(a, b)
        print("relative W difference", err, "iterations", [a[e][1] for e in a])
        assert err <= BOUND, err


@pytest.mark.parametrize("loss", ["POISSON", "LOGISTIC"])
def test_integer_weights_are_row_multiplicities(loss):
    data = make_entities(SIZES, 30, 8, seed=5, loss=loss)
    k = np.random.default_rng(7).integers(0, 4, size=data.n_rows)        # weights in {0, 1, 2, 3}
    weighted, repeated = _with_weights(data, k), _repeat_rows(data, k)
    assert repeated.n_rows == int(k.sum())
    for tol, max_iter in ((0.0, 4), (1e-8, 60)):
        a = cpu_tron(weighted, loss, 1.0, tol, max_iter)
        b = cpu_tron(repeated, loss, 1.0, tol, max_iter)
        if tol == 0.0:
            assert all(a[e][1] == 4 for e in a)
        _same(a, b)
        # the reservoir multiplier is one more factor of the weight: unit weights times mult = k
        c = cpu_tron(_with_weights(data, np.ones(data.n_rows)), loss, 1.0, tol, max_iter, mult=k)
        _same(a, c)


@pytest.mark.parametrize("loss", ["POISSON", "LOGISTIC"])
def test_zero_weight_rows_equal_removed_rows(loss):
    data = make_entities(SIZES, 30, 8, seed=6, loss=loss)
    zero = data.weights == 0
    assert 0 < zero.sum() < data.n_rows
    kept = np.nonzero(~zero)[0]
    for tol, max_iter in ((0.0, 4), (1e-8, 60)):
        a = cpu_tron(data, loss, 1.0, tol, max_iter)
        _same(a, cpu_tron(data.subset(kept), loss, 1.0, tol, max_iter))
        _same(a, cpu_tron(data, loss, 1.0, tol, max_iter, rows=kept))     # the active-row restriction


def test_entity_with_all_zero_weights_stays_at_zero():
    data = make_entities(SIZES, 30, 8, seed=5, loss="LOGISTIC")
    w = data.weights.copy()
    w[data.id_tags["userId"] == 0] = 0.0
    ref = cpu_tron(_with_weights(data, w), "LOGISTIC", 1.0, 1e-8, 60)
    w0, it0, reason0 = ref[0]
    assert not w0.any() and it0 == 0
    assert reason0 == ConvergenceReason.OBJECTIVE_NOT_IMPROVING
    assert ref[1][1] > 0 and np.abs(ref[1][0]).max() > 0
