"""``GameEstimator.set_normalization``: normalization asked for by TYPE, the contexts built by the estimator from
the statistics of the shards it has just built (``BasicStatisticalSummary.for_shard``: from the device when the
shard is tiled, on a GPU and stored in fp64, on the host otherwise). On the CPU every shard takes the host path, so
the contexts must be those built from ``BasicStatisticalSummary.compute`` and the trained models must not move.
A 2-rank gloo fit gives every rank the single-process contexts (all-reduced statistics)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from photon_ml_amd.data.game_data import generate_game_data
from photon_ml_amd.data.matrix import LabeledData
from photon_ml_amd.data.random_effect import FixedEffectDataConfiguration, RandomEffectDataConfiguration
from photon_ml_amd.estimators.game_estimator import GameEstimator
from photon_ml_amd.normalization.context import NormalizationContext
from photon_ml_amd.optimization.config import GLMOptimizationConfiguration, OptimizerConfig, RegularizationContext
from photon_ml_amd.stat.summary import BasicStatisticalSummary

HERE = os.path.dirname(os.path.abspath(__file__))
_OPT = GLMOptimizationConfiguration(OptimizerConfig("LBFGS", 60, 1e-9), RegularizationContext("L2"), 1.0)
CFG = {"global": _OPT, "items": _OPT, "per-user": _OPT}
INTERCEPT = 19           # generate_game_data: the intercept is the last column of every shard (d_global = 20)
ITEM_INTERCEPT = 5


def game_data():
    return generate_game_data(n_rows=1200, n_users=30, seed=5, task="LOGISTIC_REGRESSION")[0]


def estimator():
    return (GameEstimator(device="cpu").set_training_task("LOGISTIC_REGRESSION")
            .set_coordinate_data_configurations({"global": FixedEffectDataConfiguration("global"),
                                                 "items": FixedEffectDataConfiguration("item"),
                                                 "per-user": RandomEffectDataConfiguration("userId", "user")})
            .set_coordinate_update_sequence(["global", "items", "per-user"]))


def host_context(data, shard, intercept, kind="STANDARDIZATION"):
    return NormalizationContext.build(kind, BasicStatisticalSummary.compute(data.shards[shard]), intercept)


def assert_contexts_close(a, b):
    assert a.intercept_id == b.intercept_id
    for f in ("factors", "shifts"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None)
        if x is not None:
            torch.testing.assert_close(x, y, rtol=1e-12, atol=1e-12)


def coefficients(result, cid):
    return result.model.get(cid).glm.coefficients.means.cpu().numpy()


@pytest.fixture(scope="module")
def fits():
    """(data, estimator and result of the by-type fit, result of the fit with host-built contexts)."""
    data = game_data()
    intercepts = {"global": INTERCEPT, "item": ITEM_INTERCEPT, "user": 5}
    est = estimator().set_normalization("STANDARDIZATION", intercepts)
    seen = []
    est.coordinates_built_callback = lambda e: seen.append(sorted(e.feature_statistics))
    by_type = est.fit(data, None, [CFG])[0]
    ref = estimator().set_coordinate_normalization_contexts(
        {"global": host_context(data, "global", INTERCEPT), "items": host_context(data, "item", ITEM_INTERCEPT)})
    return data, est, by_type, ref.fit(data, None, [CFG])[0], seen


def test_contexts_by_type_equal_the_host_built_ones(fits):
    data, est, _, _, seen = fits
    assert_contexts_close(est.coordinates["global"].normalization, host_context(data, "global", INTERCEPT))
    assert_contexts_close(est.coordinates["items"].normalization, host_context(data, "item", ITEM_INTERCEPT))
    # statistics readable by shard id, for the shards fixed effects train on, when the coordinates were built
    assert seen == [["global", "item"]] and sorted(est.feature_statistics) == ["global", "item"]
    want = BasicStatisticalSummary.compute(data.shards["global"])
    for f in ("mean", "variance", "max", "min", "num_nonzeros"):
        torch.testing.assert_close(getattr(est.feature_statistics["global"], f), getattr(want, f),
                                   rtol=1e-12, atol=1e-12)


def test_models_equal_those_of_host_built_contexts(fits):
    _, _, by_type, ref, _ = fits
    for cid in ("global", "items"):
        assert np.array_equal(coefficients(by_type, cid), coefficients(ref, cid))


def test_explicit_context_wins_per_coordinate():
    data = game_data()
    explicit = host_context(data, "global", INTERCEPT, "SCALE_WITH_MAX_MAGNITUDE")
    est = (estimator().set_normalization("STANDARDIZATION", {"global": INTERCEPT, "item": ITEM_INTERCEPT})
           .set_coordinate_normalization_contexts({"global": explicit}))
    est.fit(data, None, [CFG])
    assert est.coordinates["global"].normalization is explicit
    assert est.coordinates["global"].problem.normalization is explicit
    built = est.coordinates["items"].normalization
    assert_contexts_close(built, host_context(data, "item", ITEM_INTERCEPT))
    assert est.coordinates["items"].problem.normalization is built
    assert sorted(est.feature_statistics) == ["item"]          # no statistics for a coordinate that does not need them


def test_statistics_without_normalization():
    data = game_data()
    est = estimator().set_normalization("NONE", collect_statistics=True)
    est.fit(data, None, [CFG])
    assert est.coordinates["global"].normalization is None
    assert sorted(est.feature_statistics) == ["global", "item"]


@pytest.mark.parametrize("layout", ["segmented", "tiled"])
def test_shards_off_the_gpu_take_the_host_path(layout, monkeypatch):
    """The rule of ``for_shard``: the device only for a tiled fp64 shard on a GPU. A segmented shard (whose
    ``from_device`` raises) and a tiled shard on the CPU get ``compute``."""
    from photon_ml_amd.ops.device import DeviceGLMData
    x = game_data().shards["global"]
    dev = DeviceGLMData.from_labeled(LabeledData(x, np.zeros(x.shape[0])), "cpu", "f64", chunk_rows=500, layout=layout)
    assert dev.layout == layout and not BasicStatisticalSummary.on_device(dev)

    def no_device(*a, **k):
        raise AssertionError("from_device called for a shard that is not on a GPU")
    monkeypatch.setattr(BasicStatisticalSummary, "from_device", staticmethod(no_device))
    got, want = BasicStatisticalSummary.for_shard(x, dev), BasicStatisticalSummary.compute(x)
    for f in ("mean", "variance", "max", "min", "num_nonzeros", "norm_l1", "norm_l2", "mean_abs"):
        assert torch.equal(getattr(got, f), getattr(want, f))


def test_two_ranks_hold_the_single_process_contexts(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PML_BACKEND="torch", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dist_norm_worker.py"), str(r), "2", str(port),
                               str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    for p in procs:
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, out.decode(errors="replace")[-4000:]
    r0, r1 = (np.load(tmp_path / f"norm_r{r}.npz") for r in range(2))
    data = game_data()
    want = host_context(data, "global", INTERCEPT)
    for k in ("factors", "shifts", "mean", "variance", "count"):
        assert np.array_equal(r0[k], r1[k]), k                 # both ranks: identical contexts
    assert int(r0["count"][0]) == data.n_rows
    np.testing.assert_allclose(r0["factors"], want.factors.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r0["shifts"], want.shifts.numpy(), rtol=1e-12, atol=1e-12)
    assert np.array_equal(r0["coef"], r1["coef"])
