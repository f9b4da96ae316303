"""The device statistics wired through both CLIs on the GPU: with ``--normalization STANDARDIZATION`` and a summary
directory, the statistics of the fixed-effect shard (tiled, fp64, on the GPU) come from the device copy the run
builds anyway — ``BasicStatisticalSummary.compute`` is patched to RAISE for that shard and the run must complete.
The written summary equals the host-computed one at 1e-12 and the coefficients equal those of a run whose contexts
were built on the host, to the tolerance test_cli_gpu.py uses for its CPU / GPU comparison (1e-5 relative)."""
import glob
import os

import numpy as np
import pytest

from photon_ml_amd.cli import game_training
from photon_ml_amd.data.game_data import generate_game_data
from photon_ml_amd.io.avro import read_records
from photon_ml_amd.io.data_writer import write_game_avro
from photon_ml_amd.stat.summary import BasicStatisticalSummary
from test_cli_gpu import FIXED, RANDOM, SHARDS

pytestmark = pytest.mark.gpu

D_GLOBAL = 20


def summary_records(directory):
    recs = {}
    for f in sorted(glob.glob(os.path.join(str(directory), "*.avro"))):
        for r in read_records(f)[1]:
            recs[r["featureName"], r["featureTerm"]] = r["metrics"]
    return recs


def assert_summaries_equal(a, b):
    assert a and set(a) == set(b)
    for key in a:
        assert set(a[key]) == set(b[key])
        for metric, v in a[key].items():
            assert abs(v - b[key][metric]) <= 1e-12 + 1e-12 * abs(b[key][metric]), (key, metric, v, b[key][metric])


def host_only(monkeypatch):
    monkeypatch.setattr(BasicStatisticalSummary, "on_device", staticmethod(lambda glm_data: False))


def compute_raises_for(monkeypatch, n_features):
    """``compute`` raises for a matrix with ``n_features`` columns (the fixed-effect shard); other shards pass."""
    real = BasicStatisticalSummary.compute

    def guarded(x, all_reduce=False):
        if x.shape[1] == n_features:
            raise AssertionError("the host statistics were computed for the shard that is on the GPU")
        return real(x, all_reduce=all_reduce)
    monkeypatch.setattr(BasicStatisticalSummary, "compute", staticmethod(guarded))


def _game_run(root, out, summary):
    args = ["--input-data-directories", str(root / "train"), "--root-output-directory", str(out),
            "--training-task", "LOGISTIC_REGRESSION", *SHARDS, "--coordinate-configurations", FIXED,
            "--coordinate-configurations", RANDOM, "--coordinate-update-sequence", "fixed,per-user",
            "--coordinate-descent-iterations", "1", "--output-mode", "BEST", "--device", "cuda",
            "--normalization", "STANDARDIZATION", "--data-summary-directory", str(summary)]
    res = game_training.GameTrainingDriver(game_training.build_parser().parse_args(args)).run()
    return res["best"].model.get("fixed").glm.coefficients.means.cpu().numpy(), res["index_maps"]


def test_game_training_takes_the_fixed_effect_statistics_from_the_device(tmp_path, monkeypatch):
    data, _ = generate_game_data(n_rows=1500, n_users=60, d_global=D_GLOBAL, d_user=8, seed=17,
                                 task="LOGISTIC_REGRESSION")
    write_game_avro(str(tmp_path / "train"), data, {"global": "features", "user": "userFeatures"}, n_files=2)
    with monkeypatch.context() as m:
        host_only(m)
        want, maps = _game_run(tmp_path, tmp_path / "host", tmp_path / "host-summary")
    assert maps["global"].feature_dimension != maps["user"].feature_dimension
    with monkeypatch.context() as m:
        compute_raises_for(m, maps["global"].feature_dimension)
        got, _ = _game_run(tmp_path, tmp_path / "dev", tmp_path / "dev-summary")
    for shard in ("global", "user"):
        assert_summaries_equal(summary_records(tmp_path / "dev-summary" / shard),
                               summary_records(tmp_path / "host-summary" / shard))
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)


def test_summary_is_on_disk_when_the_fit_fails(tmp_path, monkeypatch):
    """The summary is written as soon as the coordinates are built: a fit that fails in its first update leaves it."""
    from photon_ml_amd.algorithm.coordinate_descent import CoordinateDescent
    data, _ = generate_game_data(n_rows=600, n_users=20, d_global=D_GLOBAL, d_user=8, seed=3,
                                 task="LOGISTIC_REGRESSION")
    write_game_avro(str(tmp_path / "train"), data, {"global": "features", "user": "userFeatures"})

    def fail(*a, **k):
        raise RuntimeError("update failed")
    monkeypatch.setattr(CoordinateDescent, "run", fail)
    with pytest.raises(RuntimeError, match="update failed"):
        _game_run(tmp_path, tmp_path / "out", tmp_path / "summary")
    assert summary_records(tmp_path / "summary" / "global") and summary_records(tmp_path / "summary" / "user")


def test_legacy_driver_takes_the_statistics_from_its_device_shard(tmp_path, monkeypatch):
    from photon_ml_amd.cli import driver as drv
    from photon_ml_amd.estimators import game_estimator
    ref = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures")
    shards = []
    real_train = game_estimator.train_generalized_linear_model

    def spy(*a, **k):
        shards.append(k.get("glm_data"))
        return real_train(*a, **k)
    monkeypatch.setattr(drv, "train_generalized_linear_model", spy)

    def run(name):
        args = ["--training-data-directory", f"{ref}/heart.avro", "--validating-data-directory",
                f"{ref}/heart_validation.avro", "--output-directory", str(tmp_path / name), "--task",
                "LOGISTIC_REGRESSION", "--num-iterations", "100", "--convergence-tolerance", "1e-10",
                "--regularization-weights", "0.1,10", "--normalization-type", "STANDARDIZATION", "--optimizer", "TRON",
                "--device", "cuda", "--summarization-output-dir", str(tmp_path / f"{name}-summary")]
        d = drv.Driver(drv.build_parser().parse_args(args))
        d.run()
        return d, drv.read_text_model(str(tmp_path / name / drv.LEARNED_MODELS_TEXT))

    with monkeypatch.context() as m:
        host_only(m)
        _, want = run("host")
    with monkeypatch.context() as m:
        m.setattr(BasicStatisticalSummary, "compute", staticmethod(
            lambda *a, **k: (_ for _ in ()).throw(AssertionError("host statistics computed"))))
        d, got = run("dev")
    assert d.glm_data is not None and d.glm_data.layout == "tiled" and shards[-1] is d.glm_data   # built once, reused
    assert_summaries_equal(summary_records(tmp_path / "dev-summary"), summary_records(tmp_path / "host-summary"))
    for lam in want:
        assert set(want[lam]) == set(got[lam])
        for k, c in want[lam].items():
            assert abs(c - got[lam][k]) <= 1e-5 * max(1.0, abs(c)), (lam, k, c, got[lam][k])
