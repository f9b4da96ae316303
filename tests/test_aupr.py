"""``AUPR`` / ``AUPR:tag`` on the host: parsing, the definition (``aupr_weighted``), the multi-evaluator's host loop,
a small GAME fit and the CLIs.

Definition (``evaluators.aupr_weighted``): rows sorted by score descending, tie groups by ``==``; a group with
positive weight ``gp`` adds ``gp (p + q) / 2``, ``p`` / ``q`` the precision after / before the group (``q = p`` when
nothing with weight precedes it); the sum over P; NaN without rows or when a class is missing. With unit weights
this is the trapezoid of ``diagnostics/evaluation.py::binary_metrics`` (``Evaluation.scala:84``): both sum at most
33 terms per group of ``boundary_case()`` (scores on a grid of 1/4) with a few roundings each, far inside 1e-12."""
import math
import os

import numpy as np
import pytest
import torch

from multi_eval_cases import BOUNDARY_LENGTHS, boundary_case

from photon_ml_amd.diagnostics.evaluation import AREA_UNDER_PRECISION_RECALL, binary_metrics
from photon_ml_amd.evaluation.evaluators import (AUPREvaluator, AUPRMultiEvaluator, Evaluator, aupr_weighted,
                                                 build_evaluator, parse_evaluator_type)


def host_group_aupr(codes, labels, weights, scores) -> np.ndarray:
    """``aupr_weighted`` per group on CPU fp64 tensors, rows in input order (the oracle of the device tests too)."""
    order = np.argsort(codes, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(codes))])
    s, y, w = (torch.from_numpy(np.ascontiguousarray(a[order])) for a in (scores, labels, weights))
    out = np.full(len(ptr) - 1, np.nan)
    for g in range(len(ptr) - 1):
        a, b = ptr[g], ptr[g + 1]
        if b > a:
            out[g] = aupr_weighted(s[a:b], y[a:b], w[a:b])
    return out


def bits(x: float) -> int:
    return int(np.float64(x).view(np.int64))


def test_parsing():
    for name in ("AUPR", "aupr", " Aupr "):
        t = parse_evaluator_type(name)
        assert t.name == "AUPR" and not t.is_multi and t.k is None
    for name in ("AUPR:userId", "aupr:userId"):
        t = parse_evaluator_type(name)
        assert t.name == "AUPR:userId" and t.id_tag == "userId" and t.is_multi and t.k is None
    assert parse_evaluator_type("AUC:userId").name == "AUC:userId"          # the longer name did not capture it
    with pytest.raises(ValueError, match="Unsupported evaluator type"):
        parse_evaluator_type("AUPRX")
    y = np.array([1.0, 0.0, 1.0, 0.0])
    e = build_evaluator("aupr", y)
    assert type(e) is AUPREvaluator and e.name == "AUPR" and e.higher_is_better and e.better_than(0.6, 0.5)
    m = build_evaluator("AUPR:userId", y, id_tags={"userId": np.array([0, 0, 1, 1])})
    assert type(m) is AUPRMultiEvaluator and m.name == "AUPR:userId" and m.higher_is_better
    with pytest.raises(ValueError, match="id tag"):
        build_evaluator("AUPR:userId", y, id_tags={})


def test_hand_example():
    """Tie groups {3}, {2, 2}, {1}: terms 1 (1 + 1) / 2 and 1 (2/3 + 1) / 2, no term for the last; over P = 2."""
    v = aupr_weighted([3.0, 2.0, 2.0, 1.0], [1.0, 0.0, 1.0, 0.0])
    assert abs(v - 11.0 / 12.0) <= 1e-15
    assert abs(build_evaluator("AUPR", [1.0, 0.0, 1.0, 0.0]).evaluate([3.0, 2.0, 2.0, 1.0]) - 11.0 / 12.0) <= 1e-15
    # -0.0 ties with 0.0: one tie group of three rows, p = q = 2/3
    assert abs(aupr_weighted([0.0, -0.0, 0.0], [1.0, 0.0, 1.0]) - 2.0 / 3.0) <= 1e-15


def test_plain_aupr_ignores_weights():
    rng = np.random.default_rng(3)
    s, y, w = rng.normal(size=200), (rng.random(200) < 0.3).astype(np.float64), rng.random(200) + 0.5
    assert build_evaluator("AUPR", y, None, w).evaluate(s) == aupr_weighted(s, y, None)
    assert aupr_weighted(s, y, w) != aupr_weighted(s, y, None)


def test_unit_weights_agree_with_the_diagnostic():
    c = boundary_case()
    ones = np.ones_like(c["weights"])
    got = host_group_aupr(c["codes"], c["labels"], ones, c["scores"])
    order = np.argsort(c["codes"], kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(c["codes"]))])
    want = np.array([binary_metrics(c["scores"][order[a:b]], c["labels"][order[a:b]])[AREA_UNDER_PRECISION_RECALL]
                     for a, b in zip(ptr[:-1], ptr[1:])])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]).max()
    print(f"max |aupr_weighted - binary_metrics| over {int(ok.sum())} groups: {err:.3e}")
    assert err <= 1e-12
    for L in BOUNDARY_LENGTHS:
        assert int(np.isfinite(got[c["lengths"] == L]).sum()) == (2 if L >= 2 else 0), L


def test_zero_weight_rows_change_nothing_bitwise():
    rng = np.random.default_rng(11)
    n = 400
    s = np.round(4.0 * rng.normal(size=n)) / 4.0
    y = (rng.random(n) < 0.35).astype(np.float64)
    w = rng.random(n) + 0.5
    base = aupr_weighted(s, y, w)
    assert math.isfinite(base)
    k = 60
    extra = {
        "tied with real rows": rng.choice(s, size=k),
        "tie groups of their own": rng.choice(s, size=k) + 0.125,
        "leading": s.max() + 1.0 + np.arange(k) % 3,
    }
    for what, es in extra.items():
        ey = (rng.random(k) < 0.5).astype(np.float64)
        at = rng.integers(0, n + 1, size=k)          # inserted anywhere; the real rows keep their order
        s2, y2, w2 = np.insert(s, at, es), np.insert(y, at, ey), np.insert(w, at, np.zeros(k))
        assert bits(aupr_weighted(s2, y2, w2)) == bits(base), what
    # all of them at once
    es = np.concatenate(list(extra.values()))
    s2, y2, w2 = np.concatenate([es, s]), np.concatenate([np.ones(3 * k), y]), np.concatenate([np.zeros(3 * k), w])
    assert bits(aupr_weighted(s2, y2, w2)) == bits(base)


def test_nan_rule():
    assert math.isnan(aupr_weighted(np.zeros(0), np.zeros(0)))
    assert math.isnan(aupr_weighted([1.0, 2.0, 3.0], [1.0, 1.0, 1.0]))
    assert math.isnan(aupr_weighted([1.0, 2.0, 3.0], [0.0, 0.0, 0.0]))
    # a class that is present only with weight 0 is missing
    assert math.isnan(aupr_weighted([1.0, 2.0, 3.0], [1.0, 0.0, 0.0], [0.0, 1.0, 1.0]))
    assert math.isnan(aupr_weighted([1.0, 2.0, 3.0], [1.0, 1.0, 0.0], [1.0, 1.0, 0.0]))
    assert aupr_weighted([2.0, 1.0], [1.0, 0.0]) == 1.0


def test_host_multi_evaluator_is_the_mean_of_the_finite_group_values():
    c = boundary_case()
    ev = AUPRMultiEvaluator("tag", c["codes"], c["labels"], None, c["weights"], device="cpu")
    got = ev.evaluate(c["scores"])
    assert ev.last_path == "host" and ev.ranking is None
    vals = host_group_aupr(c["codes"], c["labels"], c["weights"], c["scores"])
    fin = vals[np.isfinite(vals)]
    assert fin.size == 2 * (len(BOUNDARY_LENGTHS) - 1)
    assert got == float(np.mean(fin))
    keys, gv = ev.evaluate_groups(c["scores"])
    assert np.array_equal(keys, np.unique(c["codes"]))
    assert np.array_equal(np.isnan(gv.numpy()), np.isnan(vals)) and np.array_equal(gv.numpy()[~np.isnan(vals)], fin)
    # offsets are added to the scores
    off = np.where(c["labels"] > 0.5, 100.0, 0.0)
    assert AUPRMultiEvaluator("tag", c["codes"], c["labels"], off, c["weights"]).evaluate(c["scores"]) == 1.0


def small_game_fit(device, names, monkeypatch):
    """The fit of ``test_multi_eval_gpu.test_end_to_end_game_fit_and_transform`` with the evaluators ``names``;
    returns (data, estimator, result, scores every evaluator was last given)."""
    from photon_ml_amd.data.game_data import GameData
    from photon_ml_amd.data.random_effect import FixedEffectDataConfiguration, RandomEffectDataConfiguration
    from photon_ml_amd.data.synthetic import generate_game_bench_data
    from photon_ml_amd.estimators.game_estimator import GameEstimator
    from photon_ml_amd.optimization.config import GLMOptimizationConfiguration, OptimizerConfig, RegularizationContext
    raw = generate_game_bench_data(300, 12, re_dim=8, re_nnz=3, fe_dim=60, fe_nnz=5, re_vocab=1 << 12, seed=31,
                                   sizes="powerlaw", max_rows=400)
    data = GameData(raw.response, raw.shards, {"userId": raw.id_tags["entityId"]})
    seen = {}
    orig = Evaluator.evaluate

    def recording(self, scores):
        seen[self.name] = torch.as_tensor(scores).detach().to("cpu", torch.float64).clone()
        return orig(self, scores)

    monkeypatch.setattr(Evaluator, "evaluate", recording)
    cfg = GLMOptimizationConfiguration(OptimizerConfig("LBFGS", 30, 1e-8), RegularizationContext("L2"), 1.0)
    est = (GameEstimator(device=device).set_training_task("LOGISTIC_REGRESSION")
           .set_coordinate_data_configurations({"global": FixedEffectDataConfiguration("global"),
                                                "per-user": RandomEffectDataConfiguration("userId", "entity")})
           .set_coordinate_update_sequence(["global", "per-user"])
           .set_coordinate_descent_iterations(1)
           .set_validation_evaluators(names))
    res = est.fit(data, data, [{"global": cfg, "per-user": cfg}])[0]
    return data, est, res, seen


def test_game_fit_reports_the_host_values(monkeypatch):
    names = ["AUPR", "AUPR:userId"]
    data, est, res, seen = small_game_fit("cpu", names, monkeypatch)
    assert [e.name for e, _ in res.evaluations] == names
    last = est.history[0][-1]["validation"]
    z = seen["AUPR"] + torch.as_tensor(data.offsets, dtype=torch.float64)
    want = aupr_weighted(z, torch.as_tensor(data.response), None)
    assert last["AUPR"] == want and 0.2 < want < 1.0
    z = (seen["AUPR:userId"] + torch.as_tensor(data.offsets, dtype=torch.float64)).numpy()
    codes = np.unique(data.id_tags["userId"].astype(str), return_inverse=True)[1]
    vals = host_group_aupr(codes, np.asarray(data.response, dtype=np.float64),
                           np.asarray(data.weights, dtype=np.float64), z)
    fin = vals[np.isfinite(vals)]
    assert fin.size > 100
    assert abs(last["AUPR:userId"] - float(np.mean(fin))) <= 1e-12


def test_clis_select_tune_and_score_by_aupr(tmp_path):
    """game-training picks its best model by the first evaluator (AUPR), tuning takes its direction from it, and
    game-scoring evaluates both; the id tag of AUPR:userId is the random-effect type, read as for AUC:userId."""
    from photon_ml_amd.cli import game_scoring, game_training
    from photon_ml_amd.data.game_data import generate_game_data
    from photon_ml_amd.io.data_writer import write_game_avro
    data, _ = generate_game_data(n_rows=900, n_users=12, seed=3, task="LOGISTIC_REGRESSION")
    bags = {"global": "features", "user": "userFeatures"}
    write_game_avro(str(tmp_path / "train"), data.subset(np.arange(700)), bags)
    write_game_avro(str(tmp_path / "val"), data.subset(np.arange(700, 900)), bags)
    shards = ["--feature-shard-configurations", "name=global,feature.bags=features",
              "--feature-shard-configurations", "name=user,feature.bags=userFeatures,intercept=true"]
    fixed = ("name=fixed,feature.shard=global,optimizer=LBFGS,max.iter=30,tolerance=1e-8,regularization=L2,"
             "reg.weights=100|0.1")
    rand = ("name=per-user,feature.shard=user,random.effect.type=userId,optimizer=TRON,max.iter=10,tolerance=1e-8,"
            "regularization=L2,reg.weights=1")
    out = tmp_path / "out"
    args = ["--input-data-directories", str(tmp_path / "train"), "--validation-data-directories",
            str(tmp_path / "val"), "--root-output-directory", str(out), "--training-task", "LOGISTIC_REGRESSION",
            *shards, "--coordinate-configurations", fixed, "--coordinate-configurations", rand,
            "--coordinate-update-sequence", "fixed,per-user", "--coordinate-descent-iterations", "1",
            "--evaluators", "AUPR,AUPR:userId", "--output-mode", "ALL", "--device", "cpu",
            "--hyper-parameter-tuning", "RANDOM", "--hyper-parameter-tuning-iterations", "2"]
    res = game_training.GameTrainingDriver(game_training.build_parser().parse_args(args)).run()
    runs = res["explicit"] + res["tuned"]
    assert len(res["explicit"]) == 2 and len(res["tuned"]) == 2
    for r in runs:
        assert [e.name for e, _ in r.evaluations] == ["AUPR", "AUPR:userId"]
        assert all(0.0 < v <= 1.0 for _, v in r.evaluations)
    assert res["best"].evaluations[0][1] == max(r.evaluations[0][1] for r in runs)
    assert os.path.exists(out / "best" / "model-spec")
    sargs = ["--input-data-directories", str(tmp_path / "val"), "--root-output-directory", str(tmp_path / "score"),
             *shards, "--model-input-directory", str(out / "best"), "--model-id", "m", "--evaluators",
             "aupr,AUPR:userId", "--device", "cpu"]
    sres = game_scoring.GameScoringDriver(game_scoring.build_parser().parse_args(sargs)).run()
    assert [e.name for e, _ in sres["evaluations"]] == ["AUPR", "AUPR:userId"]
    for (_, got), (_, best) in zip(sres["evaluations"], res["best"].evaluations):
        assert abs(got - best) < 2e-2                   # the saved model drops coefficients below 1e-4
