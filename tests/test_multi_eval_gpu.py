"""Per-group AUC / precision@k on the GPU (``seg_rank_wave_kernel`` / ``seg_rank_block_kernel`` through
``GroupedRanking`` and ``MultiEvaluator``) against the host oracle: ``auc_weighted`` / ``precision_at_k`` per group
on CPU fp64 tensors (``AreaUnderROCCurveLocalEvaluator.scala:33-70``, ``PrecisionAtKLocalEvaluator.scala:39-51``).

With the dyadic weights of ``multi_eval_cases.boundary_case`` every sum of the AUC formula is exact in fp64 in any
order, so the device value must equal the host value bitwise; precision@k is an integer over k and always exact."""
import math

import numpy as np
import pytest
import torch

from multi_eval_cases import BOUNDARY_LENGTHS, boundary_case, host_group_values, same_bits

from photon_ml_amd.evaluation.evaluators import AUCMultiEvaluator, Evaluator, build_evaluator
from photon_ml_amd.evaluation.segmented import GroupedRanking
from photon_ml_amd.ops.native import seg_rank_eval

pytestmark = pytest.mark.gpu

KS = (0, 1, 5, 100)          # 0: AUC


@pytest.fixture(scope="module")
def case():
    c = boundary_case()
    c["host"] = {k: host_group_values(c["codes"], c["labels"], c["weights"], c["scores"], k) for k in KS}
    return c


@pytest.fixture(scope="module")
def layouts(case):
    mk = lambda wg: GroupedRanking(case["codes"], case["labels"], case["weights"], device="cuda", wg_max=wg)
    return {4096: mk(4096), 64: mk(64)}


def _dev_values(lay, scores, k):
    s = torch.as_tensor(scores, dtype=torch.float64, device="cuda")
    return lay.auc(s) if k == 0 else lay.precision_at_k(s, k)


def test_oracle_is_not_vacuous(case):
    """Exactly two groups per length >= 2 have both classes (a finite AUC); the others are NaN on the host."""
    host, lens = case["host"][0], case["lengths"]
    for L in BOUNDARY_LENGTHS:
        assert int(np.isfinite(host[lens == L]).sum()) == (2 if L >= 2 else 0), L


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("wg_max", [4096, 64])
def test_boundary_lengths_bitwise(case, layouts, wg_max, k):
    """wg_max = 4096: every class; wg_max = 64: everything above 64 rows through the pre-sorted streaming kernel
    (tie groups spanning chunks: the 10000-row group with three distinct scores). Same bits either way."""
    lay = layouts[wg_max]
    cc = lay.class_counts
    if wg_max == 4096:
        assert all(cc[c] > 0 for c in ("C16", "C64", "CWG", "LONG")), cc
    else:
        assert cc["C16"] > 0 and cc["C64"] > 0 and cc["CWG"] == 0 and cc["LONG"] == int((case["lengths"] > 64).sum())
    vals = _dev_values(lay, case["scores"], k)
    assert vals.is_cuda and vals.dtype == torch.float64 and vals.shape == (lay.n_groups,)
    got, want = vals.cpu().numpy(), case["host"][k]
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    assert bad.size == 0, [(int(g), int(case["lengths"][g]), got[g], want[g]) for g in bad[:8]]
    assert same_bits(got, want)
    fin = want[np.isfinite(want)]
    assert abs(lay.mean_finite(vals) - float(np.mean(fin))) <= 1e-12


def test_arbitrary_weights_within_1e12():
    """2000 groups of 1..512 rows, weights rand + 0.5, continuous scores with 10 % duplicated inside their group.
    Three sums of <= 512 positive terms carry relative error <= 511 * 2^-53 each, so the ratio is within about
    1.7e-13 of exact for either summation order; the bound is 1e-12 absolute."""
    rng = np.random.default_rng(17)
    lens = rng.integers(1, 513, size=2000)
    codes = np.repeat(np.arange(2000), lens)
    n = codes.size
    ptr = np.concatenate([[0], np.cumsum(lens)])
    s = rng.normal(size=n)
    dup = np.nonzero(rng.random(n) < 0.1)[0]
    s[dup] = s[ptr[codes[dup]] + rng.integers(0, 1 << 30, size=dup.size) % lens[codes[dup]]]
    y = (rng.random(n) < 0.3).astype(np.float64)
    w = rng.random(n) + 0.5
    mix = rng.permutation(n)
    codes, s, y, w = codes[mix], s[mix], y[mix], w[mix]
    lay = GroupedRanking(codes, y, w, device="cuda")
    assert lay.class_counts["C16"] > 0 and lay.class_counts["C64"] > 0 and lay.class_counts["CWG"] > 0
    got = lay.auc(torch.from_numpy(s).cuda()).cpu().numpy()
    want = host_group_values(codes, y, w, s, 0)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert ok.sum() > 1500
    err = np.abs(got[ok] - want[ok]).max()
    print(f"max |device - host| AUC over {int(ok.sum())} groups: {err:.3e}")
    assert err <= 1e-12
    for k in (1, 5):
        gk = lay.precision_at_k(torch.from_numpy(s).cuda(), k).cpu().numpy()
        assert np.array_equal(gk, host_group_values(codes, y, w, s, k))


def test_deterministic(case, layouts):
    s = torch.as_tensor(case["scores"], device="cuda")
    for k in (0, 5):
        a, b = _dev_values(layouts[4096], s, k), _dev_values(layouts[4096], s, k)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))       # the same bits, NaNs included
        assert torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


def test_nan_score_takes_the_host_loop():
    rng = np.random.default_rng(2)
    n = 3000
    ids = rng.integers(0, 40, size=n)
    y = (rng.random(n) < 0.5).astype(np.float64)
    w = rng.random(n) + 0.5
    s = rng.normal(size=n)
    s[1234] = np.nan
    ev = AUCMultiEvaluator("userId", ids, y, None, w, device="cuda")
    assert ev.ranking is not None
    assert seg_rank_eval(ev.ranking, torch.from_numpy(s).cuda()) is None
    assert seg_rank_eval(ev.ranking, torch.from_numpy(s).cuda(), 3) is None
    host = AUCMultiEvaluator("userId", ids, y, None, w, device="cpu").evaluate(s)
    got = ev.evaluate(s)
    assert ev.last_path == "host"
    assert got == host or (math.isnan(got) and math.isnan(host))
    s[1234] = 0.0
    assert ev.evaluate(s) == pytest.approx(AUCMultiEvaluator("userId", ids, y, None, w).evaluate(s), abs=1e-12)
    assert ev.last_path == "device"


def test_input_validation_raises_before_launch(case, monkeypatch):
    """A layout the kernels could read out of bounds through never reaches them."""
    monkeypatch.setenv("PML_CHECK_KERNEL_INPUTS", "1")
    s = torch.as_tensor(case["scores"], device="cuda")
    mk = lambda: GroupedRanking(case["codes"], case["labels"], case["weights"], device="cuda")
    lay = mk()
    p = lay.seg_ptr.clone()
    p[3], p[4] = lay.seg_ptr[4], lay.seg_ptr[3]
    lay.seg_ptr = p                                             # decreasing
    with pytest.raises((ValueError, AssertionError)):
        seg_rank_eval(lay, s)
    lay = mk()
    p = lay.perm.clone()
    p[0] = p[1]
    lay.perm = p                                                # repeated index
    with pytest.raises((ValueError, AssertionError)):
        seg_rank_eval(lay, s)
    lay = mk()
    big = lay.lists["C64"][:1]
    lay.lists["C16"] = torch.cat([lay.lists["C16"], big])       # a 17-row group in the 16-lane class
    lay.lists["C64"] = lay.lists["C64"][1:].contiguous()
    with pytest.raises((ValueError, AssertionError)):
        seg_rank_eval(lay, s)
    with pytest.raises((ValueError, AssertionError)):
        seg_rank_eval(mk(), s[:-1].contiguous())
    with pytest.raises((ValueError, AssertionError)):
        seg_rank_eval(mk(), s.to(torch.float32))


def test_end_to_end_game_fit_and_transform(monkeypatch):
    """GameEstimator / CoordinateDescent / GameTransformer evaluate the per-group metrics on the device and report
    what the host evaluators give for the same validation scores."""
    from photon_ml_amd.data.game_data import GameData
    from photon_ml_amd.data.random_effect import FixedEffectDataConfiguration, RandomEffectDataConfiguration
    from photon_ml_amd.data.synthetic import generate_game_bench_data
    from photon_ml_amd.estimators.game_estimator import GameEstimator, GameTransformer
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    raw = generate_game_bench_data(300, 12, re_dim=8, re_nnz=3, fe_dim=60, fe_nnz=5, re_vocab=1 << 12, seed=31,
                                   sizes="powerlaw", max_rows=400)
    data = GameData(raw.response, raw.shards, {"userId": raw.id_tags["entityId"]})
    sizes = np.unique(data.id_tags["userId"].astype(str), return_counts=True)[1]
    assert sizes.size > 250 and sizes.min() <= 16 and sizes.max() > 64          # more than one size class
    names = ["AUC", "AUC:userId", "PRECISION@3:userId"]
    seen = {}
    orig = Evaluator.evaluate

    def recording(self, scores):
        seen[self.name] = torch.as_tensor(scores).detach().to("cpu", torch.float64).clone()
        return orig(self, scores)

    monkeypatch.setattr(Evaluator, "evaluate", recording)
    cfg = GLMOptimizationConfiguration(OptimizerConfig("LBFGS", 30, 1e-8), RegularizationContext("L2"), 1.0)
    est = (GameEstimator(device="cuda").set_training_task("LOGISTIC_REGRESSION")
           .set_coordinate_data_configurations({"global": FixedEffectDataConfiguration("global"),
                                                "per-user": RandomEffectDataConfiguration("userId", "entity")})
           .set_coordinate_update_sequence(["global", "per-user"])
           .set_coordinate_descent_iterations(1)
           .set_validation_evaluators(names))
    res = est.fit(data, data, [{"global": cfg, "per-user": cfg}])[0]
    by_name = {e.name: e for e, _ in res.evaluations}
    last = est.history[0][-1]["validation"]

    def host_value(name, scores):
        return build_evaluator(name, data.response, data.offsets, data.weights, data.id_tags,
                               device="cpu").evaluate(scores)

    for name in names[1:]:
        assert by_name[name].last_path == "device" and by_name[name].labels.is_cuda
        assert abs(last[name] - host_value(name, seen[name])) <= 1e-12, name
    assert not by_name["AUC"].labels.is_cuda                                   # plain AUC keeps its placement
    scores, evals = GameTransformer(res.model, names, device="cuda").transform(data)
    for e, v in evals:
        if e.name != "AUC":
            assert e.last_path == "device"
        assert abs(v - host_value(e.name, scores.detach().cpu())) <= 1e-12, e.name
