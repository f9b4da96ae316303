"""Per-group AUPR on the GPU (the third metric of ``seg_rank_wave_kernel`` / ``seg_rank_block_kernel``, through
``GroupedRanking.aupr`` and ``AUPRMultiEvaluator``) against the host oracle: ``aupr_weighted`` per group on CPU fp64
tensors.

Bound 1e-12 absolute: a value is a sum of at most G non-negative terms over P and every term carries a few roundings.
With the dyadic weights of ``boundary_case`` every prefix is exact and G <= 33, so host and device differ by at most
(G + 4) 2^-53; with arbitrary weights and at most 512 rows per group every prefix adds at most 511 * 2^-53 relative,
about 3.4e-13 in all. The device forms the prefixes before a tie group as running total + shifted prefix, never as
inclusive prefix - group sum, which the wide-range weights would expose (about 2e-11)."""
import math

import numpy as np
import pytest
import torch

from multi_eval_cases import BOUNDARY_LENGTHS, boundary_case
from test_aupr import host_group_aupr, small_game_fit

from photon_ml_amd.evaluation.evaluators import AUPRMultiEvaluator, build_evaluator
from photon_ml_amd.evaluation.segmented import GroupedRanking
from photon_ml_amd.ops.native import seg_rank_eval

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    c = boundary_case()
    c["host"] = host_group_aupr(c["codes"], c["labels"], c["weights"], c["scores"])
    return c


@pytest.fixture(scope="module")
def layouts(case):
    mk = lambda wg: GroupedRanking(case["codes"], case["labels"], case["weights"], device="cuda", wg_max=wg)
    return {4096: mk(4096), 64: mk(64)}


def compare(got, want, what, min_finite=1):
    """The same NaN pattern and at most 1e-12 apart; prints the figure before it asserts."""
    assert got.shape == want.shape
    ok = ~np.isnan(want)
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() and not np.isnan(got[ok]).any() else float("nan")
    print(f"{what}: max |device - host| AUPR over {int(ok.sum())} finite groups: {err:.3e}")
    bad = np.nonzero(np.isnan(got) != np.isnan(want))[0]
    assert bad.size == 0, [(int(g), got[g], want[g]) for g in bad[:8]]
    assert ok.sum() >= min_finite
    assert err <= 1e-12


@pytest.mark.parametrize("wg_max", [4096, 64])
def test_boundary_lengths(case, layouts, wg_max):
    """wg_max = 4096: every class; wg_max = 64: everything above 64 rows through the pre-sorted streaming kernel. The
    case holds the single-tie-group group (257 rows) and the 10000-row group with three distinct scores, whose tie
    groups span waves and chunks."""
    lay = layouts[wg_max]
    cc = lay.class_counts
    if wg_max == 4096:
        assert all(cc[c] > 0 for c in ("C16", "C64", "CWG", "LONG")), cc
    else:
        assert cc["C16"] > 0 and cc["C64"] > 0 and cc["CWG"] == 0 and cc["LONG"] == int((case["lengths"] > 64).sum())
    vals = lay.aupr(torch.as_tensor(case["scores"], dtype=torch.float64, device="cuda"))
    assert vals.is_cuda and vals.dtype == torch.float64 and vals.shape == (lay.n_groups,)
    got, want = vals.cpu().numpy(), case["host"]
    for L in BOUNDARY_LENGTHS:
        assert int(np.isfinite(want[case["lengths"] == L]).sum()) == (2 if L >= 2 else 0), L
    compare(got, want, f"boundary wg_max={wg_max}", min_finite=28)
    fin = want[np.isfinite(want)]
    assert abs(lay.mean_finite(vals) - float(np.mean(fin))) <= 1e-12
    # the existing selectors still mean what they meant
    s = torch.as_tensor(case["scores"], dtype=torch.float64, device="cuda")
    assert torch.equal(seg_rank_eval(lay, s).view(torch.int64), seg_rank_eval(lay, s, 0, "auc").view(torch.int64))
    assert torch.equal(seg_rank_eval(lay, s, 5), seg_rank_eval(lay, s, 5, "precision"))
    with pytest.raises(ValueError):
        seg_rank_eval(lay, s, 5, "aupr")


def ragged_case(seed, kind):
    """2000 groups of 1..512 rows, 30 % positives; "arbitrary": the data of
    ``test_multi_eval_gpu.test_arbitrary_weights_within_1e12`` (continuous scores, 10 % duplicated inside their
    group, weights rand + 0.5); "wide": scores on a grid of 1/8, weights 10^(-9 u), nine orders of magnitude."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 513, size=2000)
    codes = np.repeat(np.arange(2000), lens)
    n = codes.size
    ptr = np.concatenate([[0], np.cumsum(lens)])
    s = rng.normal(size=n)
    if kind == "arbitrary":
        dup = np.nonzero(rng.random(n) < 0.1)[0]
        s[dup] = s[ptr[codes[dup]] + rng.integers(0, 1 << 30, size=dup.size) % lens[codes[dup]]]
    else:
        s = np.round(8.0 * s) / 8.0
    y = (rng.random(n) < 0.3).astype(np.float64)
    w = rng.random(n) + 0.5 if kind == "arbitrary" else 10.0 ** (-9.0 * rng.random(n))
    mix = rng.permutation(n)
    return codes[mix], y[mix], w[mix], s[mix]


@pytest.mark.parametrize("kind,seed,min_finite", [("arbitrary", 17, 1501), ("wide", 23, 1992)])
def test_ragged_groups_within_1e12(kind, seed, min_finite):
    codes, y, w, s = ragged_case(seed, kind)
    lay = GroupedRanking(codes, y, w, device="cuda")
    assert lay.class_counts["C16"] > 0 and lay.class_counts["C64"] > 0 and lay.class_counts["CWG"] > 0
    got = lay.aupr(torch.from_numpy(s).cuda()).cpu().numpy()
    compare(got, host_group_aupr(codes, y, w, s), f"{kind} weights", min_finite=min_finite)
    # the streaming kernel on the same groups
    lay0 = GroupedRanking(codes, y, w, device="cuda", wg_max=0)
    assert lay0.class_counts["LONG"] == 2000
    got0 = lay0.aupr(torch.from_numpy(s).cuda()).cpu().numpy()
    compare(got0, host_group_aupr(codes, y, w, s), f"{kind} weights, pre-sorted", min_finite=min_finite)


def test_zero_weights_on_the_device():
    """30 % of the rows at weight 0: tied with real rows, whole leading tie groups at weight 0 (the top two scores
    of every group), and one group whose positive rows all have weight 0 (NaN)."""
    rng = np.random.default_rng(41)
    lens = (3, 16, 17, 64, 65, 300, 5000, 40)
    cols = []
    for g, L in enumerate(lens):
        s = np.round(4.0 * rng.normal(size=L)) / 4.0
        y = (rng.random(L) < 0.4).astype(np.float64)
        w = rng.integers(1, 2049, size=L).astype(np.float64) / 1024.0
        w[rng.random(L) < 0.3] = 0.0
        top = np.unique(s)[-2:]
        w[np.isin(s, top)] = 0.0                       # leading tie groups of weight 0
        if L == 3:
            s, y, w = np.array([2.0, 1.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.5, 1.5])
        if L == 40:
            w[y > 0.5] = 0.0                           # positives present, all at weight 0
            assert (y > 0.5).any() and w[y < 0.5].sum() > 0
        cols.append((np.full(L, g), y, w, s))
    codes, y, w, s = (np.concatenate(c) for c in zip(*cols))
    mix = rng.permutation(codes.size)
    codes, y, w, s = codes[mix], y[mix], w[mix], s[mix]
    assert 0.25 < (w == 0).mean() < 0.5
    want = host_group_aupr(codes, y, w, s)
    assert np.isnan(want[7]) and np.isfinite(want[:7]).all() and want[0] == 1.0
    for wg in (4096, 64):
        lay = GroupedRanking(codes, y, w, device="cuda", wg_max=wg)
        compare(lay.aupr(torch.from_numpy(s).cuda()).cpu().numpy(), want, f"zero weights wg_max={wg}", min_finite=7)


def test_deterministic(case, layouts):
    s = torch.as_tensor(case["scores"], device="cuda")
    for wg in (4096, 64):
        a, b = layouts[wg].aupr(s), layouts[wg].aupr(s)
        assert torch.isnan(a).any() and torch.isfinite(a).any()
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))       # the same bits, NaNs included


def test_nan_score_takes_the_host_loop():
    rng = np.random.default_rng(2)
    n = 3000
    ids = rng.integers(0, 40, size=n)
    y = (rng.random(n) < 0.5).astype(np.float64)
    w = rng.random(n) + 0.5
    s = rng.normal(size=n)
    s[1234] = np.nan
    ev = AUPRMultiEvaluator("userId", ids, y, None, w, device="cuda")
    assert ev.ranking is not None
    assert seg_rank_eval(ev.ranking, torch.from_numpy(s).cuda(), metric="aupr") is None
    assert ev.ranking.aupr(torch.from_numpy(s).cuda()) is None
    host = AUPRMultiEvaluator("userId", ids, y, None, w, device="cpu").evaluate(s)
    got = ev.evaluate(s)
    assert ev.last_path == "host"
    assert got == host or (math.isnan(got) and math.isnan(host))
    s[1234] = 0.0
    assert abs(ev.evaluate(s) - AUPRMultiEvaluator("userId", ids, y, None, w).evaluate(s)) <= 1e-12
    assert ev.last_path == "device"


def test_end_to_end_game_fit_and_transform(monkeypatch):
    from photon_ml_amd.estimators.game_estimator import GameTransformer
    names = ["AUPR", "AUPR:userId"]
    data, est, res, seen = small_game_fit("cuda", names, monkeypatch)
    by_name = {e.name: e for e, _ in res.evaluations}
    last = est.history[0][-1]["validation"]

    def host_value(name, scores):
        return build_evaluator(name, data.response, data.offsets, data.weights, data.id_tags,
                               device="cpu").evaluate(scores)

    assert by_name["AUPR:userId"].last_path == "device" and by_name["AUPR:userId"].labels.is_cuda
    assert not by_name["AUPR"].labels.is_cuda                                  # plain AUPR is placed like plain AUC
    for name in names:
        assert math.isfinite(last[name])
        assert abs(last[name] - host_value(name, seen[name])) <= 1e-12, name
    scores, evals = GameTransformer(res.model, names, device="cuda").transform(data)
    assert [e.name for e, _ in evals] == names
    for e, v in evals:
        if e.name != "AUPR":
            assert e.last_path == "device"
        assert abs(v - host_value(e.name, scores.detach().cpu())) <= 1e-12, e.name
