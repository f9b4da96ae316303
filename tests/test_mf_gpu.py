"""Matrix-factorization coordinate on the GPU: ``mf_tron_kernel`` (``PML_MF_FUSED=1``) and the materialised route over
``re_tron_tall_kernel`` (``PML_MF_FUSED=0``) against the per-entity CPU float64 TRON, and ``mf_score_kernel``.

Rules of ``tests/test_re_parity_gpu.py``: iteration-limited (tolerance 0, 4 iterations) identical iteration counts and
W to 1e-9 relative to the largest coefficient; converged (1e-8, 60) identical counts and reasons, W to 1e-6; the
margins to the same bounds. ``mf_util.REGIMES`` says on which data each regime runs and why.

Shapes (``mf_util.HALF_SIZES``): K in {1, 7, 16, 17, 32} (the two padding classes 16 / 32 and their edges); row
entities of 1, 15, 16, 17, 32, 33 and 70 rows in one launch (the staging block of 16 rows, the two-block pipeline); a
row entity all of whose rows meet one column entity; about 15 % zero-weight rows; a non-zero partial score; ids that
arrive unsorted. The data seed of a case is 1, except where the ORACLE disagrees with itself: with K = 1 every
problem is one-dimensional, Newton's method reaches machine precision within the converged regime's iterations, and
whether the last step counts as accepted is decided by the last bit of f -- on 17 of the first 19 seeds the
per-entity TRON's own LOGISTIC counts change when an entity's rows are summed in another order. Those cases use the
first seed on which the oracle agrees with itself under two row permutations and with the CPU coordinate."""
import functools

import numpy as np
import pytest
import torch

from mf_util import CONVERGED, HALF_COLS, LIMITED, LOSSES, TASKS, half_case, half_mismatches, make_mf_data, \
    mf_coordinate, oracle_half, rel_err, start_factors, with_config

pytestmark = pytest.mark.gpu

KS = (1, 7, 16, 17, 32)
SEEDS = {(1, "LOGISTIC"): 19, (1, "POISSON"): 2}


@functools.lru_cache(maxsize=None)
def _case(K, loss):
    return half_case(K, loss, SEEDS.get((K, loss), 1))


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("K", KS)
def test_half_updates_match_cpu_tron_fp64(K, loss, fused, monkeypatch):
    monkeypatch.setenv("PML_MF_FUSED", fused)
    data, partial, ref = _case(K, loss)
    c = mf_coordinate(data, loss, K, "cuda")
    bad = half_mismatches(c, partial, ref)
    assert bad == [], (K, loss, fused, bad)


def _update(data, loss, K, device, start=None, **kw):
    c = mf_coordinate(data, loss, K, device, l2=1.0, tol=0.0, max_iter=4, alternations=2, seed=11, **kw)
    m = c.update_model(c.initialize_model() if start is None else start(c), torch.from_numpy(
        0.2 * np.cos(np.arange(data.n_rows))))
    return c, m, c.score(m)


@functools.lru_cache(maxsize=None)
def _full_update_reference():
    """Entities of 20 .. 70 rows on both sides and K = 7 at unit scale: as in the random-effect parity tests no problem
    reaches its rounding floor within 4 iterations, over the four halves of two alternations."""
    data = make_mf_data([20, 33, 47, 70, 25, 64, 31, 52], 6, 3, seed=4, loss="LOGISTIC")
    _, m, s = _update(data, "LOGISTIC", 7, "cpu")
    _, mw, sw = _update(data, "LOGISTIC", 7, "cpu", start=_foreign)
    return data, (m, s), (mw, sw)


def _foreign(c):
    """A model the coordinate has never seen, holding every other row entity and all but the first column entity."""
    from photon_ml_amd.models.game import MatrixFactorizationModel
    U, V = start_factors(c, 9)
    r, k = np.arange(len(c.row_ids))[::2], np.arange(len(c.col_ids))[1:]
    return MatrixFactorizationModel("userId", "itemId", c.task, c.row_ids[r].copy(), c.col_ids[k].copy(), U[r], V[k])


@pytest.mark.parametrize("fused", ["1", "0"])
def test_full_update_matches_cpu_coordinate(fused, monkeypatch):
    """``update_model`` with two alternations from the seeded start, and from a foreign model (mapped by entity id),
    against the CPU coordinate to the iteration-limited bound; the scores that come out of the last half's solve
    against the float64 product; two runs bitwise equal."""
    monkeypatch.setenv("PML_MF_FUSED", fused)
    data, cold, warm = _full_update_reference()
    for (m_ref, s_ref), start in ((cold, None), (warm, _foreign)):
        c, m, s = _update(data, "LOGISTIC", 7, "cuda", start=start)
        assert rel_err(m.U.cpu().numpy(), m_ref.U.numpy()) < 1e-9 and rel_err(m.V.cpu().numpy(), m_ref.V.numpy()) < 1e-9
        assert rel_err(s.cpu().numpy(), s_ref.numpy()) < 1e-9
        a, b = c.codes[0].cpu().long(), c.codes[1].cpu().long()
        exact = (m.U.cpu()[a] * m.V.cpu()[b]).sum(1)
        assert rel_err(s.cpu().numpy(), exact.numpy()) < 1e-13
        st = c.half_stats
        assert [h["entities"] for h in st] == [8, 6, 8, 6] and all(h["max_iterations"] == 4 for h in st)
        _, m2, s2 = _update(data, "LOGISTIC", 7, "cuda", start=start)
        assert torch.equal(m.U, m2.U) and torch.equal(m.V, m2.V) and torch.equal(s, s2)


@pytest.mark.parametrize("fused", ["1", "0"])
def test_more_entities_than_one_wave_of_workgroups(fused, monkeypatch):
    """3000 one-row row entities behind the sized ones: more work-groups than are resident at once. Against the CPU
    coordinate (the definition), which the per-entity oracle confirms on a sample."""
    monkeypatch.setenv("PML_MF_FUSED", fused)
    data, ref = _many_reference()
    c = with_config(mf_coordinate(data, "LOGISTIC", 7, "cuda"), LIMITED["l2"], LIMITED["tol"], LIMITED["max_iter"])
    U, V = start_factors(c, 2, LIMITED["scale"])
    for side in (0, 1):
        W, z, it, rs = c.solve_half(side, U, V)
        W_ref, z_ref, it_ref, rs_ref = ref[side]
        assert torch.equal(it.cpu(), it_ref) and torch.equal(rs.cpu(), rs_ref)
        assert rel_err(W.cpu().numpy(), W_ref.numpy()) < 1e-9 and rel_err(z.cpu().numpy(), z_ref.numpy()) < 1e-9


@functools.lru_cache(maxsize=None)
def _many_reference():
    data = make_mf_data([70, 33, 17, 16] + [1] * 3000, 40, 3, seed=6, loss="LOGISTIC")
    c = with_config(mf_coordinate(data, "LOGISTIC", 7, "cpu"), LIMITED["l2"], LIMITED["tol"], LIMITED["max_iter"])
    U, V = start_factors(c, 2, LIMITED["scale"])
    ref = [c.solve_half(side, U, V) for side in (0, 1)]
    sample = list(range(0, 3004, 75))
    W_o, it_o, rs_o, _ = oracle_half(c, 0, U, V, "LOGISTIC", LIMITED["l2"], LIMITED["tol"], LIMITED["max_iter"],
                                     entities=sample)
    assert np.array_equal(ref[0][2].numpy()[sample], it_o[sample]) and rel_err(ref[0][0].numpy()[sample],
                                                                             W_o[sample]) < 1e-9
    return data, ref


EDGE_SIZES = [1, 15, 16, 17, 31, 32, 33, 48, 49]


@functools.lru_cache(maxsize=None)
def _edge_data(loss):
    return make_mf_data(EDGE_SIZES, HALF_COLS, 3, seed=3, loss=loss)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("K", (1, 15, 16, 17, 32))
def test_fused_and_materialised_routes_bitwise_equal(K, loss, monkeypatch):
    """``mf_tron_kernel`` and ``re_tron_tall_kernel`` instantiate one solver (``tron_dense_wave``) and differ only in
    how a block of 16 rows reaches LDS, so the two routes of a coordinate agree bit for bit: factors, iteration counts
    and reasons of all four halves of two alternations, and the scores. Row entities of 1 .. 49 rows (the 16-row
    block edge, the second and third block of the two-block pipeline), K at both padding classes and their edges,
    about 15 % zero-weight rows, a partial score; four trust-region iterations at small scale (every step ends on the
    region's boundary) and up to eight at unit scale (Newton steps inside it, rejected steps)."""
    data = _edge_data(loss)
    ps = torch.from_numpy(0.3 * np.cos(np.arange(data.n_rows)))
    c = mf_coordinate(data, loss, K, "cuda", alternations=2, seed=11)
    for regime in (LIMITED, dict(CONVERGED, max_iter=8)):
        with_config(c, regime["l2"], regime["tol"], regime["max_iter"])
        U, V = start_factors(c, 5, regime["scale"])
        got = {}
        for fused in ("1", "0"):
            monkeypatch.setenv("PML_MF_FUSED", fused)
            m = c.update_model(c._model(U.cuda(), V.cuda()), ps)
            got[fused] = [m.U, m.V, c.score(m)] + [t for h in c._half_raw for t in h[:2]]
            assert len(c._half_raw) == 4 and all(int(h[0].max()) > 0 for h in c._half_raw)
        for a, b in zip(got["1"], got["0"]):
            assert torch.equal(a, b), (K, loss, regime["max_iter"], float((a - b).abs().max()))


def _raw_launch(row_ptr, oid, other, W0, K, n_rows, order=None):
    from photon_ml_amd.ops import native
    dev = "cuda"
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)
    B = len(row_ptr) - 1
    rng = np.random.default_rng(0)
    y = t((rng.random(n_rows) < 0.5).astype(float), torch.float64)
    off, wt = t(0.1 * np.sin(np.arange(n_rows)), torch.float64), t(np.ones(n_rows), torch.float64)
    W = t(W0, torch.float64).reshape(-1).contiguous()
    f = torch.empty(B, dtype=torch.float64, device=dev)
    it = torch.empty(B, dtype=torch.int32, device=dev)
    rs = torch.empty(B, dtype=torch.int32, device=dev)
    z = torch.zeros(n_rows, dtype=torch.float64, device=dev)
    scr = torch.empty(2 * max(n_rows, 1), dtype=torch.float64, device=dev)
    native.mf_tron(t(np.arange(B) if order is None else order, torch.int32), t(row_ptr, torch.int64),
                   t(oid, torch.int32), t(other, torch.float64).contiguous(), y, off, wt, scr, W, f, it, rs, z, K, 0, 1.0,
                   1e-8, 30)
    torch.cuda.synchronize()
    return W.view(B, K).cpu(), it.cpu(), rs.cpu(), z.cpu()


def test_unreferenced_table_row_and_empty_entity():
    """A column entity that occurs in no row of the launched side changes nothing (bitwise), and an entity without
    rows stays at its zero start (0 iterations, GRADIENT_CONVERGED) while its neighbours are solved."""
    K, rng = 7, np.random.default_rng(3)
    other = rng.normal(size=(6, K)) * 0.3
    row_ptr = [0, 17, 17, 40]                      # the middle entity has no rows
    oid = rng.integers(0, 5, size=40)              # table row 5 is never referenced
    W0 = np.zeros((3, K))
    full = _raw_launch(row_ptr, oid, other, W0, K, 40)
    cut = _raw_launch(row_ptr, oid, other[:5], W0, K, 40)
    for a, b in zip(full, cut):
        assert torch.equal(a, b)
    W, it, rs, _ = full
    assert not W[1].any() and int(it[1]) == 0 and int(rs[1]) == 4
    assert W[0].any() and W[2].any() and int(it[0]) > 0 and int(it[2]) > 0


def test_kernel_inputs_are_validated_before_any_launch(monkeypatch):
    monkeypatch.setenv("PML_CHECK_KERNEL_INPUTS", "1")
    K, rng = 4, np.random.default_rng(1)
    other, W0 = rng.normal(size=(5, K)), np.zeros((2, K))
    oid = rng.integers(0, 5, size=20)
    _raw_launch([0, 8, 20], oid, other, W0, K, 20)
    bad = oid.copy()
    bad[7] = 5
    with pytest.raises(ValueError, match="other-side code"):
        _raw_launch([0, 8, 20], bad, other, W0, K, 20)
    bad[7] = -1
    with pytest.raises(ValueError, match="other-side code"):
        _raw_launch([0, 8, 20], bad, other, W0, K, 20)
    with pytest.raises(ValueError, match="monotone"):
        _raw_launch([0, 21, 20], oid, other, W0, K, 20)
    with pytest.raises(ValueError, match="row_ptr"):
        _raw_launch([0, 8, 19], oid, other, W0, K, 20)
    with pytest.raises(ValueError, match="launch order"):
        _raw_launch([0, 8, 20], oid, other, W0, K, 20, order=[0, 2])
    with pytest.raises(ValueError, match="factors outside"):
        _raw_launch([0, 8, 20], oid, np.zeros((5, 33)), np.zeros((2, 33)), 33, 20)


def _score_case(K, grid):
    rng = np.random.default_rng(K)
    n, I, J = 1000, 37, 23
    U, V = rng.normal(size=(I, K)), rng.normal(size=(J, K))
    if grid:
        U, V = np.round(U * 2.0 ** 20) / 2.0 ** 20, np.round(V * 2.0 ** 20) / 2.0 ** 20
    a, b = rng.integers(-1, I, size=n), rng.integers(-1, J, size=n)
    a[:3], b[:3] = [-1, 0, -1], [0, -1, -1]
    return torch.from_numpy(U), torch.from_numpy(V), torch.from_numpy(a), torch.from_numpy(b)


@pytest.mark.parametrize("K", KS)
def test_score_kernel_matches_float64_product(K):
    """``mf_score_kernel`` against ``(U[a] * V[b]).sum(1)`` in float64, -1 codes included: within 4 ulp of the row's
    largest term (K <= 32 terms, fixed order; an ulp taken as 2^-52 times the term).

    The bound is asserted on normal factors rounded to a 2^-20 grid: their products (<= 46 significant bits) and every
    partial sum of <= 32 of them are exact in float64, so the float64 reference carries no error of its own and the
    bound measures the kernel alone. On full-mantissa normal factors it cannot: against exact rational arithmetic the
    float64 reference itself is off by up to 3.7 ulp of the largest term (K = 32; 2.7 / 3.1 / 3.0 at K = 7 / 16 / 17:
    K rounded products, then the sum) and even the correctly rounded dot product by up to 2.0 (half an ulp of a sum
    that is larger than its largest term), so two correct results differ by more than 4 -- the kernel measured 0.99 /
    3.11 / 3.67 / 4.20 ulp from the float64 reference at K = 1 / 7 / 16 / 17 on one MI355X. There the kernel is held to
    the bound against the EXACT dot product instead (rational arithmetic on the host), and its distance from the
    float64 reference is printed."""
    from fractions import Fraction
    from photon_ml_amd.ops.native import mf_score
    for grid in (True, False):
        U, V, at, bt = _score_case(K, grid)
        got = mf_score(at.to(torch.int32).cuda(), bt.to(torch.int32).cuda(), U.cuda(), V.cuda()).cpu()
        n = at.numel()
        terms = U[at.clamp(min=0)] * V[bt.clamp(min=0)]
        ok = (at >= 0) & (bt >= 0)
        want = torch.where(ok, terms.sum(1), torch.zeros(n, dtype=torch.float64))
        assert torch.equal(got[~ok], torch.zeros(int((~ok).sum()), dtype=torch.float64)) and int((~ok).sum()) >= 3
        ulp = terms.abs().max(1).values * 2.0 ** -52
        worst = float(((got - want).abs() / ulp)[ok].max())
        print(f"K={K} grid={grid}: worst distance from the float64 reference {worst:.2f} ulp of the largest term")
        if grid:
            assert worst <= 4.0, (K, worst)
            continue
        exact_worst = 0.0
        for r in torch.nonzero(ok).flatten().tolist():
            exact = sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(U[at[r]], V[bt[r]]))
            exact_worst = max(exact_worst, abs(float(Fraction(float(got[r])) - exact)) / float(ulp[r]))
        print(f"K={K}: worst distance from the exact dot product {exact_worst:.2f} ulp of the largest term")
        assert exact_worst <= 4.0, (K, exact_worst)


def test_model_scores_on_the_device_match_the_host():
    data = make_mf_data([5, 9, 17], 4, 2, seed=1, loss="SQUARED")
    c = mf_coordinate(data, "SQUARED", 3, "cpu")
    U, V = start_factors(c, 1)
    m = c._model(U, V)
    ids = dict(data.id_tags)
    ids["userId"] = ids["userId"].copy()
    ids["userId"][2] = "nobody"
    from photon_ml_amd.data.game_data import GameData
    d2 = GameData(data.response, data.shards, ids)
    host, dev = m.score(d2, "cpu"), m.score(d2, "cuda").cpu()
    assert dev[2] == 0 and host[2] == 0
    assert torch.allclose(dev, host, rtol=0, atol=1e-15)
