"""The fused random-effect solvers at the edges of their size classes and on ragged rows, entity by entity against
the CPU float64 TRON (``re_parity_util.cpu_tron``), with the regimes and bounds of
``test_re_weighted_parity_gpu.py``.

The data comes from ``re_parity_util.make_ragged_entities`` (``re_boundary_cases.py`` holds the shapes,
``test_re_boundary_shapes.py`` checks on the CPU that the data is what the cases say): no intercept, exact projected
widths, rows of RAGGED = 0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 67, 68, 69, 130 entries (clipped to d_e), weights in
[0.25, 4] with about 15 % of the rows at exactly 0, base offsets ``0.3 sin(i)``. Every case first asserts, from
``c._comps``, ``fused.launches``, ``fused.quad``, ``fused.res`` and ``rs.classes``, that its entities reached the
kernel instantiation it names; a case that routes elsewhere fails.

Cases (LOGISTIC; ``lean_quad`` and ``mixed`` with all three losses):

* ``lean_scalar`` / ``lean_quad`` -- ``re_tron_lean_kernel<LOSS, J, Q>`` at d_e = 65, 255, 256 (J = 1, launch 256),
  257, 511, 512 (J = 2, launch 512), 513, 1023, 1024 (J = 4, launch 1024); scalar rows (``row_pass``, mean row
  below 12 entries) and quad-padded rows (``row_pass_q``, QUADDY = 13 ... 130 entries);
* ``narrow_scalar`` / ``narrow_quad`` -- launches narrower than their class: a coordinate of d_e = 70, 257, 513
  (launch widths 72 / J = 1, 264 / J = 2, 520 / J = 4) and one of d_e = 1009 (launch width 1016);
* ``tall`` -- ``re_tron_tall_kernel<T, LOSS>``, T = 1 .. 4 at d_e = 1, 15, 16 | 17, 32 | 33, 48 | 49, 64 (the
  Hessian inside the function evaluation up to 32) over 1, 15, 16, 17, 31, 33 and 100 rows; one entity of 65
  coefficients in the same coordinate lands in a lean launch of width 72;
* ``csr`` -- ``re_tron_csr_kernel`` at d_e = 1025, 2047, 2048; an entity of 2049 coefficients in the same
  coordinate goes to the pass path and is compared with the oracle all the same;
* ``resident`` -- ``re_tron_res_kernel`` (forced) at d_e = 65, 512 and its LDS image's width, rows of up to exactly
  64 entries, entities of cap - 1, cap, cap + 1, 2 cap and 2 cap + 1 rows (one workgroup, clusters of 2 and of 3);
  an entity with one row of 65 entries is refused by the selection and solved by a lean launch (so the resident
  launch holds every entity of the fused batch but that one);
* ``rs_small`` -- the row-space route (``seg_gram_kernel`` -> ``batched_chol_kernel`` -> ``rs_tron_*`` -> ``btrsv``
  -> ``rs_primal``) through the coordinate for 1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17 and 24 rows over n_e, n_e + 1
  and 200 coefficients: the classes of 1, 2, 4, 8, 12, 16 and 24 rows;
* ``rs_fail`` -- one row-space class whose members with a duplicated row or a row without entries fail their
  Cholesky factor: they move to the fused primal batch (``RowSpaceBatch.__init__``, ``if not good``), the healthy
  ones stay;
* ``mixed`` -- production routing, nothing forced: row-space entities, a failed factor, tall entities (16, 64), lean
  entities (257, 1009), a CSR entity (2048) and a pass-path entity (2049) write their ranges of one packed vector;
  the update run twice is bitwise the same on a second coordinate; an entity without any entry (d_e = 0) added
  to it does what the CPU coordinate does with it and changes no bit of the others.

Regimes and bounds are the project's (``test_re_weighted_parity_gpu.py``): (a) cold, tolerance 0: exactly 4
iterations and MAX_ITERATIONS on both sides; (b) cold, tolerance 1e-8, at most 60 iterations: the same iteration
count and stop reason for EVERY entity; (c) warm from a foreign model (the GPU's model of (b), halved) under the
partial score ``0.3 cos(i)``, tolerance 0. W within ``max(1e-9 (a, c) or 1e-6 (b), 8 floor)`` of the oracle, the
floor being the oracle against itself with every entity's rows permuted (``perm_seed=1``); it never looks at the
GPU. The scores of (a) on every row within ``1e-12 (1 + sum_j |x_ij w_j|)`` of the fp64 CPU product, and exactly
0.0 on rows without entries.

Seeds. They are chosen on the CPU, by the oracle alone, and hold for every case, loss and entity: the oracle takes
exactly 4 iterations and stops on MAX_ITERATIONS in (a) and in (c) (there from its own (b) model, halved), and its
iteration counts and stop reasons at tolerance 1e-8 agree under ``perm_seed`` in {None, 1, 2, 3}. There is no
allowed share of mismatches and no skipped entity.

Entities of at most 5 rows or 5 coefficients need more than that, because for them TRON is an exact Newton
iteration (CG ends within its dimension) that reaches the rounding level in 3 to 5 iterations, so "exactly 4
iterations at tolerance 0" can be decided by the last bit of ``f``; and a permutation of 1 to 3 rows samples no
other rounding (floor exactly 0). Under most seeds the oracle ITSELF does not take 4 iterations for such an entity
(847 of 1050 seeds of ``rs_small``; mostly 2 or 3 and OBJECTIVE_NOT_IMPROVING), or moves by 1e-8 and loses an
iteration when the entity's columns were permuted or the warm start changed in its last bit -- and there the GPU
differed in the same way (``rs_small``: 3 against 4 iterations for the entity of 1 row; ``mixed`` POISSON (c),
seed 11: 1.3e-8 for the entity of 3 rows, the oracle under a column permutation 1.2e-8). So for these entities the
seeds also satisfy, again on the oracle alone: counts, reasons and W (to half the bound) of (a), (b) and (c) are
unchanged under three permutations of the columns and under a warm start scaled by 1 +- 1e-15; the oracle run on
the entity's row-space form (design matrix ``chol(X X^T)``) has the same counts and reasons; and the oracle still
iterates under a limit of 5 (LOGISTIC and POISSON; for SQUARED a Newton step is exact and no seed has that margin).
The seeds of ``tall`` (6), ``rs_small`` (125) and ``mixed`` (55) are the first that passed. (``mixed`` seed 106
is rejected: run on its 257-wide entity alone under eight more row and column permutations, the oracle takes 22
or 23 POISSON iterations and moves by up to 3.3e-8 in SQUARED (a); the GPU differed there by as much.)

Measured on an MI355X (worst entity per case; each cell is "oracle floor / GPU error" relative to the entity's
largest coefficient; the last column is the worst ``|s - x.w| / (1 + sum |x w|)``). Reached: lean launches of width
256, 512, 1024 (J = 1, 2, 4; scalar and quad rows), 72, 264, 520, 1016; tall launches 16, 32, 48, 64 (T = 1 .. 4)
and the lean launch 72 next to them; CSR launch 2048 with the pass path next to it; the resident launch with
tasks of 1, 1, 2, 2, 3, 3 workgroups and the lean launch 304 next to it; row-space classes 1, 2, 4, 8, 12, 16, 24;
``mixed``: row-space classes 3, 12, 20, tall 16, 32, 64, lean 264, 1016, CSR 2048, pass path.

    case             loss      (a) limited     (b) converged   (c) warm        scores
    ---------------------------------------------------------------------------------
    lean_scalar      LOGISTIC  5e-14 / 8e-14   7e-16 / 7e-16   7e-16 / 6e-16   3e-16
    lean_quad        LOGISTIC  8e-16 / 9e-16   7e-16 / 8e-16   9e-16 / 7e-16   3e-16
    lean_quad        POISSON   4e-09 / 3e-09   6e-08 / 5e-08   3e-15 / 8e-15   3e-16
    lean_quad        SQUARED   9e-11 / 7e-10   6e-10 / 2e-09   6e-12 / 4e-11   4e-16
    narrow_scalar_a  LOGISTIC  5e-16 / 2e-15   7e-16 / 6e-16   4e-16 / 4e-16   2e-16
    narrow_scalar_b  LOGISTIC  2e-15 / 1e-15   5e-16 / 6e-16   4e-16 / 4e-16   2e-16
    narrow_quad_a    LOGISTIC  6e-16 / 9e-16   1e-15 / 6e-16   8e-16 / 6e-16   2e-16
    narrow_quad_b    LOGISTIC  4e-16 / 8e-16   3e-16 / 6e-16   4e-16 / 5e-16   3e-16
    tall             LOGISTIC  4e-16 / 1e-15   6e-16 / 5e-16   6e-16 / 7e-16   2e-16
    csr (+ pass)     LOGISTIC  6e-15 / 2e-14   6e-16 / 5e-16   6e-16 / 6e-16   3e-16
    resident         LOGISTIC  5e-16 / 9e-16   5e-16 / 7e-16   6e-16 / 5e-16   3e-16
    rs_small         LOGISTIC  3e-16 / 5e-16   3e-16 / 1e-15   2e-16 / 5e-16   3e-16
    rs_fail          LOGISTIC  9e-16 / 7e-16   8e-16 / 6e-16   8e-16 / 5e-16   5e-16
    mixed            LOGISTIC  9e-15 / 2e-15   1e-15 / 7e-16   1e-15 / 9e-16   4e-16
    mixed            POISSON   2e-15 / 6e-15   3e-04 / 8e-05   3e-14 / 3e-14   4e-16
    mixed            SQUARED   7e-08 / 3e-08   9e-10 / 1e-10   4e-08 / 3e-08   4e-16

The ``8 floor`` branch of the bound was needed by no case whose floor was below the project bound. The entity
without any entry stopped after 0 iterations with GRADIENT_CONVERGED, as on the CPU coordinate.

``rs_fail`` found a defect: the factor test of ``RowSpaceBatch`` was the sign of the pivot alone, and a duplicated
row leaves a pivot of +-eps K_jj, so 2 of the 3 entities with a duplicated row stayed in the row-space batch with
pivots of 1.6e-16 and 3.8e-17 times their diagonal entries (their results still matched the oracle to 4e-16 in
(a), (b) and (c): the near-zero pivot cancels in ``L^-T beta``). The hand-over is now decided by the pivot
relative to its diagonal entry (``row_space.RS_PIVOT_RTOL``), not by the sign of a rounding error.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from photon_ml_amd.optimization.optimizer import ConvergenceReason
from re_boundary_cases import MIXED, RS_FAIL, case_data
from re_parity_util import TASKS, _set_route, cpu_tron, foreign_model, gpu_fit, reference_floor, rel_err

pytestmark = pytest.mark.gpu

L2 = 1.0
LIMITED = (0.0, 4)           # tolerance 0: exactly 4 iterations
CONVERGED = (1e-8, 60)
BOUND = {LIMITED: 1e-9, CONVERGED: 1e-6}
LOSSES = ("LOGISTIC", "POISSON", "SQUARED")


def _res_params():
    from photon_ml_amd.ops import native
    return native.re_res_params()


def _data(name, loss="LOGISTIC"):
    if name == "resident":
        cap, rdmax, _ = _res_params()
        return case_data(name, loss, cap, rdmax)
    return case_data(name, loss)


@functools.lru_cache(maxsize=None)
def _reference(name, loss, regime):
    """The oracle's cold fit of a case (never modified) and the floor against the fit with permuted rows."""
    data = _data(name, loss)
    ref = cpu_tron(data, loss, L2, *regime)
    return ref, reference_floor(ref, cpu_tron(data, loss, L2, *regime, perm_seed=1))


def _compare(tag, regime, ref, floor, W, its, reasons):
    """Iteration counts and stop reasons equal per entity, W within max(project bound, 8 floor)."""
    bound = max(BOUND[regime], 8 * floor)
    errs = {}
    for e, (w_ref, it_ref, reason_ref) in ref.items():
        if regime == LIMITED:
            assert its[e] == it_ref == 4, (tag, e, its[e], it_ref)
            assert reasons[e] == reason_ref == ConvergenceReason.MAX_ITERATIONS, (tag, e, reasons[e], reason_ref)
        assert its[e] == it_ref, (tag, e, its[e], it_ref)
        assert reasons[e] == reason_ref, (tag, e, reasons[e], reason_ref)
        errs[e] = rel_err(W[e], w_ref)
    worst = max(errs.values())
    print(f"BOUNDARY {tag}: floor {floor:.2e} bound {bound:.2e} gpu error {worst:.2e}")
    for e, err in errs.items():
        assert err <= bound, (tag, e, err, bound, floor)


def _check_scores(tag, data, score, W):
    """The coordinate's scores against the fp64 CPU product X W_gpu, per row within 1e-12 (1 + sum_j |x_ij w_j|);
    rows without entries score exactly 0.0."""
    x, ids = data.shards["user"].tocsr(), data.id_tags["userId"]
    want, scale = np.zeros(data.n_rows), np.zeros(data.n_rows)
    for e in np.unique(ids):
        r = np.nonzero(ids == e)[0]
        want[r] = x[r] @ W[e]
        scale[r] = abs(x[r]) @ np.abs(W[e])
    assert np.isfinite(score).all()
    excess = np.abs(score - want) / (1.0 + scale)
    empty = np.diff(x.indptr) == 0
    print(f"BOUNDARY {tag}: scores, worst |s - x.w| / (1 + sum |x w|) = {excess.max():.2e}; {int(empty.sum())} rows "
          f"without entries")
    assert (excess <= 1e-12).all(), (tag, int(excess.argmax()), float(excess.max()))
    assert (score[empty] == 0.0).all(), (tag, np.nonzero(empty)[0][score[empty] != 0.0])


def _widths(fused, hess):
    return sorted(dm for dm, _, h in fused.launches if h == hess)


def _launch_entities(c, fused, dm, hess=False):
    """Entity ids of the launch of width ``dm``."""
    found = [order for d, order, h in fused.launches if d == dm and h == hess]
    assert len(found) == 1, (dm, hess, [(d, h) for d, _, h in fused.launches])
    return sorted(int(c.dataset.entity_ids[k]) for k in fused.ents[found[0].long()].tolist())


def _ids(c, ents):
    return sorted(int(c.dataset.entity_ids[k]) for k in ents.tolist())


def _three_regimes(tag, name, loss, data, monkeypatch, check_routing):
    """(a), the scores of (a), (b) and (c) of one coordinate's data against the oracle; ``check_routing(c)`` runs
    on the first coordinate, before anything is compared. Returns the coordinate and model of (a)."""
    W, its, reasons, c, m = gpu_fit(data, loss, L2, *LIMITED, monkeypatch)
    assert c.dataset.layout == "segmented"
    check_routing(c)
    first = (c, m, W)
    score = c.score(m).cpu().numpy()
    ref, floor = _reference(name, loss, LIMITED)
    _compare(f"{tag} limited", LIMITED, ref, floor, W, its, reasons)
    _check_scores(tag, data, score, W)
    W, its, reasons, c, m = gpu_fit(data, loss, L2, *CONVERGED, monkeypatch)
    check_routing(c)
    ref, floor = _reference(name, loss, CONVERGED)
    _compare(f"{tag} converged", CONVERGED, ref, floor, W, its, reasons)
    partial = 0.3 * np.cos(np.arange(data.n_rows))
    w_half = {e: W[e] * 0.5 for e in W}
    W2, its2, reasons2, c2, _ = gpu_fit(data, loss, L2, *LIMITED, monkeypatch, partial=partial,
                                        start=foreign_model(m, w_half, loss))
    check_routing(c2)
    ref2 = cpu_tron(data, loss, L2, *LIMITED, partial=partial, w0=w_half)
    floor2 = reference_floor(ref2, cpu_tron(data, loss, L2, *LIMITED, partial=partial, w0=w_half, perm_seed=1))
    _compare(f"{tag} warm", LIMITED, ref2, floor2, W2, its2, reasons2)
    return first


def _lean_only(c, n):
    rs, fused, sub = c._comps
    assert rs is None and sub is None and fused is not None and fused.B == n == len(c.dataset.entity_ids)
    assert fused.res is None and not _widths(fused, True)
    return fused


@pytest.mark.parametrize("rows,loss", [("scalar", "LOGISTIC")] + [("quad", loss) for loss in LOSSES])
def test_lean_kernel_at_every_width_class_edge(rows, loss, monkeypatch):
    """J = 1 / 2 / 4 at both ends of their width ranges, on scalar rows and on quad-padded rows (all three losses
    for the quad rows, the kernel of the benchmark workload)."""
    _set_route(f"lean_{rows}", monkeypatch)
    name = f"lean_{rows}"

    def routing(c):
        fused = _lean_only(c, 9)
        assert fused.quad == (rows == "quad")
        assert _widths(fused, False) == [256, 512, 1024]
        assert _launch_entities(c, fused, 256) == [0, 1, 2]            # 65, 255, 256: J = 1
        assert _launch_entities(c, fused, 512) == [3, 4, 5]            # 257, 511, 512: J = 2
        assert _launch_entities(c, fused, 1024) == [6, 7, 8]           # 513, 1023, 1024: J = 4
    _three_regimes(f"{name} {loss}", name, loss, _data(name, loss), monkeypatch, routing)


@pytest.mark.parametrize("rows", ["scalar", "quad"])
def test_lean_launch_narrower_than_its_class(rows, monkeypatch):
    """The LDS image of a lean launch is its widest entity rounded up to 8: 72 (J = 1), 264 (J = 2), 520 and 1016
    (J = 4) -- widths just above a J switch that are no multiple of the class."""
    _set_route(f"lean_{rows}", monkeypatch)
    for part, widths in (("a", [72, 264, 520]), ("b", [1016])):
        name = f"narrow_{rows}_{part}"

        def routing(c):
            fused = _lean_only(c, len(widths))
            assert fused.quad == (rows == "quad")
            assert _widths(fused, False) == widths
        _three_regimes(name, name, "LOGISTIC", _data(name), monkeypatch, routing)


def test_tall_kernel_every_tile_count(monkeypatch):
    """T = 1 .. 4 at both ends of their width ranges, entities of 1 and of 15 / 16 / 17 rows (the 16-row staging
    block), rows without entries and full rows; the 65-wide entity of the coordinate is a lean launch."""
    _set_route("tall", monkeypatch)
    monkeypatch.setenv("PML_RE_ROW_SPACE", "0")

    def routing(c):
        rs, fused, sub = c._comps
        assert rs is None and sub is None and fused.B == 14 and fused.res is None and not fused.quad
        assert _widths(fused, True) == [16, 32, 48, 64]
        assert _launch_entities(c, fused, 16, True) == [0, 1, 2, 10]   # d_e 1, 15, 16, 16: T = 1
        assert _launch_entities(c, fused, 32, True) == [3, 4, 11, 12]  # 17, 32, 32, 17: T = 2
        assert _launch_entities(c, fused, 48, True) == [5, 6]          # 33, 48: T = 3
        assert _launch_entities(c, fused, 64, True) == [7, 8, 9]       # 49, 64, 64: T = 4
        assert _widths(fused, False) == [72] and _launch_entities(c, fused, 72) == [13]
    _three_regimes("tall", "tall", "LOGISTIC", _data("tall"), monkeypatch, routing)


def test_csr_kernel_at_its_width_edges(monkeypatch):
    """d_e = 1025, 2047 and 2048 in the CSR kernel; 2049 is one too many and goes to the pass path, where it is
    held to the same bounds."""
    _set_route("csr", monkeypatch)

    def routing(c):
        rs, fused, sub = c._comps
        assert rs is None and fused.B == 3 and _ids(c, fused.ents) == [0, 1, 2] and fused.res is None
        assert not _widths(fused, True) and all(dm > 1024 for dm in _widths(fused, False))
        assert sub is not None and _ids(c, sub.entities) == [3]
        assert c.solver_routing()["pass_path"] == 1
    _three_regimes("csr", "csr", "LOGISTIC", _data("csr"), monkeypatch, routing)


def test_resident_kernel_at_its_capacity_edges(monkeypatch):
    """Rows of exactly 64 entries, entities of cap - 1 .. 2 cap + 1 rows, the widest LDS image; one row of 65
    entries keeps an entity out."""
    _set_route("resident", monkeypatch)
    cap, rdmax, grid = _res_params()

    def routing(c):
        rs, fused, sub = c._comps
        assert rs is None and sub is None and fused.B == 7
        # every entity of the fused batch but the one with a row of 65 entries
        assert fused.res is not None and fused.res["n"] == fused.B - 1 and fused.res["clusters"] >= 3
        assert _ids(c, fused.ents[fused.res["ent"].long()]) == list(range(6))
        assert sorted((fused.res["t0"][1:] - fused.res["t0"][:-1]).tolist()) == [1, 1, 2, 2, 3, 3]
        assert len(fused.launches) == 1 and _launch_entities(c, fused, 304) == [6]
    _three_regimes("resident", "resident", "LOGISTIC", _data("resident"), monkeypatch, routing)


def _default_routing(monkeypatch):
    """Production routing: nothing forced (the policies at their defaults whatever the environment says)."""
    import photon_ml_amd.optimization.entity_tron as et
    for k in ("PML_RE_ROW_SPACE", "PML_RE_FUSED", "PML_RE_QUAD", "PML_RS_NMAX", "PML_RE_OVERLAP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(et, "RESIDENT", "auto")


def test_row_space_small_classes_through_the_coordinate(monkeypatch):
    """Gram matrix, Cholesky factor, row-space TRON and back-map for the classes of 1 .. 24 rows."""
    _default_routing(monkeypatch)

    def routing(c):
        rs, fused, sub = c._comps
        assert fused is None and sub is None and rs is not None and rs.B == 12
        assert sorted(cl.n for cl in rs.classes) == [1, 2, 4, 8, 12, 16, 24]
    _three_regimes("rs_small", "rs_small", "LOGISTIC", _data("rs_small"), monkeypatch, routing)


def test_row_space_failed_factor_moves_to_the_fused_batch(monkeypatch):
    """A class with healthy and singular members (duplicated row; row without entries): the healthy ones stay, the
    singular ones are solved by the fused primal batch, every one matches the oracle."""
    _default_routing(monkeypatch)

    def routing(c):
        rs, fused, sub = c._comps
        assert sub is None and rs is not None and fused is not None
        assert [cl.n for cl in rs.classes] == [16]
        assert rs.B == len(RS_FAIL["healthy"]) and _ids(c, rs.ents) == list(RS_FAIL["healthy"])
        assert _ids(c, fused.ents) == list(RS_FAIL["singular"])
    _three_regimes("rs_fail", "rs_fail", "LOGISTIC", _data("rs_fail"), monkeypatch, routing)


def _mixed_routing(c, more_pass_path=()):
    rs, fused, sub = c._comps
    routes = c.solver_routing()
    passed = list(MIXED["pass_path"]) + list(more_pass_path)
    assert (routes["row_space"], routes["fused"], routes["pass_path"]) == (3, 6, len(passed)), routes
    # the class of 9 .. 12 rows holds the healthy entity of 11 rows and the failed one of 12
    assert _ids(c, rs.ents) == list(MIXED["row_space"]) and sorted(cl.n for cl in rs.classes) == [3, 12, 20]
    assert _ids(c, fused.ents) == list(MIXED["fused"]) and _ids(c, sub.entities) == passed
    assert fused.res is None and not fused.quad and routes["heavy_to_pass_path"] == 0
    assert _widths(fused, True) == [16, 32, 64] and _widths(fused, False) == [264, 1016, 2048]
    assert _launch_entities(c, fused, 32, True) == [3]                 # the failed factor (30 coefficients)
    assert _launch_entities(c, fused, 2048) == [8]


def _coefficients(m):
    if hasattr(m, "materialize"):
        m.materialize()
    return {e: np.asarray(m.coefficients_of(e).means, dtype=np.float64) for e in m.entity_ids}


@pytest.mark.parametrize("loss", LOSSES)
def test_mixed_coordinate(loss, monkeypatch):
    """Every component writes its range of one packed coefficient vector; all of it against the oracle, and the
    update run twice is bitwise reproducible."""
    _default_routing(monkeypatch)
    data = _data("mixed", loss)
    c, m, W = _three_regimes(f"mixed {loss}", "mixed", loss, data, monkeypatch, _mixed_routing)
    # a second update from the returned model (each component's own warm state), on two coordinates
    W_2 = _coefficients(c.update_model(m, None))
    Wb, _, _, cb, mb = gpu_fit(data, loss, L2, *LIMITED, monkeypatch)
    assert all(np.array_equal(W[e], Wb[e]) for e in W)
    Wb_2 = _coefficients(cb.update_model(mb, None))
    assert any(not np.array_equal(W_2[e], W[e]) for e in W)
    for e in W_2:
        assert np.array_equal(W_2[e], Wb_2[e]), (loss, e, rel_err(W_2[e], Wb_2[e]))


def _with_empty_entity(data, n=5):
    """``data`` plus one entity of ``n`` rows without any entry (d_e = 0); every other row unchanged."""
    from photon_ml_amd.data.game_data import GameData
    x, ids, r = data.shards["user"].tocsr(), data.id_tags["userId"], data.n_rows
    return GameData(np.concatenate([data.response, (np.arange(n) % 2).astype(float)]),
                    {"user": sp.vstack([x, sp.csr_matrix((n, x.shape[1]))]).tocsr()},
                    {"userId": np.concatenate([ids, np.full(n, ids.max() + 1)])},
                    offsets=np.concatenate([data.offsets, 0.3 * np.sin(np.arange(r, r + n))]),
                    weights=np.concatenate([data.weights, np.full(n, 1.5)]))


def _cpu_coordinate_fit(data, loss):
    from photon_ml_amd.algorithm.coordinates import RandomEffectCoordinate
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    cfg = GLMOptimizationConfiguration(OptimizerConfig("TRON", LIMITED[1], LIMITED[0]), RegularizationContext("L2"), L2)
    c = RandomEffectCoordinate("u", data, RandomEffectDataConfiguration("userId", "user"), cfg, TASKS[loss],
                               device="cpu", layout="segmented")
    m = c.update_model(c.initialize_model(), None)
    return _coefficients(m), c.score(m).cpu().numpy()


def test_entity_without_any_entry_in_the_mixed_coordinate(monkeypatch):
    """The yardstick for an entity whose every row is empty is the CPU coordinate (``device="cpu"``, segmented) on
    the same data: the GPU coordinate does what that one does -- no coefficients and scores of exactly 0, or the
    same exception type -- and every other entity's result is bitwise the one of the mixed coordinate without
    that entity."""
    _default_routing(monkeypatch)
    loss = "LOGISTIC"
    base = _data("mixed", loss)
    # a small stand-in for the CPU yardstick (the CPU coordinate's answer does not depend on the other entities)
    small = _with_empty_entity(case_data("narrow_scalar_a"))
    data = _with_empty_entity(base)
    e0 = int(base.id_tags["userId"].max()) + 1
    own = data.id_tags["userId"] == e0
    try:
        W_cpu, s_cpu = _cpu_coordinate_fit(small, loss)
        cpu_error = None
    except Exception as exc:                 # the CPU coordinate rejects the data: so must the GPU one
        cpu_error = type(exc)
    if cpu_error is not None:
        with pytest.raises(cpu_error):
            gpu_fit(data, loss, L2, *LIMITED, monkeypatch)
        return
    # the CPU coordinate takes the entity: no coefficients, scores of exactly 0
    e_small = int(small.id_tags["userId"].max())
    assert not W_cpu[e_small].any() and (s_cpu[small.id_tags["userId"] == e_small] == 0.0).all()
    W0, its0, reasons0, c0, m0 = gpu_fit(base, loss, L2, *LIMITED, monkeypatch)
    _mixed_routing(c0)
    s0 = c0.score(m0).cpu().numpy()
    W, its, reasons, c, m = gpu_fit(data, loss, L2, *LIMITED, monkeypatch)
    _mixed_routing(c, more_pass_path=(e0,))
    s = c.score(m).cpu().numpy()
    print(f"BOUNDARY empty entity: iterations {its[e0]}, reason {reasons[e0]}")
    assert not W[e0].any() and (s[own] == 0.0).all() and its[e0] == 0
    assert np.array_equal(s[~own], s0)
    for e in W0:
        assert np.array_equal(W[e], W0[e]) and its[e] == its0[e] and reasons[e] == reasons0[e], e
