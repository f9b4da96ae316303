"""The two persistent fused random-effect solvers with workgroups that serve more than one entity:
``re_lbfgs_csr_kernel`` (fused L-BFGS / OWL-QN) and ``re_tron_res_kernel`` (register-resident TRON).

In both a workgroup takes a ticket, solves an entity and takes the next one with its LDS, registers and workspace
slab carried over (the ``rho`` ring and the (S, Y) history slab of the OWL-QN kernel; the accumulators that are zero
"between passes", the TRON scalars in LDS and ``sV[DM..]`` of the resident kernel; the ``parity`` of ``block_sums``
restarted at every entity). The grids are Python state (``fused.launches`` holds ``(dm, order, grid)``,
``fused.res["grid"]`` the resident grid), so a test shrinks them and reuse happens at tiny shapes.

INVARIANCE. An entity's arithmetic does not depend on which workgroup solves it nor on what that workgroup solved
before: a solve with grid 1, 2, 3 or with the launch order reversed (a narrow entity before a wider one on the same
workgroup) is ``torch.equal`` to the production-grid solve in W, f, iters, reason and z; every reduced-grid solve
runs twice and equals itself. This is no correctness yardstick: each case also compares the production-grid result
with the CPU float64 oracle (``re_parity_util.cpu_owlqn`` = ``batched_lbfgs``; ``cpu_tron``) under the project's
bounds -- iteration-limited (tolerance 0): W to 1e-9 with identical iteration counts, stop reasons and (L1) zero
patterns; converged: 1e-6; ``max(bound, 8 floor)`` where the oracle's own floor (original against permuted rows)
is known. No entity is skipped and no share of mismatches allowed. The data is
``re_parity_util.make_ragged_entities`` (ragged rows, rows without entries, no intercept, weights in [0.25, 4] with
about 15 % at exactly 0, offsets ``0.3 sin(i)``); ``re_persistent_cases.py`` holds specs and seeds,
``test_re_persistent_shapes.py`` checks both on the CPU.

Cases:

* A1 ``owl_edges`` -- through the coordinate (L1, lambda 0.5; LOGISTIC and POISSON): d_e = 1, 2, 255, 256 | 257,
  511, 512 | 513, 1023, 1024 | 1025, 2047, 2048 in the launches 256, 512, 1024, 2048 and 2049 on the pass path;
  5 iterations at tolerance 0 and tolerance 1e-8 with up to 100; grids 1, 2 and 1 reversed in both regimes;
* A2 ``owl_reuse`` -- ``EntityLbfgsBatch.solve`` on 8 entities per launch (512 and 1024) whose widths go up and down
  along the launch order, all four losses, OWL (l1 = 0.5) and plain L-BFGS (l1 = 0, l2 = 0.3): grids 1, 2, 3 and
  1 reversed in the converged regime (entities stop at different counts, the ring wraps); oracle in the limited one;
* A3 ``owl_ring`` -- the ring wraps under the 1e-9 bound: ``m = 3`` over 8 iterations and ``m = 10`` over 14 at
  tolerance 0, both instantiations, widths 255 .. 2048; grid 1 next to the production grid;
* A4 ``owl_over`` -- no override: ``re_lbfgs_grid(2048) + 40`` entities of 1025 .. 2048 coefficients in one launch;
* R1 ``res_singles`` -- 20 single-workgroup entities (65 .. 1024 wide, 20 .. 130 rows, in no order), regimes (a)
  (tolerance 0, 4 iterations) and (b) (1e-8, at most 60) and the scores against the oracle; grids 1, 2, 3 (at grid 1
  one workgroup solves all 20 in ticket order); POISSON and SQUARED for invariance;
* R2 ``res_clusters`` -- tasks of 3, 3, 2, 2, 1, 1 workgroups and 8 singles (20 tickets): grids 6 and 7, so clusters
  are joined by workgroups that were busy with earlier tasks; ``check_error`` after every solve. No grid below twice
  the largest cluster is ever launched (the kernel's deadlock-freedom condition; asserted before each launch);
* R3 ``res_over`` -- no override: resident grid + 40 single-workgroup entities;
* R4 -- ``EntityTronBatch.solve`` refuses a grid smaller than its largest cluster on the host (no launch).

Measured on an MI355X: ``re_lbfgs_grid(2048)`` = 256 (the production grids of the small launches are their entity
counts, 2 .. 8), ``re_res_params()`` = (384, 1024, 256), so A4 and R3 hold 296 entities each. Worst entity per case,
"oracle floor / GPU error", each relative to the entity's largest coefficient; the floor is the oracle against itself
on permuted rows and never looks at the GPU. Launches reached: OWL-QN 256, 512, 1024, 2048 (both instantiations, all
four losses) and the pass path next to them; the resident launch with 20, 20 (clusters 3, 3, 2, 2) and 296 tickets.

    case          loss      setting                  grids             oracle floor / GPU error
    ---------------------------------------------------------------------------------------------
    owl_edges     LOGISTIC  OWL, 5 iterations        prod, 1, 2, 1 rev   1.4e-15 / 1.3e-15
    owl_edges     LOGISTIC  OWL, converged           prod, 1, 2, 1 rev   5.1e-11 / 1.2e-10   (5 .. 100 iterations)
    owl_edges     POISSON   OWL, 5 iterations        prod, 1, 2, 1 rev   4.0e-15 / 4.0e-15
    owl_edges     POISSON   OWL, converged           prod, 1, 2, 1 rev   6.0e-11 / 3.7e-11   (5 .. 100 iterations)
    owl_reuse     LOGISTIC  OWL, 5 iterations        prod (8)            1.1e-15 / 1.4e-15
    owl_reuse     LOGISTIC  L-BFGS, 5 iterations     prod (8)            1.3e-15 / 2.2e-15
    owl_reuse     POISSON   OWL, 5 iterations        prod (8)            4.8e-15 / 3.1e-15
    owl_reuse     POISSON   L-BFGS, 5 iterations     prod (8)            2.1e-15 / 3.3e-15
    owl_reuse     all four  both, converged          prod, 1, 2, 3, 1 rev  invariance only
    owl_ring      LOGISTIC  OWL, m = 3, 8 it.        prod, 1, 1 rev      3.0e-15 / 3.9e-15
    owl_ring      LOGISTIC  OWL, m = 10, 14 it.      prod, 1, 1 rev      6.3e-15 / 5.6e-15
    owl_ring      LOGISTIC  L-BFGS, m = 3, 8 it.     prod, 1, 1 rev      3.1e-15 / 2.2e-15
    owl_ring      LOGISTIC  L-BFGS, m = 10, 14 it.   prod, 1, 1 rev      3.4e-15 / 4.5e-15
    owl_ring      POISSON   OWL, m = 3, 8 it.        prod, 1, 1 rev      4.8e-15 / 4.4e-15
    owl_ring      POISSON   OWL, m = 10, 14 it.      prod, 1, 1 rev      1.3e-14 / 1.4e-14
    owl_ring      POISSON   L-BFGS, m = 3, 8 it.     prod, 1, 1 rev      4.2e-15 / 3.3e-15
    owl_ring      POISSON   L-BFGS, m = 10, 14 it.   prod, 1, 1 rev      1.8e-14 / 5.1e-14
    owl_over      LOGISTIC  OWL, 5 iterations        256 for 296         1.8e-15 / 1.7e-14
    res_singles   LOGISTIC  (a) 4 iterations         256, 1, 2, 3        6.8e-16 / 1.0e-15   (scores 3.0e-16)
    res_singles   LOGISTIC  (b) converged            256, 1, 2, 3        4.6e-16 / 6.1e-16   (6 .. 7 iterations)
    res_singles   POISSON, SQUARED  (a), (b)         256, 1, 2, 3        invariance only
    res_clusters  LOGISTIC  (a) 4 iterations         256, 6, 7           5.2e-16 / 2.1e-15
    res_clusters  LOGISTIC  (b) converged            256, 6, 7           6.0e-16 / 5.1e-16   (6 .. 8 iterations)
    res_over      LOGISTIC  (a) 4 iterations         256 for 296         1.2e-15 / 6.8e-15

Every invariance comparison was bitwise equal, no ``check_error`` raised, and the ``8 floor`` branch of the bound
was needed nowhere: the tests found no defect in either kernel. That they can see one was checked once by hand on
kernels changed for the purpose (not kept): with the number of valid history pairs surviving an entity in
``re_lbfgs_csr_kernel`` and one accumulator entry left at 1.0 after an entity in ``re_tron_res_kernel``, every test
of this file but the host-side guard failed -- the reduced-grid solves already against themselves run twice, the
oversubscribed production launches against the oracle.
"""
import functools

import numpy as np
import pytest
import torch

import re_persistent_cases as pc
from photon_ml_amd.optimization.optimizer import ConvergenceReason
from re_parity_util import (_set_route, cpu_owlqn, cpu_tron, entity_coefficients, gpu_fit, lbfgs_coordinate,
                            reference_floor, rel_err, segmented_offsets)

pytestmark = pytest.mark.gpu

L1 = 0.5
OWL, PLAIN = (0.0, L1), (0.3, 0.0)          # (l2, l1) of the two instantiations of the kernel
LIMITED, CONVERGED = (0.0, 5), (1e-8, 100)
TRON_L2 = 1.0
TRON_A, TRON_B = (0.0, 4), (1e-8, 60)


def _bound(regime, floor):
    return max(1e-9 if regime[0] == 0.0 else 1e-6, 8 * floor)


def _native():
    from photon_ml_amd.ops import native
    return native


def _assert_bitwise(tag, a, b):
    for name in ("W", "f", "iters", "reason", "z"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (tag, name)


# ---- re_lbfgs_csr_kernel -----------------------------------------------------------------------------------------

def _update(c):
    """One cold update of the coordinate: per entity id the coefficients over the global features, the iteration
    count and the reason code."""
    got = {}
    c._defer_stats = lambda it, rc, act, sec: got.update(it=it.cpu().numpy(), rc=rc.cpu().numpy())
    m = c.update_model(c.initialize_model(), None)
    m.materialize()
    W = {e: np.asarray(m.coefficients_of(e).means, dtype=np.float64) for e in m.entity_ids}
    ids = c.dataset.entity_ids
    return (W, {e: int(got["it"][i]) for i, e in enumerate(ids)}, {e: int(got["rc"][i]) for i, e in enumerate(ids)})


def _batch(data, loss):
    """The cuda coordinate of ``data`` under L1 and its solver components, nothing solved yet."""
    from photon_ml_amd.optimization.entity_lbfgs import EntityLbfgsBatch
    c = lbfgs_coordinate(data, loss, "cuda", L1)
    rs, fused, sub = c._components(L1, c.opt_config.optimizer_config)
    assert rs is None and isinstance(fused, EntityLbfgsBatch)
    return c, fused, sub


def _solver(c, fused, data, reg, regime):
    """``solve()``: one cold ``EntityLbfgsBatch.solve`` with whatever ``fused.launches`` / ``fused.m`` hold."""
    off = segmented_offsets(c, data)[fused.rows].contiguous()
    W0 = torch.zeros(int(fused.col_ptr[-1]), dtype=torch.float64, device="cuda")
    return lambda: fused.solve(c.loss, reg[0], reg[1], W0, off, *regime)


def _per_entity(c, fused, r):
    ds = c.dataset
    W = torch.zeros(int(ds.seg.col_ptr[-1]), dtype=torch.float64, device="cuda").index_copy_(0, fused.cols, r.W)
    W = entity_coefficients(ds, W)
    ids = [ds.entity_ids[k] for k in fused.ents.tolist()]
    its, rcs = r.iters.tolist(), r.reason.tolist()
    return ({e: W[e] for e in ids}, {e: int(its[b]) for b, e in enumerate(ids)},
            {e: int(rcs[b]) for b, e in enumerate(ids)})


def _launch_ids(c, fused):
    """``{launch width: entity ids in launch order}``."""
    ids = c.dataset.entity_ids
    return {dm: [int(ids[k]) for k in fused.ents[order.long()].tolist()] for dm, order, _ in fused.launches}


def _owl_invariance(tag, solve, fused, monkeypatch, grids):
    """The production-grid solve against reduced grids and the reversed order; returns the production result."""
    production = list(fused.launches)
    assert all(grid == min(_native().re_lbfgs_grid(dm), order.numel()) for dm, order, grid in production)
    base = solve()
    variants = [(f"grid {g}", [(dm, order, min(g, int(order.numel()))) for dm, order, _ in production])
                for g in grids]
    variants.append(("grid 1 reversed", [(dm, order.flip(0).contiguous(), 1) for dm, order, _ in production]))
    for what, launches in variants:
        # a workgroup of every launch serves a second entity
        assert all(grid < order.numel() for _, order, grid in launches), (tag, what)
        monkeypatch.setattr(fused, "launches", launches)
        first, second = solve(), solve()
        _assert_bitwise(f"{tag} {what} twice", first, second)
        _assert_bitwise(f"{tag} {what} vs production", first, base)
    monkeypatch.setattr(fused, "launches", production)
    _assert_bitwise(f"{tag} production again", solve(), base)
    return base


@functools.lru_cache(maxsize=None)
def _owl_reference(name, loss, reg, regime, m=10, grid=None):
    """The oracle's cold fit (never modified) and its floor against the fit with permuted rows."""
    data = pc.case_data(name, loss, grid=grid)
    ref = cpu_owlqn(data, loss, *reg, *regime, m=m)
    return ref, reference_floor(ref, cpu_owlqn(data, loss, *reg, *regime, m=m, perm_seed=1))


def _compare_owl(tag, regime, ref, floor, W, its, rcs, all_run=True):
    bound = _bound(regime, floor)
    errs = {}
    for e in W:
        w_ref, it_ref, rc_ref = ref[e]
        assert its[e] == it_ref and rcs[e] == rc_ref, (tag, e, its[e], it_ref, rcs[e], rc_ref)
        if regime[0] == 0.0 and all_run:
            assert it_ref == regime[1] and rc_ref == 1, (tag, e, it_ref, rc_ref)
        assert np.array_equal(W[e] == 0, w_ref == 0), (tag, e, "zero pattern", int(((W[e] == 0) != (w_ref == 0)).sum()))
        errs[e] = rel_err(W[e], w_ref)
    worst = max(errs.values())
    print(f"PERSISTENT {tag}: floor {floor:.1e} bound {bound:.1e} gpu error {worst:.1e} iterations "
          f"{sorted(set(its.values()))}")
    for e, err in errs.items():
        assert err <= bound, (tag, e, err, bound, floor)


@pytest.mark.parametrize("loss", ["LOGISTIC", "POISSON"])
def test_owlqn_class_edges_through_the_coordinate(loss, monkeypatch):
    """A1: every LDS class at both ends, 1024 among them, rows of 0 .. 300 entries with zero weights."""
    from photon_ml_amd.optimization.entity_lbfgs import EntityLbfgsBatch
    data = pc.case_data("owl_edges", loss)
    for regime in (LIMITED, CONVERGED):
        c = lbfgs_coordinate(data, loss, "cuda", L1, *regime)
        W, its, rcs = _update(c)
        rs, fused, sub = c._comps
        assert rs is None and isinstance(fused, EntityLbfgsBatch) and fused.B == 13
        assert [dm for dm, _, _ in fused.launches] == [256, 512, 1024, 2048]
        assert {dm: sorted(v) for dm, v in _launch_ids(c, fused).items()} == pc.OWL_EDGES_LAUNCHES
        assert sub is not None and sorted(int(c.dataset.entity_ids[k]) for k in sub.entities.tolist()) == \
            pc.OWL_EDGES_PASS_PATH and c.solver_routing()["pass_path"] == 1
        assert torch.equal(c.dataset.seg.o, segmented_offsets(c, data))
        ref, floor = _owl_reference("owl_edges", loss, OWL, regime)
        assert set(W) == set(ref) and len(W) == 14
        _compare_owl(f"owl_edges {loss} {regime}", regime, ref, floor, W, its, rcs)
        # the same launches with workgroups that serve every entity of their launch, one after another
        base = _owl_invariance(f"owl_edges {loss} {regime}", _solver(c, fused, data, OWL, regime), fused, monkeypatch,
                               (1, 2))
        Wd, itd, rcd = _per_entity(c, fused, base)
        for e in Wd:                        # the direct solve is the coordinate's solve
            assert np.array_equal(Wd[e], W[e]) and itd[e] == its[e] and rcd[e] == rcs[e], (loss, regime, e)


@pytest.mark.parametrize("reg", [OWL, PLAIN], ids=["owl", "lbfgs"])
@pytest.mark.parametrize("loss", ["LOGISTIC", "POISSON", "SQUARED", "HINGE"])
def test_lbfgs_long_reuse_chains(loss, reg, monkeypatch):
    """A2: up to 8 entities in a row on one workgroup, widths going up and down, every instantiation."""
    data = pc.case_data("owl_reuse", loss)
    c, fused, sub = _batch(data, loss)
    assert sub is None and fused.B == 16
    launches = _launch_ids(c, fused)
    assert {dm: sorted(v) for dm, v in launches.items()} == pc.OWL_REUSE_LAUNCHES
    spec = pc.OWL_REUSE
    for dm, ents in launches.items():       # a narrow entity follows a wider one and the other way round
        steps = np.sign(np.diff([spec[e][1] for e in ents]))
        assert (steps > 0).any() and (steps < 0).any(), (dm, ents)
    base = _owl_invariance(f"owl_reuse {loss} {reg}", _solver(c, fused, data, reg, CONVERGED), fused, monkeypatch,
                           (1, 2, 3))
    its = base.iters.tolist()
    assert max(its) > fused.m, its                              # the ring wraps
    if loss == "LOGISTIC":
        assert len(set(its)) > 4, its                           # entities stop at different iteration counts
    if loss in ("LOGISTIC", "POISSON"):
        ref, floor = _owl_reference("owl_reuse", loss, reg, LIMITED)
        _compare_owl(f"owl_reuse {loss} {reg}", LIMITED, ref, floor,
                     *_per_entity(c, fused, _solver(c, fused, data, reg, LIMITED)()))


@pytest.mark.parametrize("reg", [OWL, PLAIN], ids=["owl", "lbfgs"])
@pytest.mark.parametrize("loss", ["LOGISTIC", "POISSON"])
def test_lbfgs_history_ring_wraps_under_the_tight_bound(loss, reg, monkeypatch):
    """A3: (i) 3 history pairs over 8 iterations, (ii) 10 over 14, tolerance 0: every slot of the ring is
    rewritten while W is held to 1e-9; on the production grid and on one workgroup for all of a launch."""
    data = pc.case_data("owl_ring", loss)
    c, fused, sub = _batch(data, loss)
    assert sub is None and fused.B == 11
    assert {dm: sorted(v) for dm, v in _launch_ids(c, fused).items()} == pc.OWL_RING_LAUNCHES
    for m, iters in ((3, 8), (10, 14)):
        assert m <= _native().RE_LBFGS_M and iters > m
        monkeypatch.setattr(fused, "m", m)
        regime = (0.0, iters)
        base = _owl_invariance(f"owl_ring {loss} {reg} m={m}", _solver(c, fused, data, reg, regime), fused,
                               monkeypatch, (1,))
        ref, floor = _owl_reference("owl_ring", loss, reg, regime, m)
        _compare_owl(f"owl_ring {loss} {reg} m={m} {iters} iterations", regime, ref, floor,
                     *_per_entity(c, fused, base))


def test_owlqn_more_entities_than_resident_workgroups():
    """A4: nothing overridden -- the class-2048 launch of the coordinate holds 40 entities more than its grid."""
    g = _native().re_lbfgs_grid(2048)
    data = pc.case_data("owl_over", "LOGISTIC", grid=g)
    c = lbfgs_coordinate(data, "LOGISTIC", "cuda", L1, *LIMITED)
    W, its, rcs = _update(c)
    rs, fused, sub = c._comps
    B = g + 40
    assert rs is None and sub is None and fused.B == B == len(W)
    assert [(dm, int(order.numel()), grid) for dm, order, grid in fused.launches] == [(2048, B, g)] and g < B
    print(f"PERSISTENT owl_over: re_lbfgs_grid(2048) = {g}, {B} entities, {data.shards['user'].nnz} non-zeros")
    ref, floor = _owl_reference("owl_over", "LOGISTIC", OWL, LIMITED, grid=g)
    _compare_owl("owl_over LOGISTIC", LIMITED, ref, floor, W, its, rcs)


# ---- re_tron_res_kernel ------------------------------------------------------------------------------------------

def _res_data(name, loss="LOGISTIC"):
    cap, rdmax, grid = _native().re_res_params()
    if name == "res_clusters":
        return pc.case_data(name, loss, cap, rdmax)
    if name == "res_over":
        return pc.case_data(name, loss, grid=grid)
    return pc.case_data(name, loss)


@functools.lru_cache(maxsize=None)
def _tron_reference(name, regime):
    data = _res_data(name)
    ref = cpu_tron(data, "LOGISTIC", TRON_L2, *regime)
    return ref, reference_floor(ref, cpu_tron(data, "LOGISTIC", TRON_L2, *regime, perm_seed=1))


def _compare_tron(tag, regime, ref, floor, W, its, reasons):
    bound = _bound(regime, floor)
    errs = {}
    assert set(W) == set(ref)
    for e, (w_ref, it_ref, reason_ref) in ref.items():
        if regime == TRON_A:
            assert it_ref == 4 and reason_ref == ConvergenceReason.MAX_ITERATIONS, (tag, e, it_ref, reason_ref)
        assert its[e] == it_ref and reasons[e] == reason_ref, (tag, e, its[e], it_ref, reasons[e], reason_ref)
        errs[e] = rel_err(W[e], w_ref)
    worst = max(errs.values())
    print(f"PERSISTENT {tag}: floor {floor:.1e} bound {bound:.1e} gpu error {worst:.1e} iterations "
          f"{sorted(set(its.values()))}")
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
    excess = np.abs(score - want) / (1.0 + scale)
    empty = np.diff(x.indptr) == 0
    print(f"PERSISTENT {tag}: scores, worst |s - x.w| / (1 + sum |x w|) = {excess.max():.1e}")
    assert np.isfinite(score).all() and (excess <= 1e-12).all(), (tag, int(excess.argmax()), float(excess.max()))
    assert empty.any() and (score[empty] == 0.0).all(), tag


def _res_solver(c, fused, data, regime):
    """``solve()``: one cold ``EntityTronBatch.solve`` with whatever ``fused.res["grid"]`` holds; the error flag of
    the launch is checked after every solve, and no grid below twice the largest cluster is launched."""
    off = segmented_offsets(c, data)[fused.rows].contiguous()
    W0 = torch.zeros(int(fused.col_ptr[-1]), dtype=torch.float64, device="cuda")

    def solve():
        assert fused.res["grid"] >= 2 * fused.res["kmax"] or fused.res["kmax"] == 1, fused.res["grid"]
        r = fused.solve(c.loss, TRON_L2, W0, off, *regime)
        r.check_error()
        return r
    return solve


def _res_invariance(tag, solve, fused, monkeypatch, grids):
    production = fused.res["grid"]
    assert production == _native().re_res_params()[2]
    base = solve()
    for g in grids:
        assert g < fused.res["tickets"] and g < production, (tag, g)     # a workgroup takes a second ticket
        monkeypatch.setitem(fused.res, "grid", g)
        first, second = solve(), solve()
        _assert_bitwise(f"{tag} grid {g} twice", first, second)
        _assert_bitwise(f"{tag} grid {g} vs production", first, base)
    monkeypatch.setitem(fused.res, "grid", production)
    _assert_bitwise(f"{tag} production again", solve(), base)
    return base


def _resident_only(c, n, clusters, tickets):
    rs, fused, sub = c._comps
    assert rs is None and sub is None and fused.B == n
    assert fused.res is not None and fused.res["n"] == n and fused.res["clusters"] == clusters
    assert fused.res["tickets"] == tickets and fused.launches == []
    return fused


def _res_entities(c, fused, r):
    ds = c.dataset
    W = torch.zeros(int(ds.seg.col_ptr[-1]), dtype=torch.float64, device="cuda").index_copy_(0, fused.cols, r.W)
    return entity_coefficients(ds, W)


def _res_oracle_and_invariance(name, n, clusters, tickets, grids, monkeypatch, scores=False):
    """Regimes (a) and (b) of the production grid against the oracle, then against the reduced grids."""
    data = _res_data(name)
    for regime in (TRON_A, TRON_B):
        W, its, reasons, c, m = gpu_fit(data, "LOGISTIC", TRON_L2, *regime, monkeypatch)
        fused = _resident_only(c, n, clusters, tickets)
        ref, floor = _tron_reference(name, regime)
        _compare_tron(f"{name} LOGISTIC {regime}", regime, ref, floor, W, its, reasons)
        if scores and regime == TRON_A:
            _check_scores(name, data, c.score(m).cpu().numpy(), W)
        base = _res_invariance(f"{name} LOGISTIC {regime}", _res_solver(c, fused, data, regime), fused, monkeypatch,
                               grids)
        Wd = _res_entities(c, fused, base)
        assert all(np.array_equal(Wd[e], W[e]) for e in W), (name, regime)       # the coordinate's own solve
    return c, fused


def test_resident_singles_on_one_two_and_three_workgroups(monkeypatch):
    """R1: 20 single-workgroup entities; at grid 1 one workgroup solves them all in ticket order."""
    _set_route("resident", monkeypatch)
    c, fused = _res_oracle_and_invariance("res_singles", 20, 0, 20, (1, 2, 3), monkeypatch, scores=True)
    order = [int(c.dataset.entity_ids[k]) for k in fused.ents[fused.res["ent"].long()].tolist()]
    steps = np.sign(np.diff([pc.RES_SINGLE_WIDTHS[e] for e in order]))
    assert (steps > 0).sum() >= 4 and (steps < 0).sum() >= 4, order        # narrow after wide and wide after narrow


@pytest.mark.parametrize("loss", ["POISSON", "SQUARED"])
def test_resident_singles_invariance_other_losses(loss, monkeypatch):
    _set_route("resident", monkeypatch)
    data = _res_data("res_singles", loss)
    for regime in (TRON_A, TRON_B):
        _, _, _, c, _ = gpu_fit(data, loss, TRON_L2, *regime, monkeypatch)
        fused = _resident_only(c, 20, 0, 20)
        _res_invariance(f"res_singles {loss} {regime}", _res_solver(c, fused, data, regime), fused, monkeypatch,
                        (1, 2, 3))


def test_resident_clusters_joined_by_busy_workgroups(monkeypatch):
    """R2: 20 tickets on 6 and on 7 workgroups: the clusters of 2 are formed by workgroups coming from the
    clusters of 3, the singles follow on whichever workgroup is free."""
    _set_route("resident", monkeypatch)
    cap, rdmax, grid = _native().re_res_params()
    assert grid >= 14
    c, fused = _res_oracle_and_invariance("res_clusters", 14, 4, 20, (6, 7), monkeypatch)
    t0 = fused.res["t0"].tolist()
    assert [b - a for a, b in zip(t0, t0[1:])] == [3, 3, 2, 2] + [1] * 10 and fused.res["kmax"] == 3
    tasks = [int(c.dataset.entity_ids[k]) for k in fused.ents[fused.res["ent"].long()].tolist()]
    assert sorted(tasks[:2]) == [4, 5] and sorted(tasks[2:4]) == [2, 3] and sorted(tasks[4:]) == [0, 1] + list(
        range(6, 14))


def test_resident_more_tickets_than_workgroups(monkeypatch):
    """R3: nothing overridden -- the resident grid + 40 single-workgroup entities in one launch."""
    _set_route("resident", monkeypatch)
    cap, rdmax, grid = _native().re_res_params()
    data = _res_data("res_over")
    B = grid + 40
    W, its, reasons, c, m = gpu_fit(data, "LOGISTIC", TRON_L2, *TRON_A, monkeypatch)
    fused = _resident_only(c, B, 0, B)
    assert fused.res["tickets"] == B > grid == fused.res["grid"]
    print(f"PERSISTENT res_over: re_res_params() = {(cap, rdmax, grid)}, {B} entities")
    ref, floor = _tron_reference("res_over", TRON_A)
    _compare_tron("res_over LOGISTIC", TRON_A, ref, floor, W, its, reasons)


def test_resident_grid_below_the_largest_cluster_is_refused_on_the_host(monkeypatch):
    """R4: a grid that cannot hold the largest cluster raises before anything is launched."""
    from photon_ml_amd.algorithm.coordinates import RandomEffectCoordinate
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    _set_route("resident", monkeypatch)
    data = _res_data("res_clusters")
    cfg = GLMOptimizationConfiguration(OptimizerConfig("TRON", 4, 0.0), RegularizationContext("L2"), TRON_L2)
    c = RandomEffectCoordinate("u", data, RandomEffectDataConfiguration("userId", "user"), cfg, "LOGISTIC_REGRESSION",
                               device="cuda", layout="segmented")
    rs, fused, sub = c._components(0.0, cfg.optimizer_config)
    assert fused.res["kmax"] == 3 and fused.res["grid"] >= 2 * fused.res["kmax"]
    launched = []
    monkeypatch.setattr(_native(), "re_tron_res", lambda *a, **k: launched.append(a))
    monkeypatch.setitem(fused.res, "grid", fused.res["kmax"] - 1)
    off = segmented_offsets(c, data)[fused.rows].contiguous()
    with pytest.raises(ValueError, match="cluster of 3"):
        fused.solve(c.loss, TRON_L2, None, off, 0.0, 4)
    assert not launched
