"""The data of the persistent random-effect kernel cases (``re_persistent_cases.py``) is what the cases say it is,
and their seeds satisfy, on the oracle alone, what ``test_re_persistent_gpu.py`` relies on: under the original and a
permuted row order the CPU float64 oracle (``re_parity_util.cpu_owlqn`` / ``cpu_tron``) takes the same iterations,
stops for the same reasons and (OWL-QN) leaves the same zero pattern for EVERY entity, and its two results differ by
a floor far below the project's bounds. No GPU. A change of the generator that moves a seed off these criteria fails
here.

Floors. The floor is rounding noise of the oracle and moves with the number of CPU threads that sum (measured on two
machines, limited regimes: OWL-QN 9e-16 .. 2e-13, TRON 4e-16 .. 1.3e-15; OWL-QN converged 1e-11 .. 4e-10). The
assertions are therefore ``8 floor <= bound / 100``: 1e-12 for the iteration-limited regimes (bound 1e-9) and 1e-9
for the converged ones (bound 1e-6), so the project's bounds stand and ``max(bound, 8 floor)`` never widens them.

The oversubscribed cases follow the run-time grids on the device; here they are built for the MI355X's grids
(``NOMINAL_GRID``), the resident cases for the compiled ``pml_re_res_cap`` / ``pml_re_res_dmax``."""
import numpy as np
import pytest

import re_persistent_cases as pc
from photon_ml_amd.optimization.optimizer import ConvergenceReason
from re_boundary_cases import CSR_ROWS, QUADDY, RAGGED, RAGGED64, SCALAR
from re_parity_util import cpu_owlqn, cpu_tron, make_ragged_entities, reference_floor

LIMITED_FLOOR, CONVERGED_FLOOR = 1e-12, 1e-9


def _res_params():
    from photon_ml_amd.ops.native import require_re_lib
    lib = require_re_lib()
    return int(lib.pml_re_res_cap()), int(lib.pml_re_res_dmax())


def _case(name, loss="LOGISTIC"):
    cap, rdmax = _res_params() if name == "res_clusters" else (None, None)
    grid = pc.NOMINAL_GRID if name in ("owl_over", "res_over") else None
    return pc.case_spec(name, cap, rdmax, grid), pc.case_data(name, loss, cap, rdmax, grid)


def _entities(data):
    x, ids = data.shards["user"].tocsr(), data.id_tags["userId"]
    lens = np.diff(x.indptr)
    for e in np.unique(ids):
        r = np.nonzero(ids == e)[0]
        yield int(e), r, lens[r], x[r]


ALL_CASES = ["owl_edges", "owl_ring", "owl_reuse", "owl_over", "res_singles", "res_clusters", "res_over"]


@pytest.mark.parametrize("name", ALL_CASES)
def test_generator_claims(name):
    """Exact projected widths, the row-length cycle of the spec, weights in [0.25, 4] with 5 to 30 % at exactly 0,
    offsets 0.3 sin(i), no intercept column."""
    (spec, seed), data = _case(name)
    x = data.shards["user"].tocsr()
    assert x.has_canonical_format and (x.data != 0).all()
    assert len(np.unique(data.id_tags["userId"])) == len(spec)
    base = 0
    for (e, r, lens, xe), (n, d, lengths) in zip(_entities(data), spec):
        assert len(r) == n and list(lens) == [min(lengths[i % len(lengths)], d) for i in range(n)], (name, e)
        assert np.array_equal(np.unique(xe.indices), np.arange(base, base + d)), (name, e)
        base += d
    assert x.shape[1] == base                                     # no column beyond the entities' own blocks
    w = data.weights
    assert 0.05 < (w == 0).mean() < 0.3 and set(np.unique(w * 4)) <= set(range(17)) and w.max() == 4.0
    assert np.array_equal(data.offsets, 0.3 * np.sin(np.arange(data.n_rows)))
    again = make_ragged_entities(spec, seed)
    assert (again.shards["user"] != x).nnz == 0 and np.array_equal(again.response, data.response)


def _class_of(d):
    return next(c for c in pc.LBFGS_CLASSES if d <= c)


def test_owl_edges_shapes():
    """Both ends of every LDS class, the cycles of the issue's table, rows without entries and rows past 64 entries
    in the same launch."""
    (spec, _), data = _case("owl_edges")
    assert [d for _, d, _ in spec] == [1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049]
    assert [n for n, _, _ in spec] == [40, 30, 100, 130, 75, 150, 200, 130, 260, 180, 130, 200, 260, 150]
    assert [c for _, _, c in spec] == [RAGGED, RAGGED, QUADDY, SCALAR, QUADDY, SCALAR, QUADDY, SCALAR, QUADDY, QUADDY,
                                       CSR_ROWS, CSR_ROWS, CSR_ROWS, CSR_ROWS]
    for dm, ents in pc.OWL_EDGES_LAUNCHES.items():
        assert ents == [e for e, (_, d, _) in enumerate(spec) if d <= 2048 and _class_of(d) == dm]
        assert dm in [spec[e][1] for e in ents]                   # an entity of exactly the class width
    assert pc.OWL_EDGES_PASS_PATH == [e for e, (_, d, _) in enumerate(spec) if d > 2048]
    lens = {e: set(ln) for e, _, ln, _ in _entities(data)}
    assert all(0 in lens[e] for e in (0, 1, 3, 5, 7, 10, 11, 12, 13))          # rows without any entry
    assert all(max(lens[e]) == 130 for e in range(2, 10)) and all(max(lens[e]) == 300 for e in range(10, 14))
    # the ring case: the same entities without the narrow two and the pass-path one
    ring, _ = pc.case_spec("owl_ring")
    assert ring == spec[2:13]
    for dm, ents in pc.OWL_RING_LAUNCHES.items():
        assert ents == [e for e, (_, d, _) in enumerate(ring) if _class_of(d) == dm]
    for loss in ("POISSON", "SQUARED"):
        other = pc.case_data("owl_edges", loss)
        assert (other.shards["user"] != data.shards["user"]).nnz == 0
        assert not np.array_equal(other.response, data.response)


def _launch_order(data, ents):
    """The launch order of the fused batch: descending non-zeros (stable)."""
    nnz = {e: int(ln.sum()) for e, _, ln, _ in _entities(data)}
    return sorted(ents, key=lambda e: -nnz[e])


def test_owl_reuse_widths_go_up_and_down_along_the_launch_order():
    (spec, _), data = _case("owl_reuse")
    assert len(spec) == 16
    for dm, ents in pc.OWL_REUSE_LAUNCHES.items():
        assert len(ents) >= 6 and ents == [e for e, (_, d, _) in enumerate(spec) if _class_of(d) == dm]
        widths = [spec[e][1] for e in _launch_order(data, ents)]
        steps = np.sign(np.diff(widths))
        # a narrow entity after a wider one and a wider one after a narrow one, more than once each
        assert (steps > 0).sum() >= 2 and (steps < 0).sum() >= 2, (dm, widths)
        assert dm in widths and min(widths) <= dm // 2 + 50
    assert {c for _, _, c in spec} == {QUADDY, RAGGED, SCALAR}


def test_oversubscribed_shapes():
    g = pc.NOMINAL_GRID
    (spec, _), data = _case("owl_over")
    assert len(spec) == g + 40 and all(1024 < d <= 2048 for _, d, _ in spec)
    assert len({d for _, d, _ in spec}) > 200 and data.shards["user"].nnz < 700_000
    (spec, _), data = _case("res_over")
    cap, rdmax = _res_params()
    assert len(spec) == g + 40 and all(64 < d <= rdmax and n <= cap for n, d, _ in spec)
    assert all(ln.max() <= 64 for _, _, ln, _ in _entities(data))


def test_resident_shapes():
    cap, rdmax = _res_params()
    (spec, _), data = _case("res_singles")
    assert len(spec) == 20 and all(n <= cap and 64 < d <= rdmax and c == RAGGED64 for n, d, c in spec)
    assert {65, 256, 257, 512, 513, 1023, 1024} <= {d for _, d, _ in spec}
    widths = [spec[e][1] for e in _launch_order(data, range(20))]          # the ticket order of the singles
    steps = np.sign(np.diff(widths))
    assert (steps > 0).sum() >= 4 and (steps < 0).sum() >= 4, widths
    (spec, _), data = _case("res_clusters")
    assert [-(-n // cap) for n, _, _ in spec] == [1, 1, 2, 2, 3, 3] + [1] * 8
    assert spec[6:] == pc.RES_SINGLES[:8]
    assert all(ln.max() <= 64 for _, _, ln, _ in _entities(data))


# ---- the seeds, on the oracle alone ------------------------------------------------------------------------------

def _owl_pair(name, loss, l2, l1, tol, max_iter, m=10):
    _, data = _case(name, loss)
    a = cpu_owlqn(data, loss, l2, l1, tol, max_iter, m=m)
    b = cpu_owlqn(data, loss, l2, l1, tol, max_iter, m=m, perm_seed=1)
    for e in a:
        assert a[e][1] == b[e][1] and a[e][2] == b[e][2], (name, loss, e, a[e][1:], b[e][1:])
        assert np.array_equal(a[e][0] == 0, b[e][0] == 0), (name, loss, e, "zero pattern")
    return a, reference_floor(a, b)


def _all_ran(ref, max_iter):
    return all(it == max_iter and rc == 1 for _, it, rc in ref.values())


@pytest.mark.parametrize("loss", ["LOGISTIC", "POISSON"])
def test_owl_edges_seed_limited(loss):
    ref, floor = _owl_pair("owl_edges", loss, 0.0, 0.5, 0.0, 5)
    assert _all_ran(ref, 5) and floor <= LIMITED_FLOOR, floor
    assert all(np.count_nonzero(w) > 0 for w, _, _ in ref.values())


@pytest.mark.parametrize("loss", ["LOGISTIC", "POISSON"])
def test_owl_edges_seed_converged(loss):
    ref, floor = _owl_pair("owl_edges", loss, 0.0, 0.5, 1e-8, 100)
    assert floor <= CONVERGED_FLOOR, floor
    assert len({it for _, it, _ in ref.values()}) >= 3            # entities stop at different iteration counts


@pytest.mark.parametrize("l2,l1", [(0.0, 0.5), (0.3, 0.0)])
@pytest.mark.parametrize("loss", ["LOGISTIC", "POISSON"])
def test_owl_ring_seed(loss, l2, l1):
    """Every entity runs all iterations under both row orders with a floor <= 1e-12 (measured: <= 2e-13), with 3
    history pairs over 8 iterations (the ring wraps twice) and with 10 over 14 (it wraps once)."""
    for m, max_iter in ((3, 8), (10, 14)):
        ref, floor = _owl_pair("owl_ring", loss, l2, l1, 0.0, max_iter, m=m)
        assert _all_ran(ref, max_iter) and floor <= LIMITED_FLOOR, (m, floor)


@pytest.mark.parametrize("l2,l1", [(0.0, 0.5), (0.3, 0.0)])
@pytest.mark.parametrize("loss", ["LOGISTIC", "POISSON"])
def test_owl_reuse_seed(loss, l2, l1):
    ref, floor = _owl_pair("owl_reuse", loss, l2, l1, 0.0, 5)
    assert _all_ran(ref, 5) and floor <= LIMITED_FLOOR, floor


def test_owl_over_seed():
    ref, floor = _owl_pair("owl_over", "LOGISTIC", 0.0, 0.5, 0.0, 5)
    assert _all_ran(ref, 5) and floor <= LIMITED_FLOOR, floor


def _tron_pair(name, regime):
    _, data = _case(name)
    a = cpu_tron(data, "LOGISTIC", 1.0, *regime)
    b = cpu_tron(data, "LOGISTIC", 1.0, *regime, perm_seed=1)
    assert all(a[e][1:] == b[e][1:] for e in a), name
    return a, reference_floor(a, b)


@pytest.mark.parametrize("name", ["res_singles", "res_clusters"])
def test_resident_seeds(name):
    """(a): exactly 4 iterations to the limit; (b): 6 to 8 iterations, converged on the function values; counts and
    reasons unchanged under the permuted rows."""
    ref, floor = _tron_pair(name, (0.0, 4))
    assert all(it == 4 and rc == ConvergenceReason.MAX_ITERATIONS for _, it, rc in ref.values())
    assert floor <= LIMITED_FLOOR, floor
    ref, floor = _tron_pair(name, (1e-8, 60))
    assert all(6 <= it <= 8 and rc == ConvergenceReason.FUNCTION_VALUES_CONVERGED for _, it, rc in ref.values())
    assert floor <= CONVERGED_FLOOR, floor


def test_res_over_seed():
    ref, floor = _tron_pair("res_over", (0.0, 4))
    assert all(it == 4 and rc == ConvergenceReason.MAX_ITERATIONS for _, it, rc in ref.values())
    assert floor <= LIMITED_FLOOR, floor
