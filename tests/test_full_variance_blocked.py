"""Planning of the blocked FULL-variance route (``optimization/variance.py``): the size classes above ``VAR_MMAX``,
the route masks and the chunking, all pure tensor arithmetic that runs without a GPU; and the plan on a CPU device,
which routes every entity to the torch definition whatever ``blocked_mmax`` says.
"""
import numpy as np
import torch

from full_variance_util import BlockProblem, relative_error
from photon_ml_amd.ops.native import VAR_BLOCKED_DMAX, VAR_BLOCKED_MMAX, VAR_MMAX
from photon_ml_amd.optimization import variance as V


def test_class_bounds_increase_and_end_at_the_cap():
    bounds = V.blocked_class_bounds(VAR_BLOCKED_MMAX, VAR_MMAX)
    assert VAR_BLOCKED_MMAX == 1024 and VAR_MMAX == 128
    assert all(a < b for a, b in zip(bounds, bounds[1:]))
    assert bounds[0] > VAR_MMAX and bounds[-1] == 1024
    # neighbouring bounds differ by at most a third: padding to the class's largest member at most 2.4x the work
    assert all(3 * b <= 4 * a for a, b in zip((VAR_MMAX,) + bounds, bounds))
    # off, and a cap between two bounds
    assert V.blocked_class_bounds(0, VAR_MMAX) == () and V.blocked_class_bounds(VAR_MMAX, VAR_MMAX) == ()
    assert V.blocked_class_bounds(200, VAR_MMAX) == (160, 192, 200)
    assert V.blocked_class_bounds(129, VAR_MMAX) == (129,)


def test_every_order_lands_in_the_first_class_that_holds_it():
    bounds = V.blocked_class_bounds(VAR_BLOCKED_MMAX, VAR_MMAX)
    m = torch.arange(VAR_MMAX + 1, VAR_BLOCKED_MMAX + 1)
    cls = V.blocked_class_of(m, bounds).tolist()
    for mi, k in zip(m.tolist(), cls):
        assert 0 <= k < len(bounds)
        assert mi <= bounds[k] and (k == 0 or mi > bounds[k - 1])
    assert int(V.blocked_class_of(torch.tensor([1025]), bounds)) == len(bounds)


def test_route_masks():
    shapes = [(40, 40), (10, 30), (129, 129), (129, 200), (200, 129), (0, 7), (1025, 1025), (1025, 1100),
              (1024, 1024), (1024, 2048), (1024, 2049), (128, 5000), (5000, 128), (4100, 129), (300, 0)]
    n_e = torch.tensor([s[0] for s in shapes])
    d_e = torch.tensor([s[1] for s in shapes])
    bp, br = V.blocked_route_masks(n_e, d_e, True, VAR_MMAX, VAR_BLOCKED_MMAX, VAR_BLOCKED_DMAX)
    assert [shapes[i] for i in torch.nonzero(bp).squeeze(1).tolist()] == \
        [(129, 129), (200, 129), (1024, 1024), (4100, 129)]
    # (1024, 2049) is wider than the row-space kernels' LDS images
    assert [shapes[i] for i in torch.nonzero(br).squeeze(1).tolist()] == [(129, 200), (1024, 2048)]
    for args in ((False, VAR_MMAX, VAR_BLOCKED_MMAX), (True, VAR_MMAX, 0), (True, VAR_MMAX, VAR_MMAX)):
        bp, br = V.blocked_route_masks(n_e, d_e, args[0], args[1], args[2], VAR_BLOCKED_DMAX)
        assert not bool(bp.any()) and not bool(br.any())
    bp, br = V.blocked_route_masks(n_e, d_e, True, VAR_MMAX, 129, VAR_BLOCKED_DMAX)
    assert int(bp.sum()) == 3 and int(br.sum()) == 1


def test_merging_of_short_handed_classes():
    """From the largest class down, neighbours share a launch while the group holds at most 256 entities."""
    merge = V.blocked_merge_classes
    assert merge([]) == [] and merge([0, 0, 0]) == []
    assert merge([456, 271, 332, 211, 115, 136, 64, 36, 32, 20]) == [[0], [1], [2], [3], [4, 5], [6, 7, 8, 9]]
    assert merge([7, 0, 0, 3]) == [[0, 3]]
    assert merge([300, 0, 256, 1]) == [[0], [2], [3]]
    assert merge([5, 5, 5], limit=10) == [[0], [1, 2]]
    for counts in ([1] * 10, [255, 1, 0, 2, 254], [1000, 1000]):
        groups = merge(counts)
        assert [k for g in groups for k in g] == [k for k, c in enumerate(counts) if c]
        assert all(len(g) == 1 or sum(counts[k] for k in g) <= V.BLOCKED_MERGE_ENTITIES for g in groups)


def test_chunk_entities():
    assert V.blocked_chunk_entities(1024, V.DEFAULT_BLOCKED_WORKSPACE_BYTES) >= 256     # every CU of an MI355X busy
    assert V.blocked_chunk_entities(1024, 1) == 1
    assert V.blocked_chunk_entities(129, 3 * 8 * 129 * 129 + 5) == 3


def test_cpu_plan_routes_everything_to_torch():
    p = BlockProblem([(129, 129), (129, 200), (200, 129), (0, 7), (20, 20), (6, 25)], seed=5)
    rp, cp, csr, c = p.tensors("cpu")
    want = p.numpy_variances(0.1, cond_max=1e6)
    want[p.col_ptr[3]:p.col_ptr[4]] = 1.0 / 0.1
    for blocked in (0, VAR_BLOCKED_MMAX, 10 ** 6):
        plan = V.SegmentedFullVariance(rp, cp, csr, blocked_mmax=blocked)
        assert plan.classes == [] and plan.blocked_classes == []
        got, stats = plan.compute(c, 0.1)
        assert stats["primal"] == 0 and stats["row_space"] == 0 and stats["torch"] == 5 and stats["empty"] == 1
        if blocked:
            assert stats["blocked_primal"] == 0 and stats["blocked_row_space"] == 0
        else:
            assert stats == {"primal": 0, "row_space": 0, "torch": 5, "empty": 1, "failed_factors": 0}
        assert relative_error(got.numpy(), want) <= 1e-9
    assert np.isfinite(want).all()
