"""Normalization for random-effect coordinates on the GPU: the shifted fused TRON (``re_tron_csr_kernel<LOSS,
true>``) against the CPU definition (``SegmentedGLMData`` with a shift, the pass path) and the independent dense
oracle of ``re_norm_util``; scale-only contexts across the row-space, lean, tall and fused OWL-QN routes; routing
under shifts.

Bounds are those of ``test_re_parity_gpu.py``: iteration-limited (tolerance 0, 2 iterations) identical iteration
counts and W to 1e-9 relative; converged (tolerance 1e-8) identical iteration counts and stop reasons, W to 1e-6
relative.
"""
import numpy as np
import pytest
import torch

import re_norm_util as U

pytestmark = pytest.mark.gpu

# (rows, coefficients) per entity, one launch set: d_e = 1 (intercept only), 2, 64 / 65 and 256 / 257 / 300 (across
# the 256-thread stride of the sweeps and the first class edge), 1025 and 2048 (the widest class); n_e = 1; n_e = 100
# (more rows than one pass keeps in flight: 4 waves x 16 rows)
SHAPES = [(5, 1), (1, 2), (40, 64), (30, 65), (20, 256), (100, 257), (60, 300), (12, 1025), (10, 2048), (1, 30)]
LAM = 1.5
# Two iterations in the limited regime: the launch set must hold entities of one and two coefficients, and Newton
# steps bring those to their optimum to rounding by the third or fourth iteration, where accepting a step -- and
# with it the iteration count -- is decided by rounding alone (measured: the one-row, two-coefficient entity took 3
# iterations on the GPU and 4 on the CPU with W equal to 5e-14). After two iterations every entity still takes real steps.
REGIMES = {"limited": (0.0, 2, 1e-9), "converged": (1e-8, 200, 1e-6)}
# Poisson: the standardized columns have unit variance whatever the input, so from zero the first trust region
# (||g0|| ~ sqrt(n d)) reaches margins where exp() overflows, and a weakly regularized solve spends its first
# iterations in rejected steps whose f - f_new cancels catastrophically: two correct fp64 implementations then part
# ways by far more than rounding (seen on the CPU between the dense oracle and the pass-path definition at lambda
# 1.5 .. 50). A strong L2 weight keeps the iterates where the comparison is about rounding.
TASK_LAM = {"POISSON_REGRESSION": 300.0}
# squared loss: the first full CG solve reaches the optimum of a one- or two-coefficient entity to rounding, after
# which accept / reject (and so the iteration count) is decided by rounding alone: one iteration in the limited
# regime. Likewise the strongly regularized Poisson case: its smallest entities are at their optimum to rounding
# after two iterations.
TASK_LIMITED_ITERS = {"LINEAR_REGRESSION": 1, "POISSON_REGRESSION": 2}


def _cfg(task, regime):
    tol, iters, _ = REGIMES[regime]
    if regime == "limited":
        iters = TASK_LIMITED_ITERS.get(task, iters)
    return U.opt_config("TRON", "L2", TASK_LAM.get(task, LAM), tol, iters)
CASES = [("first", "LOGISTIC_REGRESSION"), ("last", "LOGISTIC_REGRESSION"), ("middle", "LOGISTIC_REGRESSION"),
         ("middle", "POISSON_REGRESSION"), ("last", "LINEAR_REGRESSION")]

_CACHE = {}


def _setup(intercept, task):
    """Data, context and the CPU references of one case (computed once, shared by the tests, never changed)."""
    key = (intercept, task)
    if key not in _CACHE:
        data, icpt = U.make_data(SHAPES, intercept, seed=11, task=task)
        ctx = U.build_context(data, "STANDARDIZATION", icpt)
        ref = {}
        for regime in REGIMES:
            cfg = _cfg(task, regime)
            W_or, _, it_or, rc_or = U.oracle(data, ctx, icpt, cfg, task)
            W_cpu, it_cpu, rc_cpu, _ = U.run(U.coordinate(data, cfg, task, normalization=ctx))
            ref[regime] = (cfg, W_or, it_or, rc_or, W_cpu, it_cpu, rc_cpu)
        _CACHE[key] = (data, icpt, ctx, ref)
    return _CACHE[key]


def _gpu(data, cfg, task, ctx, **kw):
    return U.coordinate(data, cfg, task, device="cuda", layout="segmented", normalization=ctx, **kw)


def _assert_shifted_routing(c, n_fused, n_pass=0):
    r = c.solver_routing()
    assert r.get("shifted") is True and r["row_space"] == 0 and r["lean"] == 0 and r["hessian"] == 0
    assert "resident" not in r
    assert r["fused"] == n_fused and r["pass_path"] == n_pass
    rs, fused, sub = c._comps
    assert rs is None and fused.res is None and fused.shift is not None
    assert all(not is_h and dm in (256, 512, 1024, 2048) for dm, _, is_h in fused.launches)


@pytest.mark.parametrize("intercept,task", CASES)
def test_shifted_fused_kernel_matches_cpu_definition_and_oracle(intercept, task):
    data, icpt, ctx, ref = _setup(intercept, task)
    for regime, (_, _, bound) in REGIMES.items():
        cfg, W_or, it_or, rc_or, W_cpu, it_cpu, rc_cpu = ref[regime]
        # the CPU definition itself meets the bounds against the oracle
        assert np.array_equal(it_cpu, it_or) and np.array_equal(rc_cpu, rc_or)
        assert U.rel_err(W_cpu, W_or) <= bound
        c = _gpu(data, cfg, task, ctx)
        W, it, rc, m = U.run(c)
        _assert_shifted_routing(c, len(SHAPES))
        e_cpu, e_or = U.rel_err(W, W_cpu), U.rel_err(W, W_or)
        print(f"{intercept} {task} {regime}: vs CPU definition {e_cpu:.3e}, vs oracle {e_or:.3e}")
        assert np.array_equal(it, it_cpu) and np.array_equal(rc, rc_cpu)
        assert e_cpu <= bound and e_or <= bound
        # the margins written by the solve are the true margins X w
        D = data.shards["user"].shape[1]
        xw = np.asarray(data.shards["user"] @ W.T)[np.arange(data.n_rows), data.id_tags["userId"]]
        s = c.score(m).cpu().numpy()
        assert np.abs(s - xw).max() <= 1e-9 * max(1.0, np.abs(xw).max()), D


@pytest.mark.parametrize("intercept,task", [CASES[0], CASES[3]])
def test_shifted_fused_kernel_is_bitwise_repeatable(intercept, task):
    data, icpt, ctx, ref = _setup(intercept, task)
    cfg = ref["limited"][0]
    c = _gpu(data, cfg, task, ctx)
    W1, it1, _, _ = U.run(c)
    W2, it2, _, _ = U.run(c)                     # a fresh start model: the same launches from zero again
    assert np.array_equal(W1, W2) and np.array_equal(it1, it2)
    W3, _, _, _ = U.run(_gpu(data, cfg, task, ctx))
    assert np.array_equal(W1, W3)


@pytest.mark.parametrize("intercept,task", [CASES[0], CASES[2]])
def test_shifted_fused_kernel_foreign_warm_start(intercept, task):
    """A model the coordinate did not return enters through T^-1; the second update of the same coordinate starts
    from its cached transformed-space state. Both reproduce the oracle's solve from the same w."""
    data, icpt, ctx, ref = _setup(intercept, task)
    # one iteration per update: the second update is every entity's second iteration overall, still a real step
    # (see REGIMES; with two per update the one-row, two-coefficient entity is at its optimum to rounding)
    cfg = U.opt_config("TRON", "L2", LAM, 0.0, 1)
    W1, _, it1, _ = U.oracle(data, ctx, icpt, cfg, task)
    W_ref, _, it_ref, _ = U.oracle(data, ctx, icpt, cfg, task, start_w=W1)
    c = _gpu(data, cfg, task, ctx)
    W, it, _, _ = U.run(c, start=U.dense_model(c, W1))
    assert np.array_equal(it, it_ref)
    assert U.rel_err(W, W_ref) <= 1e-9
    c2 = _gpu(data, cfg, task, ctx)
    Wa, ita, _, ma = U.run(c2)
    assert np.array_equal(ita, it1) and U.rel_err(Wa, W1) <= 1e-9
    Wb, itb, _, _ = U.run(c2, start=ma)
    assert np.array_equal(itb, it_ref)
    assert U.rel_err(Wb, W_ref) <= 1e-9


# ---- scale-only contexts: every route runs unchanged on the folded CSR
# row space (n_e <= d_e), tall (d_e <= 64 < n_e), lean (64 < d_e <= 1024, n_e > d_e). Every entity draws its
# features from one common pool, so each feature is non-zero in a good share of ALL rows and its shard-wide variance
# -- hence its factor -- stays O(1); a feature that only one small entity holds has a shard-wide standard deviation
# near 0.1 and a factor near 10, which costs the per-entity problems two to three digits of conditioning.
SCALE_SHAPES = [(10, 40), (20, 30), (33, 80), (150, 20), (90, 50), (140, 100), (200, 130), (1, 1), (70, 3)]


@pytest.mark.parametrize("norm_type", ["SCALE_WITH_MAX_MAGNITUDE", "SCALE_WITH_STANDARD_DEVIATION"])
@pytest.mark.parametrize("solver", ["tron", "owlqn"])
def test_scale_only_routes_match_cpu_definition(norm_type, solver):
    task = "LOGISTIC_REGRESSION"
    key = ("scale", norm_type)
    if key not in _CACHE:
        data, icpt = U.make_data(SCALE_SHAPES, "middle", seed=17, task=task, shared=130)
        _CACHE[key] = (data, icpt, U.build_context(data, norm_type, icpt))
    data, icpt, ctx = _CACHE[key]
    opt, reg = ("TRON", "L2") if solver == "tron" else ("LBFGS", "ELASTIC_NET")
    for regime, (tol, iters, bound) in REGIMES.items():
        cfg = U.opt_config(opt, reg, LAM, tol, iters)
        W_or, _, it_or, rc_or = U.oracle(data, ctx, icpt, cfg, task)
        W_cpu, it_cpu, rc_cpu, _ = U.run(U.coordinate(data, cfg, task, normalization=ctx))
        assert np.array_equal(it_cpu, it_or) and np.array_equal(rc_cpu, rc_or) and U.rel_err(W_cpu, W_or) <= bound
        c = _gpu(data, cfg, task, ctx)
        W, it, rc, _ = U.run(c)
        r = c.solver_routing()
        rs, fused, sub = c._comps
        assert "shifted" not in r and sub is None
        if solver == "tron":
            assert r["row_space"] >= 3 and r["row_space"] + r["fused"] == len(SCALE_SHAPES)
            kinds = {(bool(is_h), dm <= 1024) for dm, _, is_h in fused.launches}
            assert (True, True) in kinds and (False, True) in kinds   # tall (Hessian) and lean launches
        else:
            assert rs is None and getattr(fused, "kind", "") == "lbfgs" and r["fused"] == len(SCALE_SHAPES)
        e_cpu = U.rel_err(W, W_cpu)
        print(f"{norm_type} {solver} {regime}: vs CPU definition {e_cpu:.3e}, vs oracle {U.rel_err(W, W_or):.3e}")
        assert np.array_equal(it, it_cpu) and np.array_equal(rc, rc_cpu)
        assert e_cpu <= bound and U.rel_err(W, W_or) <= bound


# ---- routing under shifts
def test_routing_under_shifts():
    """No entity on the row-space or lean routes; an entity of more than 2048 coefficients on the pass path (with
    shifts), next to the fused launch; L-BFGS coordinates take the pass path whole."""
    task = "LOGISTIC_REGRESSION"
    shapes = [(6, 2100), (8, 10), (20, 300), (150, 20), (3, 70)]
    data, icpt = U.make_data(shapes, "first", seed=23, task=task)
    ctx = U.build_context(data, "STANDARDIZATION", icpt)
    cfg = U.opt_config("TRON", "L2", LAM, 0.0, 4)
    W_cpu, it_cpu, rc_cpu, _ = U.run(U.coordinate(data, cfg, task, normalization=ctx))
    c = _gpu(data, cfg, task, ctx)
    W, it, rc, _ = U.run(c)
    _assert_shifted_routing(c, len(shapes) - 1, n_pass=1)
    sub = c._comps[2]
    assert sub.seg.shift is not None and int(sub.entities[0]) == 0
    assert np.array_equal(it, it_cpu) and np.array_equal(rc, rc_cpu)
    assert U.rel_err(W, W_cpu) <= 1e-9
    # the same data without normalization uses the row-space and lean routes
    plain = U.coordinate(data, cfg, task, device="cuda", layout="segmented")
    U.run(plain)
    r = plain.solver_routing()
    assert "shifted" not in r and r["row_space"] > 0
    # L-BFGS / OWL-QN under shifts: no fused components, the pass path over the whole coordinate
    cfg_l = U.opt_config("LBFGS", "ELASTIC_NET", LAM, 0.0, 4)
    Wl_cpu, itl_cpu, _, _ = U.run(U.coordinate(data, cfg_l, task, normalization=ctx))
    cl = _gpu(data, cfg_l, task, ctx)
    Wl, itl, _, _ = U.run(cl)
    assert cl.solver_routing() == {}
    assert np.array_equal(itl, itl_cpu) and U.rel_err(Wl, Wl_cpu) <= 1e-9
