"""Saturated margins and zero-weight rows through every loss epilogue on the GPU.

Every kernel family carries its own copy of the pointwise terms ``wt l``, ``wt l'``, ``wt l''``. Two contracts:

C1. A row of weight exactly 0.0 adds exactly 0 to F, S, the gradient, the Hessian terms and every cached per-row value
    (``coef``, ``dzz``, ``D``), for any finite margin -- Poisson margins where ``exp`` overflows included
    (``wx`` in ``glm_kernels.hip`` / ``re_kernels.hip``; ``weighted`` in ``function/losses.py``).
C2. For weight > 0 the terms agree with the ``decimal`` reference of ``saturated_util`` within 4 rounding units
    (``saturated_util.bound_units``: 4 x the host's own worst error where that is above 1 unit; it never is) over the
    margin table 0 .. 1e4, both signs; an exact term beyond the largest double gives +inf, not NaN.

Pointwise (B): ``native.loss_sum`` (``ls_eval_kernel`` at t = 0, and with the margins as the direction at t = 1),
``DeviceGLMData`` on an identity design (one entry 1.0 per row, w = 0, the margins in the offsets) in both layouts and
the three precisions -- ``value_grad_sums`` (``g_j = wt_j l'_j``), ``hdiag_sums`` and ``hv_sums`` with v = 1
(``wt_j l''_j``, the latter through the ``dzz`` cache), ``zero_point_sums`` -- and the margin line search with
``z0 = 0``, ``zd = 2 z``, ``t = 0.5`` (``z0 + t zd`` exact with or without an fma): ``ls_begin`` at t0 = 0.5 (the
direction pass's first trial), ``ls_eval``, ``ls_eval_many`` (bitwise the single-step results) and
``ls_finish_sums``. One data set per magnitude band (|z| <= 1, 40, 104.5, 709.75, beyond); a sum is held to the
bound times the sum of its rows' units. Row weights alternate 1 and 0.5 (exact products). Per-row terms pass through
the row vectors' type (``DeviceGLMData.coef.dtype``: fp32 for the f32 and bf16 precisions), which adds one rounding
into that type (``saturated_util.stream_unit``); Poisson margins of 89 and above are left out of those precisions.

Solvers (C): ``native.rs_tron`` directly and every route of ``test_re_weighted_parity_gpu.py`` plus the OWL-QN kernel
through ``RandomEffectCoordinate``: a partial score of +800 on the zero-weight rows changes nothing, bit for bit, and
the fit matches the CPU float64 TRON on the rows of non-zero weight; LOGISTIC fits with saturated partial scores
(+-40, +-700 on 10 % of the weighted rows) match the oracle under the same partial scores.

Measured on an MI355X (worst error over the table in fp64 units; the bound is 4; every test prints its figures).
``loss_sum``, both modes alike:

    loss      per-entry l   band sums F
    LOGISTIC  0.46          0.60
    POISSON   0.47          0.21
    SQUARED   0.03          0.52
    HINGE     0.01          0.00

``DeviceGLMData`` in f64, tiled and segmented alike (F: ``value_grad_sums``, ``zero_point_sums``, ``ls_begin``'s first
trial, ``ls_eval`` and ``ls_finish_sums`` all give the same figure; l' rows: ``g``, ``coef`` and the finished line
search; l'' rows: ``dzz``, ``hv_sums``, ``hdiag_sums``):

    loss      F     S     line-search D   rows l'   rows l''   P (hv)
    LOGISTIC  0.60  0.22  0.15            0.54      0.54       0.12
    POISSON   0.21  0.41  0.36            0.46      0.46       0.21
    SQUARED   0.52  0.00  0.01            0.02      0.00       0.00
    HINGE     0.00  0.00  0.00            0.00      -          -

f32 and bf16 precisions (fp32 row vectors): the sums as in f64; per-row terms as a share of their bound (4 fp64 units
+ one fp32 rounding): LOGISTIC 0.68 (l') / 0.62 (l''), SQUARED 0.80 (l'), POISSON 1.00 -- ``e^z`` at z = 2^-24 is
``1 + 2^-24 + 2^-49``, just above a tie, and rounds up to ``1 + 2^-23``: the largest relative error a rounding to
nearest can make, ``u / (1 + u)`` -- and P 0.30 / 0.57.

The solvers (tolerance 0, 4 iterations; "oracle floor / GPU error" relative to the entity's largest coefficient, the
worst entity; the bound is max(1e-9, 8 floor)); equality with the fit under a partial score of 0 held bit for bit on
every route, cold in both regimes and warm at tolerance 1e-8:

    route        POISSON, +800 on w=0   LOGISTIC, +800 on w=0   LOGISTIC, saturated partial scores
    rs           3e-12 / 2e-11          1e-15 / 9e-16           6e-16 / 6e-16
    rs_big       1e-13 / 2e-13          1e-15 / 2e-15           2e-11 / 6e-11
    lean_quad    1e-10 / 2e-10          7e-16 / 9e-16           7e-13 / 5e-13
    lean_scalar  5e-15 / 3e-14          6e-16 / 6e-16           8e-15 / 8e-15
    resident     1e-10 / 2e-10          7e-16 / 8e-16           7e-13 / 4e-13
    tall         2e-09 / 6e-10          5e-16 / 1e-15           1e-13 / 5e-14
    csr          4e-14 / 6e-14          7e-16 / 1e-15           2e-15 / 5e-15
    dense_wide   2e-14 / 2e-14          1e-15 / 3e-15           5e-12 / 4e-12
    dense_hess   1e-13 / 1e-14          6e-16 / 9e-16           2e-14 / 2e-14
    pass         1e-10 / 1e-10          7e-16 / 1e-15           7e-13 / 4e-13
    OWL-QN (against batched_lbfgs on the CPU, bound 1e-9): 1e-15, 6e-16, 2e-15

What each guard is seen by (the guard put back to a plain product, one site at a time, POISSON cases fail):
``ls_eval_kernel`` -- ``test_loss_sum`` and ``zero_point_sums`` in ``test_device_glm_passes``; ``fwd_finish`` (the
gradient input) -- ``g`` in ``test_device_glm_passes`` and ``test_poisson_overflow_is_inf_not_nan``;
``rs_tron_kernel`` -- all eight ``test_rs_tron_ignores_zero_weight_rows[POISSON-*-2-*]``; the lean kernel's
zero-point sums -- the warm step of ``test_route_ignores_zero_weight_rows[lean_quad / lean_scalar-POISSON]`` (11 and
13 iterations against 8); the scalar row pass of ``re_kernels.hip`` -- the ``lean_scalar`` and ``csr`` routes and
``test_owlqn_ignores_zero_weight_rows[POISSON]``. LOGISTIC never overflows (``exp(-|z|)``), so its cases guard
against a later change of the formula, not against today's code.
"""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import saturated_util as su
from photon_ml_amd.optimization.optimizer import ConvergenceReason
from re_parity_util import (ROUTES, SHAPES, _check_routing, _set_route, cpu_tron, foreign_model, gpu_fit,
                            make_entities, reference_floor, rel_err)

pytestmark = pytest.mark.gpu

# zero-weight copies appended for C1 (margins whose Poisson exp overflows; +-1e4 for the other losses)
C1_MARGINS = {"POISSON": (710.0, 745.0, 1e4), "LOGISTIC": (1e4, -1e4), "SQUARED": (1e4, -1e4), "HINGE": (1e4, -1e4)}
STREAM_OF = {torch.float64: "f64", torch.float32: "f32", torch.bfloat16: "bf16"}


def _weights(n):
    return np.where(np.arange(n) % 2 == 0, 1.0, 0.5)


def _c1_rows(loss):
    return [(z, y) for z in C1_MARGINS[loss] for y in su.LABELS[loss]]


class Worst:
    """Worst error per quantity, in fp64 units (and as a share of the bound where a stream rounding is allowed)."""

    def __init__(self, tag):
        self.tag, self.units, self.share = tag, {}, {}

    def add(self, what, units, share):
        self.units[what] = max(self.units.get(what, 0.0), units)
        self.share[what] = max(self.share.get(what, 0.0), share)

    def report(self):
        print(f"SATURATED {self.tag}: " + ", ".join(f"{k} {v:.2f}u/{self.share[k]:.2f}" for k, v in self.units.items()))


def _check_value(worst, what, got, ex, units, loss, term, stream="f64"):
    """``got`` against the exact value ``ex`` whose rounding units are ``units``: within ``bound_units`` units plus
    one rounding into the stream type."""
    allowed = su.Decimal(su.bound_units(loss, term)) * units + su.stream_unit(stream, ex)
    err_u = su.error_units(got, ex, units)
    share = su.error_units(got, ex, allowed)
    worst.add(what, err_u if stream == "f64" else 0.0, share)
    assert share <= 1.0, (worst.tag, what, float(got), float(ex) if not su.overflows(ex) else "overflow", err_u, share)


def _check_sum(worst, what, got, loss, term, rows, ws, factor=None, stream="f64"):
    tot, units = su.weighted_sum(loss, term, rows, ws, factor)
    _check_value(worst, what, got, tot, units, loss, term, stream)


def _check_rows(worst, what, got, loss, term, rows, ws, stream):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (len(rows),)
    for i, ((z, y), w) in enumerate(zip(rows, ws)):
        tot, units = su.weighted_sum(loss, term, [(z, y)], [w])
        _check_value(worst, what, got[i], tot, units, loss, term, stream)


# ---------------------------------------------------------------------------------------------------------------
# B. native.loss_sum

def _dev(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, device="cuda")


def _loss_sum(loss, rows, ws, as_offsets):
    from photon_ml_amd.ops import native
    z, y, w = _dev([r[0] for r in rows]), _dev([r[1] for r in rows]), _dev(ws)
    out = native.loss_sum(su.LOSS_IDS[loss], torch.zeros_like(z), y, w, z) if as_offsets else \
        native.loss_sum(su.LOSS_IDS[loss], z, y, w)
    assert out is not None
    return float(out)


@pytest.mark.parametrize("as_offsets", [False, True], ids=["t0", "offsets_t1"])
@pytest.mark.parametrize("loss", su.LOSSES)
def test_loss_sum(loss, as_offsets):
    worst = Worst(f"loss_sum {loss} {'offsets' if as_offsets else 'margins'}")
    for z, y in su.table(loss):                       # per-entry l from 1-element calls, weights 1 and 0.5
        for w in (1.0, 0.5):
            _check_sum(worst, "l", _loss_sum(loss, [(z, y)], [w], as_offsets), loss, "l", [(z, y)], [w])
    extra = _c1_rows(loss)
    for b, rows in enumerate(su.band_rows(loss)):
        ws = _weights(len(rows))
        got = _loss_sum(loss, rows, ws, as_offsets)
        _check_sum(worst, f"F band{b}", got, loss, "l", rows, ws)
        # C1: zero-weight rows of overflowing margins, appended and interleaved, add exactly 0
        with_zero = _loss_sum(loss, rows + extra, np.concatenate([ws, np.zeros(len(extra))]), as_offsets)
        assert with_zero == got, (loss, b, with_zero, got)
        with_zero = _loss_sum(loss, extra + rows, np.concatenate([np.zeros(len(extra)), ws]), as_offsets)
        _check_sum(worst, f"F band{b}", with_zero, loss, "l", rows, ws)
    assert _loss_sum(loss, extra, np.zeros(len(extra)), as_offsets) == 0.0
    if loss == "POISSON":                             # weight > 0 at z = 710: +inf, not NaN
        assert _loss_sum(loss, [(710.0, 3.0), (0.5, 0.0)], [0.5, 1.0], as_offsets) == float("inf")
    worst.report()


# ---------------------------------------------------------------------------------------------------------------
# B. DeviceGLMData on an identity design

def _identity_data(rows, ws, offsets=True):
    from photon_ml_amd.data.matrix import LabeledData
    n = len(rows)
    z = np.array([r[0] for r in rows])
    return LabeledData(sp.identity(n, format="csr"), np.array([r[1] for r in rows]), z if offsets else np.zeros(n),
                       np.asarray(ws, dtype=np.float64))


def _passes(loss, layout, precision, rows, ws):
    """Every pointwise pass of ``DeviceGLMData`` over ``rows`` (an identity design): a dict of host results."""
    from photon_ml_amd.ops.device import DeviceGLMData
    lo = su.loss_object(loss)
    n = len(rows)
    dev = DeviceGLMData.from_labeled(_identity_data(rows, ws), "cuda", precision, layout=layout)
    assert dev.n_rows == n and dev.dim == n
    out = {"stream": STREAM_OF[dev.coef.dtype]}
    zero = torch.zeros(n, dtype=torch.float64, device="cuda")
    dev.track_hessian = True
    f, s, g = dev.value_grad_sums(lo, zero, 0.0)
    out.update(F=f, S=s, g=g.cpu().numpy(), coef=dev.coef[:n].double().cpu().numpy())
    if lo.twice_differentiable:
        out["dzz"] = dev.dzz[:n].double().cpu().numpy()
        h, p = dev.hv_sums(lo, zero, 0.0, torch.ones(n, dtype=torch.float64, device="cuda"), 0.0)
        out.update(hv=h.cpu().numpy(), P=p)
        out["hdiag"] = dev.hdiag_sums(lo, zero).cpu().numpy()
    dev.track_hessian = False
    zp = dev.zero_point_sums(lo, 0.0)
    out.update(zF=zp[0], zS=zp[1], zC=zp[2], zX=zp[3])
    # margin line search: z0 = 0 (offsets 0, w0 = 0), zd = 2 z, t = 0.5
    ls = DeviceGLMData.from_labeled(_identity_data(rows, ws, offsets=False), "cuda", precision, layout=layout)
    d = _dev([2.0 * r[0] for r in rows])
    assert ls.ls_begin(zero, 0.0, d, 0.0, t0=0.5, loss=lo)
    out["ls_first"] = ls.ls_eval(lo, 0.5)                   # the direction pass's own first trial (fwd_finish)
    assert ls.ls_begin(zero, 0.0, d, 0.0, t0=1.0, loss=lo)
    out["ls_half"] = ls.ls_eval(lo, 0.5)                    # ls_eval_kernel
    out["ls_quarter"] = ls.ls_eval(lo, 0.25)
    out["ls_many"] = ls.ls_eval_many(lo, [0.5, 0.25])       # ls_eval_multi_kernel
    f, s, g = ls.ls_finish_sums(lo, 0.5, 0.5 * d, 0.0)      # ls_eval_kernel, final
    out.update(lsF=f, lsS=s, lsg=g.cpu().numpy(), lscoef=ls.coef[:n].double().cpu().numpy())
    return out


SUMS = ("F", "S", "P", "zF", "zS", "zC", "zX", "lsF", "lsS")
VECTORS = ("g", "coef", "dzz", "hv", "hdiag", "lsg", "lscoef")
PAIRS = ("ls_first", "ls_half")


@pytest.mark.parametrize("precision", ["f64", "f32", "bf16"])
@pytest.mark.parametrize("layout", ["tiled", "segmented"])
@pytest.mark.parametrize("loss", su.LOSSES)
def test_device_glm_passes(loss, layout, precision):
    worst = Worst(f"DeviceGLMData {loss} {layout} {precision}")
    extra = _c1_rows(loss)
    for b, rows in enumerate(su.band_rows(loss, stream=precision != "f64")):
        ws = _weights(len(rows))
        n = len(rows)
        r = _passes(loss, layout, precision, rows, ws)
        st = r["stream"]
        assert st == ("f64" if precision == "f64" else "f32")
        zd = [2.0 * z for z, _ in rows]
        # sums (fp64 accumulation of fp64 terms; P sums the streamed l'')
        _check_sum(worst, "F", r["F"], loss, "l", rows, ws)
        _check_sum(worst, "S", r["S"], loss, "dl", rows, ws)
        _check_sum(worst, "zero F", r["zF"], loss, "l", rows, ws)
        _check_sum(worst, "zero S", r["zS"], loss, "dl", rows, ws)
        assert r["zX"] == float(n)
        for key in PAIRS:
            _check_sum(worst, key + " F", r[key][0], loss, "l", rows, ws)
            _check_sum(worst, key + " D", r[key][1], loss, "dl", rows, ws, factor=zd)
        _check_sum(worst, "finish F", r["lsF"], loss, "l", rows, ws)
        _check_sum(worst, "finish S", r["lsS"], loss, "dl", rows, ws)
        # one pass over several step lengths: bitwise the single-step results
        # (t = 0.25 is the margin z / 2: checked for equality with the single step only)
        assert _same(r["ls_many"][0], r["ls_half"]) and _same(r["ls_many"][1], r["ls_quarter"])
        # per-row terms through the row vectors' type
        for key in ("g", "coef", "lsg", "lscoef"):
            _check_rows(worst, key, r[key], loss, "dl", rows, ws, st)
        if "dzz" in r:
            for key in ("dzz", "hv", "hdiag"):
                _check_rows(worst, key, r[key], loss, "d2", rows, ws, st)
            _check_sum(worst, "P", r["P"], loss, "d2", rows, ws, stream=st)
        # ||c||^2 of the stored coefficients: each c_i within its bound, so c_i^2 within 2 |c_i| bound_i (+ the square's
        # and the sum's own roundings, 4 x 2^-52 of the total)
        cs = [su.weighted_sum(loss, "dl", [row], [w]) for row, w in zip(rows, ws)]
        with su.localcontext() as ctx:
            ctx.prec = su.PREC
            ex_c = sum((t * t for t, _ in cs), su.Decimal(0))
            al_c = sum((2 * abs(t) * (su.Decimal(su.bound_units(loss, "dl")) * u + su.stream_unit(st, t))
                        for t, u in cs), su.Decimal(0)) + 4 * su.EPS64 * ex_c + su.TINY64
        assert su.error_units(r["zC"], ex_c, al_c) <= 1.0, (worst.tag, b, r["zC"])
        # C1: zero-weight rows of overflowing margins appended -- every sum and gradient entry equal to the result
        # without them (checked against the reference above: finite, or +inf where the band's own exact value exceeds
        # the largest double; never NaN), their own entries 0
        rz = _passes(loss, layout, precision, rows + extra, np.concatenate([ws, np.zeros(len(extra))]))
        for key in SUMS:
            if key in r and key != "zX":
                assert rz[key] == r[key], (worst.tag, key, rz[key], r[key])       # a NaN equals nothing
        for key in PAIRS + ("ls_quarter",):
            assert _same(rz[key], r[key]), (worst.tag, key, rz[key], r[key])
        assert _same(rz["ls_many"][0], r["ls_many"][0]) and _same(rz["ls_many"][1], r["ls_many"][1])
        for key in VECTORS:
            if key in r:
                assert not np.isnan(rz[key]).any(), (worst.tag, key)
                assert np.array_equal(rz[key][:n], r[key]), (worst.tag, key)
                assert not rz[key][n:].any(), (worst.tag, key, rz[key][n:])
    worst.report()


def _same(a, b):
    """Bitwise-equal values up to the sign of zero (inf == inf; a NaN equals nothing)."""
    return bool(np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)))


def test_poisson_overflow_is_inf_not_nan():
    """A weight > 0 row at the Poisson margin 710: F = +inf (and the row's gradient entry), not NaN; next to it a
    zero-weight row at the same margin still adds 0."""
    rows = [(710.0, 3.0), (0.5, 0.0), (710.0, 0.0)]
    for layout in ("tiled", "segmented"):
        r = _passes("POISSON", layout, "f64", rows, [0.5, 1.0, 0.0])
        assert r["F"] == r["zF"] == r["lsF"] == float("inf") and r["ls_half"][0] == float("inf")
        assert r["g"][0] == float("inf") and r["hdiag"][0] == float("inf")
        one = su.weighted_sum("POISSON", "dl", [rows[1]], [1.0])
        assert su.error_units(r["g"][1], *one) <= su.bound_units("POISSON", "dl")
        assert r["g"][2] == 0.0 and r["hdiag"][2] == 0.0 and r["hv"][2] == 0.0 and r["lsg"][2] == 0.0


# ---------------------------------------------------------------------------------------------------------------
# C. native.rs_tron: o = 800 on the zero-weight rows changes nothing

@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("n,variant", [(n, v) for v in (2, 5) for n in (7, 20, 33, 64)] + [(80, 5), (128, 5)])
@pytest.mark.parametrize("loss", ["POISSON", "LOGISTIC"])
def test_rs_tron_ignores_zero_weight_rows(loss, n, warm, variant):
    """B = 64 problems built as ``test_kernels_gpu._check_rs_tron`` builds them (rows past each problem's count have
    weight 0): ``rs_tron_kernel`` (variant 2) and ``rs_tron_dpp_kernel`` (the default variant) for n <= 64,
    ``rs_tron_big_kernel`` above."""
    from photon_ml_amd.ops.native import require_glm_lib, rs_tron
    g = torch.Generator(device="cuda").manual_seed(7 * n + int(warm))
    B = 64
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)
    L = torch.tril(rnd(B, n, n)) * 0.5
    L.diagonal(dim1=1, dim2=2).copy_(torch.rand(B, n, dtype=torch.float64, device="cuda", generator=g) + 0.5)
    nvalid = torch.randint(1, n + 1, (B,), device="cuda", generator=g)
    nvalid[0] = 1                                     # at least one problem with zero-weight rows, whatever the draw
    valid = torch.arange(n, device="cuda").unsqueeze(0) < nvalid.unsqueeze(1)
    w = torch.where(valid, torch.rand(B, n, dtype=torch.float64, device="cuda", generator=g) + 0.5, 0.0)
    z = rnd(B, n)
    y = (z > 0).double() if loss == "LOGISTIC" else z.abs().round()
    o = 0.1 * rnd(B, n)
    b0 = 0.3 * rnd(B, n) if warm else torch.zeros(B, n, dtype=torch.float64, device="cuda")
    assert n == 1 or bool((w == 0).any())
    lib = require_glm_lib()
    lib.pml_rs_set_variant(variant)
    try:
        res = []
        for fill in (0.0, 800.0):
            zout = torch.full_like(b0, float("nan"))
            off = torch.where(w == 0, torch.full_like(o, fill), o)
            res.append((*rs_tron(L, y, off, w, b0, su.LOSS_IDS[loss], 0.7, 1e-9, 30, zout=zout), zout))
    finally:
        lib.pml_rs_set_variant(int(os.environ.get("PML_RS_VARIANT", "5")))
    for name, a, b in zip(("beta", "f", "iters", "reason", "zout"), *res):
        assert bool(torch.isfinite(b.double()).all()), (loss, n, name)
        assert torch.equal(a, b), (loss, n, name)
    assert int(res[1][2].max()) > 1


# ---------------------------------------------------------------------------------------------------------------
# C. the fused solvers through RandomEffectCoordinate

L2 = 1.0
LIMITED = (0.0, 4)
CONVERGED = (1e-8, 60)
SOLVER_LOSSES = ("POISSON", "LOGISTIC")


@functools.lru_cache(maxsize=None)
def _data(shape, loss):
    sizes, d_pool, nnz_row, dense, seed = SHAPES[shape]
    return make_entities(sizes, d_pool, nnz_row, seed, dense_pool=dense, loss=loss)


@functools.lru_cache(maxsize=None)
def _dropped_reference(shape, loss):
    """The oracle on the rows of non-zero weight only (shared by the routes of a shape, never modified), and its
    floor under a permutation of each entity's rows."""
    data = _data(shape, loss)
    rows = np.nonzero(data.weights != 0)[0]
    ref = cpu_tron(data, loss, L2, *LIMITED, rows=rows)
    return ref, reference_floor(ref, cpu_tron(data, loss, L2, *LIMITED, rows=rows, perm_seed=1))


@functools.lru_cache(maxsize=None)
def _saturated_partial(shape):
    """About 10 % of the weighted rows get a partial score from {+-40, +-700}; zero-weight rows stay at 0."""
    data = _data(shape, "LOGISTIC")
    rng = np.random.default_rng(5)
    p = np.where(rng.random(data.n_rows) < 0.1, rng.choice([40.0, -40.0, 700.0, -700.0], size=data.n_rows), 0.0)
    p[data.weights == 0] = 0.0
    assert (p != 0).sum() > 20
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _saturated_reference(shape):
    data, p = _data(shape, "LOGISTIC"), _saturated_partial(shape)
    ref = cpu_tron(data, "LOGISTIC", L2, *LIMITED, partial=p)
    return ref, reference_floor(ref, cpu_tron(data, "LOGISTIC", L2, *LIMITED, partial=p, perm_seed=1))


def _against_oracle(tag, ref, floor, W, its, reasons):
    """Tolerance 0 / 4 iterations: every entity at MAX_ITERATIONS after 4 on both sides, W within max(1e-9, 8 floor)."""
    bound = max(1e-9, 8 * floor)
    worst = 0.0
    for e, (w_ref, it_ref, reason_ref) in ref.items():
        assert its[e] == it_ref == 4, (tag, e, its[e], it_ref)
        assert reasons[e] == reason_ref == ConvergenceReason.MAX_ITERATIONS, (tag, e, reasons[e], reason_ref)
        assert np.isfinite(W[e]).all(), (tag, e)
        err = rel_err(W[e], w_ref)
        worst = max(worst, err)
        assert err <= bound, (tag, e, err, bound, floor)
    print(f"SATURATED {tag}: floor {floor:.2e} bound {bound:.2e} gpu error {worst:.2e}")


@pytest.mark.parametrize("loss", SOLVER_LOSSES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_route_ignores_zero_weight_rows(route, loss, monkeypatch):
    """A partial score of +800 on the zero-weight rows (0 elsewhere): W, iteration counts and stop reasons finite and
    equal, per entity, to the GPU fit under a partial score of 0, at tolerance 0 / 4 iterations and at tolerance
    1e-8; at tolerance 0 the fit also matches the oracle on the rows of non-zero weight."""
    shape, layout = _set_route(route, monkeypatch)
    data = _data(shape, loss)
    assert (data.weights == 0).sum() > 10
    p800 = np.where(data.weights == 0, 800.0, 0.0)
    for regime, name in ((LIMITED, "limited"), (CONVERGED, "converged")):
        W0, its0, reasons0, c, _ = gpu_fit(data, loss, L2, *regime, monkeypatch, partial=np.zeros(data.n_rows),
                                           layout=layout)
        _check_routing(route, c, data)
        W, its, reasons, c, m = gpu_fit(data, loss, L2, *regime, monkeypatch, partial=p800, layout=layout)
        _check_routing(route, c, data)
        for e in W0:
            assert np.isfinite(W[e]).all(), (route, loss, name, e)
            assert its[e] == its0[e] and reasons[e] == reasons0[e], (route, loss, name, e, its[e], its0[e])
            assert np.array_equal(W[e], W0[e]), (route, loss, name, e, float(np.abs(W[e] - W0[e]).max()))
        if regime == LIMITED:
            ref, floor = _dropped_reference(shape, loss)
            _against_oracle(f"{route} {loss} zero-weight rows at +800", ref, floor, W, its, reasons)
            w_half, m_cold = {e: W[e] * 0.5 for e in W}, m
    # warm from a foreign model (the limited fit, halved) at tolerance 1e-8: the zero point's f(0) and ||g(0)|| set the
    # stopping tolerances (the lean kernel's zero-point sums over the rows' offsets), so a NaN there changes the counts
    base = np.where(data.weights == 0, 0.0, 0.3 * np.cos(np.arange(data.n_rows)))
    fits = [gpu_fit(data, loss, L2, *CONVERGED, monkeypatch, partial=base + extra,
                    start=foreign_model(m_cold, w_half, loss), layout=layout) for extra in (0.0, p800)]
    (W0, its0, reasons0, _, _), (W, its, reasons, _, _) = fits
    for e in W0:
        assert np.isfinite(W[e]).all(), (route, loss, "warm", e)
        assert its[e] == its0[e] and reasons[e] == reasons0[e], (route, loss, "warm", e, its[e], its0[e])
        assert np.array_equal(W[e], W0[e]), (route, loss, "warm", e, float(np.abs(W[e] - W0[e]).max()))
    assert max(its.values()) > 1


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_with_saturated_partial_scores(route, monkeypatch):
    """LOGISTIC under partial scores of +-40 and +-700 on about 10 % of the weighted rows: tolerance 0, 4 iterations,
    against the oracle under the same partial scores. No allowed share of mismatching entities."""
    shape, layout = _set_route(route, monkeypatch)
    data, p = _data(shape, "LOGISTIC"), _saturated_partial(shape)
    W, its, reasons, c, _ = gpu_fit(data, "LOGISTIC", L2, *LIMITED, monkeypatch, partial=p, layout=layout)
    _check_routing(route, c, data)
    ref, floor = _saturated_reference(shape)
    _against_oracle(f"{route} LOGISTIC saturated partial scores", ref, floor, W, its, reasons)


# the OWL-QN kernel (re_lbfgs_csr_kernel, L1) on the weighted "lean" shape; its yardstick is batched_lbfgs on the CPU

OWL_LIMITED = (0.0, 5, 1e-9)
OWL_CONVERGED = (1e-8, 100, 1e-6)


@pytest.mark.parametrize("loss", SOLVER_LOSSES)
def test_owlqn_ignores_zero_weight_rows(loss):
    from re_parity_util import TASKS
    from test_re_owlqn_gpu import assert_parity, assert_routed, coordinate, update
    data = _data("lean", loss)
    p800 = np.where(data.weights == 0, 800.0, 0.0)
    for tol, max_iter, bound in (OWL_LIMITED, OWL_CONVERGED):
        c = coordinate(data, TASKS[loss], "L1", 0.5, tol, max_iter, "cuda")
        base = update(c, np.zeros(data.n_rows))
        assert_routed(c)
        c = coordinate(data, TASKS[loss], "L1", 0.5, tol, max_iter, "cuda")
        got = update(c, p800)
        assert_routed(c)
        for e in base[0]:
            assert np.isfinite(got[0][e]).all(), (loss, tol, e)
            assert got[1][e] == base[1][e] and got[2][e] == base[2][e], (loss, tol, e)
            assert np.array_equal(got[0][e], base[0][e]), (loss, tol, e)
        if tol == 0.0:
            ref = update(coordinate(data, TASKS[loss], "L1", 0.5, tol, max_iter, "cpu"), np.zeros(data.n_rows))
            assert_parity(got, ref, bound, f"SATURATED owlqn {loss} zero-weight rows at +800")


def test_owlqn_with_saturated_partial_scores():
    from test_re_owlqn_gpu import assert_parity, assert_routed, coordinate, update
    data, p = _data("lean", "LOGISTIC"), np.array(_saturated_partial("lean"))
    tol, max_iter, bound = OWL_LIMITED
    c = coordinate(data, "LOGISTIC_REGRESSION", "L1", 0.5, tol, max_iter, "cuda")
    got = update(c, p)
    assert_routed(c)
    ref = update(coordinate(data, "LOGISTIC_REGRESSION", "L1", 0.5, tol, max_iter, "cpu"), p)
    assert all(np.isfinite(w).all() for w in got[0].values())
    assert_parity(got, ref, bound, "SATURATED owlqn LOGISTIC saturated partial scores")
