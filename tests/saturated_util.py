"""Saturated margins for the pointwise loss terms (not a test file): the margin table, a ``decimal`` reference of
``(l, l', l'')`` for the formulas of ``function/losses.py``, the rounding unit of each term and the bound the GPU
kernels are held to.

Reference. 800 significant digits, so that ``1 + e^-746`` keeps its small part (80 digits round it away: the
logistic loss at z = -700 would be 0 where the true value is 9.86e-305); below ``e = 1e-390`` the series
``log1p(e) = e - e^2 / 2`` stands in (next term below 1e-1170 relative to nothing the doubles can hold).
``sigmoid - 1`` and ``1 - sigmoid`` are formed without a subtraction (``p = e / (1 + e)``, ``q = 1 / (1 + e)``).

Rounding unit of a term (``unit``): ``2^-52 |exact| + 2^-1074``; logistic ``l'`` and ``l''`` add an absolute
``2^-52`` (the sigmoid is rounded at 1 before ``s - 1`` / ``1 - s``); Poisson ``l`` and ``l'`` use the operands of
their subtraction, ``2^-52 (|e^z| + |y z|)`` and ``2^-52 (|e^z| + |y|)``.

Bound in fp64 (``bound_units``): 4 units, or 4 x the host's own worst error on the table where that is above 1 unit.
The host is ``function/losses.py`` in torch fp64 on the CPU, measured here against the same reference
(``host_worst_units``); the GPU result is never looked at. The factor 4: the device terms chain three functions
(``exp``, ``log1p``, divide) that need not be correctly rounded, where glibc's nearly are.

In the f32 and bf16 precisions the per-row vectors (``coef``, ``dzz``) are fp32 (the bf16 precision narrows only the
matrix values), so a per-row term is rounded once more into fp32: ``stream_unit`` adds ``2^-24 |exact| + 2^-149``
(the unit roundoff and the smallest subnormal) to the fp64 bound; the GPU test asserts that type. Entries whose exact
term exceeds fp32's largest finite value (``STREAM_LEFT_OUT``: Poisson margins of 89 and above, ``e^89 = 4.5e38``)
are left out of those two precisions.
"""
import functools
from decimal import Decimal, localcontext

import numpy as np
import torch

PREC = 800
DBL_MAX = Decimal(float(np.finfo(np.float64).max))
TWO = Decimal(2)
EPS64, TINY64 = TWO ** -52, TWO ** -1074
STREAM = {"f32": (TWO ** -24, TWO ** -149)}

LOSSES = ("LOGISTIC", "POISSON", "SQUARED", "HINGE")
LOSS_IDS = {"LOGISTIC": 0, "POISSON": 1, "SQUARED": 2, "HINGE": 3}
TERMS = ("l", "dl", "d2")

MAGNITUDES = (0.0, 2.0 ** -60, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23,
              17.0, 36.5, 36.75, 37.5, 40.0,
              88.5, 89.0, 103.5, 104.5,
              700.0, 708.0, 709.75, 710.0, 745.0, 746.0, 1e4)
LABELS = {"LOGISTIC": (0.0, 1.0), "HINGE": (0.0, 1.0), "POISSON": (0.0, 3.0), "SQUARED": (0.25, -3.0)}
MAX_MAGNITUDE = {"POISSON": 746.0}
BANDS = (1.0, 40.0, 104.5, 709.75, float("inf"))      # |z| <= edge, each band above the one before
# f32 / bf16 row streams: Poisson terms e^z beyond the type's largest finite value (3.4e38)
STREAM_LEFT_OUT = {"POISSON": tuple(m for m in MAGNITUDES if 89.0 <= m <= 746.0)}


def loss_object(name):
    from photon_ml_amd.function import losses
    return {"LOGISTIC": losses.LOGISTIC, "POISSON": losses.POISSON, "SQUARED": losses.SQUARED,
            "HINGE": losses.SMOOTHED_HINGE}[name]


@functools.lru_cache(maxsize=None)
def table(loss, stream=False):
    """The (z, y) entries of a loss, band after band: every magnitude with both signs, every label. ``stream``:
    without the entries left out of the f32 / bf16 row streams."""
    out = []
    for m in MAGNITUDES:
        if m > MAX_MAGNITUDE.get(loss, float("inf")):
            continue
        for z in (m, -m):
            if stream and z in STREAM_LEFT_OUT.get(loss, ()):
                continue
            for y in LABELS[loss]:
                out.append((z, y))
    return tuple(out)


def band_of(z):
    return next(b for b, edge in enumerate(BANDS) if abs(z) <= edge)


def band_rows(loss, stream=False):
    """Per band, the entries of :func:`table` in it."""
    rows = [[] for _ in BANDS]
    for z, y in table(loss, stream):
        rows[band_of(z)].append((z, y))
    return rows


def _log1p_small(e):
    return e - e * e / 2 if e < Decimal("1e-390") else (1 + e).ln()


@functools.lru_cache(maxsize=None)
def exact(loss, z, y):
    """``(l, l', l'')`` of ``function/losses.py`` at float margin ``z`` and label ``y`` as Decimals."""
    with localcontext() as ctx:
        ctx.prec = PREC
        zd, yd = Decimal(z), Decimal(y)
        if loss == "LOGISTIC":
            e = (-abs(zd)).exp()
            lp = _log1p_small(e)
            p, q = e / (1 + e), 1 / (1 + e)          # the small and the large one of sigmoid(z), sigmoid(-z)
            s, s_m1 = (q, -p) if zd >= 0 else (p, -q)
            pos = y > 0.5
            zz = -zd if pos else zd
            return (max(zz, Decimal(0)) + lp, s_m1 if pos else s, p * q)
        if loss == "POISSON":
            e = zd.exp()
            return (e - yd * zd, e - yd, e)
        if loss == "SQUARED":
            d = zd - yd
            return (d * d / 2, d, Decimal(1))
        if loss == "HINGE":
            yy = Decimal(-1) if y < 0.5 else Decimal(1)
            t = yy * zd
            l = Decimal("0.5") - t if t <= 0 else ((1 - t) * (1 - t) / 2 if t < 1 else Decimal(0))
            d = Decimal(-1) if t < 0 else (t - 1 if t < 1 else Decimal(0))
            return (l, d * yy, Decimal(0))
        raise ValueError(loss)


def unit(loss, term, z, y):
    """The rounding unit of a term (module docstring), a Decimal."""
    with localcontext() as ctx:
        ctx.prec = PREC
        ex = exact(loss, z, y)[TERMS.index(term)]
        if loss == "POISSON" and term in ("l", "dl"):
            e = exact(loss, z, y)[2]
            other = abs(Decimal(y) * Decimal(z)) if term == "l" else abs(Decimal(y))
            return EPS64 * (abs(e) + other) + TINY64
        u = EPS64 * abs(ex) + TINY64
        if loss == "LOGISTIC" and term in ("dl", "d2"):
            u += EPS64
        return u


def stream_unit(precision, ex):
    """What one rounding into the row stream's type adds to the bound of a per-row term of exact value ``ex``."""
    if precision == "f64":
        return Decimal(0)
    eps, tiny = STREAM[precision]
    with localcontext() as ctx:
        ctx.prec = PREC
        return eps * abs(ex) + tiny


def overflows(ex):
    """The exact value exceeds the largest double: the result must be an infinity of its sign."""
    return abs(ex) > DBL_MAX


def error_units(got, ex, u):
    """|got - exact| in units ``u`` (``got`` a float; an exact value beyond the largest double demands the infinity
    of its sign: 0 units if met, inf otherwise; NaN is always inf units)."""
    got = float(got)
    if got != got:
        return float("inf")
    if overflows(ex):
        return 0.0 if got == (float("inf") if ex > 0 else float("-inf")) else float("inf")
    if got in (float("inf"), float("-inf")):
        return float("inf")
    with localcontext() as ctx:
        ctx.prec = PREC
        return float(abs(Decimal(got) - ex) / u)


def host_terms(loss, zs, ys):
    """``function/losses.py`` in torch fp64 on the CPU: (l, dl, d2) arrays (hinge: d2 = 0)."""
    lo = loss_object(loss)
    z = torch.tensor(zs, dtype=torch.float64)
    y = torch.tensor(ys, dtype=torch.float64)
    l, dl = lo.loss_and_dz(z, y)
    d2 = lo.dzz(z, y) if lo.twice_differentiable else torch.zeros_like(z)
    return l.numpy(), dl.numpy(), d2.numpy()


@functools.lru_cache(maxsize=None)
def host_worst_units(loss):
    """Worst error of the host's fp64 terms over the table, in units, per term: ``{term: units}``."""
    rows = table(loss)
    got = host_terms(loss, [z for z, _ in rows], [y for _, y in rows])
    return {t: max(error_units(got[k][i], exact(loss, z, y)[k], unit(loss, t, z, y)) for i, (z, y) in enumerate(rows))
            for k, t in enumerate(TERMS)}


def bound_units(loss, term):
    """The fp64 bound of a term in units: 4, or 4 x the host's own worst error where that is above 1 unit."""
    return 4.0 * max(1.0, host_worst_units(loss)[term])


def weighted_sum(loss, term, rows, weights, factor=None):
    """Exact ``sum_i w_i term_i [factor_i]`` over ``rows`` ((z, y) entries) and the sum of the rows' units, scaled
    alike: ``(Decimal sum, Decimal units)``. Rows of weight 0 add nothing. Weights and factors are floats. A term
    that itself exceeds the largest double enters as the infinity of its sign whatever its weight (C2: the term is
    +inf before the weight scales it), so the sum is that infinity."""
    with localcontext() as ctx:
        ctx.prec = PREC
        k = TERMS.index(term)
        tot, units = Decimal(0), Decimal(0)
        for i, ((z, y), w) in enumerate(zip(rows, weights)):
            if w == 0.0:
                continue
            c = Decimal(float(w)) * (Decimal(1) if factor is None else Decimal(float(factor[i])))
            ex = exact(loss, z, y)[k]
            if overflows(ex):
                ex = Decimal("Infinity") if ex > 0 else Decimal("-Infinity")
            tot += c * ex
            units += abs(c) * unit(loss, term, z, y)
        return tot, units + TINY64
