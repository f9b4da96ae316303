"""FULL coefficient variances: the diagonal of the inverse Hessian.

For a GLM with margins ``z = X w + o``, row curvature ``c_i = weight_i * l''(z_i, y_i) >= 0`` and L2 weight ``lam``
the Hessian is ``H = X^T diag(c) X + lam I`` and the FULL variance of coefficient j is ``(H^-1)_jj`` (the posterior
variance under the Laplace approximation; later Photon ML releases call it ``VarianceComputationType.FULL``). The
SIMPLE variance ``1 / (H_jj + EPSILON)`` ignores every correlation between features and is never larger.

This module is the DEFINITION in plain fp64 torch, on any device:

* :func:`segmented_full_variance` walks the entities of a block-diagonal CSR (``SegmentedGLMData`` + its kept CSR),
* :func:`dense_full_variance` the problems of a dense ``BatchedGLMData`` bucket,
* :func:`hessian_full_variance` one dense Hessian (the fixed effect).

Each forms ``H_e`` densely and returns ``diag(H_e^-1)``: Cholesky first, and where ``cholesky_ex`` reports a bad pivot
``torch.linalg.pinv`` (the later reference's definition). It is the CPU path of the feature, the yardstick of the GPU
tests and the GPU path of the entities the HIP kernels do not take (``m = min(n_e, d_e) > 128``, a failed factor),
batched by size bucket in chunks sized by a memory budget.

:func:`row_space_full_variance` is the Woodbury form the HIP row-space route implements, written once in torch as a
second yardstick: with ``B = diag(sqrt c) X_e`` and ``lam I + B B^T = G G^T``, ``var_j = (1 - |G^-1 b_j|^2) / lam``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

DEFAULT_BUDGET_BYTES = 256 << 20


def _inv_diag(H: torch.Tensor) -> torch.Tensor:
    """``diag(H^-1)`` of the SPD batch ``H [B, d, d]`` (fp64): squared column norms of ``G^-1`` for ``H = G G^T``;
    problems whose factorisation fails use the pseudo-inverse."""
    B, d, _ = H.shape
    if B == 0 or d == 0:
        return H.new_zeros(B, d)
    G, info = torch.linalg.cholesky_ex(H)
    eye = torch.eye(d, dtype=H.dtype, device=H.device).expand(B, d, d)
    Y = torch.linalg.solve_triangular(G, eye, upper=False)
    var = (Y * Y).sum(1)
    bad = info != 0
    if bool(bad.any()):
        var[bad] = torch.diagonal(torch.linalg.pinv(H[bad], hermitian=True), dim1=1, dim2=2)
    return var


def hessian_full_variance(H: torch.Tensor) -> torch.Tensor:
    """``diag(H^-1)`` of one dense Hessian ``H [d, d]``."""
    return _inv_diag(H.to(torch.float64).unsqueeze(0))[0]


def dense_full_variance(X: torch.Tensor, c: torch.Tensor, l2: float,
                        budget_bytes: int = DEFAULT_BUDGET_BYTES) -> torch.Tensor:
    """FULL variances ``[B, d]`` of a dense padded batch ``X [B, n, d]`` with row curvature ``c [B, n]`` (0 on
    padding rows): ``diag((X_b^T diag(c_b) X_b + l2 I)^-1)`` per problem, in chunks of the batch."""
    B, n, d = X.shape
    out = torch.empty(B, d, dtype=torch.float64, device=X.device)
    per = 8 * (2 * n * d + 4 * d * d) + 1
    step = max(1, int(budget_bytes // per))
    eye = torch.eye(d, dtype=torch.float64, device=X.device)
    for a in range(0, B, step):
        Xc = X[a:a + step].to(torch.float64)
        H = torch.bmm(Xc.transpose(1, 2) * c[a:a + step].to(torch.float64).unsqueeze(1), Xc) + l2 * eye
        out[a:a + step] = _inv_diag(H)
    return out


def _entity_dense(nip, pos, val, rows0, ne, cb, n: int, d: int) -> torch.Tensor:
    """Dense ``X [B, n, d]`` (zero padded) of entities given by their first row ``rows0``, row count ``ne`` and
    coefficient base ``cb`` in the block-diagonal CSR."""
    dev = val.device
    B = int(rows0.numel())
    X = torch.zeros(B, n, d, dtype=torch.float64, device=dev)
    tot = int(ne.sum())
    if tot == 0:
        return X
    bidx = torch.repeat_interleave(torch.arange(B, device=dev), ne, output_size=tot)
    start = torch.cumsum(ne, 0) - ne
    slot = torch.arange(tot, device=dev) - start[bidx]
    rows = rows0[bidx] + slot
    k0 = nip[rows]
    nk = nip[rows + 1] - k0
    nnz = int(nk.sum())
    if nnz == 0:
        return X
    ridx = torch.repeat_interleave(torch.arange(tot, device=dev), nk, output_size=nnz)
    kk = torch.arange(nnz, device=dev) - (torch.cumsum(nk, 0) - nk)[ridx] + k0[ridx]
    b = bidx[ridx]
    X[b, slot[ridx], pos[kk] - cb[b]] = val[kk].to(torch.float64)
    return X


def _pow2(x: torch.Tensor) -> torch.Tensor:
    """Smallest power of two >= x (x >= 1), elementwise on int64."""
    return torch.pow(2, torch.ceil(torch.log2(x.clamp(min=1).to(torch.float64)))).to(torch.int64)


def segmented_full_variance(row_ptr: torch.Tensor, col_ptr: torch.Tensor, csr, c: torch.Tensor, l2: float,
                            ents: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                            budget_bytes: int = DEFAULT_BUDGET_BYTES) -> Tuple[torch.Tensor, int]:
    """FULL variances of the entities of a block-diagonal problem, packed like ``col_ptr``.

    ``row_ptr`` / ``col_ptr``: each entity's rows and coefficient range; ``csr = (indptr, columns, values)`` over the
    rows with GLOBAL (packed) columns; ``c``: curvature per row; ``ents``: the entities to compute (default: all).
    Writes ``diag(H_e^-1)``, ``H_e = X_e^T diag(c) X_e + l2 I``, into ``out[col_ptr[e]:col_ptr[e + 1]]`` (a new vector
    when ``out`` is None; the other entities' entries are left as they are, 0 in a new vector). Entities are batched
    by size bucket (rows and coefficients rounded up to powers of two) in chunks of ``budget_bytes``. Returns
    ``(out, number of entities handled)``."""
    dev = c.device
    nip, pos, val = (t.to(dev) for t in csr)
    row_ptr, col_ptr = row_ptr.to(dev), col_ptr.to(dev)
    if out is None:
        out = torch.zeros(int(col_ptr[-1]), dtype=torch.float64, device=dev)
    if ents is None:
        ents = torch.arange(row_ptr.numel() - 1, device=dev)
    ents = ents.to(dev)
    d_e = col_ptr[ents + 1] - col_ptr[ents]
    ents = ents[d_e > 0]
    if ents.numel() == 0:
        return out, 0
    n_e = row_ptr[ents + 1] - row_ptr[ents]
    d_e = col_ptr[ents + 1] - col_ptr[ents]
    key = _pow2(n_e) * (1 << 32) + _pow2(d_e)
    order = torch.argsort(key, stable=True)
    ents, n_e, d_e, key = ents[order], n_e[order], d_e[order], key[order]
    ukeys, counts = torch.unique_consecutive(key, return_counts=True)
    lo = 0
    for cnt in counts.tolist():
        e, ne, de = ents[lo:lo + cnt], n_e[lo:lo + cnt], d_e[lo:lo + cnt]
        lo += cnt
        n, d = max(int(ne.max()), 1), int(de.max())
        per = 8 * (2 * n * d + 4 * d * d) + 1
        step = max(1, int(budget_bytes // per))
        ar = torch.arange(d, device=dev)
        for a in range(0, cnt, step):
            ec, nec, dec = e[a:a + step], ne[a:a + step], de[a:a + step]
            r0, cb = row_ptr[ec], col_ptr[ec]
            X = _entity_dense(nip, pos, val, r0, nec, cb, n, d)
            slot = torch.arange(n, device=dev).unsqueeze(0)
            zero = torch.zeros((), dtype=torch.float64, device=dev)
            if c.numel():
                cc = torch.where(slot < nec.unsqueeze(1),
                                 c[(r0.unsqueeze(1) + slot).clamp(max=c.numel() - 1)].to(torch.float64), zero)
            else:
                cc = zero.expand(ec.numel(), n)
            H = torch.bmm(X.transpose(1, 2) * cc.unsqueeze(1), X)
            # padding coefficients (beyond d_e) get a unit diagonal: they do not couple with the entity's own
            keep = ar.unsqueeze(0) < dec.unsqueeze(1)
            H = H + torch.diag_embed(torch.where(keep, torch.full((), float(l2), dtype=torch.float64, device=dev),
                                                 torch.ones((), dtype=torch.float64, device=dev)))
            var = _inv_diag(H)
            out[(cb.unsqueeze(1) + ar.unsqueeze(0))[keep]] = var[keep]
    return out, int(ents.numel())


class SegmentedFullVariance:
    """FULL variances of a segmented random-effect coordinate on the GPU: the routing of its entities, built once
    per dataset (it depends on the data only), and :meth:`compute` per update.

    With ``m = min(n_e, d_e)``: entities with ``m <= VAR_MMAX`` take the HIP kernels, one launch sequence per size
    class (bounds from ``row_space.SIZE_CLASSES``, a class padded to its largest member as ``RowSpaceBatch`` does) —
    the primal route (``var_normal`` -> ``batched_cholesky`` -> ``chol_colnorm``) when ``d_e <= n_e``, else the
    row-space route (``seg_gram`` -> ``var_scale_gram`` -> ``batched_cholesky`` -> ``chol_colnorm``). The rest (larger
    ``m``, an entity too wide for ``seg_gram``'s LDS image, a failed factor, the shapes measured slower on the HIP path)
    goes to :func:`segmented_full_variance`. Entities without rows get ``1 / l2``. The HIP routes need the canonical
    CSR (strictly increasing columns inside a row); without it every entity takes the torch path."""

    # Measured slower on the HIP path than in the batched torch fallback (profiles/full_variance_device.md): the
    # row-space class of 97 .. 112 rows when the entity is narrow too (d_e ~ n_e: 3.6 vs 3.0 us per entity at
    # d_e = 101, where the fallback's d_e x d_e Hessians are tiny). Row-space entities with more than
    # ROW_SPACE_TORCH_ROWS rows and at most ROW_SPACE_TORCH_COLS coefficients go to the fallback; with wide entities
    # (d_e = 1001) the same class is 30x faster on the HIP path and stays there.
    ROW_SPACE_TORCH_ROWS = 96
    ROW_SPACE_TORCH_COLS = 128

    def __init__(self, row_ptr: torch.Tensor, col_ptr: torch.Tensor, csr, mmax: Optional[int] = None):
        from ..ops.native import SEG_GRAM_DMAX, VAR_MMAX, VAR_PRIMAL, VAR_ROW_SPACE, check_var_class
        from .row_space import SIZE_CLASSES, _canonical_csr
        dev = row_ptr.device
        self.row_ptr, self.col_ptr = row_ptr.contiguous(), col_ptr.contiguous()
        mmax = VAR_MMAX if mmax is None else min(int(mmax), VAR_MMAX)
        self.d_total = int(col_ptr[-1])
        n_e = row_ptr[1:] - row_ptr[:-1]
        d_e = col_ptr[1:] - col_ptr[:-1]
        m = torch.minimum(n_e, d_e)
        canon = _canonical_csr(csr, dev) if dev.type == "cuda" else None
        self.csr = tuple(t.contiguous() for t in canon) if canon is not None else tuple(t.to(dev) for t in csr)
        live = (d_e > 0) & (n_e > 0)
        hip = live & (m <= mmax) if canon is not None else torch.zeros_like(live)
        primal = hip & (d_e <= n_e)
        rsp = hip & (n_e < d_e) & (d_e <= SEG_GRAM_DMAX)
        rsp &= ~((n_e > self.ROW_SPACE_TORCH_ROWS) & (d_e <= self.ROW_SPACE_TORCH_COLS))
        self.classes = []                     # (route, n, ents, nv, dmax, maxnnz)
        bounds = torch.tensor([b for b in SIZE_CLASSES if b <= mmax], device=dev)
        for route, mask in ((VAR_PRIMAL, primal), (VAR_ROW_SPACE, rsp)):
            ents = torch.nonzero(mask).squeeze(1)
            if ents.numel() == 0:
                continue
            me = m[ents]
            cls_of = torch.searchsorted(bounds, me)
            order = torch.argsort(cls_of, stable=True)
            ents, me, cls_of = ents[order], me[order], cls_of[order]
            counts = torch.bincount(cls_of, minlength=bounds.numel()).tolist()
            lo = 0
            for cnt in counts:
                if cnt == 0:
                    continue
                e, nv = ents[lo:lo + cnt].contiguous(), me[lo:lo + cnt].contiguous()
                lo += cnt
                nip = self.csr[0]
                st = torch.stack([nv.max(), d_e[e].max(), (nip[row_ptr[e + 1]] - nip[row_ptr[e]]).max()]).tolist()
                n = int(st[0])
                check_var_class(route, n, e, self.row_ptr, self.col_ptr, nv, self.csr)
                self.classes.append((route, n, e, nv, int(st[1]), int(st[2])))
        self.rest = torch.nonzero(live & ~(primal | rsp)).squeeze(1)
        self.counts = {"primal": int(primal.sum()), "row_space": int(rsp.sum()),
                       "torch": int(self.rest.numel()), "empty": int(((d_e > 0) & (n_e == 0)).sum())}

    def compute(self, c: torch.Tensor, l2: float, timings: Optional[list] = None) -> Tuple[torch.Tensor, dict]:
        """Variances packed like ``col_ptr`` for the row curvature ``c`` (fp64 per row) and ``l2 > 0``; and the
        number of entities per route (``torch`` includes the entities whose factor failed). ``timings``: a list that
        receives ``(route, n, entities, start event, end event)`` per class (benchmarks only)."""
        from ..ops.native import (VAR_PRIMAL, VAR_ROW_SPACE, batched_cholesky, chol_colnorm, seg_gram, var_normal,
                                  var_scale_gram)
        if not l2 > 0:
            raise ValueError("FULL variances of a random-effect coordinate need an L2 weight > 0")
        dev = self.row_ptr.device
        c = c.to(dev, torch.float64).contiguous()
        if c.numel() < int(self.row_ptr[-1]):
            raise ValueError("FULL variance: the row curvature is shorter than the rows")
        out = torch.full((self.d_total,), 1.0 / l2, dtype=torch.float64, device=dev)
        rp, cp = self.row_ptr, self.col_ptr
        failed = []
        for route, n, e, nv, dmax, maxnnz in self.classes:
            if timings is not None:
                ev0 = torch.cuda.Event(enable_timing=True)
                ev0.record()
            if route == VAR_PRIMAL:
                A = var_normal(e, n, rp, cp, self.csr, c, l2, validated=True)
            else:
                A = seg_gram(e, n, rp, cp, *self.csr, dmax=dmax, maxnnz=maxnnz)
                var_scale_gram(A, e, rp, c, l2, validated=True)
            L, info = batched_cholesky(A, nv)
            chol_colnorm(route, L, nv, e, rp, cp, out, l2, self.csr if route == VAR_ROW_SPACE else None,
                         c if route == VAR_ROW_SPACE else None, validated=True)
            failed.append((e, info))
            if timings is not None:
                ev1 = torch.cuda.Event(enable_timing=True)
                ev1.record()
                timings.append((route, n, int(e.numel()), ev0, ev1))
        rest = self.rest
        if failed:
            any_bad = torch.stack([(i != 0).any() for _, i in failed]).tolist()      # one readback for all classes
            bad = [e[i != 0] for (e, i), b in zip(failed, any_bad) if b]
            if bad:
                rest = torch.cat([rest] + bad)
        n_torch = 0
        if rest.numel():
            _, n_torch = segmented_full_variance(rp, cp, self.csr, c, l2, ents=rest, out=out)
        stats = dict(self.counts)
        stats["torch"] = n_torch
        stats["failed_factors"] = int(rest.numel() - self.rest.numel())
        return out, stats


def dense_full_variance_device(X: torch.Tensor, c: torch.Tensor, l2: float) -> Tuple[torch.Tensor, int]:
    """FULL variances ``[B, d]`` of a dense bucket on the GPU: ``A = X^T diag(c) X + l2 I`` by ``torch.bmm``, then
    ``batched_cholesky`` and ``chol_colnorm`` with identity right-hand sides for ``d <= VAR_MMAX``; wider buckets and
    failed factors use :func:`dense_full_variance`. Returns the variances and the number of problems the torch path
    handled."""
    from ..ops.native import VAR_MMAX, VAR_PRIMAL, batched_cholesky, chol_colnorm
    B, n, d = X.shape
    if not X.is_cuda or d > VAR_MMAX or B == 0 or d == 0:
        return dense_full_variance(X, c, l2), B
    X = X.to(torch.float64)
    A = torch.bmm(X.transpose(1, 2) * c.to(torch.float64).unsqueeze(1), X)
    A = (A + l2 * torch.eye(d, dtype=torch.float64, device=X.device)).contiguous()
    nv = torch.full((B,), d, dtype=torch.int64, device=X.device)
    L, info = batched_cholesky(A, nv)
    ptr = torch.arange(B + 1, dtype=torch.int64, device=X.device) * d
    out = torch.empty(B * d, dtype=torch.float64, device=X.device)
    chol_colnorm(VAR_PRIMAL, L, nv, torch.arange(B, dtype=torch.int64, device=X.device), ptr, ptr, out)
    out = out.view(B, d)
    bad = info != 0
    n_bad = int(bad.sum())
    if n_bad:
        out[bad] = dense_full_variance(X[bad], c[bad], l2)
    return out, n_bad


def row_space_full_variance(X: torch.Tensor, c: torch.Tensor, l2: float) -> torch.Tensor:
    """The Woodbury (row-space) form of the FULL variance of ONE entity ``X [n, d]`` with curvature ``c [n]`` and
    ``l2 > 0``: ``B = diag(sqrt c) X``, ``l2 I + B B^T = G G^T``, ``var_j = (1 - |G^-1 b_j|^2) / l2``. Holds no
    ``1 / c_i``, so rows with ``c_i = 0`` are fine. Equals :func:`dense_full_variance` up to rounding; this is what the
    HIP row-space route computes for ``n < d``."""
    if not l2 > 0:
        raise ValueError("the row-space form needs l2 > 0")
    X = X.to(torch.float64)
    Bm = torch.sqrt(c.to(torch.float64)).unsqueeze(1) * X
    A = Bm @ Bm.T + l2 * torch.eye(X.shape[0], dtype=torch.float64, device=X.device)
    G = torch.linalg.cholesky(A)
    Y = torch.linalg.solve_triangular(G, Bm, upper=False)
    return (1.0 - (Y * Y).sum(0)) / l2
