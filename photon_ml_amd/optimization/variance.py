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
tests and the GPU path of the entities the HIP kernels do not take (``m = min(n_e, d_e) > 1024``, or ``> 128`` with the
blocked route off; a row-space entity wider than the kernels' LDS images; a failed factor), batched by size bucket in
chunks sized by a memory budget.

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


# Blocked route (VAR_MMAX < m <= VAR_BLOCKED_MMAX): upper bounds of the size classes. The work per entity grows like
# n^3 and every member of a class is padded to the class's largest member, so neighbouring bounds differ by at most a
# third (at most 2.4x the work of the smallest member); multiples of 32 keep the 16-wide panels and MFMA tiles full.
BLOCKED_SIZE_CLASSES = (160, 192, 256, 320, 384, 512, 640, 768, 896, 1024)

# Workspace of the blocked route per chunk of a class: one fp64 [n, n] slab per entity (8 MiB at order 1024). 4 GiB
# hold 512 slabs of order 1024, two work-groups for each of the 256 compute units of an MI355X.
DEFAULT_BLOCKED_WORKSPACE_BYTES = 4 << 30


def blocked_class_bounds(blocked_mmax: int, mmax: int = 128) -> Tuple[int, ...]:
    """Increasing upper bounds of the blocked size classes for factor orders in ``(mmax, blocked_mmax]``; empty when
    the route is off (``blocked_mmax <= mmax``). The last bound is ``blocked_mmax`` itself."""
    blocked_mmax = int(blocked_mmax)
    if blocked_mmax <= mmax:
        return ()
    bounds = [b for b in BLOCKED_SIZE_CLASSES if mmax < b <= blocked_mmax]
    if not bounds or bounds[-1] < blocked_mmax:
        bounds.append(blocked_mmax)
    return tuple(bounds)


def blocked_class_of(m: torch.Tensor, bounds) -> torch.Tensor:
    """Index of the first class of ``bounds`` that holds each factor order of ``m`` (``len(bounds)`` when none does)."""
    return torch.searchsorted(torch.tensor(list(bounds), dtype=m.dtype, device=m.device), m)


def blocked_route_masks(n_e: torch.Tensor, d_e: torch.Tensor, canonical: bool, mmax: int, blocked_mmax: int,
                        dmax: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Which entities take the blocked primal and the blocked row-space route: live (rows and coefficients), a
    canonical CSR, ``mmax < min(n_e, d_e) <= blocked_mmax``; primal when ``d_e <= n_e``, else row space, and there only
    with ``d_e <= dmax`` (the LDS images of the row-space kernels hold one fp64 per coefficient). Pure tensor
    arithmetic on any device."""
    m = torch.minimum(n_e, d_e)
    ok = (n_e > 0) & (d_e > 0) & (m > mmax) & (m <= blocked_mmax)
    if not canonical or blocked_mmax <= mmax:
        ok = torch.zeros_like(ok)
    return ok & (d_e <= n_e), ok & (n_e < d_e) & (d_e <= dmax)


# A blocked launch runs one work-group per entity and a work-group fills a compute unit, so a class with at most this
# many members (the compute units of an MI355X) lasts as long as its largest member whatever the others' orders are:
# neighbouring classes are merged while they stay within it (one launch sequence instead of several short-handed ones).
BLOCKED_MERGE_ENTITIES = 256


def blocked_merge_classes(counts, limit: int = BLOCKED_MERGE_ENTITIES):
    """Groups of neighbouring size classes that share one launch sequence: from the largest class down, a class joins
    the group above it while the group then holds at most ``limit`` entities. ``counts``: entities per class in
    increasing class order. Returns the groups as lists of class indices, in increasing order; classes without
    entities belong to no group."""
    groups, cur, total = [], [], 0
    for k in range(len(counts) - 1, -1, -1):
        if counts[k] == 0:
            continue
        if cur and total + counts[k] > limit:
            groups.append(cur[::-1])
            cur, total = [], 0
        cur.append(k)
        total += counts[k]
    if cur:
        groups.append(cur[::-1])
    return groups[::-1]


def blocked_chunk_entities(n: int, workspace_bytes: int) -> int:
    """Entities per launch of a blocked class of order ``n`` under the workspace budget (at least one)."""
    return max(1, int(workspace_bytes) // (8 * int(n) * int(n)))


class SegmentedFullVariance:
    """FULL variances of a segmented random-effect coordinate on the GPU: the routing of its entities, built once
    per dataset (it depends on the data only), and :meth:`compute` per update.

    With ``m = min(n_e, d_e)``: entities with ``m <= VAR_MMAX`` take the HIP kernels, one launch sequence per size
    class (bounds from ``row_space.SIZE_CLASSES``, a class padded to its largest member as ``RowSpaceBatch`` does) —
    the primal route (``var_normal`` -> ``batched_cholesky`` -> ``chol_colnorm``) when ``d_e <= n_e``, else the
    row-space route (``seg_gram`` -> ``var_scale_gram`` -> ``batched_cholesky`` -> ``chol_colnorm``). The rest (larger
    ``m``, an entity too wide for ``seg_gram``'s LDS image, a failed factor, the shapes measured slower on the HIP path)
    goes to :func:`segmented_full_variance`. Entities without rows get ``1 / l2``. The HIP routes need the canonical
    CSR (strictly increasing columns inside a row); without it every entity takes the torch path.

    ``blocked_mmax`` (0: off; at most ``VAR_BLOCKED_MMAX``) turns on the blocked route for ``VAR_MMAX < m <=
    blocked_mmax``: the same two routes with the matrices in a global workspace and one work-group per entity
    (``var_blocked_assemble`` -> ``blocked_cholesky`` -> ``var_blocked_colnorm``), per size class of
    ``BLOCKED_SIZE_CLASSES`` (neighbouring classes of few members share a launch sequence:
    :func:`blocked_merge_classes`) and in chunks of ``blocked_workspace_bytes`` (one fp64 ``[n, n]`` slab per entity).
    Row-space entities need ``d_e <= VAR_BLOCKED_DMAX`` (2048); wider ones stay on the torch path. The counts then
    carry ``blocked_primal`` and ``blocked_row_space``."""

    # Measured slower on the HIP path than in the batched torch fallback (profiles/full_variance_device.md): the
    # row-space class of 97 .. 112 rows when the entity is narrow too (d_e ~ n_e: 3.6 vs 3.0 us per entity at
    # d_e = 101, where the fallback's d_e x d_e Hessians are tiny). Row-space entities with more than
    # ROW_SPACE_TORCH_ROWS rows and at most ROW_SPACE_TORCH_COLS coefficients go to the fallback; with wide entities
    # (d_e = 1001) the same class is 30x faster on the HIP path and stays there.
    ROW_SPACE_TORCH_ROWS = 96
    ROW_SPACE_TORCH_COLS = 128

    def __init__(self, row_ptr: torch.Tensor, col_ptr: torch.Tensor, csr, mmax: Optional[int] = None,
                 blocked_mmax: int = 0, blocked_workspace_bytes: int = DEFAULT_BLOCKED_WORKSPACE_BYTES):
        from ..ops.native import (SEG_GRAM_DMAX, VAR_BLOCKED_DMAX, VAR_BLOCKED_MMAX, VAR_MMAX, VAR_PRIMAL,
                                  VAR_ROW_SPACE, check_var_blocked_class, check_var_class, var_blocked_dcap)
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
        # blocked route: (route, n, ents, nv, dcap) per size class
        self.blocked_classes = []
        self.blocked_workspace_bytes = int(blocked_workspace_bytes)
        blocked_mmax = min(int(blocked_mmax), VAR_BLOCKED_MMAX)
        self.blocked = blocked_mmax > VAR_MMAX
        bprimal, brsp = blocked_route_masks(n_e, d_e, canon is not None, VAR_MMAX, blocked_mmax, VAR_BLOCKED_DMAX)
        bbounds = blocked_class_bounds(blocked_mmax, VAR_MMAX)
        for route, mask in ((VAR_PRIMAL, bprimal), (VAR_ROW_SPACE, brsp)):
            ents = torch.nonzero(mask).squeeze(1)
            if ents.numel() == 0:
                continue
            me = m[ents]
            cls_of = blocked_class_of(me, bbounds)
            order = torch.argsort(cls_of, stable=True)
            ents, me, cls_of = ents[order], me[order], cls_of[order]
            lo = 0
            counts = torch.bincount(cls_of, minlength=len(bbounds)).tolist()
            for group in blocked_merge_classes(counts):
                cnt = sum(counts[k] for k in group)
                e, nv = ents[lo:lo + cnt].contiguous(), me[lo:lo + cnt].contiguous()
                lo += cnt
                n, dmax = (int(v) for v in torch.stack([nv.max(), d_e[e].max()]).tolist())
                dcap = var_blocked_dcap(dmax) if route == VAR_ROW_SPACE else None
                check_var_blocked_class(route, n, e, self.row_ptr, self.col_ptr, nv, self.csr, dcap=dcap)
                self.blocked_classes.append((route, n, e, nv, dcap))
        self.rest = torch.nonzero(live & ~(primal | rsp | bprimal | brsp)).squeeze(1)
        self.counts = {"primal": int(primal.sum()), "row_space": int(rsp.sum()),
                       "torch": int(self.rest.numel()), "empty": int(((d_e > 0) & (n_e == 0)).sum())}
        if self.blocked:
            self.counts["blocked_primal"] = int(bprimal.sum())
            self.counts["blocked_row_space"] = int(brsp.sum())

    def compute(self, c: torch.Tensor, l2: float, timings: Optional[list] = None,
                workspace_bytes: Optional[int] = None) -> Tuple[torch.Tensor, dict]:
        """Variances packed like ``col_ptr`` for the row curvature ``c`` (fp64 per row) and ``l2 > 0``; and the
        number of entities per route (``torch`` includes the entities whose factor failed). ``timings``: a list that
        receives ``(route, n, entities, start event, end event)`` per class, the blocked classes (``n > VAR_MMAX``)
        after the others (benchmarks only). ``workspace_bytes``: the blocked route's workspace budget for this call
        (default: the plan's ``blocked_workspace_bytes``); the chunking does not change any result."""
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
        if self.blocked_classes:
            from ..ops.native import blocked_cholesky, var_blocked_assemble, var_blocked_colnorm
            budget = self.blocked_workspace_bytes if workspace_bytes is None else int(workspace_bytes)
            steps = [min(int(e.numel()), blocked_chunk_entities(n, budget)) for _, n, e, _, _ in self.blocked_classes]
            work = torch.empty(max(s * n * n for s, (_, n, *_) in zip(steps, self.blocked_classes)),
                               dtype=torch.float64, device=dev)
            for step, (route, n, e, nv, dcap) in zip(steps, self.blocked_classes):
                if timings is not None:
                    ev0 = torch.cuda.Event(enable_timing=True)
                    ev0.record()
                rs = route == VAR_ROW_SPACE
                for a in range(0, int(e.numel()), step):
                    ec, nvc = e[a:a + step], nv[a:a + step]
                    A = var_blocked_assemble(route, ec, n, rp, cp, self.csr, c, l2, work, dcap, validated=True)
                    L, info = blocked_cholesky(A, nvc)
                    var_blocked_colnorm(route, L, nvc, ec, rp, cp, out, l2, self.csr if rs else None,
                                        c if rs else None, dcap, validated=True)
                    failed.append((ec, info))
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
