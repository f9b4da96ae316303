"""Fused per-entity L-BFGS / OWL-QN for random-effect entities under L1 or elastic-net regularization.

The reference picks OWL-QN for LBFGS + {L1, ELASTIC_NET} on every coordinate
(``photon-lib/.../optimization/OptimizerFactory.scala:38-80``, ``RegularizationContext.scala:38-147``) and runs it
once per entity (``photon-api/.../optimization/SingleNodeOptimizationProblem.scala:85-103``). L1 has no row-space
form (``row_space.row_space_eligible``) and no TRON, so before this solver such a coordinate ran
``batched.batched_lbfgs`` over the whole block-diagonal problem: ~40 grid-wide launches per iteration, one host
synchronisation per line-search trial, every entity waiting for the slowest. Here ONE persistent launch per LDS
size class (``re_lbfgs_csr_kernel``, ``ops/csrc/re_kernels.hip``) runs every entity's complete OWL-QN in a
workgroup: coefficient vectors in LDS, each function evaluation one read of the entity's CSR rows, the (S, Y)
history in a global workspace per resident workgroup. The kernel is a transcription of ``batched_lbfgs``: same
two-loop, pseudo-gradient, orthant projection, line search and convergence rules.

Entities wider than ``FUSED_DMAX`` or longer than ``FUSED_MAX_ROWS`` stay on the block-diagonal pass path
(``batched.batched_lbfgs`` over ``RandomEffectDataset.entity_subset``).
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from .entity_tron import _CLASSES, FUSED_DMAX, FUSED_MAX_ROWS, FusedResult, fused_enabled

LBFGS_LOSSES = (0, 1, 2, 3)          # logistic, Poisson, squared, smoothed hinge (first-order solver)


def fused_lbfgs_eligible(loss, optimizer: str, l1: float, constraints, device, shift: bool = False) -> bool:
    """The fused OWL-QN applies to L-BFGS with an L1 weight (L1 / elastic net) on the GPU, without constraints and
    without a normalization shift in the data (``SegmentedGLMData.shift``: the pass path takes those)."""
    return (fused_enabled() and optimizer == "LBFGS" and l1 > 0 and not constraints and not shift
            and torch.device(device).type == "cuda" and getattr(loss, "loss_id", -1) in LBFGS_LOSSES)


class EntityLbfgsBatch:
    """The entities of a segmented random-effect coordinate that the fused L-BFGS / OWL-QN kernel solves.

    ``mask`` [E] bool: candidate entities. Entities with data and ``d_e <= FUSED_DMAX``, ``n_e <=
    FUSED_MAX_ROWS``, fewer than 2^31 non-zeros are taken (``self.mask``); ``ents`` / ``rows`` / ``cols`` are their
    parent entity indices, parent row positions and parent coefficient positions (as ``EntityTronBatch``)."""

    kind = "lbfgs"
    # read by RandomEffectCoordinate.solver_routing (no TRON-only variants here)
    n_heavy = 0
    quad = False
    res = None

    def __init__(self, ds, mask: torch.Tensor):
        from ..ops.native import RE_LBFGS_M, csr_gather_rows, re_lbfgs_grid
        seg = ds.seg
        dev = seg.y.device
        if dev.type != "cuda":
            raise RuntimeError("EntityLbfgsBatch runs on the GPU only (the CPU path is batched_lbfgs)")
        if getattr(ds, "_seg_csr", None) is None:
            raise RuntimeError("EntityLbfgsBatch needs the segmented CSR of the dataset")
        n_e = seg.row_ptr[1:] - seg.row_ptr[:-1]
        d_e = seg.col_ptr[1:] - seg.col_ptr[:-1]
        pnip, ppos, pval = (t.to(dev) for t in ds._seg_csr)
        # the kernel addresses an entity's entries with 32-bit offsets from its first entry
        e_nnz = pnip[seg.row_ptr[1:]] - pnip[seg.row_ptr[:-1]]
        sel = (mask.to(dev) & (n_e > 0) & (d_e > 0) & (d_e <= FUSED_DMAX) & (n_e <= FUSED_MAX_ROWS)
               & (e_nnz < (1 << 31)))
        self.mask = sel
        self.ents = torch.nonzero(sel).squeeze(1)
        self.B = int(self.ents.numel())
        self.W: Optional[torch.Tensor] = None          # last solution (warm start of the next solve)
        self.launches = []
        if self.B == 0:
            return
        from ..ops.native import check_lds_add_order
        check_lds_add_order(dev)                       # row passes accumulate with same-address ds_add_f64
        ne, de = n_e[self.ents], d_e[self.ents]
        self.row_ptr = torch.zeros(self.B + 1, dtype=torch.int64, device=dev)
        torch.cumsum(ne, 0, out=self.row_ptr[1:])
        self.col_ptr = torch.zeros(self.B + 1, dtype=torch.int64, device=dev)
        torch.cumsum(de, 0, out=self.col_ptr[1:])
        n_rows = int(self.row_ptr[-1])
        row_sel, col_sel = ds.entity_rows(sel)
        row_nnz = pnip[row_sel + 1] - pnip[row_sel]
        nip = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(row_nnz, 0, out=nip[1:])
        cbase = seg.col_ptr[seg.row_entity[row_sel]]               # parent column of the entity's local 0
        self.lcol, self.val = csr_gather_rows(pnip, ppos, pval, row_sel, nip, cbase, torch.int16)
        self.nip = nip
        if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1" and self.lcol.numel():
            assert int(self.lcol.min()) >= 0 and int(self.lcol.max()) < int(de.max()), "local column range"
        self.rows, self.cols = row_sel, col_sel
        self.y, self.w = seg.y[row_sel].contiguous(), seg.w[row_sel].contiguous()
        self.n_rows = n_rows
        self.nnz = int(nip[-1])
        self.scr = torch.empty(4 * max(n_rows, 1), dtype=torch.float64, device=dev)
        # launch classes by LDS size; inside a class the largest entities first (they bound the launch's tail)
        ent_nnz = nip[self.row_ptr[1:]] - nip[self.row_ptr[:-1]]
        cls = torch.searchsorted(torch.tensor(_CLASSES, device=dev), de)
        self.m = RE_LBFGS_M
        ws = 0
        for c, dm in enumerate(_CLASSES):
            idx = torch.nonzero(cls == c).squeeze(1)
            if idx.numel() == 0:
                continue
            order = idx[torch.argsort(ent_nnz[idx], descending=True, stable=True)]
            grid = min(re_lbfgs_grid(dm), int(idx.numel()))        # persistent grid: resident workgroups
            self.launches.append((dm, order.to(torch.int32).contiguous(), grid))
            ws = max(ws, grid * 2 * self.m * dm)
        # the (S, Y) history of the resident workgroups (launches run one after another on the stream) and the
        # dequeue counter, allocated once
        self.hist = torch.empty(ws, dtype=torch.float64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)

    def solve(self, loss, l2: float, l1: float, W0: Optional[torch.Tensor], offsets: torch.Tensor, tol: float,
              max_iter: int, max_ls: int = 30, npass: Optional[torch.Tensor] = None) -> FusedResult:
        """Solve every entity of the batch from ``W0`` (packed over the batch's coefficients; None = the last
        solution, or zeros the first time) with L-BFGS (``l1 == 0``) or OWL-QN. ``offsets``: per batch row."""
        from ..ops.native import re_lbfgs_csr
        dev = self.y.device
        if W0 is None:
            W0 = self.W if self.W is not None else torch.zeros(int(self.col_ptr[-1]), dtype=torch.float64,
                                                                device=dev)
        W = W0.to(torch.float64).contiguous().clone()
        f = torch.empty(self.B, dtype=torch.float64, device=dev)
        iters = torch.empty(self.B, dtype=torch.int32, device=dev)
        reason = torch.empty(self.B, dtype=torch.int32, device=dev)
        z = torch.empty(self.n_rows, dtype=torch.float64, device=dev)
        off = offsets.to(dev, torch.float64).contiguous()
        assert off.numel() == self.n_rows and W.numel() == int(self.col_ptr[-1])
        for dm, order, grid in self.launches:
            re_lbfgs_csr(order, self.row_ptr, self.col_ptr, self.nip, self.lcol, self.val, self.y, off, self.w,
                         self.scr, W, f, iters, reason, z, loss.loss_id, l2, l1, tol, max_iter, dm, self.hist,
                         self.ticket, grid, m=self.m, max_ls=max_ls, npass=npass)
        self.W = W
        return FusedResult(W, f, iters.to(torch.long), reason.to(torch.long), z)
