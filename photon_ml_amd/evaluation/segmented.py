"""Device-resident per-group ranking metrics (K12: ``AUC:tag``, ``AUPR:tag``, ``PRECISION@k:tag``).

:class:`GroupedRanking` is the group layout of one evaluator, built once: labels, weights and group ids never
change between evaluations, so an evaluation only reads the scores (once, through ``perm``) and the group-ordered
weight / positive-flag arrays contiguously. Groups are bucketed by length into size classes, each with its own
execution in ``ops/csrc/game_kernels.hip`` (``ops/native.py::seg_rank_eval``):

======  ===================  ==========================================================================
class   rows                 execution
======  ===================  ==========================================================================
C16     1..16                four groups per wave, one 16-lane row each
C64     17..64               one wave per group, rows in registers
CWG     65..``wg_max``       one 256-thread workgroup per group, bitonic sort in LDS (<= 48 KB)
LONG    > ``wg_max``         rows pre-sorted by two stable torch sorts, streamed by one workgroup per group
======  ===================  ==========================================================================

A class takes no group longer than ``wg_max``, so a small ``wg_max`` pushes small groups through LONG
(``wg_max = 0``: every group). The layout knows nothing about where its rows came from: under a process group
``MultiEvaluator`` routes every row to the rank that owns its group and hands the layout the routed rows' group
codes, labels and weights (a rank that owns nothing builds the empty layout, ``n = 0``).

Reference: ``photon-api/.../evaluation/MultiEvaluator.scala:49-64``, ``AreaUnderROCCurveLocalEvaluator.scala:33-70``,
``PrecisionAtKLocalEvaluator.scala:39-51``; the per-group area under the precision/recall curve is the weighted
form of ``photon-diagnostics/.../Evaluation.scala:84`` (``evaluators.aupr_weighted``), a third metric of the same
kernels over the same layout.
"""
from __future__ import annotations

from typing import Dict

import torch

from ..constants import POSITIVE_RESPONSE_THRESHOLD
from ..ops.native import SEG_RANK_CLASSES, SEG_RANK_WG_CAP, seg_rank_caps, seg_rank_eval


class GroupedRanking:
    """Group layout for per-group AUC / AUPR / precision@k. ``group_codes``: dense int64 group code of every row
    (``np.unique(..., return_inverse=True)``); ``labels`` / ``weights``: per row. On ``device="cpu"`` only the
    layout is built (the metrics are HIP kernels)."""

    def __init__(self, group_codes, labels, weights=None, device=None, wg_max: int = SEG_RANK_WG_CAP):
        if not 0 <= int(wg_max) <= SEG_RANK_WG_CAP:
            raise ValueError(f"wg_max must be in [0, {SEG_RANK_WG_CAP}]: {wg_max}")
        self.wg_max = int(wg_max)
        self.device = torch.device(device) if device is not None else torch.as_tensor(labels).device
        dev = self.device
        group = torch.as_tensor(group_codes, dtype=torch.int64, device=dev)
        y = torch.as_tensor(labels, dtype=torch.float64, device=dev)
        self.n = int(group.numel())
        w = torch.ones(self.n, dtype=torch.float64, device=dev) if weights is None else torch.as_tensor(
            weights, dtype=torch.float64, device=dev)
        if y.numel() != self.n or w.numel() != self.n:
            raise ValueError("group codes, labels and weights must have one entry per row")
        if self.n and int(group.min()) < 0:
            raise ValueError("group codes must be >= 0")
        self.n_groups = int(group.max()) + 1 if self.n else 0
        self.perm = torch.sort(group, stable=True).indices.contiguous()
        counts = torch.bincount(group, minlength=self.n_groups)
        self.seg_ptr = torch.zeros(self.n_groups + 1, dtype=torch.int64, device=dev)
        self.seg_ptr[1:] = torch.cumsum(counts, 0)
        self.wts = w[self.perm].contiguous()
        self.flag = (y[self.perm] > POSITIVE_RESPONSE_THRESHOLD).to(torch.uint8).contiguous()
        caps = seg_rank_caps(self.wg_max)
        self.lists: Dict[str, torch.Tensor] = {}
        lo = 0
        for c in SEG_RANK_CLASSES:
            hi = caps[c]
            m = counts > lo if hi is None else (counts > lo) & (counts <= hi)
            self.lists[c] = torch.nonzero(m).flatten().contiguous()
            lo = lo if hi is None else max(lo, hi)
        cw = counts[self.lists["CWG"]]
        self.cwg_pad = 64
        while cw.numel() and self.cwg_pad < int(cw.max()):
            self.cwg_pad <<= 1
        # LONG groups: their group-ordered slots, the dense LONG index of every such row, and the row ranges
        lg = self.lists["LONG"]
        ll = counts[lg]
        self.long_ptr = torch.zeros(lg.numel() + 1, dtype=torch.int64, device=dev)
        self.long_ptr[1:] = torch.cumsum(ll, 0)
        self.long_gid = torch.repeat_interleave(torch.arange(lg.numel(), dtype=torch.int64, device=dev), ll)
        self.long_rows = (torch.arange(self.long_gid.numel(), dtype=torch.int64, device=dev)
                          - self.long_ptr[:-1][self.long_gid] + self.seg_ptr[:-1][lg][self.long_gid]).contiguous()

    @property
    def class_counts(self) -> Dict[str, int]:
        return {c: int(t.numel()) for c, t in self.lists.items()}

    def _eval(self, scores, k: int, metric=None):
        if self.device.type != "cuda":
            raise RuntimeError("GroupedRanking evaluates on a GPU only (HIP kernels); on the CPU it holds the "
                               "layout, use MultiEvaluator's host loop for values")
        s = torch.as_tensor(scores, dtype=torch.float64, device=self.device).contiguous()
        if s.numel() != self.n:
            raise ValueError(f"expected {self.n} scores, got {s.numel()}")
        return seg_rank_eval(self, s, k, metric)

    def auc(self, scores):
        """Weighted tie-grouped AUC of every group (fp64 device tensor, NaN where a class is missing); None when
        a score is NaN."""
        return self._eval(scores, 0)

    def aupr(self, scores):
        """Weighted tie-grouped area under the precision/recall curve of every group (``evaluators.aupr_weighted``;
        fp64 device tensor, NaN where a class is missing); None when a score is NaN."""
        return self._eval(scores, 0, "aupr")

    def precision_at_k(self, scores, k: int):
        """Precision@k of every group (fp64 device tensor); None when a score is NaN."""
        if k <= 0:
            raise ValueError(f"Position k must be greater than 0: {k}")
        return self._eval(scores, int(k))

    @staticmethod
    def finite_sums(values: torch.Tensor) -> torch.Tensor:
        """(sum, count) of the finite entries as two fp64 on the host (one device reduction, one readback)."""
        ok = torch.isfinite(values)
        tot = torch.where(ok, values, torch.zeros_like(values)).sum()
        return torch.stack([tot, ok.sum().to(torch.float64)]).cpu()

    @staticmethod
    def mean_finite(values: torch.Tensor) -> float:
        """Mean over the finite entries (one device reduction, one readback); NaN when there are none."""
        r = GroupedRanking.finite_sums(values)
        return float(r[0] / r[1]) if float(r[1]) > 0 else float("nan")
