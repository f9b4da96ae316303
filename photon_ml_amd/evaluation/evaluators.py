"""Evaluators over score arrays aligned with the samples (no joins: scores, labels, offsets, weights and group ids
share the sample order).

Reference: ``photon-lib/.../evaluation/{Evaluator,EvaluatorType}.scala`` (evaluate = f(score + offset), betterThan),
``photon-api/.../evaluation/*.scala``:
  * AUC (global; MLlib BinaryClassificationMetrics -> UNWEIGHTED, Appendix C.5) ``AreaUnderROCCurveEvaluator``
  * local weighted AUC with tie groups ``AreaUnderROCCurveLocalEvaluator.scala:33-70``
  * AUPR: area under the precision/recall curve, the trapezoid of ``photon-diagnostics/.../Evaluation.scala:84``
    (MLlib ``areaUnderPR``, ``diagnostics/evaluation.py::binary_metrics``) as an evaluator: global and UNWEIGHTED
    like AUC, weighted per group (:func:`aupr_weighted`)
  * RMSE = sqrt(sum w (z-y)^2/2 / N) — the reference's definition, kept for parity (Appendix C.1)
  * logistic / poisson / squared / smoothed-hinge loss sums
  * multi-evaluators grouped by an id tag: AUC:tag, AUPR:tag and PRECISION@k:tag, mean over groups with finite values
    (``MultiEvaluator.scala:49-64``, ``PrecisionAtKLocalEvaluator.scala:39-51``)
  * name parsing ``AUC``, ``RMSE``, ``LOGISTIC_LOSS``, ..., ``PRECISION@5:queryId``, ``AUC:userId``, ``AUPR``,
    ``AUPR:userId``.

Sorting-based metrics run on the device (torch sort / segmented reductions), so the whole validation pass stays
in HBM; the per-group metrics of a GPU run are HIP kernels over a group layout built once (``segmented.py``).

Under a process group no metric gathers rows:
  * ``AUC:tag`` / ``AUPR:tag`` / ``PRECISION@k:tag`` route every row once to the rank that owns its group
    (``parallel/sharding.py``: ``entity_keys`` -> ``EntityPartitioner`` -> ``RowRouter``), an evaluation routes the
    scores (one all-to-all of 8 B per row, device to device under RCCL), evaluates the owned groups locally and
    all-reduces (sum, count) of the finite values;
  * plain ``AUC`` is :func:`auc_distributed`: local sort, regular sampling, one all-to-all of score
    buckets, integer counts per bucket (``ops/native.py::auc_counts``), a three-integer all-gather. Only when a
    score is NaN do all ranks take the old gather path together;
  * plain ``AUPR`` is :func:`aupr_distributed`: the same bucket exchange, then integer class counts per bucket (one
    small all-gather), every rank's own tie-group terms from int64 cumulative counts, and the partial sums added in
    rank order on every rank.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from ..constants import POSITIVE_RESPONSE_THRESHOLD, TaskType
from ..function import losses as L


def _t(x, device=None):
    return torch.as_tensor(x, dtype=torch.float64, device=device)


def auc_weighted(scores: torch.Tensor, labels: torch.Tensor, weights: Optional[torch.Tensor] = None) -> float:
    """Weighted ROC AUC with tied scores counted as half (trapezoid), vectorised (K11)."""
    s = _t(scores)
    y = _t(labels, s.device)
    w = torch.ones_like(s) if weights is None else _t(weights, s.device)
    if s.numel() == 0:
        return float("nan")
    order = torch.argsort(s, descending=True, stable=True)
    s, y, w = s[order], y[order], w[order]
    pos = torch.where(y > POSITIVE_RESPONSE_THRESHOLD, w, torch.zeros_like(w))
    neg = w - pos
    # group ties
    new_group = torch.ones_like(s, dtype=torch.bool)
    new_group[1:] = s[1:] != s[:-1]
    gid = torch.cumsum(new_group.to(torch.int64), 0) - 1
    ng = int(gid[-1].item()) + 1
    gp = torch.zeros(ng, dtype=torch.float64, device=s.device).index_add_(0, gid, pos)
    gn = torch.zeros(ng, dtype=torch.float64, device=s.device).index_add_(0, gid, neg)
    tp_before = torch.cumsum(gp, 0) - gp
    raw = torch.sum(tp_before * gn + gp * gn / 2.0)
    tp, tn = gp.sum(), gn.sum()
    return float(raw / (tp * tn))


def aupr_weighted(scores: torch.Tensor, labels: torch.Tensor, weights: Optional[torch.Tensor] = None) -> float:
    """Weighted area under the precision/recall curve, vectorised, on the device of ``scores``.

    Rows sorted by score descending form tie groups g = 1..G (``==``); with ``gp_g`` / ``gn_g`` the group's positive
    / negative weight and ``TP_g`` / ``FP_g`` their inclusive prefix sums,

        AUPR = (1 / TP_G) sum over groups with gp_g > 0 of gp_g (p_g + q_g) / 2,
        p_g = TP_g / (TP_g + FP_g),   q_g = TP_{g-1} / (TP_{g-1} + FP_{g-1}) if that denominator is > 0 else p_g,

    NaN without rows or when a class has no weight. With unit weights this is the trapezoid of
    ``diagnostics/evaluation.py::binary_metrics`` (points (R_g, p_g), first point (0, p_1)). The prefixes before a
    group are the inclusive prefixes SHIFTED by one group, never inclusive prefix minus the group's sums (that
    difference cancels when weights span many orders of magnitude). A group without positive weight makes no recall
    step and adds nothing, and rows of weight 0 never change the value."""
    s = _t(scores)
    y = _t(labels, s.device)
    w = torch.ones_like(s) if weights is None else _t(weights, s.device)
    if s.numel() == 0:
        return float("nan")
    order = torch.argsort(s, descending=True, stable=True)
    s, y, w = s[order], y[order], w[order]
    pos = torch.where(y > POSITIVE_RESPONSE_THRESHOLD, w, torch.zeros_like(w))
    neg = w - pos
    new_group = torch.ones_like(s, dtype=torch.bool)
    new_group[1:] = s[1:] != s[:-1]
    gid = torch.cumsum(new_group.to(torch.int64), 0) - 1
    ng = int(gid[-1].item()) + 1
    gp = torch.zeros(ng, dtype=torch.float64, device=s.device).index_add_(0, gid, pos)
    gn = torch.zeros(ng, dtype=torch.float64, device=s.device).index_add_(0, gid, neg)
    return _aupr_of_groups(gp, gn, torch.cumsum(gp, 0), torch.cumsum(gn, 0))


def _aupr_terms(gp, tp, fp, tp_before, fp_before) -> torch.Tensor:
    """Sum of ``gp (p + q) / 2`` over the tie groups with ``gp > 0`` (all arguments fp64, one entry per group)."""
    keep = gp > 0
    gp, tp, fp, tp_before, fp_before = gp[keep], tp[keep], fp[keep], tp_before[keep], fp_before[keep]
    p = tp / (tp + fp)
    den = tp_before + fp_before
    q = torch.where(den > 0, tp_before / torch.where(den > 0, den, torch.ones_like(den)), p)
    return torch.sum(gp * (p + q) / 2.0)


def _aupr_of_groups(gp, gn, tp, fp) -> float:
    P, N = float(tp[-1]), float(fp[-1])
    if not (P > 0 and N > 0):
        return float("nan")
    zero = torch.zeros(1, dtype=torch.float64, device=gp.device)
    return float(_aupr_terms(gp, tp, fp, torch.cat([zero, tp[:-1]]), torch.cat([zero, fp[:-1]])) / tp[-1])


def precision_at_k(scores, labels, k: int) -> float:
    s = _t(scores)
    y = _t(labels, s.device)
    order = torch.argsort(s, descending=True, stable=True)[:k]
    hits = int((y[order] > POSITIVE_RESPONSE_THRESHOLD).sum())
    return hits / k


def _dist():
    from ..parallel.dist import is_dist
    return is_dist()


def _allsum(*vals: float) -> List[float]:
    """Sum scalars over the process group (one collective)."""
    from ..parallel.dist import all_reduce_
    from ..parallel.sharding import comm_device
    t = torch.tensor(vals, dtype=torch.float64, device=comm_device())
    all_reduce_(t)
    return t.tolist()


def _gather(t: torch.Tensor) -> torch.Tensor:
    from ..parallel.sharding import all_gather_varlen
    return torch.cat([x.to(t.device) for x in all_gather_varlen(t.detach().cpu())])


def _rank() -> int:
    from ..parallel.dist import rank
    return rank()


AUC_SAMPLES = 64      # regular samples per rank that place the score-bucket splitters of auc_distributed


def _gather_fixed(t: torch.Tensor) -> torch.Tensor:
    """All-gather equally long small 1-D tensors; [world, len] on the host."""
    import torch.distributed as dist
    from ..parallel.dist import world_size
    from ..parallel.sharding import comm_device
    dev = comm_device()
    t = t.to(dev)
    outs = [torch.empty_like(t) for _ in range(world_size())]
    dist.all_gather(outs, t)
    return torch.stack(outs).cpu()


def _score_buckets(scores: torch.Tensor, flags: torch.Tensor, info: Optional[dict]):
    """Steps 1 to 3 of :func:`auc_distributed`, shared by the bucketed global metrics: local sort, regular samples
    and the collective NaN decision, one all-to-all of score buckets. Returns ``(path, scores, flags)``:
    ``"buckets"`` with the received bucket sorted descending (bucket 0, on rank 0, holds the highest scores; a tie
    group never straddles ranks), ``"gather"`` with this rank's rows in row order when some rank saw a NaN (every
    rank gets the same answer), ``"empty"`` when no rank holds a row. Fills ``info`` (``path``, ``bucket_rows``)."""
    from ..parallel.dist import world_size
    from ..parallel.sharding import RowRouter
    P = world_size()
    s = _t(scores) + 0.0
    dev = s.device
    f = torch.as_tensor(flags, device=dev).to(torch.uint8)
    n = int(s.numel())
    s0, f0 = s, f                                           # row order, for the gather path
    s, order = torch.sort(s, descending=True)
    f = f[order]
    S = AUC_SAMPLES
    head = torch.zeros(2 + S, dtype=torch.float64, device=dev)
    if n:
        pos = (2 * torch.arange(S, dtype=torch.int64, device=dev) + 1) * n // (2 * S)
        head[0] = 1.0
        head[1] = torch.isnan(s).any().to(torch.float64)
        head[2:] = s[pos]
    got = _gather_fixed(head).numpy()
    if info is not None:
        info.update(path="buckets", bucket_rows=0)
    if np.any(got[:, 1] != 0.0):
        if info is not None:
            info["path"] = "gather"
        return "gather", s0, f0
    samples = np.sort(got[got[:, 0] != 0.0, 2:].ravel())[::-1]
    if samples.size == 0:                                  # no rank holds a row
        return "empty", None, None
    split = torch.from_numpy(np.ascontiguousarray(samples[[k * samples.size // P for k in range(1, P)]])).to(dev)
    # rows of bucket <= k: those with score >= split[k] (the shard is descending: search its negation)
    ends = torch.searchsorted(-s, -split, right=True).tolist()
    bounds = [0] + ends + [n]
    router = RowRouter.from_counts([bounds[k + 1] - bounds[k] for k in range(P)])
    rs, rf = router.exchange(s), router.exchange(f)
    if info is not None:
        info["bucket_rows"] = int(rs.numel())
    if sum(1 for c in router.recv_counts if c) > 1:         # segments of several ranks: merge them by a sort
        rs, o = torch.sort(rs, descending=True)
        rf = rf[o]
    return "buckets", rs, rf


def auc_distributed(scores: torch.Tensor, flags: torch.Tensor, info: Optional[dict] = None) -> float:
    """Exact unweighted AUC of the rows of ALL ranks without gathering them; every rank passes its
    shard's ``scores`` (fp64) and positive ``flags`` (uint8) and gets the same value, bitwise the value
    ``auc_weighted`` gives on the concatenated rows while ``P N < 2^53``.

    1. ``scores + 0.0`` (so -0.0 ties with 0.0 in the radix sort), sorted descending locally.
    2. ``AUC_SAMPLES`` regular samples per rank and a NaN flag, one small all-gather; the sorted samples give
       ``world - 1`` splitters. If any rank saw a NaN, every rank takes the gather path (``auc_weighted`` on all
       rows): a collective decision.
    3. The bucket of a row is the number of splitters strictly greater than its score -- a function of the value, so
       a tie group never straddles ranks; buckets are contiguous in the sorted shard. One all-to-all each for the
       scores and the flags (``RowRouter.exchange``).
    4. The receiver sorts its bucket (segments of several ranks) and counts ``(2 raw, P, N)`` as integers (``auc_counts``: HIP on a GPU).
    5. The three integers of every rank are all-gathered and combined in Python ints: bucket b adds
       ``2 raw_b + 2 P_before_b N_b`` (``P_before_b``: positives of the higher-score buckets).

    Steps 1 to 3 are :func:`_score_buckets`. ``info`` (optional dict) receives ``path`` ("buckets" / "gather") and
    ``bucket_rows`` (rows received here)."""
    from ..ops.native import auc_counts
    path, rs, rf = _score_buckets(scores, flags, info)
    if path == "gather":
        return auc_weighted(_gather(rs), _gather(rf.to(torch.float64)), None)
    if path == "empty":
        return float("nan")
    counts = auc_counts(rs.contiguous(), rf.contiguous())
    allc = _gather_fixed(counts).tolist()
    tot2 = tp = tn = 0
    for raw2, pb, nb in allc:                               # bucket 0 holds the highest scores
        tot2 += int(raw2) + 2 * tp * int(nb)
        tp += int(pb)
        tn += int(nb)
    if tp + tn >= 1 << 31:
        raise ValueError(f"auc_distributed: {tp + tn} rows; the integer counts are kept below 2^31 rows")
    if tp == 0 or tn == 0:
        return float("nan")
    return (tot2 / 2.0) / (float(tp) * float(tn))


def aupr_distributed(scores: torch.Tensor, flags: torch.Tensor, info: Optional[dict] = None) -> float:
    """Unweighted AUPR (:func:`aupr_weighted` with unit weights) of the rows of ALL ranks without gathering them;
    every rank passes its shard's ``scores`` (fp64) and positive ``flags`` (uint8) and gets the same bits.

    The score buckets are those of :func:`auc_distributed` (:func:`_score_buckets`; a NaN on any rank sends every
    rank down the gather path). Then every rank counts the positives and negatives of its bucket as integers, one
    small all-gather makes the counts of the higher-score buckets and the totals known exactly, and the rank sums
    the terms of its own tie groups with torch ops where the bucket lives: ``TP_g`` / ``FP_g`` are int64 cumulative
    counts plus the counts before the bucket, converted to fp64 (exact below 2^53 rows), the prefixes before a group
    are those of the group above it. The partial sums are all-gathered and added in rank order on every rank."""
    path, rs, rf = _score_buckets(scores, flags, info)
    if path == "gather":
        return aupr_weighted(_gather(rs), _gather(rf.to(torch.float64)), None)
    if path == "empty":
        return float("nan")
    dev = rs.device
    nb = int(rs.numel())
    c = torch.cumsum(rf.to(torch.int64), 0)                  # positives through every row of the bucket
    pb = int(c[-1]) if nb else 0
    allc = _gather_fixed(torch.tensor([pb, nb - pb], dtype=torch.int64)).tolist()
    me = _rank()
    p_before = sum(int(r[0]) for r in allc[:me])
    n_before = sum(int(r[1]) for r in allc[:me])
    P, N = sum(int(r[0]) for r in allc), sum(int(r[1]) for r in allc)
    part = torch.zeros(1, dtype=torch.float64, device=dev)
    if nb:
        last = torch.ones(nb, dtype=torch.bool, device=dev)
        last[:-1] = rs[1:] != rs[:-1]
        ends = torch.nonzero(last).flatten()                 # closing row of every tie group
        tp_i = c[ends] + p_before
        fp_i = ends + 1 - c[ends] + n_before
        head = torch.tensor([[p_before], [n_before]], dtype=torch.int64, device=dev)
        tpb_i, fpb_i = torch.cat([head[0], tp_i[:-1]]), torch.cat([head[1], fp_i[:-1]])
        f64 = lambda t: t.to(torch.float64)
        part = _aupr_terms(f64(tp_i - tpb_i), f64(tp_i), f64(fp_i), f64(tpb_i), f64(fpb_i)).reshape(1)
    parts = _gather_fixed(part).flatten().tolist()
    if P == 0 or N == 0:
        return float("nan")
    tot = 0.0
    for v in parts:                                          # rank order: the same bits on every rank
        tot += v
    return tot / float(P)


class Evaluator:
    """Evaluates ``scores + offsets`` against the labels. Under a process group every rank holds a row shard:
    additive metrics (losses, RMSE) all-reduce their sums, plain AUC exchanges score buckets and the
    per-group metrics route their rows to the groups' owners (C18); no metric gathers rows."""

    name = "EVALUATOR"
    higher_is_better = True

    def __init__(self, labels, offsets=None, weights=None, device=None):
        self.distributed = _dist()
        self.labels = _t(labels, device)
        n = self.labels.numel()
        self.offsets = torch.zeros(n, dtype=torch.float64, device=self.labels.device) if offsets is None else _t(
            offsets, self.labels.device)
        self.weights = torch.ones(n, dtype=torch.float64, device=self.labels.device) if weights is None else _t(
            weights, self.labels.device)

    def evaluate(self, scores) -> float:
        s = _t(scores, self.labels.device) + self.offsets
        return self._evaluate(s)

    def _evaluate(self, s: torch.Tensor) -> float:
        raise NotImplementedError

    def better_than(self, a: float, b: float) -> bool:
        return a > b if self.higher_is_better else a < b

    def __repr__(self):
        return self.name


class AUCEvaluator(Evaluator):
    name = "AUC"

    def __init__(self, labels, offsets=None, weights=None, device=None):
        super().__init__(labels, offsets, weights, device)
        self.last_info: dict = {}
        if self.distributed:
            self.flags = (self.labels > POSITIVE_RESPONSE_THRESHOLD).to(torch.uint8)

    def _evaluate(self, s):
        if self.distributed:
            return auc_distributed(s, self.flags, self.last_info)
        return auc_weighted(s, self.labels, None)  # MLlib AUC ignores weights


class AUPREvaluator(Evaluator):
    """Area under the precision/recall curve of all rows; unweighted like plain AUC (MLlib's ``areaUnderPR`` takes
    no weights). Under a process group: :func:`aupr_distributed`."""
    name = "AUPR"

    def __init__(self, labels, offsets=None, weights=None, device=None):
        super().__init__(labels, offsets, weights, device)
        self.last_info: dict = {}
        if self.distributed:
            self.flags = (self.labels > POSITIVE_RESPONSE_THRESHOLD).to(torch.uint8)

    def _evaluate(self, s):
        if self.distributed:
            return aupr_distributed(s, self.flags, self.last_info)
        return aupr_weighted(s, self.labels, None)


class RMSEEvaluator(Evaluator):
    name = "RMSE"
    higher_is_better = False

    def _evaluate(self, s):
        d = s - self.labels
        num, cnt = float(torch.sum(self.weights * 0.5 * d * d)), float(self.labels.numel())
        if self.distributed:
            num, cnt = _allsum(num, cnt)
        return math.sqrt(num / max(cnt, 1.0))


class _LossEvaluator(Evaluator):
    higher_is_better = False
    loss = None

    def evaluate(self, scores) -> float:
        s = _t(scores, self.labels.device)
        if s.is_cuda and s.dtype == torch.float64:
            # scores + offsets folded into the fused loss pass (no separate N-length add)
            from ..ops.native import loss_sum
            t = loss_sum(self.loss.loss_id, s.contiguous(), self.labels, self.weights, offsets=self.offsets)
            if t is not None:
                v = float(t)
                return _allsum(v)[0] if self.distributed else v
        return self._evaluate(s + self.offsets)

    def _evaluate(self, s):
        v = None
        if s.is_cuda:
            from ..ops.native import loss_sum
            t = loss_sum(self.loss.loss_id, s.contiguous(), self.labels, self.weights)   # one fused HIP pass
            v = None if t is None else float(t)
        if v is None:
            l, _ = self.loss.loss_and_dz(s, self.labels)
            v = float(torch.sum(self.weights * l))
        return _allsum(v)[0] if self.distributed else v


class LogisticLossEvaluator(_LossEvaluator):
    name = "LOGISTIC_LOSS"
    loss = L.LOGISTIC


class PoissonLossEvaluator(_LossEvaluator):
    name = "POISSON_LOSS"
    loss = L.POISSON


class SquaredLossEvaluator(_LossEvaluator):
    name = "SQUARED_LOSS"
    loss = L.SQUARED


class SmoothedHingeLossEvaluator(_LossEvaluator):
    name = "SMOOTHED_HINGE_LOSS"
    loss = L.SMOOTHED_HINGE


class MultiEvaluator(Evaluator):
    """Per-group local metric, mean over groups whose value is finite.

    Under a process group a group's rows can sit on several ranks, so every row is routed ONCE, at construction,
    to the rank that owns its group (the 64-bit ``entity_keys`` of the ids, one ``EntityPartitioner`` and one
    ``RowRouter``); labels and weights travel with it. An evaluation routes ``scores + offsets`` (one all-to-all),
    evaluates the owned groups here and all-reduces (sum, count) of the finite values. Routed rows arrive ordered
    by source rank, then local position -- the order of the concatenation rank 0, rank 1, ... -- so ties at
    position k of precision@k resolve as on the concatenated rows. Every rank issues the same collectives in the
    same order whatever path it took locally (``last_path``)."""

    def __init__(self, ids, labels, offsets=None, weights=None, device=None):
        super().__init__(labels, offsets, weights, device)
        ids = np.asarray(ids)
        dev = self.labels.device
        self.router = None
        if self.distributed:
            from ..parallel.sharding import EntityPartitioner, RowRouter, entity_keys
            keys = entity_keys(ids, dev)
            self.router = RowRouter(EntityPartitioner.build_t(keys).owner_t(keys))
            # the group layout below is over the rows this rank OWNS
            self._y, self._w = self.router.forward(self.labels), self.router.forward(self.weights)
            uniq, inv = torch.unique(self.router.forward(keys), sorted=True, return_inverse=True)
            self.group = inv.to(torch.int64)
            uniq = uniq.cpu().numpy()
        else:
            uniq, inv = np.unique(ids.astype(str) if ids.dtype == object else ids, return_inverse=True)
            self.group = torch.as_tensor(inv, dtype=torch.int64, device=dev)
            self._y, self._w = self.labels, self.weights
        self.n_groups = len(uniq)
        self.group_keys = uniq
        self.last_path = "host"
        # GPU runs evaluate every group in HIP kernels over a layout built once (K12)
        self.ranking = None
        if self.labels.is_cuda:
            from .segmented import GroupedRanking
            self.ranking = GroupedRanking(self.group, self._y, self._w, dev)

    def _local(self, s, y, w) -> float:
        raise NotImplementedError

    def _device_values(self, s) -> Optional[torch.Tensor]:
        """Per-group values from the HIP kernels; None when they decline (a NaN score)."""
        raise NotImplementedError

    def _values(self, s):
        """The metric of every group, NaN where it is undefined: an fp64 device tensor from the HIP kernels
        (``last_path == "device"``) or a list of floats from the host loop (``"host"``). Under a process group:
        of every group this rank owns, from the routed scores."""
        if self.router is not None:
            s = self.router.forward(s)
        vals = self._device_values(s) if self.ranking is not None else None
        self.last_path = "host" if vals is None else "device"
        return self._host_values(s) if vals is None else vals

    def evaluate_groups(self, scores):
        """``(group_keys, values)``: the sorted distinct group ids and the local metric of every group for
        ``scores + offsets`` as an fp64 tensor on the evaluator's device, NaN where it is undefined. Under a process
        group every rank must call this (the scores are routed) and gets the groups it OWNS, keyed by their stable
        64-bit hashes: the ranks' key sets are disjoint and their union is every group."""
        vals = self._values(_t(scores, self.labels.device) + self.offsets)
        return self.group_keys, torch.as_tensor(vals, dtype=torch.float64, device=self.labels.device)

    def _evaluate(self, s):
        vals = self._values(s)
        if self.distributed:
            if self.last_path == "device":
                tot, cnt = self.ranking.finite_sums(vals).tolist()
            else:
                vals = [v for v in vals if math.isfinite(v)]
                tot, cnt = float(np.sum(vals)) if vals else 0.0, float(len(vals))
            tot, cnt = _allsum(tot, cnt)
            return tot / cnt if cnt > 0 else float("nan")
        if self.last_path == "device":
            return self.ranking.mean_finite(vals)
        vals = [v for v in vals if math.isfinite(v)]
        return float(np.mean(vals)) if vals else float("nan")

    def _host_values(self, s) -> List[float]:
        order = torch.argsort(self.group, stable=True)
        g = self.group[order]
        s, y, w = s[order], self._y[order], self._w[order]
        counts = torch.bincount(g, minlength=self.n_groups).cpu().numpy()
        starts = np.concatenate([[0], np.cumsum(counts)])
        vals = [float("nan")] * self.n_groups
        s_c, y_c, w_c = s.cpu(), y.cpu(), w.cpu()
        for i in range(self.n_groups):
            a, b = starts[i], starts[i + 1]
            if b > a:
                vals[i] = self._local(s_c[a:b], y_c[a:b], w_c[a:b])
        return vals


class AUCMultiEvaluator(MultiEvaluator):
    def __init__(self, id_tag: str, ids, labels, offsets=None, weights=None, device=None):
        super().__init__(ids, labels, offsets, weights, device)
        self.id_tag = id_tag
        self.name = f"AUC:{id_tag}"

    def _local(self, s, y, w):
        return auc_weighted(s, y, w)

    def _device_values(self, s):
        return self.ranking.auc(s)


class AUPRMultiEvaluator(MultiEvaluator):
    def __init__(self, id_tag: str, ids, labels, offsets=None, weights=None, device=None):
        super().__init__(ids, labels, offsets, weights, device)
        self.id_tag = id_tag
        self.name = f"AUPR:{id_tag}"

    def _local(self, s, y, w):
        return aupr_weighted(s, y, w)

    def _device_values(self, s):
        return self.ranking.aupr(s)


class PrecisionAtKMultiEvaluator(MultiEvaluator):
    def __init__(self, k: int, id_tag: str, ids, labels, offsets=None, weights=None, device=None):
        if k <= 0:
            raise ValueError(f"Position k must be greater than 0: {k}")
        super().__init__(ids, labels, offsets, weights, device)
        self.k = k
        self.id_tag = id_tag
        self.name = f"PRECISION@{k}:{id_tag}"

    def _local(self, s, y, w):
        return precision_at_k(s, y, self.k)

    def _device_values(self, s):
        return self.ranking.precision_at_k(s, self.k)


# --------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class EvaluatorType:
    name: str
    id_tag: Optional[str] = None
    k: Optional[int] = None

    @property
    def is_multi(self) -> bool:
        return self.id_tag is not None

    def __str__(self):
        return self.name


SIMPLE_TYPES = ("AUC", "AUPR", "RMSE", "LOGISTIC_LOSS", "POISSON_LOSS", "SMOOTHED_HINGE_LOSS", "SQUARED_LOSS")
_P_AT_K = re.compile(r"(?i:PRECISION)@(\d+):(.*)")
_AUC_TAG = re.compile(r"(?i:AUC):(.*)")
_AUPR_TAG = re.compile(r"(?i:AUPR):(.*)")


def parse_evaluator_type(name: str) -> EvaluatorType:
    """``Utils.evaluatorParser`` (CLI/util/Utils.scala:308-322)."""
    n = name.strip()
    m = _P_AT_K.fullmatch(n)
    if m:
        k = int(m.group(1))
        if k <= 0:
            raise ValueError(f"Position k must be greater than 0: {k}")
        return EvaluatorType(f"PRECISION@{k}:{m.group(2)}", m.group(2), k)
    m = _AUC_TAG.fullmatch(n)
    if m:
        return EvaluatorType(f"AUC:{m.group(1)}", m.group(1))
    m = _AUPR_TAG.fullmatch(n)
    if m:
        return EvaluatorType(f"AUPR:{m.group(1)}", m.group(1))
    up = n.upper()
    if up in SIMPLE_TYPES:
        return EvaluatorType(up)
    raise ValueError(f"Unsupported evaluator type: {name}")


def build_evaluator(etype, labels, offsets=None, weights=None, id_tags: Optional[dict] = None, device=None):
    """EvaluatorFactory.buildEvaluator."""
    if isinstance(etype, str):
        etype = parse_evaluator_type(etype)
    simple = {"AUC": AUCEvaluator, "AUPR": AUPREvaluator, "RMSE": RMSEEvaluator,
              "LOGISTIC_LOSS": LogisticLossEvaluator, "POISSON_LOSS": PoissonLossEvaluator,
              "SMOOTHED_HINGE_LOSS": SmoothedHingeLossEvaluator, "SQUARED_LOSS": SquaredLossEvaluator}
    if not etype.is_multi:
        return simple[etype.name](labels, offsets, weights, device)
    if id_tags is None or etype.id_tag not in id_tags:
        raise ValueError(f"id tag {etype.id_tag} required by evaluator {etype.name} not present in the data")
    ids = id_tags[etype.id_tag]
    if etype.k is not None:
        return PrecisionAtKMultiEvaluator(etype.k, etype.id_tag, ids, labels, offsets, weights, device)
    if etype.name.startswith("AUPR:"):
        return AUPRMultiEvaluator(etype.id_tag, ids, labels, offsets, weights, device)
    return AUCMultiEvaluator(etype.id_tag, ids, labels, offsets, weights, device)


def default_validation_evaluator(task) -> str:
    """GameEstimator.scala:519-540: AUC for logistic/SVM, RMSE for linear, Poisson loss for Poisson."""
    task = TaskType.parse(task)
    return {TaskType.LOGISTIC_REGRESSION: "AUC", TaskType.SMOOTHED_HINGE_LOSS_LINEAR_SVM: "AUC",
            TaskType.LINEAR_REGRESSION: "RMSE", TaskType.POISSON_REGRESSION: "POISSON_LOSS"}[task]


def training_loss_evaluator_type(task) -> str:
    """GameEstimator.scala:437-459."""
    task = TaskType.parse(task)
    return {TaskType.LOGISTIC_REGRESSION: "LOGISTIC_LOSS", TaskType.LINEAR_REGRESSION: "SQUARED_LOSS",
            TaskType.POISSON_REGRESSION: "POISSON_LOSS",
            TaskType.SMOOTHED_HINGE_LOSS_LINEAR_SVM: "SMOOTHED_HINGE_LOSS"}[task]
