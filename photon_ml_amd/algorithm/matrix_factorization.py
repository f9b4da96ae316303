"""Matrix-factorization GAME coordinate: the interaction of two kinds of random effects in a latent space.

The reference advertises the model (``README.md:80-83``: "captures interactions between two types of random effects
(e.g., user and item) in the latent space") and ships its Avro schema (``LatentFactorAvro.avsc``), but no training
code; this coordinate is the alternating scheme the model suggests, built from the project's per-entity TRON.

A sample r has a row-side entity i = a(r) and a column-side entity j = b(r); the coordinate's score is ``u_i . v_j``
(K factors each) and, given the partial score o_r of the other coordinates, it minimises

    sum_r wt_r l(y_r, o_r + u_a(r) . v_b(r)) + lambda/2 (||U||_F^2 + ||V||_F^2).

One ``update_model`` runs ``alternations`` rounds of two half-updates. With V fixed, every u_i is an independent
K-coefficient GLM over the rows of entity i whose feature vectors are the v_b(r) (L2 weight lambda, warm start
u_i); then the same for every v_j with the U just computed. Each half minimises a convex sub-problem from a warm
start, so the objective never increases from one half to the next.

The CPU path is the definition: per half it materialises ``F = Other[oid]`` in fp64 and solves the entities with
``optimization.batched.batched_tron`` over zero-padded dense batches (the TRON the fused random-effect kernels are
tested against). On a GPU a half is ONE launch: ``mf_tron_kernel`` (``ops/csrc/mf_kernels.hip``, one wave per
entity, the feature rows gathered from the small factor table) or, with ``PML_MF_FUSED=0``, ``re_tron_tall_kernel``
over a materialised copy of the gathered rows (the A/B baseline; ``profiles/mf_fused.md`` decides the default).
"""
from __future__ import annotations

import logging
import os
import time
from typing import Optional

import numpy as np
import torch

from ..constants import TaskType
from ..data.game_data import GameData
from ..data.random_effect import MatrixFactorizationDataConfiguration
from ..function.losses import loss_for_task
from ..models.game import MatrixFactorizationModel, _id_keys, entity_codes, pair_scores
from ..ops.backend import default_device
from ..optimization.batched import BatchedGLMData, batched_tron
from ..optimization.config import GLMOptimizationConfiguration, OptimizerType, RegularizationType
from ..parallel.dist import is_dist
from .coordinates import Coordinate, random_effect_tracker_stats

log = logging.getLogger(__name__)

MAX_FACTORS = 32
# which device route solves a half-update (profiles/mf_fused.md): 1 = mf_tron_kernel, 0 = the materialised copy
MF_FUSED_DEFAULT = "1"


def fused_route() -> bool:
    return os.environ.get("PML_MF_FUSED", MF_FUSED_DEFAULT) != "0"


class _Side:
    """One side's layout, built once per dataset: the rows sorted by this side's entity (``perm``, ``row_ptr``) and
    the OTHER side's entity code of every sorted row (``oid``, int32), plus labels and weights in that order."""

    def __init__(self, codes: np.ndarray, other_codes: np.ndarray, n_entities: int, y: torch.Tensor, wt: torch.Tensor,
                 device):
        perm = np.argsort(codes, kind="stable")
        counts = np.bincount(codes, minlength=n_entities).astype(np.int64)
        self.n_entities = n_entities
        self.counts = counts
        self.row_ptr_host = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.perm = torch.from_numpy(perm.astype(np.int64)).to(device)
        self.row_ptr = torch.from_numpy(self.row_ptr_host).to(device)
        self.oid = torch.from_numpy(other_codes[perm].astype(np.int32)).to(device)
        self.y = y[self.perm].contiguous()
        self.wt = wt[self.perm].contiguous()
        self.order = torch.from_numpy(np.argsort(-counts, kind="stable").astype(np.int32)).to(device)
        self._classes = None

    def classes(self):
        """Entities grouped by padded row count (powers of two) for the dense batches of the CPU definition:
        ``(entities [B], rows [B, n] (clamped), mask [B, n])`` per class."""
        if self._classes is None:
            out = []
            cap = np.maximum(self.counts, 1)
            cls = np.ceil(np.log2(cap)).astype(np.int64)
            for c in np.unique(cls):
                ents = np.nonzero(cls == c)[0]
                n = 1 << int(c)
                idx = self.row_ptr_host[ents][:, None] + np.arange(n)[None, :]
                mask = np.arange(n)[None, :] < self.counts[ents][:, None]
                idx = np.where(mask, idx, 0)
                dev = self.perm.device
                out.append((torch.from_numpy(ents).to(dev), torch.from_numpy(idx).to(dev),
                            torch.from_numpy(mask).to(dev)))
            self._classes = out
        return self._classes


class MatrixFactorizationCoordinate(Coordinate):
    def __init__(self, coordinate_id: str, data: GameData, data_config: MatrixFactorizationDataConfiguration,
                 opt_config: GLMOptimizationConfiguration, task, device=None, prior=None):
        self.coordinate_id = coordinate_id
        self.data = data
        self.data_config = data_config
        self.task = TaskType.parse(task)
        self.device = torch.device(device) if device is not None else default_device()
        K = data_config.num_factors
        if not 1 <= K <= MAX_FACTORS:
            raise ValueError(f"coordinate {coordinate_id}: {K} latent factors outside 1..{MAX_FACTORS}")
        if self.task == TaskType.SMOOTHED_HINGE_LOSS_LINEAR_SVM:
            raise ValueError(f"coordinate {coordinate_id}: matrix factorization does not support the smoothed hinge "
                             f"loss (TRON needs a twice differentiable loss)")
        if prior is not None:
            raise ValueError(f"coordinate {coordinate_id}: a prior model (incremental training) is not supported for "
                             f"matrix factorization")
        if is_dist():
            raise ValueError(f"coordinate {coordinate_id}: matrix factorization is not supported under a process group")
        for tag in (data_config.row_effect_type, data_config.col_effect_type):
            if tag not in data.id_tags:
                raise ValueError(f"coordinate {coordinate_id}: id tag {tag} missing from the data (have "
                                 f"{sorted(data.id_tags)})")
        self.set_config(opt_config)                 # raises on what the coordinate cannot combine with
        self.K = K
        self.loss = loss_for_task(self.task)
        dev = self.device
        self.row_ids, a = np.unique(_id_keys(data.id_tags[data_config.row_effect_type]), return_inverse=True)
        self.col_ids, b = np.unique(_id_keys(data.id_tags[data_config.col_effect_type]), return_inverse=True)
        a, b = a.reshape(-1).astype(np.int64), b.reshape(-1).astype(np.int64)
        y = torch.from_numpy(np.asarray(data.response, dtype=np.float64)).to(dev)
        wt = torch.from_numpy(np.asarray(data.weights, dtype=np.float64)).to(dev)
        self.base_offsets = torch.from_numpy(np.asarray(data.offsets, dtype=np.float64)).to(dev)
        self.sides = (_Side(a, b, len(self.row_ids), y, wt, dev), _Side(b, a, len(self.col_ids), y, wt, dev))
        self.codes = (torch.from_numpy(a.astype(np.int32)).to(dev), torch.from_numpy(b.astype(np.int32)).to(dev))
        self.n_rows = int(y.numel())
        self._scr = None
        self._returned = None          # (model, scores) of the last update: its scores came out of the solve
        self._half_raw = []            # (iterations, reasons, seconds) of every half of the last update
        self.last_passes = None        # GPU: (row passes, TRON iterations) summed over the last update's entities

    # The tracker statistics are reduced on first read (a device synchronisation), as the random-effect
    # coordinate's are: off the coordinate-descent critical path unless someone looks at them.
    @property
    def half_stats(self) -> list:
        """``random_effect_tracker_stats`` of every half of the last update (row, column, row, ...)."""
        return [random_effect_tracker_stats(*h) for h in self._half_raw]

    @property
    def last_stats(self) -> dict:
        return random_effect_tracker_stats(*self._half_raw[-1]) if self._half_raw else {}

    def solve_half(self, side: int, U: torch.Tensor, V: torch.Tensor, partial_score: Optional[torch.Tensor] = None):
        """One half-update from the factors (U, V): ``side`` 0 solves every row entity given V, 1 every column entity
        given U. Returns (the solved side's factors, the margins u . v per row in the data's order, iterations,
        reason codes)."""
        off = self.base_offsets if partial_score is None else \
            self.base_offsets + partial_score.detach().to(self.device, torch.float64)
        W0, other = (U, V) if side == 0 else (V, U)
        W, z, it, rs, _ = self._half(side, W0.to(self.device), other.to(self.device), off)
        scores = torch.empty_like(z)
        scores[self.sides[side].perm] = z
        return W, scores, it, rs

    # ---- configuration ---------------------------------------------------------------------------------------
    def set_config(self, opt_config: GLMOptimizationConfiguration):
        """Swap the optimisation configuration (lambda grid, tuning): nothing of the layout depends on it."""
        cid = self.coordinate_id
        oc = opt_config.optimizer_config
        if oc.optimizer_type != OptimizerType.TRON:
            raise ValueError(f"coordinate {cid}: matrix factorization is solved by TRON only (got "
                             f"{oc.optimizer_type.value})")
        if opt_config.regularization_context.regularization_type in (RegularizationType.L1,
                                                                     RegularizationType.ELASTIC_NET):
            raise ValueError(f"coordinate {cid}: matrix factorization supports L2 regularization only (got "
                             f"{opt_config.regularization_context.regularization_type.value})")
        if oc.constraint_map:
            raise ValueError(f"coordinate {cid}: box constraints are not supported for matrix factorization")
        if opt_config.down_sampling_rate != 1.0:
            raise ValueError(f"coordinate {cid}: down-sampling (rate {opt_config.down_sampling_rate}) is not supported "
                             f"for matrix factorization")
        self.opt_config = opt_config

    @property
    def l2(self) -> float:
        cfg = self.opt_config
        return cfg.regularization_context.l2_weight(cfg.regularization_weight)

    # ---- models ----------------------------------------------------------------------------------------------
    def _seeded_v(self) -> torch.Tensor:
        dc = self.data_config
        rng = np.random.default_rng(dc.seed)
        v = rng.normal(0.0, dc.init_std, size=(len(self.col_ids), self.K))
        return torch.from_numpy(v).to(self.device)

    def _model(self, U: torch.Tensor, V: torch.Tensor) -> MatrixFactorizationModel:
        dc = self.data_config
        return MatrixFactorizationModel(dc.row_effect_type, dc.col_effect_type, self.task, self.row_ids, self.col_ids,
                                        U, V)

    def initialize_model(self) -> MatrixFactorizationModel:
        U = torch.zeros(len(self.row_ids), self.K, dtype=torch.float64, device=self.device)
        return self._model(U, self._seeded_v())

    def _own(self, model: MatrixFactorizationModel) -> bool:
        return model.row_ids is self.row_ids and model.col_ids is self.col_ids and model.num_factors == self.K

    def _factors_of(self, model: Optional[MatrixFactorizationModel]):
        """(U, V) on this coordinate's entity tables. A model the coordinate did not produce (a loaded model, a warm
        start from other data) is mapped by entity id; entities absent from it start at 0 on the row side and at
        their seeded draw on the column side."""
        if model is None:
            model = self.initialize_model()
        if not isinstance(model, MatrixFactorizationModel):
            raise ValueError(f"coordinate {self.coordinate_id}: expected a MatrixFactorizationModel, got "
                             f"{type(model).__name__}")
        if self._own(model):
            return model.U.to(self.device), model.V.to(self.device)
        if model.num_factors != self.K:
            raise ValueError(f"coordinate {self.coordinate_id}: the model has {model.num_factors} factors, the "
                             f"coordinate {self.K}")
        U = torch.zeros(len(self.row_ids), self.K, dtype=torch.float64, device=self.device)
        V = self._seeded_v()
        for tab, ids, src_ids, src in ((U, self.row_ids, model.row_ids, model.U), (V, self.col_ids, model.col_ids,
                                                                                  model.V)):
            pos = entity_codes(src_ids, ids)
            have = np.nonzero(pos >= 0)[0]
            if len(have):
                tab[torch.from_numpy(have).to(self.device)] = src.to(self.device)[
                    torch.from_numpy(pos[have].astype(np.int64)).to(self.device)]
        return U, V

    # ---- one half-update -------------------------------------------------------------------------------------
    def _half(self, s: int, W0: torch.Tensor, other: torch.Tensor, off: torch.Tensor):
        """Solve every entity of side ``s`` (0 = rows) given the other side's factors. Returns (W, margins per
        SORTED row, iterations, reasons, row passes or None)."""
        side = self.sides[s]
        oc = self.opt_config.optimizer_config
        off_s = off[side.perm].contiguous()
        if self.device.type == "cuda":
            return self._half_device(side, W0, other, off_s, oc)
        F = other[side.oid.long()]                                   # the materialised features, fp64
        W = W0.clone()
        z = torch.zeros(self.n_rows, dtype=torch.float64)
        iters = torch.zeros(side.n_entities, dtype=torch.long)
        reasons = torch.zeros(side.n_entities, dtype=torch.long)
        for ents, idx, mask in side.classes():
            X = torch.where(mask.unsqueeze(-1), F[idx], torch.zeros((), dtype=torch.float64))
            wz = torch.where(mask, side.wt[idx], torch.zeros((), dtype=torch.float64))
            bd = BatchedGLMData(X, side.y[idx], off_s[idx], wz)
            res = batched_tron(bd, self.loss, self.l2, W0[ents], oc.tolerance, oc.maximum_iterations)
            W[ents] = res.W
            iters[ents], reasons[ents] = res.iters, res.reason
            z[idx[mask]] = torch.bmm(X, res.W.unsqueeze(-1)).squeeze(-1)[mask]
        return W, z, iters, reasons, None

    def _half_device(self, side: _Side, W0, other, off_s, oc):
        from ..ops import native
        dev, K, n, B = self.device, self.K, self.n_rows, side.n_entities
        W = W0.to(torch.float64).reshape(-1).contiguous().clone()
        f = torch.empty(B, dtype=torch.float64, device=dev)
        iters = torch.empty(B, dtype=torch.int32, device=dev)
        reasons = torch.empty(B, dtype=torch.int32, device=dev)
        npass = torch.zeros(B, dtype=torch.int32, device=dev)
        z = torch.empty(n, dtype=torch.float64, device=dev)
        if self._scr is None:
            self._scr = torch.empty(4 * max(n, 1), dtype=torch.float64, device=dev)
        other = other.to(torch.float64).contiguous()
        if fused_route():
            native.mf_tron(side.order, side.row_ptr, side.oid, other, side.y, off_s, side.wt, self._scr, W, f, iters,
                           reasons, z, K, self.loss.loss_id, self.l2, oc.tolerance, oc.maximum_iterations, npass=npass)
        else:
            # the already tested tall kernel over a materialised copy of the gathered rows (dense CSR rows)
            val = other[side.oid.long()].reshape(-1).contiguous()
            ar = lambda k, step: torch.arange(k + 1, dtype=torch.int64, device=dev) * step
            lcol = torch.arange(K, dtype=torch.int16, device=dev).repeat(n)
            native.re_tron_csr(side.order, side.row_ptr, ar(B, K), ar(n, K), lcol, val, side.y, off_s, side.wt,
                               self._scr, W, f, iters, reasons, z, self.loss.loss_id, self.l2, oc.tolerance,
                               oc.maximum_iterations, 5, 20, 16 if K <= 16 else 32, npass=npass, hessian=True)
        return W.view(B, K), z, iters.to(torch.long), reasons.to(torch.long), npass

    # ---- Coordinate interface --------------------------------------------------------------------------------
    def update_model(self, model: Optional[MatrixFactorizationModel], partial_score: Optional[torch.Tensor] = None):
        U, V = self._factors_of(model)
        off = self.base_offsets if partial_score is None else \
            self.base_offsets + partial_score.detach().to(self.device, torch.float64)
        raw = []
        passes = iters_total = None
        z, last = None, 0
        for _ in range(self.data_config.alternations):
            for s in (0, 1):
                t0 = time.time()
                W0, other = (U, V) if s == 0 else (V, U)
                W, z, it, rs, npass = self._half(s, W0, other, off)
                if s == 0:
                    U = W
                else:
                    V = W
                last = s
                if npass is not None:
                    passes = npass.sum() if passes is None else passes + npass.sum()
                    iters_total = it.sum() if iters_total is None else iters_total + it.sum()
                raw.append((it, rs, time.time() - t0))
                if log.isEnabledFor(logging.INFO):
                    log.info("MF %s %s half: %s", self.coordinate_id, "row" if s == 0 else "column",
                             random_effect_tracker_stats(*raw[-1]))
        self._half_raw = raw
        self.last_passes = None if passes is None else (passes, iters_total)
        out = self._model(U, V)
        if self.device.type == "cuda":
            # the margins of the solution came out of the last half's solve, in that side's sorted row order
            scores = torch.empty_like(z)
            scores[self.sides[last].perm] = z
        else:
            scores = pair_scores(U, V, self.codes[0], self.codes[1])
        self._returned = (out, scores)
        return out

    def score(self, model: MatrixFactorizationModel) -> torch.Tensor:
        if self._returned is not None and self._returned[0] is model:
            return self._returned[1]
        if self._own(model):
            return pair_scores(model.U.to(self.device), model.V.to(self.device), self.codes[0], self.codes[1])
        return model.score(self.data, self.device)

    def regularization_term_value(self, model: MatrixFactorizationModel) -> float:
        if self.l2 == 0:
            return 0.0
        return 0.5 * self.l2 * (float(model.U.square().sum()) + float(model.V.square().sum()))
