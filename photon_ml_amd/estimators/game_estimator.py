"""Estimator API: GameEstimator (fit), GameTransformer (score), and the legacy GLM lambda-path trainer.

Reference:
  * ``photon-api/.../estimators/GameEstimator.scala:56-753`` — params (training task, input column names,
    coordinate data configurations, update sequence, CD iterations (default 1), normalization contexts,
    compute variance (false), tree aggregate depth (1), validation evaluators, warm start (true)); ``fit`` trains
    one GAME model per optimisation configuration in sequence, warm-starting from the previous one.
  * ``photon-api/.../transformers/GameTransformer.scala:38-308`` — score a dataset with a GameModel, optionally
    evaluate.
  * ``photon-api/.../ModelTraining.scala:35-234`` — legacy GLM training over a lambda grid sorted DESCENDING,
    each lambda warm-started from the previous model.

Datasets are built ONCE per ``fit`` (device-resident shards / buckets) and reused across configurations; a new
configuration only swaps the optimisation problem of each coordinate.
"""
from __future__ import annotations

import logging
import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..algorithm.coordinate_descent import CoordinateDescent
from ..algorithm.coordinates import FixedEffectCoordinate, RandomEffectCoordinate, ShardedRandomEffectCoordinate
from ..constants import RANDOM_SEED, TaskType, VarianceComputationType
from ..data.game_data import GameData
from ..data.matrix import LabeledData
from ..data.random_effect import (FixedEffectDataConfiguration, MatrixFactorizationDataConfiguration,
                                  RandomEffectDataConfiguration)
from ..evaluation.evaluators import (build_evaluator, default_validation_evaluator, parse_evaluator_type,
                                     training_loss_evaluator_type)
from ..models.game import GameModel
from ..normalization.context import NormalizationContext, NormalizationType
from ..ops.backend import default_device, make_glm_data
from ..optimization.config import (GLMOptimizationConfiguration, OptimizerConfig, OptimizerType,
                                   RegularizationContext)
from ..optimization.problem import GLMOptimizationProblem
from ..parallel.dist import DistributedGLMData, is_dist
from ..stat.summary import BasicStatisticalSummary

log = logging.getLogger(__name__)

DEFAULT_TREE_AGGREGATE_DEPTH = 1


@dataclass
class GameResult:
    model: GameModel
    evaluations: Optional[list]
    config: Dict[str, GLMOptimizationConfiguration]


class GameEstimator:
    def __init__(self, device=None, precision: str = "f64"):
        self.training_task: Optional[TaskType] = None
        self.coordinate_data_configurations: "OrderedDict[str, object]" = OrderedDict()
        self.coordinate_update_sequence: Optional[List[str]] = None
        self.coordinate_descent_iterations = 1
        self.coordinate_normalization_contexts: Dict[str, NormalizationContext] = {}
        self.normalization_type = NormalizationType.NONE          # see set_normalization
        self.intercept_indices_by_shard: Dict[str, Optional[int]] = {}
        self.collect_statistics = False
        self.normalize_random_effects = False                     # see set_random_effect_normalization
        self.feature_statistics: Dict[str, BasicStatisticalSummary] = {}   # by feature shard id, filled by fit
        self.coordinates_built_callback = None
        self.variance_computation_type = VarianceComputationType.NONE   # compute_variance: its boolean view
        self.tree_aggregate_depth = DEFAULT_TREE_AGGREGATE_DEPTH
        self.validation_evaluators: Optional[List[str]] = None
        self.use_warm_start = True
        self.device = torch.device(device) if device is not None else default_device()
        self.precision = precision
        self.event_callback = None
        self.coordinates = None
        self.history: List[list] = []
        self.checkpoint_directory: Optional[str] = None
        self.resume = False
        self.prior_model: Optional[GameModel] = None

    # fluent setters mirroring Spark ML Params ------------------------------------------------------------
    def set_training_task(self, t):
        self.training_task = TaskType.parse(t)
        return self

    def set_coordinate_data_configurations(self, cfgs):
        self.coordinate_data_configurations = OrderedDict(cfgs)
        return self

    def set_coordinate_update_sequence(self, seq):
        self.coordinate_update_sequence = list(seq)
        return self

    def set_coordinate_descent_iterations(self, n: int):
        if n <= 0:
            raise ValueError("coordinate descent iterations must be > 0")
        self.coordinate_descent_iterations = n
        return self

    def set_coordinate_normalization_contexts(self, ctxs):
        self.coordinate_normalization_contexts = dict(ctxs)
        return self

    def set_normalization(self, normalization_type, intercept_indices_by_shard=None,
                          collect_statistics: bool = False):
        """Ask for normalization by TYPE: every fixed-effect coordinate without an explicit context
        (:meth:`set_coordinate_normalization_contexts` wins per coordinate) gets a ``NormalizationContext`` built
        from the statistics of the shard the estimator has just put on the device — taken from the device when
        that shard is tiled, on a GPU and stored in fp64 (``BasicStatisticalSummary.for_shard``), computed on the
        host otherwise, all-reduced under a process group. ``intercept_indices_by_shard``: feature shard id ->
        intercept index (or None). ``collect_statistics``: compute and keep the statistics even when the type is
        NONE (a data summary without normalization). They stay readable in ``feature_statistics`` by shard id, and
        ``coordinates_built_callback(estimator)`` runs as soon as every coordinate is built, before the first
        update. Random-effect coordinates ignore normalization unless
        :meth:`set_random_effect_normalization` switches it on."""
        self.normalization_type = NormalizationType.parse(normalization_type)
        self.intercept_indices_by_shard = dict(intercept_indices_by_shard or {})
        self.collect_statistics = bool(collect_statistics)
        return self

    def set_random_effect_normalization(self, b: bool):
        """Normalization for random-effect coordinates too (default False: they ignore it). When on, every
        random-effect coordinate gets a context: the explicit one of :meth:`set_coordinate_normalization_contexts`
        if its id is there, otherwise one built by TYPE (:meth:`set_normalization`) from the statistics of its whole
        feature shard over all rows -- per shard, not per entity -- computed on the host. Each entity's problem is
        then solved in the normalized space (penalties on the transformed coefficients) and the model comes back in
        the original space. Not combinable with a prior model on the same coordinate, the RANDOM projector or a
        process group; a type with shifts (STANDARDIZATION) needs an intercept among every trained entity's features
        and supports no coefficient variances (ValueError naming the coordinate, before any training)."""
        self.normalize_random_effects = bool(b)
        return self

    def _random_effect_context(self, data: GameData, cid: str, shard_id: str) -> Optional[NormalizationContext]:
        """The context of random-effect coordinate ``cid`` (None: it ignores normalization)."""
        if not self.normalize_random_effects:
            return None
        explicit = self.coordinate_normalization_contexts.get(cid)
        if explicit is not None:
            return explicit
        if self.normalization_type == NormalizationType.NONE:
            return None
        if is_dist():
            raise ValueError(f"coordinate {cid}: normalization of a random effect is not supported under a process "
                             f"group")
        st = self._coordinate_statistics(data, shard_id, None)       # host path: the shard has no tiled copy
        return NormalizationContext.build(self.normalization_type, st, self.intercept_indices_by_shard.get(shard_id))

    def _coordinate_statistics(self, data: GameData, shard_id: str, glm_data) -> BasicStatisticalSummary:
        if shard_id not in self.feature_statistics:
            from ..utils.timing import Timed
            where = "device" if BasicStatisticalSummary.on_device(glm_data) else "host"
            with Timed(f"Calculate statistics for feature shard {shard_id} ({where})"):
                self.feature_statistics[shard_id] = BasicStatisticalSummary.for_shard(
                    data.shards[shard_id], glm_data, all_reduce=is_dist())
        return self.feature_statistics[shard_id]

    def set_compute_variance(self, b: bool):
        """Legacy switch: True = SIMPLE variances ``1 / (H_jj + EPSILON)``, False = none."""
        self.compute_variance = bool(b)
        return self

    def set_variance_computation_type(self, t):
        """``NONE``, ``SIMPLE`` (``1 / (H_jj + EPSILON)``) or ``FULL`` (``(H^-1)_jj``: per entity for random effects,
        for fixed effects up to 2048 coefficients); see ``constants.VarianceComputationType``."""
        self.variance_computation_type = VarianceComputationType.parse(t)
        return self

    @property
    def compute_variance(self) -> bool:
        return self.variance_computation_type != VarianceComputationType.NONE

    @compute_variance.setter
    def compute_variance(self, b):
        self.variance_computation_type = VarianceComputationType.parse(b)

    def set_tree_aggregate_depth(self, d: int):
        if d <= 0:
            raise ValueError("tree aggregate depth must be > 0")
        self.tree_aggregate_depth = d
        # the reduction-shape knob maps to the RCCL all-reduce algorithm (depth >= 2 -> tree, else RCCL's choice)
        from ..parallel.dist import set_allreduce_algo
        set_allreduce_algo(tree_depth=d)
        return self

    def set_validation_evaluators(self, evs):
        self.validation_evaluators = [e if isinstance(e, str) else e.name for e in evs]
        return self

    def set_entity_placement(self, coordinate: Optional[str] = "auto"):
        """Multi-GPU only: place every training row on the owner of its entity in one random-effect coordinate at
        the start of ``fit`` (parallel/placement.py), so that coordinate needs no per-update routing and the fixed
        effects train on the placed rows. ``"auto"``: the first random-effect coordinate of the update sequence;
        None: no placement (every random-effect coordinate routes its rows)."""
        self.entity_placement = coordinate
        return self

    def set_warm_start(self, b: bool):
        self.use_warm_start = bool(b)
        return self

    def set_initial_model(self, model: Optional[GameModel]):
        """Start the first configuration from a saved model (e.g. ``load_game_model``) instead of zeros; the
        reference has no such option (warm start only in-process)."""
        self.initial_model = model
        return self

    def set_prior_model(self, model: Optional[GameModel]):
        """Incremental training: use a saved model (e.g. ``load_game_model`` of yesterday's run, with variances) as a
        Gaussian prior. Every coordinate the model holds trains with ``lambda/2 sum_j (w_j - mu_j)^2 / sigma_j^2`` in
        place of its L2 term, ``mu`` / ``sigma^2`` the prior's means / variances (per entity and feature for a random
        effect); a coefficient without a prior (a new entity or feature, a model saved without variances) keeps ``mu
        = 0`` resp. ``sigma^2 = 1``, i.e. plain L2, as do coordinates absent from the model. Separate from
        :meth:`set_initial_model`, which only chooses the starting point. Entities present only in the prior model
        are not carried into the trained model, and the prior term has no weight of its own beyond ``lambda``."""
        self.prior_model = model
        return self

    def _prior_for(self, cid: str, random_effect: bool):
        from ..models.game import FixedEffectModel, RandomEffectModel
        m = None if self.prior_model is None else self.prior_model.get(cid)
        if isinstance(self.coordinate_data_configurations.get(cid), MatrixFactorizationDataConfiguration):
            return m       # the coordinate refuses any prior, with its name
        if m is not None and not isinstance(m, RandomEffectModel if random_effect else FixedEffectModel):
            raise ValueError(f"coordinate {cid}: the prior model holds a {type(m).__name__} for it")
        return m

    def set_checkpoint_directory(self, directory: Optional[str], resume: bool = False):
        """Checkpoint coordinate descent after every coordinate update (one state file per configuration and
        rank); with ``resume`` an interrupted fit continues where it stopped (see utils/checkpoint.py)."""
        self.checkpoint_directory = directory
        self.resume = bool(resume)
        return self

    # ----------------------------------------------------------------------------------------------------
    def validate_params(self):
        if self.training_task is None:
            raise ValueError("training task is required")
        if not self.coordinate_data_configurations:
            raise ValueError("coordinate data configurations are required")
        seq = self.coordinate_update_sequence or list(self.coordinate_data_configurations)
        missing = [c for c in seq if c not in self.coordinate_data_configurations]
        if missing:
            raise ValueError(f"coordinates {missing} in the update sequence have no data configuration")
        return seq

    def _build_coordinates(self, data: GameData, first_cfg: Dict[str, GLMOptimizationConfiguration], seq):
        from ..ops.warmup import runtime_warmup
        from ..utils.timing import Timed
        dev = self.device if self.device is not None else default_device()
        with Timed("Device runtime warm-up (first kernel launches of the process)"):
            self.runtime_warmup_s = runtime_warmup(dev)
        coords = OrderedDict()
        # the first random-effect shard built after a fixed-effect coordinate is copied to the device while the GPU
        # builds the fixed-effect layout (a host CSR shard no fixed effect reads; GPU only)
        fe_shards = {dc.feature_shard_id for dc in self.coordinate_data_configurations.values()
                     if isinstance(dc, FixedEffectDataConfiguration)}
        seen_fe = False
        for cid in seq:
            dc = self.coordinate_data_configurations[cid]
            if isinstance(dc, MatrixFactorizationDataConfiguration):
                continue                       # no feature shard
            if not isinstance(dc, RandomEffectDataConfiguration):
                seen_fe = True
            elif seen_fe and dc.feature_shard_id not in fe_shards:
                data.prefetch_shard(dc.feature_shard_id, dev)
                break
        for cid in seq:
            dc = self.coordinate_data_configurations[cid]
            oc = first_cfg[cid]
            if isinstance(dc, MatrixFactorizationDataConfiguration):
                from ..algorithm.matrix_factorization import MatrixFactorizationCoordinate
                if self.compute_variance or cid in self.coordinate_normalization_contexts \
                        or self.normalization_type != NormalizationType.NONE:
                    log.info("coordinate %s: normalization and variance settings do not apply to matrix factorization "
                             "(no features, no variances)", cid)
                coords[cid] = MatrixFactorizationCoordinate(cid, data, dc, oc, self.training_task, self.device,
                                                            prior=self._prior_for(cid, False))
            elif isinstance(dc, RandomEffectDataConfiguration):
                cls = ShardedRandomEffectCoordinate if is_dist() else RandomEffectCoordinate
                coords[cid] = cls(cid, data, dc, oc, self.training_task, self.variance_computation_type, self.device,
                                  prior=self._prior_for(cid, True),
                                  normalization=self._random_effect_context(data, cid, dc.feature_shard_id))
            else:
                explicit = self.coordinate_normalization_contexts.get(cid)
                prior = self._prior_for(cid, False)
                if prior is not None and explicit is None and self.normalization_type != NormalizationType.NONE:
                    raise ValueError(f"coordinate {cid}: {self.normalization_type.value} normalization cannot be "
                                     f"combined with a prior model on the same coordinate (the two transforms are not "
                                     f"composed)")
                co = coords[cid] = FixedEffectCoordinate(cid, data, dc, oc, self.training_task, explicit,
                                                         self.variance_computation_type, self.device,
                                                         self.precision, prior=prior)
                by_type = explicit is None and self.normalization_type != NormalizationType.NONE
                if by_type or self.collect_statistics:
                    st = self._coordinate_statistics(data, co.shard_id, co.glm_data)
                    if by_type:
                        co.normalization = NormalizationContext.build(
                            self.normalization_type, st, self.intercept_indices_by_shard.get(co.shard_id))
                        co.set_config(oc)
        return coords

    def _place(self, data: GameData, seq) -> GameData:
        """Entity-aligned placement of the training rows (see :meth:`set_entity_placement`)."""
        want = getattr(self, "entity_placement", "auto")
        if not is_dist() or want is None:
            return data
        re_cids = [c for c in seq if isinstance(self.coordinate_data_configurations[c], RandomEffectDataConfiguration)]
        cid = re_cids[0] if want == "auto" and re_cids else want
        if cid not in re_cids:
            return data
        from ..parallel.placement import place_rows_by_entity
        re_type = self.coordinate_data_configurations[cid].random_effect_type
        if getattr(getattr(data, "placement", None), "re_type", None) == re_type:
            return data
        dev = self.device if self.device is not None else default_device()
        return place_rows_by_entity(data, re_type, dev)

    def _validation_evaluators(self, validation: GameData):
        names = self.validation_evaluators or [default_validation_evaluator(self.training_task)]
        # per-group metrics (AUC:tag, AUPR:tag, PRECISION@k:tag) live on the training device: their kernels read the
        # scores where score_rows_kernel wrote them; the simple evaluators keep their placement, except plain AUC /
        # AUPR under a process group on a GPU: their bucket exchange and counts run where the scores are
        dev = self.device if self.device is not None else default_device()
        types = [parse_evaluator_type(n) for n in names]
        return [build_evaluator(t, validation.response, validation.offsets, validation.weights, validation.id_tags,
                                device=dev if _evaluates_on(t, dev) else None) for t in types]

    def fit(self, data: GameData, validation: Optional[GameData],
            configurations: Sequence[Dict[str, GLMOptimizationConfiguration]]) -> List[GameResult]:
        seq = self.validate_params()
        if not configurations:
            raise ValueError("at least one optimization configuration is required")
        for cfg in configurations:
            missing = [c for c in seq if c not in cfg]
            if missing:
                raise ValueError(f"optimization configuration missing coordinates {missing}")
        data = self._place(data, seq)
        self.feature_statistics = {}
        self.coordinates = self._build_coordinates(data, configurations[0], seq)
        if self.coordinates_built_callback is not None:
            self.coordinates_built_callback(self)
        train_eval = build_evaluator(training_loss_evaluator_type(self.training_task), data.response, data.offsets,
                                     data.weights)
        val_evals = self._validation_evaluators(validation) if validation is not None else []
        if val_evals:
            # random-guess baseline of every validation metric (GameEstimator.scala:496-500)
            gen = torch.Generator().manual_seed(RANDOM_SEED)
            rnd = torch.rand(validation.n_rows, generator=gen, dtype=torch.float64)
            for e in val_evals:
                log.info("Random guessing based baseline evaluation metric for %s: %s", e.name,
                         e.evaluate(rnd))
        results, prev = [], getattr(self, "initial_model", None)
        for i, cfg in enumerate(configurations):
            for cid, c in self.coordinates.items():
                c.set_config(cfg[cid])
            cd = CoordinateDescent(self.coordinates, train_eval, validation, val_evals,
                                   event_callback=self.event_callback)
            ck, tag = None, ""
            if self.checkpoint_directory:
                from ..utils.checkpoint import Checkpointer
                import json as _json
                ck = Checkpointer(self.checkpoint_directory, f"cd-state-{i}")
                tag = _json.dumps({c: cfg[c].to_json() for c in sorted(cfg)}, sort_keys=True)
                if not self.resume and ck.exists():
                    os.remove(ck.path)
            model, evals = cd.run(self.coordinate_descent_iterations, prev if (self.use_warm_start or i == 0) else None, ck,
                                  tag)
            self.history.append(cd.history)
            results.append(GameResult(model, evals, cfg))
            if self.use_warm_start:
                prev = model
        return results


def _evaluates_on(etype, device) -> bool:
    """Whether the evaluator ``etype`` is built on the scoring ``device``: the per-group metrics always, plain AUC
    and AUPR under a process group with a GPU device (single-process placement of the simple evaluators is
    unchanged)."""
    if etype.is_multi:
        return True
    return (etype.name in ("AUC", "AUPR") and device is not None and torch.device(device).type == "cuda"
            and is_dist())


class GameTransformer:
    def __init__(self, model: GameModel, validation_evaluators: Optional[Sequence[str]] = None, device=None):
        """``device`` defaults to the current GPU (the HIP scoring kernels, K5/K6) and to the CPU without one."""
        self.model = model
        self.validation_evaluators = list(validation_evaluators or [])
        self.device = torch.device(device) if device is not None else default_device()

    def transform(self, data: GameData):
        """Return (scores WITHOUT offsets, evaluations or None)."""
        return self._evaluate(data, self.model.score(data, self.device), self.device)

    def _evaluate(self, data: GameData, scores, multi_device=None):
        """``multi_device``: where the per-group evaluators (and, under a process group on a GPU, plain AUC / AUPR)
        live (None: with the labels, on the host)."""
        evals = None
        if self.validation_evaluators:
            evals = []
            for n in self.validation_evaluators:
                t = parse_evaluator_type(n)
                e = build_evaluator(t, data.response, data.offsets, data.weights, data.id_tags,
                                    device=multi_device if _evaluates_on(t, multi_device) else None)
                evals.append((e, e.evaluate(scores)))
        return scores, evals

    def transform_spilled(self, data: GameData, path: str, chunk_rows: int = 1 << 24):
        """:meth:`transform` for score sets that should not stay resident (``--spill-scores-to-disk``; the
        reference persists the scores RDD with MEMORY_AND_DISK, ``GameScoringDriver.scala:55-70``): rows are
        scored ``chunk_rows`` at a time on the device and each chunk goes straight into a memory-mapped fp64 file
        at ``path`` (``.npy``), so device memory holds one chunk of scores and the host keeps only pages the OS
        chooses to. Returns (CPU tensor over the mapped file, evaluations)."""
        n = data.n_rows
        mm = np.lib.format.open_memmap(path, mode="w+", dtype=np.float64, shape=(n,))
        for lo in range(0, n, chunk_rows):
            hi = min(n, lo + chunk_rows)
            sub = data if (lo == 0 and hi == n) else data.subset(np.arange(lo, hi))
            mm[lo:hi] = self.model.score(sub, self.device).detach().to("cpu", torch.float64).numpy()
            del sub
        mm.flush()
        return self._evaluate(data, torch.from_numpy(mm))


# --------------------------------------------------------------------------------------------------------------
def train_generalized_linear_model(data: LabeledData, task, optimizer_type="LBFGS",
                                   regularization: RegularizationContext = RegularizationContext("L2"),
                                   regularization_weights: Sequence[float] = (10.0,),
                                   normalization: Optional[NormalizationContext] = None, max_iterations: int = 80,
                                   tolerance: float = 1e-6, constraint_map=None, warm_start_models=None,
                                   use_warm_start: bool = True, compute_variance: bool = False, device=None,
                                   precision: str = "f64", glm_data=None, feature_sharded: bool = False):
    """ModelTraining.trainGeneralizedLinearModel -> list of (lambda, model, tracker), lambdas DESCENDING.

    ``feature_sharded``: under a process group, shard the optimizer state over features instead of replicating
    it (``parallel/feature_sharding.py``; for models too large to replicate). ``compute_variance``: a boolean (True =
    SIMPLE) or a ``VarianceComputationType``; FULL needs at most 2048 coefficients and replicated optimizer state
    (ValueError before any training otherwise)."""
    if VarianceComputationType.parse(compute_variance) == VarianceComputationType.FULL and feature_sharded:
        raise ValueError("FULL variances are not supported with feature-sharded optimizer state")
    device = torch.device(device) if device is not None else default_device()
    gdata = glm_data if glm_data is not None else make_glm_data(data, device, precision)
    view = DistributedGLMData(gdata) if is_dist() and not feature_sharded else gdata
    lams = sorted(regularization_weights, reverse=True)
    out = []
    prev = None
    for lam in lams:
        cfg = GLMOptimizationConfiguration(OptimizerConfig(optimizer_type, max_iterations, tolerance, constraint_map),
                                           regularization, lam)
        prob = GLMOptimizationProblem(cfg, task, normalization, compute_variance, feature_sharded=feature_sharded)
        init = None
        if warm_start_models and lam in warm_start_models:
            init = warm_start_models[lam]
        elif use_warm_start and prev is not None:
            init = prev
        model = prob.run(view, init, dim=gdata.dim)
        out.append((lam, model, prob.tracker))
        prev = model
    return out
