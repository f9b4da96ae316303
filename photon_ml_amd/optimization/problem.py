"""GLM optimisation problems: objective + optimizer + model construction (+ variances).

Reference: ``photon-api/.../optimization/GeneralizedLinearOptimizationProblem.scala:39-174`` (create the model in
the ORIGINAL space from transformed-space coefficients; regularisation term value = L1 part (OWL-QN weight) +
L2 part), ``DistributedOptimizationProblem.scala:43-203`` (variances = 1/(Hdiag + EPSILON), λ updates,
``runWithSampling``) and ``SingleNodeOptimizationProblem.scala``. One class serves the distributed and the
single-node case: the data backend decides where the aggregation runs.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..constants import EPSILON, TaskType, VarianceComputationType
from ..function.losses import loss_for_task
from ..function.objective import GLMObjective
from ..models.glm import Coefficients, GeneralizedLinearModel, model_for_task
from ..normalization.context import NormalizationContext, no_normalization
from .config import GLMOptimizationConfiguration, build_optimizer
from .lbfgs import OWLQN


FULL_VARIANCE_DMAX = 2048      # FULL variances of one GLM: the dense D x D Hessian is built from D products


class GLMOptimizationProblem:
    """``compute_variance``: a :class:`VarianceComputationType` or the legacy boolean (True = SIMPLE). FULL builds the
    dense Hessian from ``D`` Hessian-vector products of the objective on unit vectors (which all-reduce under a
    process group and fold the normalization as every other product does) and inverts it with torch; it is
    supported for ``D <= FULL_VARIANCE_DMAX`` and not with feature-sharded optimizer state (checked by
    :meth:`check_full_variance` as soon as the dimension is known).

    ``prior``: ``(mu, sigma)`` fp64 vectors of a Gaussian prior (incremental training): the penalty becomes ``lambda/2
    sum (w_j - mu_j)^2 / sigma_j^2``. With ``w = mu + sigma v`` that is plain L2 on ``v``; the factor ``sigma`` rides
    the coefficient-side normalization machinery (a factors-only context, ``NormalizationContext.prior_scaling``), so
    the data (possibly bf16 tiles) is not rescaled. The CALLER adds the prior margins ``X mu`` to the data's offsets
    (``FixedEffectCoordinate`` does at build). Not combinable with another normalization, L1 / elastic net, box
    constraints or feature-sharded optimizer state (ValueError here, naming ``name``)."""

    def __init__(self, config: GLMOptimizationConfiguration, task, normalization: Optional[NormalizationContext] = None,
                 compute_variance: bool = False, track_state: bool = True, feature_sharded: bool = False,
                 prior=None, name: str = "fixed effect"):
        self.config = config
        self.prior = None
        if prior is not None:
            from .config import RegularizationType
            rt = config.regularization_context.regularization_type
            if rt in (RegularizationType.L1, RegularizationType.ELASTIC_NET):
                raise ValueError(f"coordinate {name}: {rt.value} regularization cannot be combined with a prior model "
                                 f"(the L1 term lives on w, the optimizer on (w - mu) / sigma)")
            if normalization is not None and not normalization.is_identity:
                raise ValueError(f"coordinate {name}: normalization cannot be combined with a prior model on the same "
                                 f"coordinate (the two transforms are not composed)")
            if feature_sharded:
                raise ValueError(f"coordinate {name}: feature-sharded optimizer state cannot be combined with a prior "
                                 f"model")
            if config.optimizer_config.constraint_map:
                raise ValueError(f"coordinate {name}: box constraints cannot be combined with a prior model")
            mu = torch.as_tensor(prior[0], dtype=torch.float64)
            sigma = torch.as_tensor(prior[1], dtype=torch.float64)
            if mu.shape != sigma.shape or not bool(torch.isfinite(mu).all()):
                raise ValueError(f"coordinate {name}: prior means must be finite and match the standard deviations")
            self.prior = (mu, sigma)
            # sigma = 1 everywhere (a prior model saved without variances): no factors, every fast path stays
            normalization = None if bool((sigma == 1.0).all()) else NormalizationContext.prior_scaling(sigma)
        # optimizer state sharded over features across the process group (parallel/feature_sharding.py); the
        # data passed to run() is then this rank's row shard, not a DistributedGLMData wrapper
        self.feature_sharded = feature_sharded
        self.checkpointer, self.checkpoint_every = None, 1
        self.task = TaskType.parse(task)
        self.loss = loss_for_task(self.task)
        self.normalization = normalization or no_normalization()
        self.variance_type = VarianceComputationType.parse(compute_variance)
        self.compute_variance = self.variance_type != VarianceComputationType.NONE
        if self.variance_type == VarianceComputationType.FULL and feature_sharded:
            raise ValueError("FULL variances are not supported with feature-sharded optimizer state")
        self.track_state = track_state
        reg = config.regularization_context
        lam = config.regularization_weight
        self.objective = GLMObjective(self.loss, reg.l2_weight(lam), self.normalization)
        self.optimizer = build_optimizer(config.optimizer_config, self.normalization, reg, lam, track_state)

    def update_regularization_weight(self, lam: float):
        reg = self.config.regularization_context
        self.config = self.config.with_reg_weight(lam)
        self.objective.l2_weight = reg.l2_weight(lam)
        if isinstance(self.optimizer, OWLQN):
            self.optimizer.l1_weight = reg.l1_weight(lam)

    def check_full_variance(self, dim: int, name: str = "fixed effect"):
        """Raise before any training when FULL variances cannot be computed for a problem of ``dim`` coefficients."""
        if (self.variance_type == VarianceComputationType.FULL and self.loss.twice_differentiable
                and int(dim) > FULL_VARIANCE_DMAX):
            raise ValueError(f"coordinate {name}: FULL variances need D <= {FULL_VARIANCE_DMAX}, got D = {int(dim)}")

    def _variances(self, data, w_t: torch.Tensor) -> torch.Tensor:
        """Transformed-space variances at ``w_t``: SIMPLE = 1 / (H_jj + EPSILON), FULL = (H^-1)_jj."""
        if self.variance_type != VarianceComputationType.FULL:
            if self.prior is not None:
                # H_v,jj = sigma_j^2 h_jj + lambda at the margins of w = mu + sigma v (the offsets hold X mu); the
                # plain diagonal below ignores normalization factors (Appendix C.3), the prior's must count
                sg = self.prior[1].to(w_t)
                h = data.hdiag_sums(self.loss, sg * w_t)
                return 1.0 / (sg * sg * h.to(w_t) + self.objective.l2_weight + EPSILON)
            return 1.0 / (self.objective.hessian_diagonal(data, w_t) + EPSILON)
        from .variance import hessian_full_variance
        d = w_t.numel()
        self.check_full_variance(d)
        H = torch.empty(d, d, dtype=torch.float64, device=w_t.device)
        unit = torch.zeros(d, dtype=torch.float64, device=w_t.device)
        for j in range(d):
            unit[j] = 1.0
            H[:, j] = self.objective.hessian_vector(data, w_t, unit).to(H)
            unit[j] = 0.0
        return hessian_full_variance(0.5 * (H + H.T)).to(w_t.device)

    @property
    def tracker(self):
        return self.optimizer.tracker

    def _device_of(self, data):
        return getattr(data, "device", torch.device("cpu"))

    def run(self, data, initial: Optional[GeneralizedLinearModel] = None, dim: Optional[int] = None
            ) -> GeneralizedLinearModel:
        dev = self._device_of(data)
        d = dim if dim is not None else data.dim
        self.check_full_variance(d)
        w0 = (initial.coefficients.means.to(dev, torch.float64) if initial is not None
              else torch.zeros(d, dtype=torch.float64, device=dev))
        if self.prior is not None:
            if self.prior[0].numel() != d:
                raise ValueError(f"prior model has {self.prior[0].numel()} coefficients, the data {d}")
            if initial is not None:
                w0 = w0 - self.prior[0].to(w0)       # the optimizer divides by sigma: v0 = (w0 - mu) / sigma
        if self.feature_sharded:
            return self._run_feature_sharded(data, w0)
        if self.optimizer.needs_hessian and hasattr(data, "track_hessian"):
            data.track_hessian = True
        if self.checkpointer is not None:
            w_t = self._optimize_checkpointed(data, w0)
        else:
            w_t, _ = self.optimizer.optimize(self.objective, data, w0)
        variances = None
        if self.compute_variance and self.loss.twice_differentiable and self.prior is not None:
            sg = self.prior[1].to(w_t)
            variances = sg * sg * self._variances(data, w_t)         # H_w^-1 = S H_v^-1 S: exact, SIMPLE and FULL
        elif self.compute_variance and self.loss.twice_differentiable:
            variances = self.normalization.model_to_original_space(self._variances(data, w_t))
        means = self.normalization.model_to_original_space(w_t)
        if self.prior is not None:
            means = self.prior[0].to(means) + means                  # w = mu + sigma v
        model = model_for_task(self.task, Coefficients(means.detach(), None if variances is None else variances))
        model.validate_coefficients()
        return model

    def enable_checkpointing(self, checkpointer, every: int = 1):
        """Save the optimizer state every ``every`` iterations (and resume from an existing checkpoint)."""
        self.checkpointer, self.checkpoint_every = checkpointer, max(1, int(every))
        return self

    def _optimize_checkpointed(self, data, w0):
        opt = self.optimizer
        if not self.checkpointer.load_optimizer(opt, device=w0.device):
            opt.start(self.objective, data, w0)
        while not opt.is_done():
            opt.step(self.objective, data)
            if opt.current.iter % self.checkpoint_every == 0:
                self.checkpointer.save_optimizer(opt)
        if opt.tracker is not None:
            opt.tracker.convergence_reason = opt.convergence_reason()
        return opt.current.coefficients

    def _run_feature_sharded(self, data, w0: torch.Tensor) -> GeneralizedLinearModel:
        from ..parallel.feature_sharding import optimize_feature_sharded
        local = getattr(data, "local", data)
        reg = self.config.regularization_context
        opt = build_optimizer(self.config.optimizer_config, None, reg, self.config.regularization_weight,
                              self.track_state)
        self.optimizer = opt
        means, _, sobj = optimize_feature_sharded(opt, self.objective, local, w0, self.normalization)
        variances = None
        if self.compute_variance and self.loss.twice_differentiable:
            from ..parallel.feature_sharding import all_gather_shards
            w_t = self.normalization.model_to_transformed_space(means.clone())
            hd = all_gather_shards(sobj.hessian_diagonal(local, sobj.layout.slice(w_t)), sobj.layout, sobj.group)
            variances = self.normalization.model_to_original_space(1.0 / (hd + EPSILON))
        model = model_for_task(self.task, Coefficients(means.detach(), variances))
        model.validate_coefficients()
        return model

    def regularization_term_value(self, model: GeneralizedLinearModel) -> float:
        w = model.coefficients.means
        reg = self.config.regularization_context
        lam = self.config.regularization_weight
        if self.prior is not None:
            v = (w.to(torch.float64) - self.prior[0].to(w.device)) / self.prior[1].to(w.device)
            return 0.5 * reg.l2_weight(lam) * float(torch.dot(v, v))
        return reg.l1_weight(lam) * float(w.abs().sum()) + 0.5 * reg.l2_weight(lam) * float(torch.dot(w, w))
