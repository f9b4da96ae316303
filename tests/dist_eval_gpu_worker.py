"""End-to-end worker of tests/test_dist_eval_gpu.py: one GAME fit and one ``GameTransformer`` pass on the GPU with the
validation evaluators ``AUC``, ``AUC:userId`` and ``PRECISION@3:userId``, either under a one-rank RCCL group
(``forced``: ``PML_FORCE_DIST=1``, every evaluator on the device, no row gather) or without a group (``plain``).
Every evaluation of plain ``AUC`` is checked here against ``auc_weighted`` on the scores it was given, bitwise; the
test compares what the two modes report.

    python dist_eval_gpu_worker.py MODE OUT
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

NAMES = ["AUC", "AUC:userId", "PRECISION@3:userId"]


def main(mode, out):
    from photon_ml_amd.parallel.dist import init_distributed, is_dist
    init_distributed("nccl" if mode == "forced" else None)
    assert is_dist() == (mode == "forced")
    import torch.distributed as dist
    from multi_eval_cases import same_bits
    from photon_ml_amd.data.game_data import GameData
    from photon_ml_amd.data.random_effect import FixedEffectDataConfiguration, RandomEffectDataConfiguration
    from photon_ml_amd.data.synthetic import generate_game_bench_data
    from photon_ml_amd.estimators.game_estimator import GameEstimator, GameTransformer
    from photon_ml_amd.evaluation import evaluators
    from photon_ml_amd.evaluation.evaluators import AUCEvaluator, auc_weighted
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    raw = generate_game_bench_data(300, 12, re_dim=8, re_nnz=3, fe_dim=60, fe_nnz=5, re_vocab=1 << 12, seed=31,
                                   sizes="powerlaw", max_rows=400)
    data = GameData(raw.response, raw.shards, {"userId": raw.id_tags["entityId"]})

    gathers = []
    orig_gather = evaluators._gather
    evaluators._gather = lambda t: (gathers.append(int(t.numel())), orig_gather(t))[1]
    checked = []
    orig = AUCEvaluator._evaluate

    def checking(self, s):
        v = orig(self, s)
        want = auc_weighted(s.detach().cpu(), self.labels.cpu(), None)
        assert same_bits(np.array([v]), np.array([want])), (v, want)
        checked.append(v)
        return v

    AUCEvaluator._evaluate = checking
    cfg = GLMOptimizationConfiguration(OptimizerConfig("LBFGS", 30, 1e-8), RegularizationContext("L2"), 1.0)
    est = (GameEstimator(device="cuda").set_training_task("LOGISTIC_REGRESSION")
           .set_coordinate_data_configurations({"global": FixedEffectDataConfiguration("global"),
                                                "per-user": RandomEffectDataConfiguration("userId", "entity")})
           .set_coordinate_update_sequence(["global", "per-user"])
           .set_coordinate_descent_iterations(1)
           .set_validation_evaluators(NAMES))
    res = est.fit(data, data, [{"global": cfg, "per-user": cfg}])[0]
    by_name = {e.name: e for e, _ in res.evaluations}
    for name in NAMES[1:]:
        assert by_name[name].last_path == "device" and by_name[name].labels.is_cuda, name
    # plain AUC moves to the device only under a group
    assert by_name["AUC"].labels.is_cuda == (mode == "forced")
    fit_vals = [float(v) for _, v in res.evaluations]
    _, evals = GameTransformer(res.model, NAMES, device="cuda").transform(data)
    for e, _ in evals:
        if e.name != "AUC":
            assert e.last_path == "device", e.name
        assert e.labels.is_cuda == (e.name != "AUC" or mode == "forced"), e.name
    assert len(checked) >= 3 and not gathers, (len(checked), gathers)
    np.save(os.path.join(out, f"{mode}_fit.npy"), np.array(fit_vals))
    np.save(os.path.join(out, f"{mode}_transform.npy"), np.array([float(v) for _, v in evals]))
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    print(f"{mode} ok", flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
