"""Worker body of the two-process (gloo, CPU) FULL-variance test in test_full_variance.py: a data-parallel fixed
effect plus an entity-sharded random effect trained with ``VarianceComputationType.FULL``."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def worker_data():
    from photon_ml_amd.data.game_data import generate_game_data
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    data, _ = generate_game_data(n_rows=1200, n_users=24, n_items=5, seed=17, task="LOGISTIC_REGRESSION")
    cfg = GLMOptimizationConfiguration(OptimizerConfig("TRON", 50, 1e-10), RegularizationContext("L2"), 1.0)
    return data, {"global": cfg, "per-user": cfg}


def worker_estimator():
    from photon_ml_amd.data.random_effect import FixedEffectDataConfiguration, RandomEffectDataConfiguration
    from photon_ml_amd.estimators.game_estimator import GameEstimator
    return (GameEstimator(device="cpu").set_training_task("LOGISTIC_REGRESSION")
            .set_coordinate_data_configurations({"global": FixedEffectDataConfiguration("global"),
                                                 "per-user": RandomEffectDataConfiguration("userId", "user")})
            .set_coordinate_update_sequence(["global", "per-user"])
            .set_coordinate_descent_iterations(2)
            .set_variance_computation_type("FULL"))


def main(rank, world, port, out):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                       "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank), "PML_BACKEND": "torch"})
    from photon_ml_amd.parallel.dist import init_distributed
    init_distributed("gloo")
    data, cfgs = worker_data()
    local = data.subset(np.arange(rank, data.n_rows, world))
    res = worker_estimator().fit(local, None, [cfgs])[0]
    fe = res.model.get("global").glm.coefficients
    np.save(f"{out}/fe_r{rank}.npy", np.stack([fe.means.numpy(), fe.variances.numpy()]))
    re = res.model.get("per-user")           # this rank's entities only
    part = {}
    for eid in re.entity_ids:
        co = re.coefficients_of(eid)
        part[str(eid)] = [co.means.numpy().tolist(), co.variances.numpy().tolist()]
    with open(f"{out}/re_r{rank}.json", "w") as f:
        json.dump(part, f)
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
