"""Worker body of the two-rank (gloo, CPU) incremental-training test in test_incremental.py: one entity-sharded GAME
fit with a prior model; also the shared problem definition the single-process reference uses."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def problem():
    """(training data, prior GameModel): squared loss, 1600 rows, 40 users. The prior is yesterday's model in the
    realistic sense: the truth plus a perturbation of 0.02 per coefficient, for the fixed effect and for 30 of the 40
    users on 5 of their 6 features, with variances in [0.25, 4]. Low noise (1e-3) and a prior near the optimum keep the
    objective small at the solution: a solver that runs until f stops changing pins w to ~sqrt(eps f / h), and the
    comparison at 1e-8 absolute needs that well below 1e-8 (at f ~ 1e3 it is ~1e-8 itself, prior or not)."""
    import scipy.sparse as sp
    from photon_ml_amd.data.game_data import GameData
    from photon_ml_amd.models.game import FixedEffectModel, GameModel, RandomEffectModel
    from photon_ml_amd.models.glm import Coefficients, model_for_task
    rng = np.random.default_rng(23)
    n, n_users, dg, du = 1600, 40, 10, 6
    users = rng.integers(0, n_users, n)
    xg = rng.normal(size=(n, dg)) * (rng.random((n, dg)) < 0.5)
    xu = rng.normal(size=(n, du)) * (rng.random((n, du)) < 0.6)
    xg[:, -1] = xu[:, -1] = 1.0
    wg, wu = rng.normal(size=dg), rng.normal(size=(n_users, du)) * 0.8
    y = xg @ wg + np.einsum("ij,ij->i", xu, wu[users]) + 1e-3 * rng.normal(size=n)
    names = np.array([f"u{u:02d}" for u in range(n_users)])
    data = GameData(y, {"global": sp.csr_matrix(xg), "user": sp.csr_matrix(xu)},
                    {"userId": names[users].astype(object)})
    fe = FixedEffectModel(model_for_task("LINEAR_REGRESSION", Coefficients(
        torch.from_numpy(wg + 0.02 * rng.normal(size=dg)), torch.from_numpy(rng.uniform(0.25, 4.0, dg)))), "global")
    keys = (np.arange(30)[:, None] * du + np.arange(du - 1)[None, :]).reshape(-1)
    mu = (wu[:30, :du - 1] + 0.02 * rng.normal(size=(30, du - 1))).reshape(-1)
    re = RandomEffectModel("userId", "user", "LINEAR_REGRESSION", names[:30], du, keys, mu,
                           rng.uniform(0.25, 4.0, keys.size))
    return data, GameModel(OrderedDict([("global", fe), ("per-user", re)]))


def configuration():
    from photon_ml_amd.optimization.config import GLMOptimizationConfiguration, OptimizerConfig, RegularizationContext
    # tolerance 0: every solve runs until the objective stops changing at all (squared loss: a few TRON iterations), so
    # the one- and two-process fits differ by rounding only, not by where "function values converged" fired
    cfg = GLMOptimizationConfiguration(OptimizerConfig("TRON", 60, 0.0), RegularizationContext("L2"), 1.0)
    return {"global": cfg, "per-user": cfg}


def estimator(prior):
    from photon_ml_amd.data.random_effect import FixedEffectDataConfiguration, RandomEffectDataConfiguration
    from photon_ml_amd.estimators.game_estimator import GameEstimator
    return (GameEstimator(device="cpu").set_training_task("LINEAR_REGRESSION")
            .set_coordinate_data_configurations({"global": FixedEffectDataConfiguration("global"),
                                                 "per-user": RandomEffectDataConfiguration("userId", "user")})
            .set_coordinate_update_sequence(["global", "per-user"]).set_coordinate_descent_iterations(3)
            .set_prior_model(prior))


def main(rank, world, port, out):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                       "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank), "PML_BACKEND": "torch"})
    from photon_ml_amd.parallel.dist import init_distributed
    init_distributed("gloo")
    data, prior = problem()
    local = data.subset(np.arange(rank, data.n_rows, world))
    model = estimator(prior).fit(local, None, [configuration()])[0].model
    np.save(f"{out}/fe_r{rank}.npy", model.get("global").glm.coefficients.means.numpy())
    users = model.get("per-user")
    ids = np.asarray(users.entity_ids)
    np.savez(f"{out}/re_r{rank}.npz", ids=ids, W=np.stack([users.coefficients_of(e).means.numpy() for e in ids]))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
