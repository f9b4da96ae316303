"""Storage precision of a random-effect coordinate (``RandomEffectDataConfiguration.storage_precision``) on the CPU:
the rounding definition, that training on raw data at a narrow precision is training at ``f64`` on pre-rounded data,
and the configuration checks (dataclass, value range, CLI key)."""
import numpy as np
import pytest
import torch

from photon_ml_amd.data.game_data import GameData
from re_parity_util import TASKS, make_ragged_entities

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
SPEC = [(40, 70, [1, 2, 3, 4, 5]), (30, 300, [16, 65]), (25, 20, [7])]


def rounded(data, precision):
    """``data`` with its feature values pre-rounded by the definition ``v.to(f32).to(dtype).to(f64)``."""
    x = data.shards["user"].tocsr().copy()
    x.data = torch.from_numpy(x.data).to(torch.float32).to(DTYPES[precision]).to(torch.float64).numpy()
    return GameData(data.response, {"user": x}, data.id_tags, offsets=data.offsets, weights=data.weights)


def coordinate(data, precision="f64", name="u", loss="LOGISTIC", device="cpu"):
    from photon_ml_amd.algorithm.coordinates import RandomEffectCoordinate
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration
    from photon_ml_amd.optimization.config import (GLMOptimizationConfiguration, OptimizerConfig,
                                                   RegularizationContext)
    cfg = GLMOptimizationConfiguration(OptimizerConfig("TRON", 6, 1e-8), RegularizationContext("L2"), 1.0)
    return RandomEffectCoordinate(name, data, RandomEffectDataConfiguration("userId", "user",
                                                                            storage_precision=precision),
                                  cfg, TASKS[loss], device=device, layout="segmented")


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_dataset_values_follow_the_rounding_definition(precision):
    data = make_ragged_entities(SPEC, seed=5)
    raw = coordinate(data).dataset._seg_csr[2]
    got = coordinate(data, precision).dataset._seg_csr[2]
    want = raw.to(torch.float32).to(DTYPES[precision]).to(torch.float64)
    assert got.dtype == torch.float64 and torch.equal(got, want) and not torch.equal(got, raw)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_cpu_training_on_raw_equals_f64_on_prerounded(precision):
    data = make_ragged_entities(SPEC, seed=6, loss="POISSON")
    partial = torch.from_numpy(0.3 * np.cos(np.arange(data.n_rows)))
    a = coordinate(data, precision, loss="POISSON")
    b = coordinate(rounded(data, precision), loss="POISSON")
    ma, mb = a.update_model(a.initialize_model(), partial), b.update_model(b.initialize_model(), partial)
    assert torch.equal(a.score(ma), b.score(mb))
    for e in ma.entity_ids:
        assert np.array_equal(ma.coefficients_of(e).means, mb.coefficients_of(e).means), e
    assert a.solver_routing().get("narrow", 0) == 0 and "narrow" not in b.solver_routing()


def test_configuration_is_validated():
    from photon_ml_amd.data.random_effect import RandomEffectDataConfiguration
    assert RandomEffectDataConfiguration("userId", "user").storage_precision == "f64"
    with pytest.raises(ValueError, match="storage precision"):
        RandomEffectDataConfiguration("userId", "user", storage_precision="f16")
    data = make_ragged_entities(SPEC, seed=7)
    x = data.shards["user"].tocsr().copy()
    x.data[3] = 1e39                                   # finite in fp64, infinite in f32
    big = GameData(data.response, {"user": x}, data.id_tags, offsets=data.offsets, weights=data.weights)
    with pytest.raises(ValueError, match="per-user.*not finite"):
        coordinate(big, "f32", name="per-user")
    coordinate(big, "f64", name="per-user")


def test_cli_key_parses_and_round_trips():
    from photon_ml_amd.cli.params import coordinate_configuration_to_string, parse_coordinate_configuration
    base = "name=per-user,feature.shard=user,optimizer=TRON,max.iter=5,tolerance=1e-6,regularization=L2,reg.weights=1"
    re_cfg = base + ",random.effect.type=userId"
    (name, cc), = parse_coordinate_configuration(re_cfg + ",storage.precision=bf16").items()
    assert cc.data_configuration.storage_precision == "bf16"
    text = coordinate_configuration_to_string(name, cc)
    assert "storage.precision=bf16" in text
    assert parse_coordinate_configuration(text)[name].data_configuration.storage_precision == "bf16"
    (_, plain), = parse_coordinate_configuration(re_cfg).items()
    assert plain.data_configuration.storage_precision == "f64"
    assert "storage.precision" not in coordinate_configuration_to_string(name, plain)
    with pytest.raises(ValueError, match="storage precision"):
        parse_coordinate_configuration(re_cfg + ",storage.precision=half")
    with pytest.raises(ValueError, match="per-user"):
        parse_coordinate_configuration(base + ",storage.precision=bf16")
    with pytest.raises(ValueError, match="mf"):
        parse_coordinate_configuration("name=mf,row.effect.type=userId,col.effect.type=itemId,latent.factors=4,"
                                       "optimizer=TRON,max.iter=5,tolerance=1e-6,storage.precision=bf16")
