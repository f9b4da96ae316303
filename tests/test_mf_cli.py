"""``game-training`` then ``game-scoring`` with a matrix-factorization coordinate (CPU, a tiny Avro set with two id
columns), the coordinate-configuration syntax and its ``--write-config`` / ``--config-file`` round trip."""
import os

import numpy as np
import pytest

from photon_ml_amd.cli import game_scoring, game_training
from photon_ml_amd.cli.params import (coordinate_configuration_to_string, expand_game_configurations,
                                      load_config_file, parse_args_with_config, parse_coordinate_configuration)
from photon_ml_amd.data.game_data import generate_game_data
from photon_ml_amd.data.random_effect import MatrixFactorizationDataConfiguration
from photon_ml_amd.io.data_writer import write_game_avro
from photon_ml_amd.io.score_io import load_scores
from photon_ml_amd.models.game import MatrixFactorizationModel

SHARDS = ["--feature-shard-configurations", "name=global,feature.bags=features"]
FIXED = "name=fixed,feature.shard=global,optimizer=LBFGS,max.iter=50,tolerance=1e-8,regularization=L2,reg.weights=0.1"
MF = ("name=user-song,row.effect.type=userId,col.effect.type=songId,latent.factors=8,optimizer=TRON,max.iter=20,"
      "tolerance=1e-7,regularization=L2,reg.weights=0.1|1,mf.alternations=2,mf.seed=7")


@pytest.fixture(scope="module")
def avro(tmp_path_factory):
    root = tmp_path_factory.mktemp("mf")
    data, _ = generate_game_data(n_rows=900, n_users=15, n_items=10, seed=5, task="LINEAR_REGRESSION")
    data.id_tags["songId"] = data.id_tags.pop("itemId")
    rng = np.random.default_rng(0)
    u = np.array([int(s[1:]) for s in data.id_tags["userId"]])
    it = np.array([int(s[1:]) for s in data.id_tags["songId"]])
    data.response = data.response + (rng.normal(size=(15, 2))[u] * rng.normal(size=(10, 2))[it]).sum(1)
    tr, va = data.subset(np.arange(700)), data.subset(np.arange(700, 900))
    bags = {"global": "features"}
    for d in (tr, va):
        d.shards = {"global": d.shards["global"]}
    write_game_avro(str(root / "train"), tr, bags, n_files=2)
    write_game_avro(str(root / "val"), va, bags)
    return root


def test_coordinate_configuration_syntax():
    cc = parse_coordinate_configuration(MF)["user-song"]
    dc = cc.data_configuration
    assert isinstance(dc, MatrixFactorizationDataConfiguration) and cc.is_matrix_factorization
    assert not cc.is_random_effect and cc.id_tag_names == ["userId", "songId"]
    assert (dc.row_effect_type, dc.col_effect_type, dc.num_factors, dc.alternations, dc.seed, dc.init_std) == \
        ("userId", "songId", 8, 2, 7, 0.1)
    oc = cc.optimization_configuration
    assert oc.optimizer_config.optimizer_type.value == "TRON" and oc.optimizer_config.maximum_iterations == 20
    assert oc.optimizer_config.tolerance == 1e-7
    assert [c.regularization_weight for c in cc.expand_optimization_configurations()] == [1.0, 0.1]
    both = dict(parse_coordinate_configuration(FIXED))
    both["user-song"] = cc
    assert len(expand_game_configurations(both)) == 2
    # the string form parses back to the same configuration
    again = parse_coordinate_configuration(coordinate_configuration_to_string("user-song", cc))["user-song"]
    assert again == cc
    for bad in (MF.replace("row.effect.type=userId,", ""), MF + ",feature.shard=global",
                MF + ",random.effect.type=userId"):
        with pytest.raises(ValueError, match="matrix-factorization"):
            parse_coordinate_configuration(bad)
    # every other configuration is parsed as before, its errors included
    with pytest.raises(ValueError, match="requires 'feature.shard'"):
        parse_coordinate_configuration("name=x,optimizer=TRON,max.iter=3,tolerance=1e-3")


def _train_args(avro, out):
    return ["--input-data-directories", str(avro / "train"), "--validation-data-directories", str(avro / "val"),
            "--root-output-directory", str(out), "--training-task", "LINEAR_REGRESSION", *SHARDS,
            "--coordinate-configurations", FIXED, "--coordinate-configurations", MF,
            "--coordinate-update-sequence", "fixed,user-song", "--coordinate-descent-iterations", "2",
            "--evaluators", "RMSE", "--output-mode", "ALL", "--device", "cpu"]


def test_training_then_scoring(avro, tmp_path):
    out = tmp_path / "train-out"
    cfg_path = str(tmp_path / "train.yaml")
    parser = game_training.build_parser()
    args = _train_args(avro, out)
    direct = parser.parse_args(args)
    parse_args_with_config(parser, args + ["--write-config", cfg_path])
    assert MF in load_config_file(cfg_path)["coordinate-configurations"]
    from_file = parse_args_with_config(game_training.build_parser(), ["--config-file", cfg_path])
    skip = ("config_file", "write_config")
    assert {k: v for k, v in vars(from_file).items() if k not in skip} == \
        {k: v for k, v in vars(direct).items() if k not in skip}
    driver = game_training.GameTrainingDriver(from_file)
    assert driver.id_tags() == ["songId", "userId"]
    res = driver.run()
    assert len(res["explicit"]) == 2 and res["best"] is not None
    m = res["best"].model.get("user-song")
    assert isinstance(m, MatrixFactorizationModel) and m.num_factors == 8 and len(m.row_ids) == 15
    # the interaction term pays: validation RMSE of the best model against a fixed effect alone
    alone = game_training.GameTrainingDriver(game_training.build_parser().parse_args(
        ["--input-data-directories", str(avro / "train"), "--validation-data-directories", str(avro / "val"),
         "--root-output-directory", str(tmp_path / "alone"), "--training-task", "LINEAR_REGRESSION", *SHARDS,
         "--coordinate-configurations", FIXED, "--coordinate-update-sequence", "fixed",
         "--coordinate-descent-iterations", "1", "--evaluators", "RMSE", "--device", "cpu"])).run()
    assert res["best"].evaluations[0][1] < 0.9 * alone["best"].evaluations[0][1]
    for d in ["best", "models/0", "models/1"]:
        mf = out / d / "matrix-factorization" / "user-song"
        assert (mf / "id-info").read_text().split("\n")[:3] == ["userId", "songId", "8"]
        assert os.path.exists(mf / "row-latent-factors" / "part-00000.avro")
        assert os.path.exists(mf / "col-latent-factors" / "part-00000.avro")
        assert os.path.exists(out / d / "fixed-effect" / "fixed" / "coefficients" / "part-00000.avro")

    sout = tmp_path / "score-out"
    sdriver = game_scoring.GameScoringDriver(game_scoring.build_parser().parse_args(
        ["--input-data-directories", str(avro / "val"), "--root-output-directory", str(sout), *SHARDS,
         "--model-input-directory", str(out / "best"), "--model-id", "m1", "--evaluators", "RMSE", "--device", "cpu"]))
    sres = sdriver.run()
    assert sdriver.id_tags() == ["songId", "userId"]
    recs = load_scores(str(sout / "scores"))
    assert len(recs) == 200
    pred = np.array([r["predictionScore"] for r in recs])
    assert np.allclose(pred, sres["scores"].numpy() + sres["data"].offsets)
    loaded = sdriver.model.get("user-song")
    assert np.array_equal(loaded.U.numpy(), m.U.cpu().numpy()) and np.array_equal(loaded.V.numpy(), m.V.cpu().numpy())
    # the saved fixed effect drops coefficients below the sparsity threshold; the MF factors are exact
    assert abs(sres["evaluations"][0][1] - res["best"].evaluations[0][1]) < 5e-3
