"""ConfigLoader default/fallback semantics (config_loader.rs:66-554)."""
import json
import os

import pytest

from relayrl_prototype_amd.config import (
    DEFAULT_CONFIG_CONTENT,
    REINFORCE_FALLBACK,
    ConfigLoader,
    resolve_config_json_path,
)
from tests import reference_fixtures


@pytest.fixture
def tmpcwd(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("RRL_QUIET_CONFIG", "1")
    return tmp_path


def test_default_file_created_and_parsed(tmpcwd):
    c = ConfigLoader("REINFORCE")  # no path -> ./relayrl_config.json created
    assert (tmpcwd / "relayrl_config.json").exists()
    assert json.loads((tmpcwd / "relayrl_config.json").read_text()) == json.loads(DEFAULT_CONFIG_CONTENT)
    p = c.get_algorithm_params()["REINFORCE"]
    assert p == {"discrete": True, "with_vf_baseline": False, "seed": 1, "traj_per_epoch": 8, "gamma": 0.98,
                 "lam": 0.97, "pi_lr": 3e-4, "vf_lr": 1e-3, "train_vf_iters": 80}
    assert c.get_train_server() == {"prefix": "tcp://", "host": "127.0.0.1", "port": "50051"}
    assert c.get_traj_server()["port"] == "7776"
    assert c.get_agent_listener()["port"] == "7777"
    assert c.get_tb_params() == {"launch_tb_on_startup": True, "scalar_tags": ["AverageEpRet", "LossQ"],
                                 "global_step_tag": "Epoch"}
    assert c.get_client_model_path() == os.path.join(str(tmpcwd), "client_model.pt")
    assert c.get_server_model_path() == os.path.join(str(tmpcwd), "server_model.pt")
    assert c.get_max_traj_length() == 1000
    assert c.get_grpc_idle_timeout() == 30


def test_unparseable_falls_back_everywhere(tmpcwd):
    (tmpcwd / "bad.json").write_text("{ not json")
    c = ConfigLoader("REINFORCE", str(tmpcwd / "bad.json"))
    assert c.get_algorithm_params() == {"REINFORCE": REINFORCE_FALLBACK}
    assert c.get_train_server() == {"prefix": "tcp://", "host": "*", "port": "7776"}
    assert c.get_traj_server() == {"prefix": "tcp://", "host": "*", "port": "7777"}
    assert c.get_agent_listener() == {"prefix": "tcp://", "host": "*", "port": "7778"}
    # model paths fall back swapped (config_loader.rs:504-534)
    assert c.get_client_model_path().endswith("server_model.pt")
    assert c.get_server_model_path().endswith("client_model.pt")
    assert c.get_tb_params() == {"launch_tb_on_startup": False, "scalar_tags": ["AverageEpRet", "StdEpRet"],
                                 "global_step_tag": "Epoch"}


def test_wrong_shape_section_fails_whole_document(tmpcwd):
    cfg = json.loads(DEFAULT_CONFIG_CONTENT)
    del cfg["algorithms"]["REINFORCE"]["lam"]  # serde: missing field -> whole parse fails
    (tmpcwd / "c.json").write_text(json.dumps(cfg))
    c = ConfigLoader("REINFORCE", str(tmpcwd / "c.json"))
    assert c.get_algorithm_params() == {"REINFORCE": REINFORCE_FALLBACK}
    assert c.get_train_server()["host"] == "*"


def test_missing_sections_individual_fallbacks(tmpcwd):
    (tmpcwd / "c.json").write_text(json.dumps({"max_traj_length": 77, "algorithms": {"C51": {"x": 1}}}))
    c = ConfigLoader("REINFORCE", str(tmpcwd / "c.json"))
    assert c.get_max_traj_length() == 77
    assert c.get_algorithm_params() == {"REINFORCE": REINFORCE_FALLBACK}
    assert ConfigLoader("NOPE", str(tmpcwd / "c.json")).get_algorithm_params() is None
    assert ConfigLoader("DQN", str(tmpcwd / "c.json")).get_algorithm_params() is None
    assert ConfigLoader(None, str(tmpcwd / "c.json")).get_algorithm_params() is None


def test_top_level_tensorboard_block_accepted(tmpcwd):
    (tmpcwd / "d.json").write_text(open(reference_fixtures.DEFAULT_CONFIG).read())  # the reference's own default
    c = ConfigLoader("REINFORCE", str(tmpcwd / "d.json"))
    assert c.get_tb_params()["scalar_tags"] == ["AverageEpRet", "LossQ"]


def test_example_configs_load(tmpcwd):
    base = reference_fixtures.EXAMPLES  # the relayrl_config.json of every reference example
    n = 0
    for root, _, files in os.walk(base):
        for f in files:
            if f == "relayrl_config.json":
                c = ConfigLoader("REINFORCE", os.path.join(root, f))
                p = c.get_algorithm_params()["REINFORCE"]
                assert set(p) == set(REINFORCE_FALLBACK)
                n += 1
    assert n >= 8


def test_resolve_creates_missing(tmpcwd):
    p = resolve_config_json_path(str(tmpcwd / "sub" / "x.json"))
    assert os.path.exists(p)


def test_ppo_and_mi355x_blocks(tmpcwd):
    cfg = json.loads(DEFAULT_CONFIG_CONTENT)
    cfg["algorithms"]["PPO"] = {"clip_ratio": 0.1, "pi_lr": 1e-3}
    cfg["mi355x"] = {"envs_per_actor": 128}
    (tmpcwd / "c.json").write_text(json.dumps(cfg))
    c = ConfigLoader("PPO", str(tmpcwd / "c.json"))
    p = c.get_algorithm_params()["PPO"]
    assert p["clip_ratio"] == 0.1 and p["pi_lr"] == 1e-3 and p["gamma"] == 0.99
    assert c.get_mi355x_params()["envs_per_actor"] == 128
