"""Recorded data of the reference project that the compatibility tests need (tests/golden/).

* ``reference_examples/``: the ``relayrl_config.json`` of every reference example and one
  ``progress.txt`` its logger wrote, under the example's own relative path.
* ``reference_default_config.json``: the reference's default configuration.
* ``reference_client_model/``: the weights of the ``client_model.pt`` the reference's CartPole
  examples ship (``pi_params.npy``: its six raw fp32 storages W1 b1 W2 b2 W3 b3, concatenated)
  and the member names of that TorchScript archive (``members.json``).  The archive itself
  holds TorchScript source, so it is not stored: ``client_model_bytes()`` re-creates a
  PolicyWithoutBaseline archive with these weights through the project's own exporter, whose
  member layout ``test_wire_compat`` holds to ``members.json``.
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXAMPLES = os.path.join(GOLDEN, "reference_examples")
DEFAULT_CONFIG = os.path.join(GOLDEN, "reference_default_config.json")
PROGRESS = os.path.join(EXAMPLES, "REINFORCE_without_baseline", "box2d", "lunar_lander", "grpc", "logs",
                        "relayrl-reinforce-info", "relayrl-reinforce-info_s298690001", "progress.txt")


def client_model_pi() -> np.ndarray:
    """Flat fp32 policy weights [4, 128, 128, 2] of the reference's shipped client_model.pt."""
    return np.load(os.path.join(GOLDEN, "reference_client_model", "pi_params.npy"))


def client_model_members() -> list:
    with open(os.path.join(GOLDEN, "reference_client_model", "members.json")) as f:
        return json.load(f)["members"]


def client_model_bytes() -> bytes:
    """``torch.jit.save`` bytes of a PolicyWithoutBaseline(4, 2) that carries the reference's weights."""
    import torch

    from relayrl_prototype_amd.models.policies import build_policy_module, torchscript_bytes

    return torchscript_bytes(build_policy_module(4, 2, 128, torch.from_numpy(client_model_pi()), None))


def client_model_file(directory) -> str:
    path = os.path.join(str(directory), "client_model.pt")
    with open(path, "wb") as f:
        f.write(client_model_bytes())
    return path
