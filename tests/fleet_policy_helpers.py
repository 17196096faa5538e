"""What the several-policies tests share (tests/test_gpu_fleet_policies.py, tests/test_fleet_policies_host.py):
K distinct exported test policies of one architecture, and hand-built policy files of any widths with or without
a normaliser for the constructor's refusals. Test infrastructure only."""

import numpy as np
import pytest
import torch

from open_duck_playground_amd import onnx_export, ppo
from open_duck_playground_amd.onnx_export import _bytes, _int, _str, node, tensor, value_info

f32 = np.float32


def export_policies(directory, seeds, prefix="policy"):
    """``ppo.ActorCritic(101, 212, 14, ...)`` under each seed, its normaliser fed 500 rows of its own (so mean and
    std differ between the files too), exported to ONNX: the paths."""
    paths = []
    for seed in seeds:
        torch.manual_seed(int(seed))
        net = ppo.ActorCritic(101, 212, 14, ppo.PPOConfig())
        rng = np.random.default_rng(1000 + int(seed))
        net.obs_norm.update(torch.tensor(rng.normal(0.1 * seed, 1.0 + 0.05 * seed, size=(500, 101)), dtype=torch.float32))
        path = str(directory / f"{prefix}_{seed}.onnx")
        onnx_export.export_onnx(net, 14, 101, output_path=path)
        paths.append(path)
    return paths


def graph_file(path, widths, seed=0, normaliser=True):
    """A policy file of Gemm layers ``widths`` (obs, hidden..., actions) with random weights; ``normaliser=False``
    leaves the Sub / Div pair on the input out. Returns ``path``."""
    rng = np.random.default_rng(seed)
    layers = [(rng.normal(size=(a, b)).astype(f32), rng.normal(size=b).astype(f32)) for a, b in zip(widths, widths[1:])]
    if normaliser:
        blob = onnx_export.policy_graph(layers, rng.normal(size=widths[0]).astype(f32),
                                        rng.uniform(0.5, 2.0, widths[0]).astype(f32), widths[0], widths[-1])
    else:
        nodes, inits, x = [], [], "obs"
        for i, (w, b) in enumerate(layers):
            inits += [tensor(f"w{i}", w), tensor(f"b{i}", b)]
            nodes.append(node("Gemm", [x, f"w{i}", f"b{i}"], [f"z{i}"], f"gemm{i}"))
            x = f"z{i}"
            if i < len(layers) - 1:
                nodes += [node("Sigmoid", [x], [f"s{i}"], f"sig{i}"), node("Mul", [x, f"s{i}"], [f"a{i}"], f"mul{i}")]
                x = f"a{i}"
        nodes.append(node("Tanh", [x], ["y"], "tanh"))
        graph = (b"".join(_bytes(1, n) for n in nodes) + _str(2, "g") + b"".join(_bytes(5, t) for t in inits)
                 + _bytes(11, value_info("obs", [1, widths[0]])) + _bytes(12, value_info("y", [1, widths[-1]])))
        blob = _int(1, 6) + _bytes(7, graph) + _bytes(8, _str(1, "") + _int(2, 11))
    with open(path, "wb") as f:
        f.write(blob)
    return str(path)


@pytest.fixture(scope="module")
def policy_files(tmp_path_factory):
    """Three distinct seeded, untrained test policies (seeds 3, 4, 5)."""
    return export_policies(tmp_path_factory.mktemp("onnx_multi"), (3, 4, 5))
