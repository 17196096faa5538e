"""bench.py --dump-outputs / --full: what a run writes and what a plain run leaves out.

The GPU tests call bench.main() in this process (64 envs, 3 timed steps); the sampling rule of
dump_outputs is checked on CPU tensors."""

import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _run(monkeypatch, capsys, args):
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1"] + args)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(path):
    return {f: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


@pytest.mark.gpu
def test_dump_outputs_is_the_last_timed_state_and_repeats(gpu, monkeypatch, capsys, tmp_path):
    args = ["--envs", "64", "--steps", "3", "--warmup", "2"]
    d = _run(monkeypatch, capsys, args + ["--dump-outputs", str(tmp_path / "a")])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["finite"] and d["cpu_baseline"] is None
    assert d["value"] == pytest.approx(64 * 3 / (d["ms_per_step"] * 3 / 1e3), rel=1e-6)
    a = _load(tmp_path / "a")
    assert {"obs_state.npy", "obs_privileged_state.npy", "reward.npy", "done.npy", "qpos.npy", "qvel.npy",
            "info_step.npy", "env_rows.npy"} <= set(a)
    assert a["obs_state.npy"].shape == (64, 101) and a["obs_state.npy"].dtype == np.float32
    assert all(x.dtype in (np.float32, np.float64) and x.size > 0 and np.isfinite(x).all() for x in a.values())
    assert "info_current_reference_motion.npy" not in a   # empty without imitation: not written
    assert (a["env_rows.npy"] == np.arange(64)).all()
    assert a["info_step.npy"].max() == 5   # warm-up + timed steps (an env that fell starts again at 0)
    # the same steps through Joystick directly (bench.py's workload C2: seed, action pool, wrappers)
    from open_duck_playground_amd.joystick import Joystick, wrap_for_brax_training
    env = wrap_for_brax_training(Joystick("flat_terrain", num_envs=64, device=gpu, use_imitation=False),
                                 episode_length=1000)
    st = env.reset(rng=0)
    g = torch.Generator(device=gpu)
    g.manual_seed(1234)
    pool = [torch.rand(64, env.action_size, device=gpu, generator=g) * 2 - 1 for _ in range(8)]
    for i in [0, 1] + [0, 1, 2]:   # 2 warm-up steps, then 3 timed ones: both start at the pool's head
        st = env.step(st, pool[i])
    for name, t in (("obs_state", st.obs["state"]), ("obs_privileged_state", st.obs["privileged_state"]),
                    ("reward", st.reward), ("done", st.done), ("qpos", st.data.qpos), ("qvel", st.data.qvel),
                    ("ctrl", st.data.ctrl), ("info_last_act", st.info["last_act"]),
                    *((f"metrics_{k.replace('/', '_')}", v) for k, v in st.metrics.items())):
        assert np.array_equal(a[name + ".npy"], t.cpu().numpy()), name
    _run(monkeypatch, capsys, args + ["--dump-outputs", str(tmp_path / "b")])
    b = _load(tmp_path / "b")
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    # one more timed step is another state: --steps sets how many steps ran
    _run(monkeypatch, capsys, ["--envs", "64", "--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path / "c")])
    c = _load(tmp_path / "c")
    assert c["info_step.npy"].max() == 6 and not np.array_equal(a["qpos.npy"], c["qpos.npy"])


@pytest.mark.gpu
def test_full_adds_the_cpu_baselines(gpu, monkeypatch, capsys):
    d = _run(monkeypatch, capsys, ["--envs", "64", "--steps", "3", "--warmup", "2", "--full", "--cpu-budget", "0.2",
                                   "--cpu-threads", "2"])
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["c1"]["envs"] == 1


def test_dump_outputs_samples_env_rows_above_the_size_limit(monkeypatch, tmp_path):
    import bench
    from open_duck_playground_amd.joystick import Data, State
    n = 1000
    g = torch.Generator().manual_seed(0)
    f = lambda *s: torch.rand(n, *s, generator=g)  # noqa: E731
    st = State(data=Data(qpos=f(21), qvel=f(20), qacc_warmstart=f(20), ctrl=f(14)),
               obs={"state": f(101), "privileged_state": f(172)}, reward=f(), done=f(),
               metrics={"reward/alive": f()}, info={"step": torch.arange(n, dtype=torch.int32), "command": f(7),
                                                    "current_reference_motion": f(0)})
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    for rank, sfx in ((0, ".npy"), (1, ".rank1.npy")):
        bench.dump_outputs(str(tmp_path), st, n, rank, 2)
    z = {k: np.load(tmp_path / k) for k in os.listdir(tmp_path)}
    rows = z["env_rows.npy"].astype(int)
    assert all(v.size > 0 for v in z.values()) and "info_current_reference_motion.npy" not in z
    assert 0 < len(rows) < n and (np.diff(rows) > 0).all() and (rows == z["env_rows.rank1.npy"]).all()
    assert sum(os.path.getsize(tmp_path / k) for k in z) <= 200_000   # whole files, headers included
    assert (z["info_step.npy"] == rows).all() and z["info_step.npy"].dtype == np.float64
    assert np.array_equal(z["obs_state.npy"], st.obs["state"].numpy()[rows])
    assert np.array_equal(z["metrics_reward_alive.npy"], st.metrics["reward/alive"].numpy()[rows])
