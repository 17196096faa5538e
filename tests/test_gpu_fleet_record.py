"""The fleet loop's flight recorder on the GPU (include/duck_fleet.h duck_fleet_record; sim2sim.FleetInfer's
set_recorder / recorded / replay): the kernel alone against its numpy restatement
(tests/fleet_record_reference.py) and its refusals, then the loop: the recorder changes nothing, graph replay
against eager, the frames against copies the test keeps itself, the replay of a recorded robot, and the
command line."""

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from open_duck_playground_amd import native
from open_duck_playground_amd.sim2sim import FRAME_SENSORS, FleetInfer, aux_fields, frame_fields
from tests import fleet_record_reference as K
from tests import fleet_reference as R
from tests.fleet_helpers import bits, c_desc, commands, dev, policy_file, stream  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SENTINEL = np.int32(0x7FC0BEEF)       # a NaN with a payload that no input below holds


# --- the kernel alone -----------------------------------------------------------------------
def _desc(nq, nv, nu):
    """fleet_reference's synthetic descriptor at the given sizes: the aux record starts at write_aux's rows."""
    sens_off = 4 * nv + nu
    return R.make_desc(nu=nu, nq=nq, nv=nv, sens_off=sens_off, con_off=sens_off + 14, naux=sens_off + 14 + 12 + 5,
                       act_qpos=[min(7 + a, nq - 1) for a in range(nu)], act_dof=[min(6 + a, nv - 1) for a in range(nu)])


SPECIAL = np.array([0x7FC12345, 0x7F800001, -0x00345678, -0x80000000, 0x00000001, -0x7FFFFFFF, 0x007FFFFF],
                   np.int64).astype(np.int32)      # quiet / signalling / negative NaNs with payloads, -0, denormals


def _inputs(d, n, rng):
    out = {}
    for name, shape in (("qpos", (d.nq, n)), ("qvel", (d.nv, n)), ("warm", (d.nv, n)), ("aux", (d.naux, n)),
                        ("ctl", (n, R.ctl_size(d.nu))), ("obs", (n, R.obs_size(d.nu))), ("action", (n, d.nu))):
        a = rng.normal(size=shape).astype(f32)
        pick = rng.integers(0, 4 * len(SPECIAL), size=shape)
        w = a.view(np.int32)
        w[pick < len(SPECIAL)] = SPECIAL[pick[pick < len(SPECIAL)]]     # a quarter of the words
        assert not (w == SENTINEL).any()
        out[name] = a
    return out


def _record(L, D, n, depth, post, x, alive, head, after, ring, gpu):
    return L.duck_fleet_record(C.byref(D), n, depth, post, x["qpos"].data_ptr(), x["qvel"].data_ptr(),
                               x["warm"].data_ptr(), x["aux"].data_ptr(), x["ctl"].data_ptr(), x["obs"].data_ptr(),
                               x["action"].data_ptr(), alive.data_ptr(), head.data_ptr(), after.data_ptr(),
                               ring.data_ptr(), stream(gpu))


def _death_calls(n, calls, variant):
    """The call (from 1) before which robot e's alive is cleared; 0: never. Robots 0, 3, 6, ... never die, robot 1
    is dead from the start, the others die at calls spread over the run. A single robot: by ``variant``."""
    if n == 1:
        return np.array([0 if variant == 0 else 2])
    e = np.arange(n)
    dies = 2 + (5 * e) % (calls - 1)
    dies[e % 3 == 0] = 0
    dies[1] = 1
    return dies


@pytest.mark.parametrize("n,nq,nv,nu,depth,post", [(1, 21, 20, 14, 1, 0), (17, 9, 8, 3, 3, 0), (130, 21, 20, 14, 4, 2),
                                                  (17, 23, 22, 16, 5, 1)])
def test_record_kernel_alone(gpu, n, nq, nv, nu, depth, post):
    """2 depth + 3 calls on fresh inputs full of NaN payloads, -0 and denormals; ring, head and after against the
    restatement as int32 after every call; a guard ring and guard counters behind the last robot."""
    L = native.lib()
    d = _desc(nq, nv, nu)
    D = c_desc(d)
    F = K.frame_size(nq, nv, nu)
    assert F == sum(w for _, w in frame_fields(nq, nv, nu).values())
    calls = 2 * depth + 3
    for variant in range(2 if n == 1 else 1):
        rng = np.random.default_rng(400 + n + nu + variant)
        dies = _death_calls(n, calls, variant)
        assert n == 1 or ((dies == 0).sum() * 3 >= n and dies[1] == 1 and len(set(dies[dies > 0])) >= 2)
        ring = np.full((n, depth, F), SENTINEL, np.int32)
        head, after, alive = np.zeros(n, np.int32), np.zeros(n, np.int32), np.ones(n, f32)
        ring_d = torch.full((n + 1, depth, F), int(SENTINEL), dtype=torch.int32, device=gpu)
        head_d, after_d = dev(np.append(head, 7).astype(np.int32), gpu), dev(np.append(after, 7).astype(np.int32), gpu)
        frozen_calls = 0
        for call in range(1, calls + 1):
            newly = (dies > 0) & (dies == call)
            alive[newly] = np.where(np.arange(n)[newly] % 2 == 0, f32(0.0), f32(-0.0))    # -0 is dead too
            x = _inputs(d, n, rng)
            wrote = K.record_step(d, depth, post, alive=alive, head=head, after=after, ring=ring, **x)
            frozen_calls += int((~wrote).sum())
            xd = {k: dev(v, gpu) for k, v in x.items()}
            native.check(_record(L, D, n, depth, post, xd, dev(alive, gpu), head_d, after_d, ring_d, gpu), L)
            got_ring, got_head, got_after = ring_d.cpu().numpy(), head_d.cpu().numpy(), after_d.cpu().numpy()
            np.testing.assert_array_equal(got_ring[:n], ring)
            np.testing.assert_array_equal(got_head[:n], head)
            np.testing.assert_array_equal(got_after[:n], after)
            assert (got_ring[n] == SENTINEL).all() and got_head[n] == 7 and got_after[n] == 7
        # the schedule did what it was built for: frozen robots, untouched slots that kept the sentinel, and a
        # robot alive throughout whose ring wrapped
        if (dies > 0).any():
            assert frozen_calls > 0
        if n > 1:
            assert head[1] == post + 1 and after[1] == post + 1
            if post + 1 < depth:
                assert (ring[1, post + 1:] == SENTINEL).all()
            assert head[0] == calls and after[0] == 0


def test_record_arguments(gpu):
    L = native.lib()
    n, nq, nv, nu, depth = 5, 9, 8, 3, 2
    d = _desc(nq, nv, nu)
    D = c_desc(d)
    F = K.frame_size(nq, nv, nu)
    x = {k: dev(v, gpu) for k, v in _inputs(d, n, np.random.default_rng(1)).items()}
    alive = torch.ones(n, device=gpu)
    head, after = torch.zeros(n, dtype=torch.int32, device=gpu), torch.zeros(n, dtype=torch.int32, device=gpu)
    ring = torch.full((n, depth, F), int(SENTINEL), dtype=torch.int32, device=gpu)
    ptrs = [x[k].data_ptr() for k in ("qpos", "qvel", "warm", "aux", "ctl", "obs", "action")] + \
        [alive.data_ptr(), head.data_ptr(), after.data_ptr(), ring.data_ptr()]

    def call(desc=D, n=n, depth=depth, post=0, null=None):
        p = [None if k == null else v for k, v in enumerate(ptrs)]
        return L.duck_fleet_record(None if desc is None else C.byref(desc), n, depth, post, *p, stream(gpu))

    EINVAL = native.HEADERS.consts["DUCK_EINVAL"]
    assert call(desc=None) == EINVAL and b"duck_fleet_record: null pointer" in L.duck_last_error()
    for k in range(len(ptrs)):
        assert call(null=k) == EINVAL and b"duck_fleet_record: null pointer" in L.duck_last_error(), k
    assert call(depth=0) == EINVAL and b"depth >= 1" in L.duck_last_error()
    assert call(post=-1) == EINVAL and b"post >= 0" in L.duck_last_error()
    for bad in (-1, (1 << 27) + 1):
        assert call(n=bad) == EINVAL and b"bad size" in L.duck_last_error()
    small = c_desc(d)
    small.sens_off, small.naux = 0, 4 * nv + nu - 1        # the sensors fit, the actuator_force rows do not
    assert call(desc=small) == EINVAL and b"4 nv + nu" in L.duck_last_error()
    outside = c_desc(d)
    outside.local_linvel = d.naux - d.sens_off - 2
    assert call(desc=outside) == EINVAL and b"sensor address outside the aux record" in L.duck_last_error()
    wide = c_desc(d)
    wide.nu = 17
    assert call(desc=wide) == EINVAL
    assert call(n=0) == native.HEADERS.consts["DUCK_OK"]
    torch.cuda.synchronize()
    assert (ring.cpu().numpy() == SENTINEL).all() and (head == 0).all() and (after == 0).all()     # nothing ran
    native.check(call(), L)                                 # and the same arguments do record
    assert (head == 1).all() and not (ring[:, 0].cpu().numpy() == SENTINEL).any() and (ring[:, 1].cpu().numpy() == SENTINEL).all()


# --- the loop --------------------------------------------------------------------------------
def _disturbed_fleet(path, n, gpu, **kw):
    """DR, a 3-segment schedule, drawn pushes first at period 2 and every 3 after, noise at level 1."""
    table = commands(2 * 3, seed=21).reshape(2, 3, 7)
    return FleetInfer("flat_terrain", path, n, device=gpu, randomize=7, command_schedule=(table, np.arange(n) % 2, 5),
                      pushes=(2, 3, (0.1, 0.5), (0.0, 6.0)), noise=(1.0, 3), **kw)


def _flipped(q):
    """(0, 1, 0, 0) * q: the base turned by pi about the world's x (test_fallen_robot_stops_counting's)."""
    w, x, y, z = q[3:7]
    out = q.copy()
    out[3:7] = [-x, w, -z, y]
    return out


def test_recorder_does_not_change_the_loop(policy_file, gpu):
    a = _disturbed_fleet(policy_file, 9, gpu)
    b = _disturbed_fleet(policy_file, 9, gpu, recorder=(4, 1))
    assert a.ring is None and b.ring is not None and a.disturbed() and b.disturbed()
    a.run(11)
    b.run(11)
    for x, y in zip(a.state(), b.state()):
        np.testing.assert_array_equal(bits(x), bits(y))
    for name in ("warm", "ctl", "obs", "acc", "alive", "tick"):
        np.testing.assert_array_equal(bits(getattr(a, name).cpu().numpy()), bits(getattr(b, name).cpu().numpy()))
    assert (b.rec_head.cpu().numpy() == 11).all() and (b.tick.cpu().numpy() == 11).all()


def test_graph_replay_equals_eager_recording(policy_file, gpu, monkeypatch):
    monkeypatch.setattr(FleetInfer, "CHUNK", 5)
    a = _disturbed_fleet(policy_file, 8, gpu, recorder=(7, 1))       # a depth that does not divide the chunk
    b = _disturbed_fleet(policy_file, 8, gpu, recorder=(7, 1))
    for f in (a, b):                                                 # one robot falls at once: its ring freezes
        q = f.state()[0]
        q[1] = _flipped(q[1])
        f.load_state(qpos=q)
    a.run(3)      # the first call is eager
    assert a.graph is None
    a.run(20)     # four replays of the 5-period graph
    assert a.graph is not None and a.graph[1] == 5
    b.run(23)
    assert b.graph is None
    for name in ("ring", "rec_head", "rec_after", "alive", "ctl"):
        np.testing.assert_array_equal(bits(getattr(a, name).cpu().numpy()), bits(getattr(b, name).cpu().numpy()))
    head, up = a.rec_head.cpu().numpy(), a.alive.cpu().numpy() != 0
    assert head[1] == 2 and not up[1] and up.any() and (head[up] == 23).all() and a.periods_done == 23
    assert list(a.recorded(int(np.flatnonzero(up)[0]))["period"]) == list(range(17, 24))
    assert list(a.recorded(1)["period"]) == [1, 2]


def test_frames_are_the_truth(policy_file, gpu):
    """Six robots driven one period at a time; after each period the test keeps its own copy of everything a
    frame holds. Robot 1 starts flipped, robot 3 is flipped after period 4, robot 5 gets a NaN velocity after
    period 6. With recorder=(6, 1) and 10 periods the rule of include/duck_fleet.h gives: robots 0, 2, 4 periods
    5..10; robot 1 (fell in period 1) 1..2; robot 3 (fell in period 5) 1..6; robot 5 (fell in period 7: the fall
    frame and one more) 3..8."""
    fleet = FleetInfer("flat_terrain", policy_file, 6, device=gpu, recorder=(6, 1))
    fleet.set_commands(commands(6, seed=31))
    m = fleet.model
    q = fleet.state()[0]
    q[1] = _flipped(q[1])
    fleet.load_state(qpos=q)
    aux = aux_fields(m)
    names = m.names["sensor"]
    sens_rows = [aux["sensordata"][0] + int(m.sensor_adr[names.index(s)]) for s in
                 ("gyro", "accelerometer", "upvector", "local_linvel")]
    assert FRAME_SENSORS == ("gyro", "accelerometer", "upvector", "local_linvel")
    kept = []
    for period in range(1, 11):
        fleet.run(1)
        a = fleet.aux.cpu().numpy()
        force = a[aux["actuator_force"][0]:][:aux["actuator_force"][1]].T
        kept.append({"qpos": fleet.qpos.t().cpu().numpy(), "qvel": fleet.qvel.t().cpu().numpy(),
                     "qacc_warmstart": fleet.warm.t().cpu().numpy(), "ctl": fleet.ctl.cpu().numpy(),
                     "obs": fleet.obs.cpu().numpy(), "action": fleet.action.cpu().numpy(), "actuator_force": force,
                     "sensors": np.concatenate([a[r:r + 3].T for r in sens_rows], axis=1)})
        if period == 4:
            q = fleet.state()[0]
            q[3] = _flipped(q[3])
            fleet.load_state(qpos=q)
        if period == 6:
            v = fleet.state()[1]
            v[5, 0] = np.nan
            fleet.load_state(qvel=v)
    assert fleet.graph is None
    # the premises first
    rep = fleet.report()
    assert list(rep["periods"]) == [10, 0, 10, 4, 10, 6] and list(rep["fell"]) == [False, True, False, True, False, True]
    want = {0: range(5, 11), 2: range(5, 11), 4: range(5, 11), 1: range(1, 3), 3: range(1, 7), 5: range(3, 9)}
    for robot, periods in want.items():
        rec = fleet.recorded(robot)
        assert list(rec["period"]) == list(periods), robot
        assert rec["fell"] == (robot % 2 == 1)
        assert set(rec) == set(fleet.frame_fields) | {"period", "fell"}
        for name in fleet.frame_fields:
            mine = np.stack([kept[p - 1][name][robot] for p in periods])
            assert rec[name].dtype == np.float32 and rec[name].shape == mine.shape, name
            np.testing.assert_array_equal(bits(rec[name]), bits(mine), err_msg=f"robot {robot} {name}")
    nan = fleet.recorded(5)
    assert np.isnan(nan["qvel"][-1]).any() and np.isfinite(nan["qvel"][:4]).all()      # periods 3..6 finite, 7 and 8 not
    up = fleet.recorded(3)["sensors"][:, 8]
    assert (up[:4] > 0).all() and up[4] < 0                                              # upright through period 4


def _assert_replay(fleet, robot):
    """``fleet`` has run 6 periods with recorder=(6, 0): replay ``robot`` from its newest frame (period 6), run the
    fleet 6 more, and the replay's 6 periods equal the fleet's frames of periods 7..12; then replay from the
    oldest frame the fleet now holds (period 7): 5 periods equal the fleet's 8..12. (After 12 periods a ring of 6
    holds 7..12, so the replay whose 6 periods are compared with all of them starts from period 6's frame, taken
    before the fleet runs on.)"""
    assert fleet.periods_done == 6
    r = fleet.replay(robot, frame=-1)
    assert r.num_robots == 1 and r.periods_done == 6 and r.robot_offset == fleet.robot_offset + robot
    fleet.run(6)
    mine = fleet.recorded(robot)
    assert list(mine["period"]) == list(range(7, 13))
    r.set_recorder(6)
    r.run(6)
    got = r.recorded(0)
    assert list(got["period"]) == list(range(7, 13))
    for name in fleet.frame_fields:
        np.testing.assert_array_equal(bits(got[name]), bits(mine[name]), err_msg=name)
    r2 = fleet.replay(robot)                  # frame 0: period 7
    r2.set_recorder(6)
    r2.run(5)
    got = r2.recorded(0)
    assert list(got["period"]) == list(range(8, 13))
    for name in fleet.frame_fields:
        np.testing.assert_array_equal(bits(got[name]), bits(mine[name][1:]), err_msg=name)
    return mine


def test_replay_reproduces_the_recorded_periods(policy_file, gpu):
    fleet = _disturbed_fleet(policy_file, 9, gpu, recorder=(6, 0))
    fleet.run(6)
    mine = _assert_replay(fleet, 4)
    other = fleet.recorded(5)
    assert not np.array_equal(mine["obs"], other["obs"]) and not np.array_equal(mine["qvel"], other["qvel"])
    # the disturbances did act on the replayed periods: the schedule's segment 1 for periods 8, 9, then segment 2
    assert not np.array_equal(mine["ctl"][0, 70:77], mine["ctl"][-1, 70:77])
    assert (fleet.tick.cpu().numpy() == 12).all()


def test_replay_of_an_undisturbed_fleet(policy_file, gpu):
    fleet = FleetInfer("flat_terrain", policy_file, 3, device=gpu, recorder=(6, 0))
    fleet.set_commands(commands(3, seed=32))
    assert not fleet.disturbed() and fleet.dr is None
    fleet.run(6)
    _assert_replay(fleet, 2)
    with pytest.raises(native.DuckError):
        fleet.replay(2, frame=6)
    with pytest.raises(native.DuckError):
        fleet.recorded(3)
    fleet.set_recorder(None)
    assert fleet.ring is None
    with pytest.raises(native.DuckError):
        fleet.recorded(0)


def test_command_line_writes_the_falls(policy_file, gpu, tmp_path):
    out, falls = str(tmp_path / "report.json"), str(tmp_path / "falls.npz")
    subprocess.run([sys.executable, "-m", "open_duck_playground_amd.sim2sim", "-o", policy_file, "--num_robots", "32",
                    "--periods", "12", "--command_grid", "2x1x1", "--push_grid", "1x4", "--push_magnitude", "100", "100",
                    "--push_at", "2", "--record_falls", "4", "--record_out", falls, "--record_max", "5", "--out", out,
                    "--device", gpu], cwd=ROOT, check=True, timeout=300)
    doc = json.load(open(out))
    rec = doc["recorder"]
    assert rec["fallen"] >= 1                               # the premise: a push of 100 m/s does bring robots down
    assert rec == {"depth": 4, "post": 0, "fallen": rec["fallen"], "written": min(rec["fallen"], 5)}
    z = np.load(falls, allow_pickle=False)
    R_ = rec["written"]
    fields = json.loads(str(z["fields"]))
    assert fields == {k: list(v) for k, v in frame_fields(21, 20, 14).items()}
    assert set(z.files) == {"robots", "count", "period", "survived", "fields"} | set(fields)
    assert z["robots"].shape == (R_,) and z["count"].shape == (R_,) and z["period"].shape == (R_, 4)
    assert (np.diff(z["robots"]) > 0).all() and (z["count"] >= 1).all() and (z["count"] <= 4).all()
    for name, (_, w) in fields.items():
        assert z[name].shape == (R_, 4, w) and z[name].dtype == np.float32, name
    for k in range(R_):
        t = int(z["count"][k])
        period = z["period"][k]
        assert (np.diff(period[:t]) == 1).all() and (period[t:] == -1).all()
        assert period[t - 1] == z["survived"][k] + 1       # post 0: the ring ends at the fall frame
        assert t == min(4, period[t - 1])
        state = np.concatenate([z["qpos"][k, :t], z["qvel"][k, :t]], axis=1)
        fallen = (z["sensors"][k, :t, 8] < 0) | np.isnan(state).any(axis=1)      # upvector[2], or a NaN state
        assert fallen[-1] and not fallen[:-1].any()
        for name in fields:
            assert (z[name][k, t:] == 0).all()
