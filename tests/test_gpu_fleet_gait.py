"""Gait and servo load on the GPU (include/duck_fleet.h duck_fleet_gait; sim2sim.FleetInfer.set_gait): the kernel
alone against its numpy restatement (tests/fleet_gait_reference.py) and its refusals, then the loop: 33 randomised
robots, some of them pushed over, stepped a period at a time with the restatement applied to what the device held,
the launch read-only on the loop, off meaning no call, graph replay against eager, robot identity, restart, and a
followed log reproducing the record of the robot that made it. Every comparison is bit for bit."""

import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from open_duck_playground_amd import native, sim2sim
from open_duck_playground_amd.sim2sim import FleetInfer
from tests import fleet_gait_reference as G
from tests import fleet_reference as R
from tests.fleet_helpers import bits, c_desc, commands, guarded, guards_hold, host_desc, policy_file, stream  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
NAN_PAYLOAD, NEG_ZERO = np.int32(0x7FC12345), np.int32(-0x80000000)
SEED, ROBOT, PERIODS, N = 7, 20, 12, 33


def c_gait_desc(s):
    out = native.DuckFleetGaitDesc()
    for k in range(2):
        out.foot_linvel[k], out.foot_pos[k] = s.foot_linvel[k], s.foot_pos[k]
    for a, v in enumerate(s.force_sat):
        out.force_sat[a] = float(v)
    out.speed_sat = float(s.speed_sat)
    return out


def gait_desc_values(s):
    """A ctypes duck_fleet_gait_desc as plain values for the restatement."""
    return SimpleNamespace(foot_linvel=list(s.foot_linvel), foot_pos=list(s.foot_pos),
                           force_sat=[f32(v) for v in s.force_sat], speed_sat=f32(s.speed_sat))


# --- the kernel alone -----------------------------------------------------------------------
# the scripted feet of the even robots: the left foot swings over calls 1-3 with its highest sample in the middle
LEFT_CONTACT = (1, 0, 0, 0, 1, 1, 0, 1, 0)
RIGHT_CONTACT = (0, 0, 1, 1, 0, 0, 0, 1, 1)
LEFT_Z = (0.0, 0.02, 0.05, 0.03, 0.01, 0.0, 0.04, 0.0, 0.02)
RIGHT_Z = (-0.0, 0.03, 0.0, 0.0, 0.02, 0.06, 0.03, 0.01, 0.0)


@pytest.mark.parametrize("n,nu", [(1, 14), (17, 3), (130, 14), (17, 16)])
def test_gait_kernel_alone(gpu, n, nu):
    """9 calls on fresh random aux / qvel / ctl with a guard row before and after every buffer. Scripted: touchdowns
    and liftoffs of both feet, a swing of three calls with its highest sample in the middle, robots dead from the
    start and dying at calls 3 and 6 (their rows keep their bits), records that do not start at zero, |f| equal to
    its threshold and one ulp below, a +inf threshold, NaN payloads in a force, a joint velocity and a foot velocity,
    -0 inputs, the last partial wave."""
    L = native.lib()
    d = R.make_desc(nu=nu)
    s = G.make_gait_desc(d)
    s.force_sat[1] = f32(np.inf)
    Dc, Sc = c_desc(d), c_gait_desc(s)
    rng = np.random.default_rng(1200 + n + nu)
    Gw, Cw, calls = G.gait_size(nu), R.ctl_size(nu), 9
    F = G.gait_fields(nu)
    e = np.arange(n)
    scripted = e % 2 == 0
    dead0, die3, die6 = e % 7 == 3, e % 7 == 1, e % 7 == 5
    started = e % 5 == 2
    rec = np.zeros((n, Gw), f32)
    rec[started] = rng.uniform(0.5, 2.0, size=(int(started.sum()), Gw)).astype(f32)
    rec[started, F["periods"][0]] = 3
    rec[started, F["left_prev"][0]], rec[started, F["right_prev"][0]] = 1, 0
    alive = np.where(dead0, 0, 1).astype(f32)
    qvel_g, qvel_d = guarded(np.zeros((d.nv, n), f32), gpu)
    aux_g, aux_d = guarded(np.zeros((d.naux, n), f32), gpu)
    ctl_g, ctl_d = guarded(np.zeros((n, Cw), f32), gpu)
    alive_g, alive_d = guarded(alive, gpu)
    rec_g, rec_d = guarded(rec, gpu)
    seen = dict(touchdown=np.zeros(2, int), liftoff=np.zeros(2, int), first=0, later=0, force_at=0, speed_at=0, inf_at=0)
    frozen = {}
    for call in range(calls):
        qvel = (3 * rng.normal(size=(d.nv, n))).astype(f32)
        aux = rng.normal(size=(d.naux, n)).astype(f32)
        ctl = rng.normal(size=(n, Cw)).astype(f32)
        # the feet: a foot in contact has one negative slot; one in the air has positive, NaN and -0 slots
        for k, (script, zs) in enumerate(((LEFT_CONTACT, LEFT_Z), (RIGHT_CONTACT, RIGHT_Z))):
            c = np.where(scripted, bool(script[call]), rng.random(n) < 0.5)
            slots = np.abs(aux[d.con_off + d.foot_con[k]:][:4]) + f32(0.01)
            slots[1, ~c & (e % 3 == 0)] = np.nan
            slots.view(np.int32)[2, ~c & (e % 3 == 1)] = NEG_ZERO
            slots[rng.integers(0, 4, n), e] *= np.where(c, f32(-1), f32(1))
            aux[d.con_off + d.foot_con[k]:][:4] = slots
            z = aux[d.sens_off + s.foot_pos[k] + 2]
            z[scripted] = f32(zs[call])
        # the thresholds of actuator 0: exactly on (counted), one ulp below (not counted); beside a +inf threshold
        on = e % 3 == 0
        if call == 2:
            aux[4 * d.nv, on] = -s.force_sat[0]
            aux[4 * d.nv + 1, :] = f32(3e18)
        if call == 5:
            aux[4 * d.nv, on] = np.nextafter(s.force_sat[0], f32(0))
        # NaN payloads: a force, a joint velocity, a foot velocity; -0 in each kind of input
        if call == 1:
            aux.view(np.int32)[4 * d.nv + nu - 1, e % 4 == 0] = NAN_PAYLOAD
        if call == 4:
            qvel.view(np.int32)[d.act_dof[0], e % 4 == 1] = NAN_PAYLOAD + 1
        if call == 7:
            aux.view(np.int32)[d.sens_off + s.foot_linvel[0], e % 4 == 2] = NAN_PAYLOAD + 2
        if call == 0:
            aux.view(np.int32)[4 * d.nv + 2, e % 2 == 1] = NEG_ZERO
            qvel.view(np.int32)[d.act_dof[1], :] = NEG_ZERO
            aux.view(np.int32)[d.sens_off + s.foot_linvel[1] + 1, :] = NEG_ZERO
            ctl.view(np.int32)[:, 0] = NEG_ZERO
        if call == 3:
            alive[die3] = 0
        if call == 6:
            alive[die6] = 0
        for row in np.flatnonzero(alive == 0):
            frozen.setdefault(int(row), bits(rec[row]).copy())
        for t, a in ((qvel_d, qvel), (aux_d, aux), (ctl_d, ctl), (alive_d, alive)):
            t.copy_(torch.tensor(a))
        did = G.gait(d, s, qvel, aux, ctl, alive, rec)
        native.check(L.duck_fleet_gait(C.byref(Dc), C.byref(Sc), n, qvel_d.data_ptr(), aux_d.data_ptr(), ctl_d.data_ptr(),
                                       alive_d.data_ptr(), rec_d.data_ptr(), stream(gpu)), L)
        for name, got, want in (("gait", rec_d, rec), ("qvel", qvel_d, qvel), ("aux", aux_d, aux), ("ctl", ctl_d, ctl),
                                ("alive", alive_d, alive)):
            np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(want), err_msg=f"{name}, call {call}")
        for t in (qvel_g, aux_g, ctl_g, alive_g, rec_g):
            assert guards_hold(t), call
        # the restatement did what the header says
        for row, was in frozen.items():
            assert (bits(rec[row]) == was).all(), (row, call)
        assert not did.live[alive == 0].any() and did.live[alive != 0].all()
        seen["touchdown"] += did.touchdown.sum(0)
        seen["liftoff"] += did.liftoff.sum(0)
        seen["first"] += int(did.first.sum())
        seen["later"] += int((did.live & ~did.first).sum())
        seen["speed_at"] += int(did.speed_at.sum())
        seen["inf_at"] += int(did.force_at[:, 1].sum())
        if call in (2, 5):
            assert (did.force_at[on & did.live, 0] == (call == 2)).all() and (on & did.live).any()
        if call == 0:
            assert (did.first == (did.live & ~started)).all() and did.first.any()
            assert not did.touchdown[did.first].any() and not did.liftoff[did.first].any()
            assert bits(rec)[0, F["right_apex"][0]] == NEG_ZERO           # a -0 height is copied, not computed
        if call == 4:   # robot 0's left foot lands: the swing's highest sample was the middle one
            assert did.touchdown[0, 0] and bits(rec)[0, F["left_apex_sum"][0]] == bits(f32(0.05) - f32(0.01))
    assert (seen["touchdown"] > 0).all() and (seen["liftoff"] > 0).all() and seen["later"] > 0 and seen["inf_at"] == 0
    assert seen["speed_at"] > 0 and np.isnan(rec[0, F["force_sq"][0] + nu - 1]) and rec[0, F["periods"][0]] == calls
    assert rec[0, F["left_touchdowns"][0]] == 2 and rec[0, F["right_touchdowns"][0]] == 2
    if n > 1:
        assert dead0.any() and die3.any() and die6.any() and started.any() and len(frozen) == int((alive == 0).sum())
        assert not bits(rec)[dead0 & ~started].any() and (rec[die3 & ~started, F["periods"][0]] == 3).all()
        assert (rec[die6 & ~started & ~die3 & ~dead0, F["periods"][0]] == 6).all()
        assert np.isnan(rec[:, F["speed_max"][0]:][:, :nu]).sum() == 0      # a NaN never enters a maximum
        assert np.isnan(rec[:, F["work"][0]]).any() and np.isnan(rec[:, F["left_slip"][0]]).any()


def test_gait_arguments(gpu):
    L = native.lib()
    n, nu = 5, 3
    d = R.make_desc(nu=nu)
    s = G.make_gait_desc(d)
    D, S = c_desc(d), c_gait_desc(s)
    EINVAL, OK = native.HEADERS.consts["DUCK_EINVAL"], native.HEADERS.consts["DUCK_OK"]
    qvel, aux = torch.ones(d.nv, n, device=gpu), torch.ones(d.naux, n, device=gpu)
    ctl, alive = torch.zeros(n, R.ctl_size(nu), device=gpu), torch.ones(n, device=gpu)
    rec = torch.zeros(n, G.gait_size(nu), device=gpu)
    ptrs = [t.data_ptr() for t in (qvel, aux, ctl, alive, rec)]

    def call(desc=D, gd=S, n=n, null=None):
        p = [None if k == null else v for k, v in enumerate(ptrs)]
        return L.duck_fleet_gait(None if desc is None else C.byref(desc), None if gd is None else C.byref(gd), n, *p,
                                 stream(gpu))
    assert call(desc=None) == EINVAL and b"duck_fleet_gait: null pointer" in L.duck_last_error()
    assert call(gd=None) == EINVAL and b"duck_fleet_gait: null pointer" in L.duck_last_error()
    for k in range(len(ptrs)):
        assert call(null=k) == EINVAL and b"duck_fleet_gait: null pointer" in L.duck_last_error(), k
    for bad in (-1, (1 << 27) + 1):
        assert call(n=bad) == EINVAL and b"duck_fleet_gait: bad size" in L.duck_last_error()
    wide = c_desc(d)
    wide.nu = 17
    assert call(desc=wide) == EINVAL and b"duck_fleet_gait: nq, nv >= 1" in L.duck_last_error()
    for field in ("foot_linvel", "foot_pos"):
        for f in range(2):
            for adr in (-1, d.con_off - d.sens_off - 2):          # the third word would be a con_dist row
                out = c_gait_desc(s)
                getattr(out, field)[f] = adr
                assert call(gd=out) == EINVAL and b"duck_fleet_gait: foot sensor address" in L.duck_last_error(), (field, f)
            getattr(out, field)[f] = d.con_off - d.sens_off - 3   # the last three sensordata words are fine
            assert call(gd=out, n=0) == OK
    short = c_desc(d)
    short.naux = 4 * d.nv + nu - 1
    short.sens_off = short.con_off = 0
    short.foot_con[0] = short.foot_con[1] = 0
    assert call(desc=short) == EINVAL and b"duck_fleet_gait: actuator_force rows" in L.duck_last_error()
    off = c_desc(d)
    off.local_linvel = d.naux - d.sens_off - 2
    assert call(desc=off) == EINVAL and b"duck_fleet_gait: sensor address" in L.duck_last_error()
    assert call(n=0) == OK
    torch.cuda.synchronize()
    assert (rec == 0).all()                                   # nothing ran
    native.check(call(), L)
    torch.cuda.synchronize()
    F = G.gait_fields(nu)
    assert (rec[:, F["periods"][0]] == 1).all() and (rec[:, F["force_sq"][0]] == 1).all() and (rec[:, F["flight"][0]] == 1).all()


# --- the loop --------------------------------------------------------------------------------
def _pushes(rows=slice(None)):
    """A push in period 2: every third robot is thrown at 100 m/s, the others nudged."""
    e = np.arange(N)
    return (np.full(N, 2)[rows], 0, np.where(e % 3 == 0, 100.0, 0.3)[rows], np.linspace(0.0, 6.0, N)[rows])


def _fleet(policy, gpu, gait=(True,), **kw):
    fleet = FleetInfer("flat_terrain", policy, N, device=gpu, randomize=SEED, pushes=_pushes(), gait=gait, **kw)
    fleet.set_commands(commands(N, seed=41))
    return fleet


def _host(fleet, names):
    return {k: getattr(fleet, k).cpu().numpy().copy() for k in names}


LOOP = ("qpos", "qvel", "warm", "ctl", "obs", "acc", "alive")


@pytest.fixture(scope="module")
def stepped(policy_file, gpu):
    """The gaited fleet stepped eagerly a period at a time, the restatement applied after each to the aux, qvel, ctl
    and alive the device then held: the device's record, the restatement's, and the loop's buffers at the end."""
    fleet = _fleet(policy_file, gpu)
    assert fleet.gaited() and not bits(fleet.gait_records()).any()
    d, s = R.desc_values(fleet.desc), gait_desc_values(fleet.gait_desc)
    want = np.zeros((N, G.gait_size(14)), f32)
    heights = []
    for _ in range(PERIODS):
        fleet.run(1)
        h = _host(fleet, ("qvel", "aux", "ctl", "alive"))
        G.gait(d, s, h["qvel"], h["aux"], h["ctl"], h["alive"], want)
        heights.append(h["aux"][d.sens_off + s.foot_pos[0] + 2])
    assert fleet.graph is None
    return SimpleNamespace(got=fleet.gait_records(), want=want, end=_host(fleet, LOOP), rep=fleet.report(),
                           heights=np.array(heights), model=fleet.model, fields=fleet.gait_fields)


def test_the_loop_equals_the_restatement(stepped):
    np.testing.assert_array_equal(bits(stepped.got), bits(stepped.want))
    fell = stepped.rep["fell"]
    print("\n[measure] fell:", int(fell.sum()), "of", N, "periods:", stepped.rep["periods"].astype(int).tolist())
    assert 0 < fell.sum() < N                                   # the push brings some down, not all
    assert np.ptp(stepped.heights[:, ~fell], axis=0).all()      # the foot sensors are live: the heights move
    F = G.gait_fields(14)
    assert stepped.got[:, F["force_sq"][0]:][:, :14].any() and stepped.got[:, F["left_contact"][0]].any()
    assert {k: v for k, v in F.items()} == stepped.fields


def test_conditions_on_every_robot(stepped):
    g, F, m = stepped.got.astype(np.float64), G.gait_fields(14), stepped.model
    col = lambda name: g[:, F[name][0]:F[name][0] + F[name][1]]  # noqa: E731
    per = col("periods")[:, 0]
    np.testing.assert_array_equal(per, stepped.end["acc"][:, 0])
    np.testing.assert_array_equal(per, stepped.rep["periods"])
    ds, fl = col("double_support")[:, 0], col("flight")[:, 0]
    cl, cr = col("left_contact")[:, 0], col("right_contact")[:, 0]
    assert (ds + fl <= per).all() and (cl + cr - 2 * ds + ds + fl == per).all()
    for foot, c in (("left", cl), ("right", cr)):
        assert (col(f"{foot}_touchdowns")[:, 0] <= per - c + 1).all()
    limited = np.asarray(m.actuator_forcelimited, dtype=bool)
    top = np.abs(np.asarray(m.actuator_forcerange, dtype=f32)).max(1)      # the physics clamps to the float32 range
    assert limited.any() and (col("force_max")[:, limited] <= top[limited].astype(np.float64)).all()
    assert (col("force_sat") <= per[:, None]).all() and (col("speed_sat") <= per[:, None]).all()


def test_gait_is_read_only_on_the_loop_and_off_means_no_call(stepped, policy_file, gpu, monkeypatch):
    off = _fleet(policy_file, gpu, gait=None)
    assert not off.gaited() and off.gait_rec is None
    calls, real = [0], off._lib.duck_fleet_gait

    def counting(*args):
        calls[0] += 1
        return real(*args)
    monkeypatch.setattr(off._lib, "duck_fleet_gait", counting)
    off.run(PERIODS)
    assert calls[0] == 0 and off.graph is None
    for name, want in stepped.end.items():
        np.testing.assert_array_equal(bits(getattr(off, name).cpu().numpy()), bits(want), err_msg=name)
    with pytest.raises(native.DuckError, match="no gait record"):
        off.gait_records()
    off.set_gait(True)
    off.run(1)
    assert calls[0] == 1 and off.gaited()
    off.set_gait(False)
    off.run(1)
    assert calls[0] == 1 and not off.gaited()


def test_graph_replay_equals_eager_and_restart_repeats(stepped, policy_file, gpu, monkeypatch):
    monkeypatch.setattr(FleetInfer, "CHUNK", 5)
    fleet = _fleet(policy_file, gpu, recorder=(4, 0))
    fleet.run(2)
    assert fleet.graph is None
    fleet.run(10)     # two replays of the 5-period graph
    assert fleet.graph is not None and fleet.graph[1] == 5
    np.testing.assert_array_equal(bits(fleet.gait_records()), bits(stepped.got))
    for name, want in stepped.end.items():
        np.testing.assert_array_equal(bits(getattr(fleet, name).cpu().numpy()), bits(want), err_msg=name)
    fleet.restart()
    assert fleet.gaited() and not bits(fleet.gait_records()).any() and fleet.graph is not None
    fleet.set_commands(commands(N, seed=41))
    fleet.run(PERIODS)
    np.testing.assert_array_equal(bits(fleet.gait_records()), bits(stepped.got))
    fleet.reset_report()
    assert not bits(fleet.gait_records()).any() and not bits(fleet.acc.cpu().numpy()).any()
    assert fleet.graph is not None and fleet.gait_desc.speed_sat == f32(5.24)
    fleet.set_gait(True, 0.5, 0.5)                              # switching it drops the captured graph
    assert fleet.graph is None and fleet.gait_desc.speed_sat == f32(2.62)
    assert not fleet.replay(0, frame=-1).gaited()               # a frame does not carry the gait state


def test_a_robot_is_its_global_id_and_a_followed_log_repeats_its_gait(stepped, policy_file, gpu):
    """Robot 20 of 33 equals the same robot alone; and a fleet without a policy that follows the log the lone robot
    made keeps the record the lone robot kept."""
    src = FleetInfer("flat_terrain", policy_file, N, device=gpu, randomize=SEED)
    row = slice(ROBOT, ROBOT + 1)

    def lone(policy, **kw):
        one = FleetInfer("flat_terrain", policy, 1, device=gpu, randomize=0, robot_offset=ROBOT, pushes=_pushes(row),
                         gait=(True,), **kw)
        one.dr.copy_(src.dr.view(-1, N)[:, ROBOT])
        one.restart()
        return one
    one = lone(policy_file)
    one.set_commands(commands(N, seed=41)[ROBOT])
    a = one.run(PERIODS, record=True)
    mine = one.gait_records()
    np.testing.assert_array_equal(bits(mine[0]), bits(stepped.got[ROBOT]))
    assert mine[0, G.gait_fields(14)["periods"][0]] == PERIODS
    b = one.run(1, record=True)
    log = sim2sim.log_from_saved_obs(np.concatenate([a, b])[:, 0])
    assert log.shape[0] == PERIODS
    follower = lone(None, follow=(log, None))
    assert follower.following() and follower._policy_args is None and follower.gaited()
    follower.run(PERIODS)
    np.testing.assert_array_equal(bits(follower.gait_records()), bits(mine))
    assert not bits(follower.scores()).any()
