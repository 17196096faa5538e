"""Host side of the fleet loop's flight recorder (include/duck_fleet.h duck_fleet_record; sim2sim.FleetInfer's
set_recorder / recorded / replay): the header's macro and declaration, the frame's field map, the numpy
restatement of the rule (tests/fleet_record_reference.py) on constructed fall schedules, the ring's unrolling
and the command line's flags. No GPU."""

import numpy as np
import pytest

from open_duck_playground_amd import sim2sim
from open_duck_playground_amd.cabi import HEADERS
from tests import fleet_record_reference as K
from tests import fleet_reference as R

f32 = np.float32
SENTINEL = np.int32(0x7FC0BEEF)       # a NaN with a payload: no frame of the tests below holds it


# --- the C ABI --------------------------------------------------------------------------
def test_frame_size_macro():
    assert HEADERS.value("DUCK_FLEET_FRAME_SIZE(21,20,14)") == 283
    assert HEADERS.consts["DUCK_FLEET_SENS_SIZE"] == 12
    for nq, nv, nu in ((21, 20, 14), (9, 8, 3), (23, 22, 16)):
        want = nq + 2 * nv + HEADERS.value(f"DUCK_FLEET_CTL_SIZE({nu})") + HEADERS.value(f"DUCK_FLEET_OBS_SIZE({nu})") \
            + 2 * nu + HEADERS.consts["DUCK_FLEET_SENS_SIZE"]
        assert HEADERS.value(f"DUCK_FLEET_FRAME_SIZE({nq},{nv},{nu})") == want == K.frame_size(nq, nv, nu)


def test_record_is_declared_with_16_arguments():
    assert "duck_fleet_record" in HEADERS.funcs
    restype, argtypes = HEADERS.funcs["duck_fleet_record"]
    assert len(argtypes) == 16 and restype is not None


@pytest.mark.parametrize("nq,nv,nu", [(21, 20, 14), (9, 8, 3), (23, 22, 16)])
def test_frame_fields_partition_the_frame(nq, nv, nu):
    F = sim2sim.frame_fields(nq, nv, nu)
    assert list(F) == ["qpos", "qvel", "qacc_warmstart", "ctl", "obs", "action", "actuator_force", "sensors"]
    at = 0
    for name, (o, w) in F.items():
        assert o == at and w >= 1, name
        at += w
    assert at == HEADERS.value(f"DUCK_FLEET_FRAME_SIZE({nq},{nv},{nu})")
    assert F["ctl"][1] == HEADERS.value(f"DUCK_FLEET_CTL_SIZE({nu})") == sum(w for _, w in sim2sim.ctl_fields(nu).values())
    assert F["obs"][1] == HEADERS.value(f"DUCK_FLEET_OBS_SIZE({nu})")
    assert [F[k][1] for k in ("qpos", "qvel", "qacc_warmstart", "action", "actuator_force", "sensors")] == [nq, nv, nv, nu, nu, 12]
    assert len(sim2sim.FRAME_SENSORS) * 3 == F["sensors"][1] and sim2sim.FRAME_SENSORS == K.SENSORS


# --- the restatement of the rule ------------------------------------------------------------------
def _inputs(d, n, rng):
    z = lambda *s: rng.normal(size=s).astype(f32)  # noqa: E731
    return dict(qpos=z(d.nq, n), qvel=z(d.nv, n), warm=z(d.nv, n), aux=z(d.naux, n), ctl=z(n, R.ctl_size(d.nu)),
                obs=z(n, R.obs_size(d.nu)), action=z(n, d.nu))


def _run(d, n, depth, post, calls, dies_at, seed=0):
    """``calls`` calls of the restatement on fresh inputs; robot e's alive is cleared before call dies_at[e]
    (1-based; 0: never). Returns (ring, head, after, every call's frames [calls][N][F], the ring after each call)."""
    rng = np.random.default_rng(seed)
    F = K.frame_size(d.nq, d.nv, d.nu)
    ring = np.full((n, depth, F), SENTINEL, np.int32)
    head, after = np.zeros(n, np.int32), np.zeros(n, np.int32)
    alive = np.ones(n, f32)
    seen, rings = [], []
    for call in range(1, calls + 1):
        alive[(dies_at > 0) & (dies_at <= call)] = 0
        x = _inputs(d, n, rng)
        seen.append(K.frames(d, **x))
        K.record_step(d, depth, post, alive=alive, head=head, after=after, ring=ring, **x)
        rings.append(ring.copy())
    return ring, head, after, np.array(seen), rings


def test_a_robot_alive_throughout_holds_the_last_depth_calls():
    d, depth = R.make_desc(), 4
    calls = 2 * depth + 3                                   # wraps twice
    ring, head, after, seen, _ = _run(d, 2, depth, 1, calls, np.zeros(2, int))
    assert list(head) == [calls, calls] and list(after) == [0, 0]
    for e in range(2):
        frames, period = sim2sim.unroll_ring(ring[e], head[e], depth)
        assert list(period) == list(range(calls - depth + 1, calls + 1))
        np.testing.assert_array_equal(frames, seen[calls - depth:, e])
    assert not (ring == SENTINEL).any()


@pytest.mark.parametrize("post", [0, 2])
def test_a_robot_dying_at_call_c_holds_up_to_c_plus_post_and_is_frozen(post):
    d, depth, calls = R.make_desc(), 5, 12
    dies = np.array([0, 3, 7, 4])                           # robot 0 lives; 1 dies before the ring wraps; 2 after it has
    ring, head, after, seen, rings = _run(d, 4, depth, post, calls, dies)
    for e, c in enumerate(dies):
        if c == 0:
            continue
        last = c + post
        assert head[e] == last and after[e] == post + 1
        frames, period = sim2sim.unroll_ring(ring[e], head[e], depth)
        assert list(period) == list(range(max(last - depth, 0) + 1, last + 1))
        np.testing.assert_array_equal(frames, seen[period - 1, e])
        for later in rings[last - 1:]:                     # byte-identical afterwards, however the inputs change
            assert later[e].tobytes() == rings[last - 1][e].tobytes()
        held = min(last, depth)
        assert ((ring[e] == SENTINEL).all(axis=1).sum()) == depth - held   # the slots never written keep the sentinel
    assert head[0] == calls and after[0] == 0


@pytest.mark.parametrize("post", [0, 1, 3])
def test_a_robot_dead_from_the_first_call_writes_post_plus_one_frames(post):
    d, depth = R.make_desc(), 6
    ring, head, after, seen, _ = _run(d, 2, depth, post, 9, np.array([1, 0]))
    assert head[0] == post + 1 and after[0] == post + 1 and head[1] == 9
    frames, period = sim2sim.unroll_ring(ring[0], head[0], depth)
    assert list(period) == list(range(1, post + 2))
    np.testing.assert_array_equal(frames, seen[:post + 1, 0])
    assert (ring[0, post + 1:] == SENTINEL).all()


def test_depth_one_holds_the_last_written_frame():
    d = R.make_desc()
    ring, head, after, seen, _ = _run(d, 3, 1, 1, 7, np.array([0, 3, 1]))
    np.testing.assert_array_equal(ring[0, 0], seen[6, 0])       # alive: call 7
    np.testing.assert_array_equal(ring[1, 0], seen[3, 1])       # died at 3, post 1: call 4
    np.testing.assert_array_equal(ring[2, 0], seen[1, 2])       # dead from the start: call 2
    assert list(head) == [7, 4, 2] and list(after) == [0, 2, 2]
    for e in range(3):
        frames, period = sim2sim.unroll_ring(ring[e], head[e], 1, rec_base=10)
        assert list(period) == [10 + head[e]] and frames.tobytes() == ring[e].tobytes()


def test_frames_keep_their_bits():
    d = R.make_desc()
    rng = np.random.default_rng(5)
    x = _inputs(d, 2, rng)
    for a in x.values():
        w = a.view(np.int32)
        w.flat[0], w.flat[1], w.flat[2] = 0x7FC12345, np.int32(-0x80000000), 1    # a payload NaN, -0, a denormal
    fr = K.frames(d, **x)
    F = sim2sim.frame_fields(d.nq, d.nv, d.nu)
    assert fr[0, F["qpos"][0]] == 0x7FC12345 and fr[1, F["qpos"][0]] == np.int32(-0x80000000)
    o = F["ctl"][0]
    assert list(fr[0, o:o + 3]) == [0x7FC12345, np.int32(-0x80000000), 1]
    # the layout, against the named sources
    np.testing.assert_array_equal(fr[:, F["actuator_force"][0]:][:, :d.nu], x["aux"].view(np.int32)[4 * d.nv:4 * d.nv + d.nu].T)
    s = F["sensors"][0]
    for k, name in enumerate(K.SENSORS):
        row = d.sens_off + getattr(d, name)
        np.testing.assert_array_equal(fr[:, s + 3 * k:s + 3 * k + 3], x["aux"].view(np.int32)[row:row + 3].T)
    np.testing.assert_array_equal(fr[:, F["obs"][0]:][:, :F["obs"][1]], x["obs"].view(np.int32))
    np.testing.assert_array_equal(fr[:, F["qacc_warmstart"][0]:][:, :d.nv], x["warm"].view(np.int32).T)


# --- the unrolling ---------------------------------------------------------------------------------
@pytest.mark.parametrize("head,want", [(0, []), (3, [1, 2, 3]), (5, [1, 2, 3, 4, 5]), (13, [9, 10, 11, 12, 13])])
def test_unrolling_gives_period_order(head, want):
    depth, F = 5, 4
    ring = np.full((depth, F), -1.0, f32)
    for j in range(1, head + 1):                            # the j-th frame written holds j
        ring[(j - 1) % depth] = j
    frames, period = sim2sim.unroll_ring(ring, head, depth, rec_base=100)
    assert list(period) == [100 + j for j in want]
    assert frames.shape == (len(want), F) and [int(v) for v in frames[:, 0]] == want
    flat, _ = sim2sim.unroll_ring(ring.reshape(-1), head, depth)
    np.testing.assert_array_equal(flat, frames)


# --- the command line -------------------------------------------------------------------------------
def test_parser_accepts_the_recorder_flags(capsys):
    a = sim2sim.parse_arguments(["-o", "p.onnx", "--record_falls", "50", "--record_post", "3", "--record_out", "falls.npz",
                                 "--record_max", "5"])
    assert (a.record_falls, a.record_post, a.record_out, a.record_max) == (50, 3, "falls.npz", 5)
    a = sim2sim.parse_arguments(["-o", "p.onnx", "--record_falls", "8"])
    assert (a.record_falls, a.record_post, a.record_out, a.record_max) == (8, 0, None, 64)
    a = sim2sim.parse_arguments(["-o", "p.onnx"])
    assert a.record_falls is None and a.record_out is None and a.push_magnitude is None
    a = sim2sim.parse_arguments(["-o", "p.onnx", "--push_grid", "1x2", "--push_magnitude", "3", "4.5"])
    assert a.push_magnitude == [3.0, 4.5]
    plan = sim2sim.disturbance_plan(a, sim2sim.command_grid("1x1x1"))
    assert (plan["pushes"][2] == f32(3.75)).all() and plan["echo"]["push_magnitude"] == [3.0, 4.5]
    for bad in (["--record_out", "falls.npz"], ["--record_falls", "0"], ["--record_falls", "4", "--record_post", "-1"]):
        with pytest.raises(SystemExit) as e:
            sim2sim.parse_arguments(["-o", "p.onnx"] + bad)
        assert e.value.code == 2
    assert "--record_out needs --record_falls" in capsys.readouterr().err
