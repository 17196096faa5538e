"""Host side of the fleet loop's gait record (include/duck_fleet.h duck_fleet_gait; sim2sim.FleetInfer.set_gait):
the C-ABI symbol, the record's macros, the descriptor from the four shipped scenes, the refusals that need no
launch, the restatement (tests/fleet_gait_reference.py) on a scripted contact sequence, the reports on hand-made
records with known answers, and the command line. No GPU."""

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from open_duck_playground_amd import cabi, constants, native, sim2sim
from open_duck_playground_amd.mjcf import Model
from tests import fleet_gait_reference as G
from tests import fleet_reference as R
from tests.fleet_helpers import bits, host_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SCENES = ("flat_terrain", "rough_terrain", "flat_terrain_backlash", "rough_terrain_backlash")


# --- the C ABI --------------------------------------------------------------------------
def test_symbol_and_struct():
    hdr = open(os.path.join(ROOT, "include", "duck_fleet.h")).read()
    L = native.lib()
    name = "duck_fleet_gait"
    assert re.search(rf"^int {name}\(", hdr, flags=re.M)
    assert name in native.EXPORTS and name in cabi.HEADERS.funcs and getattr(L, name).argtypes is not None
    f = cabi.HEADERS.funcs[name]
    assert len(f[1]) == 9 and f[1][0] == C.POINTER(native.DuckFleetDesc) and f[1][1] is C.c_void_p
    assert "[gait], [record]" in hdr and "duck_fleet_gait_desc" not in cabi.HEADERS.structs
    assert cabi.FLEET_GAIT_HEADERS.structs["duck_fleet_gait_desc"] is native.DuckFleetGaitDesc
    assert cabi.FLEET_GAIT_HEADERS.structs["duck_fleet_desc"] is native.DuckFleetDesc and not cabi.FLEET_GAIT_HEADERS.funcs


def test_struct_layout_equals_the_c_compilers():
    """sizeof, and every field's offsetof, size and scalar type of duck_fleet_gait_desc, asserted at compile time
    through duck_fleet.h alone, which brings the descriptor's header along; and the assertions do bite."""
    S, name = native.DuckFleetGaitDesc, "duck_fleet_gait_desc"
    assert [k for k, _ in S._fields_] == ["foot_linvel", "foot_pos", "force_sat", "speed_sat"]
    assert C.sizeof(S) == 4 * (2 + 2 + native.FLEET_MAX_NU + 1) and S.force_sat.offset == 16
    names = {C.c_int: "int", C.c_float: "float"}
    lines = [f'_Static_assert(sizeof({name}) == {C.sizeof(S)}, "sizeof");']
    for field, typ in S._fields_:
        f, at = getattr(S, field), f"(({name}*)0)->{field}"
        lines.append(f'_Static_assert(offsetof({name}, {field}) == {f.offset}, "offsetof {field}");')
        lines.append(f'_Static_assert(sizeof({at}) == {f.size}, "sizeof {field}");')
        while issubclass(typ, C.Array):
            typ, at = typ._type_, at + "[0]"
        lines.append(f'_Static_assert(_Generic({at}, {names[typ]}: 1, default: 0), "type of {field}");')
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to read the headers with"

    def compiles(body, first="duck_fleet.h"):
        src = f'#include <stddef.h>\n#include "{first}"\n#include "duck_fleet.h"\n' + "\n".join(body) + "\n"
        return subprocess.run([cc, "-x", "c", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                              input=src.encode(), capture_output=True)
    for first in ("duck_fleet.h", "duck_fleet_gait.h"):       # either header first
        r = compiles(lines, first)
        assert r.returncode == 0, r.stderr.decode()
    for good, bad in ((f"sizeof({name}) == {C.sizeof(S)},", f"sizeof({name}) == {C.sizeof(S) + 4},"),
                      (f"offsetof({name}, speed_sat) == {S.speed_sat.offset},", f"offsetof({name}, speed_sat) == {S.speed_sat.offset + 4},"),
                      (f"_Generic((({name}*)0)->speed_sat, float:", f"_Generic((({name}*)0)->speed_sat, int:")):
        assert sum(good in ln for ln in lines) == 1, good
        assert compiles([ln.replace(good, bad) for ln in lines]).returncode != 0, bad


@pytest.mark.parametrize("nu", [1, 3, 14, 16])
def test_offset_macros_are_the_gait_record(nu):
    """The header's macros against the tests' own statement of the record, field by field; the fields tile
    [0, DUCK_FLEET_GAIT_SIZE(nu)); sim2sim.gait_fields is the same mapping."""
    H = cabi.HEADERS
    want = G.gait_fields(nu)
    assert H.value(f"DUCK_FLEET_GAIT_SIZE({nu})") == G.gait_size(nu) == 7 * nu + 15
    for k, name in enumerate(G.ACTUATOR_FIELDS):
        assert H.value(f"DUCK_FLEET_GAIT_{name.upper()}({nu})") == want[name][0] == k * nu
    for name in ("periods", "double_support", "flight"):
        assert H.value(f"DUCK_FLEET_GAIT_{name.upper()}({nu})") == want[name][0]
    assert H.consts["DUCK_FLEET_GAIT_FOOT_SIZE"] == len(G.FOOT_FIELDS) == 6
    for f, foot in enumerate(G.FEET):
        for name in G.FOOT_FIELDS:
            at = H.value(f"DUCK_FLEET_GAIT_FOOT({nu}, {f})") + H.consts[f"DUCK_FLEET_GAIT_FOOT_{name.upper()}"]
            assert at == want[f"{foot}_{name}"][0]
    spans = sorted(want.values())
    assert spans[0][0] == 0 and all(a + w == b for (a, w), (b, _) in zip(spans, spans[1:]))
    assert spans[-1][0] + spans[-1][1] == G.gait_size(nu)
    assert sim2sim.gait_fields(nu) == want
    assert sim2sim.GAIT_ACTUATOR_FIELDS == G.ACTUATOR_FIELDS and sim2sim.GAIT_FOOT_FIELDS == G.FOOT_FIELDS


@pytest.mark.parametrize("scene", SCENES)
def test_descriptor_comes_from_the_model(scene):
    m = Model.load(constants.task_to_xml(scene))
    d = sim2sim.gait_desc(m)
    names = m.names["sensor"]
    adr = lambda name: int(m.sensor_adr[names.index(name)])  # noqa: E731
    assert list(d.foot_linvel) == [adr("left_foot_global_linvel"), adr("right_foot_global_linvel")]
    assert list(d.foot_pos) == [adr("left_foot_pos"), adr("right_foot_pos")]
    assert all(0 <= a and a + 3 <= m.nsensordata for a in list(d.foot_linvel) + list(d.foot_pos))
    assert len(set(list(d.foot_linvel) + list(d.foot_pos))) == 4
    assert d.speed_sat == f32(5.24)
    limited = np.asarray(m.actuator_forcelimited, dtype=bool)
    top = np.abs(np.asarray(m.actuator_forcerange, dtype=np.float64)).max(1)
    assert limited.any()
    for a in range(native.FLEET_MAX_NU):
        if a < m.nu and limited[a]:
            assert d.force_sat[a] == f32(0.9 * top[a]) and d.force_sat[a] > 0
        else:
            assert d.force_sat[a] == np.inf
    half = sim2sim.gait_desc(m, force_frac=0.5, speed_frac=0.25)
    assert half.speed_sat == f32(0.25 * 5.24)
    assert [half.force_sat[a] for a in np.flatnonzero(limited)] == [f32(0.5 * top[a]) for a in np.flatnonzero(limited)]
    with pytest.raises(native.DuckError, match="fractions"):
        sim2sim.gait_desc(m, force_frac=-1.0)
    with pytest.raises(native.DuckError, match="fractions"):
        sim2sim.gait_desc(m, speed_frac=float("nan"))


def test_refusals_come_before_any_launch():
    L = native.lib()
    d, s = host_desc(), native.DuckFleetGaitDesc()
    d.sens_off, d.con_off = 94, 150
    s.foot_linvel[0], s.foot_linvel[1], s.foot_pos[0], s.foot_pos[1] = 0, 3, 6, 9
    one = C.c_void_p(16)   # (never dereferenced: every call below is refused before any launch)
    name, nptr = "duck_fleet_gait", 5
    f = getattr(L, name)

    def call(desc=C.byref(d), gd=C.byref(s), n=1, null=None):
        return f(desc, gd, n, *[None if k == null else one for k in range(nptr)], None)
    assert call(desc=None) == -1 and f"{name}: null pointer".encode() in L.duck_last_error()
    assert call(gd=None) == -1 and f"{name}: null pointer".encode() in L.duck_last_error()
    for k in range(nptr):
        assert call(null=k) == -1 and f"{name}: null pointer".encode() in L.duck_last_error(), k
    for n in (-1, (1 << 27) + 1):
        assert call(n=n) == -1 and f"{name}: bad size".encode() in L.duck_last_error()
    d.nu = 17
    assert call() == -1 and b"nu" in L.duck_last_error()
    d.nu = 14
    assert call(n=0) == 0          # an empty fleet
    for field in ("foot_linvel", "foot_pos"):
        for k in range(2):
            keep = getattr(s, field)[k]
            for adr in (-1, 150 - 94 - 2, 1 << 30):
                getattr(s, field)[k] = adr
                assert call(n=0) == -1 and f"{name}: foot sensor address".encode() in L.duck_last_error(), (field, k, adr)
            getattr(s, field)[k] = 150 - 94 - 3
            assert call(n=0) == 0
            getattr(s, field)[k] = keep
    d.naux = 4 * 20 + 14 - 1
    d.sens_off = d.con_off = 0
    assert call(n=0) == -1 and f"{name}: actuator_force rows".encode() in L.duck_last_error()


# --- the restatement -------------------------------------------------------------------------
def _scripted(contact, z, alive=None, vx=None):
    """One robot (nu = 3) through a scripted sequence: ``contact`` [T][2] booleans, ``z`` [T][2] heights. Returns
    (the record, the bookkeeping of every call)."""
    d = R.make_desc(nu=3)
    s = G.make_gait_desc(d)
    rec, did = np.zeros((1, G.gait_size(3)), f32), []
    for t in range(len(contact)):
        aux, qvel = np.ones((d.naux, 1), f32), np.full((d.nv, 1), 2, f32)
        ctl = np.zeros((1, R.ctl_size(3)), f32)
        ctl[0, :3], ctl[0, 3:6] = 0.5, 0.25
        for k in range(2):
            aux[d.con_off + d.foot_con[k] + 1] = -1 if contact[t][k] else 1
            aux[d.sens_off + s.foot_pos[k] + 2] = z[t][k]
            aux[d.sens_off + s.foot_linvel[k]] = 0.0 if vx is None else vx[t][k]
            aux[d.sens_off + s.foot_linvel[k] + 1] = 0.0
        a = np.ones(1, f32) if alive is None else np.array([alive[t]], f32)
        did.append(G.gait(d, s, qvel, aux, ctl, a, rec))
    return rec[0], did


def test_restatement_on_a_scripted_contact_sequence():
    """The first period makes no touchdown, then one touchdown per swing, and apex_sum is the hand sum."""
    left = [1, 0, 0, 0, 1, 1, 0, 0, 1, 1]
    right = [1, 1, 1, 0, 0, 1, 1, 1, 0, 1]
    zl = [0.0, 0.02, 0.05, 0.03, 0.01, 0.0, 0.04, 0.02, 0.005, 0.0]
    zr = [0.0, 0.0, 0.0, 0.06, 0.07, 0.02, 0.0, 0.0, 0.03, 0.01]
    vx = [[0.5 if t == 4 else 0.0, 0.25 if t == 5 else 0.0] for t in range(10)]
    rec, did = _scripted(list(zip(left, right)), list(zip(zl, zr)), vx=vx)
    F = G.gait_fields(3)
    get = lambda name: rec[F[name][0]:F[name][0] + F[name][1]]  # noqa: E731
    assert not did[0].touchdown.any() and not did[0].liftoff.any() and did[0].first.all()
    assert [int(x.touchdown[0, 0]) for x in did] == [0, 0, 0, 0, 1, 0, 0, 0, 1, 0]
    assert [int(x.touchdown[0, 1]) for x in did] == [0, 0, 0, 0, 0, 1, 0, 0, 0, 1]
    assert [int(x.liftoff[0, 0]) for x in did] == [0, 1, 0, 0, 0, 0, 1, 0, 0, 0]
    assert get("periods") == 10 and get("left_touchdowns") == 2 and get("right_touchdowns") == 2
    assert get("left_contact") == 5 and get("right_contact") == 7
    assert get("double_support") == 3 and get("flight") == 1          # periods 0, 5 and 9; period 3
    # the highest sample of each swing over the landing sample, summed in float32 in order
    want_l = f32(f32(f32(0.05) - f32(0.01)) + f32(f32(0.04) - f32(0.005)))
    want_r = f32(f32(f32(0.07) - f32(0.02)) + f32(f32(0.03) - f32(0.01)))
    assert bits(get("left_apex_sum")) == bits(want_l) and bits(get("right_apex_sum")) == bits(want_r)
    assert get("left_slip") == f32(0.25) and get("right_slip") == f32(0.0625)
    assert get("left_prev") == 1 and get("right_prev") == 1
    # the actuators: f = 1, w = 2, thresholds 1.0, 1.25, 1.5 and 5.24, actions 0.5 after 0.25
    assert (get("force_sq") == 10).all() and (get("force_max") == 1).all() and (get("speed_max") == 2).all()
    assert list(get("force_sat")) == [10, 0, 0] and (get("speed_sat") == 0).all()
    assert (get("work") == 20).all() and (get("action_rate") == f32(10 * 0.0625)).all()


def test_restatement_leaves_a_dead_robot_alone():
    contact, z = [(1, 0), (0, 1), (1, 1), (0, 0)], [(0.0, 0.1)] * 4
    rec, did = _scripted(contact, z, alive=[1, 1, 0, 0])
    two, _ = _scripted(contact[:2], z[:2])
    assert (bits(rec) == bits(two)).all() and not did[2].live.any() and not did[3].contact.any()
    F = G.gait_fields(3)
    assert rec[F["periods"][0]] == 2
    # a foot that starts in the air: the first period's height is its apex, its first landing is a touchdown
    assert did[1].touchdown[0, 1] and rec[F["right_apex_sum"][0]] == f32(0.1) - f32(0.1)
    assert rec[F["right_apex"][0]] == f32(0.1)


# --- the reports ----------------------------------------------------------------------------
class _Model:
    """What the reports read of a compiled model."""
    body_mass = np.array([0.0, 1.0, 0.5])
    opt_gravity = np.array([0.0, 0.0, -10.0])
    names = {"actuator": ["hip", "knee", "ankle"]}


def _record(nu=3, **fields):
    g, F = np.zeros(G.gait_size(nu), f32), G.gait_fields(nu)
    for name, v in fields.items():
        g[F[name][0]:F[name][0] + F[name][1]] = v
    return g


def test_gait_report_on_hand_made_records():
    a = _record(periods=100, force_sq=[400, 100, 0], force_max=[3, 2, 0], force_sat=[25, 0, 0], speed_max=[6, 1, 0],
                speed_sat=[10, 0, 0], work=[50, 25, 0], action_rate=[4, 1, 0], double_support=20, flight=5,
                left_contact=60, left_touchdowns=5, left_slip=0.6, left_apex_sum=0.1,
                right_contact=55, right_touchdowns=4, right_slip=0.0, right_apex_sum=0.2)
    b = _record()                                                  # a robot that survived no period
    acc = np.array([[100, 30.0, 40.0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], f32)
    rep = sim2sim.gait_report(np.stack([a, b]), acc, _Model)
    assert all(v.dtype == np.float64 and len(v) == 2 for v in rep.values())
    np.testing.assert_allclose(rep["force_rms"][0], [2, 1, 0])
    np.testing.assert_allclose(rep["force_peak"][0], [3, 2, 0])
    np.testing.assert_allclose(rep["force_sat"][0], [0.25, 0, 0])
    np.testing.assert_allclose(rep["speed_sat"][0], [0.1, 0, 0])
    np.testing.assert_allclose(rep["speed_peak"][0], [6, 1, 0])
    np.testing.assert_allclose(rep["mean_power"][0], [0.5, 0.25, 0])
    np.testing.assert_allclose(rep["action_rate_rms"][0], [0.2, 0.1, 0])
    np.testing.assert_allclose(rep["duty_factor"][0], [0.6, 0.55])
    np.testing.assert_allclose(rep["step_frequency"][0], [5 / 2.0, 4 / 2.0])     # touchdowns over 100 x 0.02 s
    np.testing.assert_allclose(rep["slip_rms"][0], [0.1, 0.0])
    np.testing.assert_allclose(rep["clearance"][0], [0.02, 0.05])
    np.testing.assert_allclose([rep["double_support"][0], rep["flight"][0]], [0.2, 0.05])
    # by hand: 75 x 0.02 J over 15 N x (|(0.3, 0.4)| m/s x 2 s) = 1.5 / 15 = 0.1
    np.testing.assert_allclose(rep["cost_of_transport"][0], 0.1)
    assert rep["periods"].tolist() == [100, 0]
    for key, v in rep.items():
        if key != "periods":
            assert np.isnan(v[1]).all(), key                       # zero periods -> NaN
    # a robot that stood still, and a foot that never landed
    c = _record(periods=10, work=[1, 0, 0], left_contact=10, right_contact=0)
    rep = sim2sim.gait_report(c[None], np.array([[10, 0, 0, 0, 0, 0]], f32), _Model)
    assert np.isnan(rep["cost_of_transport"][0]) and np.isnan(rep["clearance"][0]).all()
    assert rep["duty_factor"][0].tolist() == [1.0, 0.0] and rep["step_frequency"][0].tolist() == [0.0, 0.0]
    assert rep["slip_rms"][0][0] == 0 and np.isnan(rep["slip_rms"][0][1])
    with pytest.raises(native.DuckError, match="no gait record"):
        sim2sim.gait_report(np.zeros((1, 40), f32), acc[:1], _Model)


def test_gait_summary_pools_sums_and_maxima():
    a = _record(periods=100, force_sq=[400, 100, 0], force_max=[3, 2, 0], work=[50, 25, 0], left_contact=60,
                left_touchdowns=5, left_apex_sum=0.1, left_prev=1, left_apex=0.3, double_support=20)
    b = _record(periods=50, force_sq=[200, 50, 0], force_max=[1, 5, 0], work=[25, 0, 0], left_contact=15,
                left_touchdowns=3, left_apex_sum=0.06, flight=5)
    dead = _record()
    acc = np.array([[100, 30, 40, 0, 0, 0], [50, 0, 25, 0, 0, 0], [0, 0, 0, 0, 0, 0]], f32)
    g = np.stack([a, b, dead])
    s = sim2sim.gait_summary(g, acc, None, _Model)
    assert s["count"] == 3 and s["periods"] == 150 and s["actuators"] == ["hip", "knee", "ankle"] and s["feet"] == ["left", "right"]
    np.testing.assert_allclose(s["force_rms"], [2, 1, 0])
    assert s["force_peak"] == [3, 5, 0]
    np.testing.assert_allclose(s["duty_factor"], [0.5, 0])
    np.testing.assert_allclose(s["step_frequency"], [8 / 3.0, 0])
    np.testing.assert_allclose(s["clearance"][0], 0.02)
    assert s["clearance"][1] is None and s["slip_rms"][1] is None
    np.testing.assert_allclose([s["double_support"], s["flight"]], [20 / 150, 5 / 150])
    # 100 x 0.02 J over 15 N x (50 + 25) x 0.02 m
    np.testing.assert_allclose(s["cost_of_transport"], 2.0 / (15 * 1.5))
    import json
    json.dumps(s)
    one = sim2sim.gait_summary(g, acc, np.array([False, True, False]), _Model)
    assert one["count"] == 1 and one["periods"] == 50 and one["force_peak"] == [1, 5, 0]
    np.testing.assert_allclose(one["cost_of_transport"], 0.5 / (15 * 0.5))
    per = sim2sim.gait_report(g, acc, _Model)
    np.testing.assert_allclose(one["cost_of_transport"], per["cost_of_transport"][1])
    none = sim2sim.gait_summary(g, acc, np.array([False, False, True]), _Model)
    assert none["periods"] == 0 and none["cost_of_transport"] is None and none["force_rms"] == [None] * 3
    empty = sim2sim.gait_summary(g, acc, np.zeros(3, bool), _Model)
    assert empty["count"] == 0 and empty["force_peak"] == [None] * 3 and empty["double_support"] is None


# --- the command line ------------------------------------------------------------------------
def test_parser_and_report_without_the_flag():
    a = sim2sim.parse_arguments(["-o", "p.onnx"])
    assert a.gait is False and sim2sim.gait_plan(a) is None
    doc = {"cells": [{"command": [0, 0, 0]}], "policies": [{"policy": 0}]}
    assert sim2sim.add_gait_report(doc, None, None, _Model, [0]) is doc
    assert "gait" not in doc and "gait" not in doc["cells"][0] and "gait" not in doc["policies"][0]
    a = sim2sim.parse_arguments(["-o", "p.onnx", "--gait"])
    assert sim2sim.gait_plan(a) == (True, 0.9, 1.0)
    a = sim2sim.parse_arguments(["-o", "p.onnx", "--gait", "--gait_force_frac", "0.5", "--gait_speed_frac", "0.8"])
    assert sim2sim.gait_plan(a) == (True, 0.5, 0.8)
    with pytest.raises(SystemExit):
        sim2sim.parse_arguments(["-o", "p.onnx", "--gait", "--gait_force_frac", "-1"])


def test_report_with_the_flag():
    g = np.stack([_record(periods=10, work=[1, 0, 0]), _record(periods=20, work=[3, 0, 0]), _record(periods=5),
                  _record(periods=7)])
    acc = np.array([[10, 1, 0, 0, 0, 0], [20, 2, 0, 0, 0, 0], [5, 1, 0, 0, 0, 0], [7, 1, 0, 0, 0, 0]], f32)
    doc = {"cells": [{"command": [0, 0, 0]}, {"command": [1, 0, 0]}], "policies": [{"policy": 0}, {"policy": 1}]}
    sim2sim.add_gait_report(doc, g, acc, _Model, [0, 1, 0, 1], seg=[0, 2, 4])
    assert doc["gait"]["periods"] == 42 and doc["gait"]["count"] == 4
    assert [row["gait"]["periods"] for row in doc["cells"]] == [15, 27]
    assert [row["gait"]["periods"] for row in doc["policies"]] == [30, 12]
    only = {"cells": [{}, {}]}
    sim2sim.add_gait_report(only, g, acc, _Model, [0, 1, 0, 1])
    assert "policies" not in only and only["cells"][1]["gait"]["count"] == 2
