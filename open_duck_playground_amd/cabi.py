"""The C-ABI structs and constants of ``include/*.h`` as ctypes, read from the headers (``cdecl.py``).

Shared by the product binding (``native.py`` -> ``libduck.so``) and by the test-only
oracle binding (``tests/oracle_ffi.py`` -> ``oracle/liboracle.so``). Nothing here computes
physics; it only lays out host memory for the C side.
"""

from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List

import numpy as np

from . import cdecl
from .mjcf import Model

_I = C.POINTER(C.c_int)
_D = C.POINTER(C.c_double)

INCLUDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
# The C ABI as include/*.h states it: every struct class, constant and prototype below and in native.py
# is read from the headers. duck_mlp_problem's and duck_gather_field's pointers are device addresses,
# which callers hold as integers.
HEADERS = cdecl.Header(*(os.path.join(INCLUDE, f) for f in ("duck_model.h", "duck_env.h", "duck.h", "duck_ppo.h",
                                                            "duck_fleet.h")),
                       address_structs=("duck_mlp_problem", "duck_gather_field"))
# duck_fleet_gait's descriptor has a header of its own (duck_fleet.h declares the type and includes it), read on
# top of the others: a duck_fleet_gait_desc* parameter of HEADERS' prototypes is an address, which takes byref
FLEET_GAIT_HEADERS = cdecl.Header(os.path.join(INCLUDE, "duck_fleet_gait.h"), base=HEADERS)

# words (uint64) of duck_debug_stage_cycles' buffer
STAGE_CYCLES_WORDS = HEADERS.consts["DUCK_STAGE_CYCLES_WORDS"]

DuckModelDesc = HEADERS.structs["duck_model_desc"]
DuckEnvConfig = HEADERS.structs["duck_env_config"]
DuckRefMotion = HEADERS.structs["duck_refmotion"]


class ModelDescHolder:
    """Owns the numpy buffers a :class:`DuckModelDesc` points into."""

    def __init__(self, m: Model):
        self._keep: List[np.ndarray] = []
        d = DuckModelDesc()
        for k in ("nq", "nv", "nu", "nbody", "njnt", "ngeom", "nsite", "nsensor", "nsensordata", "npair"):
            setattr(d, k, int(getattr(m, k)))
        d.timestep = m.opt_timestep
        d.gravity[:] = list(m.opt_gravity)
        d.impratio = m.opt_impratio
        d.tolerance = m.opt_tolerance
        d.ls_tolerance = m.opt_ls_tolerance
        d.meaninertia = m.stat_meaninertia
        d.iterations = m.opt_iterations
        d.ls_iterations = m.opt_ls_iterations
        d.eulerdamp = m.opt_eulerdamp
        for name, typ in DuckModelDesc._fields_:
            if typ is _I or typ is _D:
                src = name
                if name.startswith("hull_"):
                    continue
                if name == "hfield_data":
                    continue
                arr = m.arrays[src]
                setattr(d, name, self._ptr(arr, typ))
        h = m.hulls[0]
        d.hull_nvert, d.hull_nface, d.hull_nedge = len(h.vert), len(h.face_normal), len(h.edge)
        d.hull_vert = self._ptr(h.vert, _D)
        d.hull_face_normal = self._ptr(h.face_normal, _D)
        d.hull_face_offset = self._ptr(h.face_offset, _D)
        d.hull_edge = self._ptr(h.edge, _I)
        d.hfield_nrow, d.hfield_ncol = int(m.hfield_nrow), int(m.hfield_ncol)
        d.hfield_size[:] = list(m.hfield_size)
        d.hfield_data = self._ptr(m.hfield_data if m.hfield_nrow else np.zeros(1), _D)
        self.desc = d

    def _ptr(self, arr, typ):
        if typ is _I:
            a = np.ascontiguousarray(arr, dtype=np.int32)
        else:
            a = np.ascontiguousarray(arr, dtype=np.float64)
        self._keep.append(a)
        return a.ctypes.data_as(typ)


def reference_frames(table: Dict[str, np.ndarray]) -> np.ndarray:
    """Polynomials evaluated (float64) at every phase t = i / nb: [nx, ny, nth, nb, ndim]."""
    nb = int(table["nb_steps_in_period"])
    t = np.arange(nb, dtype=np.float64) / nb
    c = np.asarray(table["coeffs"], dtype=np.float64)  # ascending powers
    out = np.zeros(c.shape[:3] + (nb, c.shape[3]))
    for k in range(c.shape[-1] - 1, -1, -1):  # Horner
        out = out * t[None, None, None, :, None] + c[:, :, :, None, :, k]
    return out


def refmotion_struct(table: Dict[str, np.ndarray]):
    r = DuckRefMotion()
    coeffs = np.ascontiguousarray(table["coeffs"], dtype=np.float64)
    frames = np.ascontiguousarray(reference_frames(table), dtype=np.float32)
    r.n_dx, r.n_dy, r.n_dtheta, r.n_dim, r.n_coef = coeffs.shape
    r.nb_steps_in_period = int(table["nb_steps_in_period"])
    r.dxs[:len(table["dxs"])] = [float(x) for x in table["dxs"]]
    r.dys[:len(table["dys"])] = [float(x) for x in table["dys"]]
    r.dthetas[:len(table["dthetas"])] = [float(x) for x in table["dthetas"]]
    r.dx_range[:] = [float(x) for x in table["dx_range"]]
    r.dy_range[:] = [float(x) for x in table["dy_range"]]
    r.dtheta_range[:] = [float(x) for x in table["dtheta_range"]]
    r.coeffs = coeffs.ctypes.data_as(C.POINTER(C.c_double))
    r.frames = frames.ctypes.data_as(C.POINTER(C.c_float))
    return r, (coeffs, frames)


# --------------------------------------------------------------------------------------
# layouts (mirror of duck_layout_make / duck_dr_layout_make in include/duck_env.h)
# --------------------------------------------------------------------------------------

@dataclass
class Layout:
    nq: int
    nv: int
    nu: int
    imitation: int
    task: int
    off: Dict[str, int]
    ioff: Dict[str, int]
    nfloat: int
    nint: int
    obs_size: int
    priv_size: int


TASK_JOYSTICK, TASK_STANDING = 0, 1


def layout(nq: int, nv: int, nu: int, imitation: bool, task: int = TASK_JOYSTICK) -> Layout:
    imitation = bool(imitation) and task == TASK_JOYSTICK
    if task == TASK_STANDING:  # standing.py:532-570
        obs = 3 + 3 + 7 + 5 * nu + 2
        priv = obs + 15 + 2 * nu + 1 + nu + 2 + 6 + 2
    else:
        obs = 3 + 3 + 7 + 6 * nu + 2 + 2
        priv = obs + 15 + 2 * nu + 1 + nu + 2 + 6 + 2 + (40 if imitation else 0) + 1 + 2
    fields = [("qpos", nq), ("qvel", nv), ("qacc_warmstart", nv), ("ctrl", nu), ("command", 7), ("last_act", nu),
              ("last_last_act", nu), ("last_last_last_act", nu), ("motor_targets", nu), ("feet_air_time", 2),
              ("last_contact", 2), ("swing_peak", 2), ("push", 2), ("action_history", 3 * nu), ("imu_history", 9),
              ("ref_motion", 40), ("imitation_phase", 2), ("metrics", 8), ("reward", 1), ("done", 1),
              ("truncation", 1), ("first_qpos", nq), ("first_qvel", nv), ("first_qacc_warmstart", nv),
              ("first_ctrl", nu), ("first_obs", obs), ("first_priv", priv)]
    off, o = {}, 0
    for k, n in fields:
        off[k] = o
        o += n
    ifields = [("rng_key", 2), ("rng_ctr", 1), ("step", 1), ("push_step", 1), ("push_interval", 1),
               ("imitation_i", 1), ("ep_steps", 1)]
    ioff, io = {}, 0
    for k, n in ifields:
        ioff[k] = io
        io += n
    return Layout(nq, nv, nu, int(imitation), int(task), off, ioff, o, io, obs, priv)


def dr_layout(nbody: int, nu: int) -> Dict[str, int]:
    out, o = {}, 0
    for k, n in [("floor_friction", 1), ("base_ipos", 3), ("body_mass", nbody), ("frictionloss", nu),
                 ("armature", nu), ("qpos0", nu), ("kp", nu)]:
        out[k] = o
        o += n
    out["nfloat"] = o
    return out


METRIC_NAMES = ["reward/tracking_lin_vel", "reward/tracking_ang_vel", "cost/torques", "cost/action_rate",
                "reward/alive", "reward/imitation", "cost/stand_still", "swing_peak"]
# standing.py:290-297 + :584-606 (slot 6 unused; swing_peak stays in slot 7)
STANDING_METRIC_NAMES = ["cost/orientation", "cost/torques", "cost/action_rate", "reward/alive", "cost/stand_still",
                         "cost/head_pos", None, "swing_peak"]


# --------------------------------------------------------------------------------------
# model fingerprint (mirror of duck_model_fingerprint in csrc/duck_capi.hip)
# --------------------------------------------------------------------------------------

def _fp_fields(d: DuckModelDesc):
    """(kind, name, count) in the hash order of duck_model_fingerprint."""
    nb, nj, nv, ng, np_, ns, nu = d.nbody, d.njnt, d.nv, d.ngeom, d.npair, d.nsite, d.nu
    out = []
    out += [("i", n, nb) for n in ("body_parentid", "body_rootid", "body_weldid", "body_jntnum", "body_jntadr",
                                   "body_dofnum", "body_dofadr")]
    out += [("f", "body_pos", 3 * nb), ("f", "body_quat", 4 * nb), ("f", "body_ipos", 3 * nb),
            ("f", "body_iquat", 4 * nb), ("f", "body_mass", nb), ("f", "body_inertia", 3 * nb),
            ("f", "body_invweight0", 2 * nb)]
    out += [("i", n, nj) for n in ("jnt_type", "jnt_qposadr", "jnt_dofadr", "jnt_bodyid", "jnt_limited")]
    out += [("f", "jnt_pos", 3 * nj), ("f", "jnt_axis", 3 * nj), ("f", "jnt_range", 2 * nj), ("f", "jnt_margin", nj),
            ("f", "jnt_solref", 2 * nj), ("f", "jnt_solimp", 5 * nj)]
    out += [("i", n, nv) for n in ("dof_bodyid", "dof_jntid", "dof_parentid")]
    out += [("f", n, nv) for n in ("dof_armature", "dof_damping", "dof_frictionloss", "dof_invweight0")]
    out += [("f", "dof_solref", 2 * nv), ("f", "dof_solimp", 5 * nv)]
    out += [("i", n, ng) for n in ("geom_type", "geom_bodyid", "geom_dataid")]
    out += [("f", "geom_pos", 3 * ng), ("f", "geom_quat", 4 * ng), ("f", "geom_rbound", ng), ("f", "geom_size", 3 * ng)]
    out += [("i", n, np_) for n in ("pair_geom1", "pair_geom2", "pair_condim")]
    out += [("f", "pair_friction", 5 * np_), ("f", "pair_solref", 2 * np_), ("f", "pair_solimp", 5 * np_),
            ("f", "pair_margin", np_)]
    return out


def model_fingerprint(m: Model) -> int:
    """Identity of a compiled kernel specialisation: FNV-1a 64 over the float32-rounded model values
    the generated header bakes (the same bytes duck_model_fingerprint hashes from a duck_model_desc)."""
    h = ModelDescHolder(m)
    d = h.desc
    buf = []
    buf.append(np.array([d.nq, d.nv, d.nu, d.nbody, d.njnt, d.ngeom, d.nsite, d.nsensor, d.nsensordata, d.npair,
                         d.iterations, d.ls_iterations, d.eulerdamp], dtype=np.int32).tobytes())
    buf.append(np.array([d.timestep, *d.gravity, d.impratio, d.tolerance, d.ls_tolerance, d.meaninertia],
                        dtype=np.float32).tobytes())

    def arr(kind, name, n):
        if n == 0:
            return b""
        p = getattr(d, name)
        a = np.ctypeslib.as_array(p, shape=(n,))
        return a.astype(np.int32 if kind == "i" else np.float32).tobytes()

    for kind, name, n in _fp_fields(d):
        buf.append(arr(kind, name, n))
    buf.append(np.array([d.hull_nvert, d.hull_nface, d.hull_nedge, d.hfield_nrow, d.hfield_ncol],
                        dtype=np.int32).tobytes())
    buf.append(arr("f", "hull_vert", 3 * d.hull_nvert))
    buf.append(arr("f", "hull_face_normal", 3 * d.hull_nface))
    buf.append(arr("f", "hull_face_offset", d.hull_nface))
    buf.append(arr("i", "hull_edge", 2 * d.hull_nedge))
    buf.append(np.array(list(d.hfield_size), dtype=np.float32).tobytes())
    ns, nu, nsen = d.nsite, d.nu, d.nsensor
    buf.append(arr("i", "site_bodyid", ns) + arr("f", "site_pos", 3 * ns) + arr("f", "site_quat", 4 * ns))
    for n in ("actuator_trnid", "actuator_ctrllimited", "actuator_forcelimited"):
        buf.append(arr("i", n, nu))
    for n in ("actuator_kp", "actuator_kv", "actuator_gear"):
        buf.append(arr("f", n, nu))
    buf.append(arr("f", "actuator_ctrlrange", 2 * nu) + arr("f", "actuator_forcerange", 2 * nu))
    for n in ("sensor_type", "sensor_objid", "sensor_adr", "sensor_dim"):
        buf.append(arr("i", n, nsen))
    buf.append(arr("f", "qpos0", d.nq))
    h64 = 1469598103934665603
    for c in b"".join(buf):
        h64 = ((h64 ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h64
