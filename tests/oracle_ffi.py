"""ctypes binding of the CPU oracle (oracle/liboracle.so) — test infrastructure only.

Used by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg as the checker;
the product path never imports this module.
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

import numpy as np

from open_duck_playground_amd import cabi, cdecl
from open_duck_playground_amd.cabi import (DuckEnvConfig, DuckRefMotion, ModelDescHolder, dr_layout, layout,
                                           refmotion_struct)
from open_duck_playground_amd.mjcf import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ORACLE_LIB selects another build of the same checker (oracle/Makefile ASAN=1: liboracle_asan.so)
LIB = os.environ.get("ORACLE_LIB") or os.path.join(ROOT, "oracle", "liboracle.so")

# oracle/duck_oracle.h on top of the product's headers (the same struct classes): oracle_data, the prototypes
HEADERS = cdecl.Header(os.path.join(ROOT, "oracle", "duck_oracle.h"), base=cabi.HEADERS)
MAXQ, MAXV, MAXU, MAXSD, MAXBODY, MAXSITE, MAXGEOM, MAXCON = (
    HEADERS.consts["DUCK_MAX" + k] for k in ("Q", "V", "U", "SENSORDATA", "BODY", "SITE", "GEOM", "CON"))


class OracleData(HEADERS.structs["oracle_data"]):
    def arr(self, name, n=None):
        a = np.ctypeslib.as_array(getattr(self, name))
        return a if n is None else a[:n]


def build(force: bool = False) -> str:
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < max(
            os.path.getmtime(os.path.join(ROOT, "oracle", f)) for f in ("duck_oracle.c", "duck_oracle.h")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")] +
                              (["ASAN=1"] if LIB.endswith("_asan.so") else []))
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        HEADERS.bind(L)   # argtypes and restype of every function duck_oracle.h declares
        if os.environ.get("ORACLE_HF_BAND_SCALE"):  # A/B of a kernel built with -DDUCK_HF_POINT_BAND=...
            L.oracle_set_hf_band_scale(float(os.environ["ORACLE_HF_BAND_SCALE"]))
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class OracleModel:
    def __init__(self, m: Model, dr: Optional[np.ndarray] = None):
        self.m = m
        self._holder = ModelDescHolder(m)
        L = lib()
        self.ptr = L.oracle_model_create(C.byref(self._holder.desc))
        if not self.ptr:
            raise RuntimeError("oracle_model_create failed")
        self.base_ptr = None
        if dr is not None:
            self.base_ptr = self.ptr
            self.ptr = L.oracle_model_randomized(self.base_ptr, _dp(np.ascontiguousarray(dr, dtype=np.float64)))

    def dr_sample(self, seed: int, env_id: int) -> np.ndarray:
        out = np.zeros(dr_layout(self.m.nbody, self.m.nu)["nfloat"])
        lib().oracle_dr_sample(self.ptr, seed, env_id, _dp(out))
        return out

    def __del__(self):
        try:
            lib().oracle_model_destroy(self.ptr)
            if self.base_ptr:
                lib().oracle_model_destroy(self.base_ptr)
        except Exception:
            pass

    def new_data(self, qpos=None, qvel=None, ctrl=None, warm=None) -> OracleData:
        d = OracleData()
        m = self.m
        q = qpos if qpos is not None else m.key_qpos[0]
        d.arr("qpos")[:m.nq] = q
        if qvel is not None:
            d.arr("qvel")[:m.nv] = qvel
        if ctrl is not None:
            d.arr("ctrl")[:m.nu] = ctrl
        if warm is not None:
            d.arr("qacc_warmstart")[:m.nv] = warm
        return d

    def forward(self, d: OracleData):
        lib().oracle_forward(self.ptr, C.byref(d))

    def step(self, d: OracleData, n: int = 1):
        lib().oracle_step(self.ptr, C.byref(d), n)


class OracleEnv:
    """Single-env Joystick on the oracle (fstate/istate in duck_env.h layout, stride 1)."""

    def __init__(self, model: OracleModel, cfg: DuckEnvConfig, table=None):
        self.model = model
        self.cfg = cfg
        self.L = layout(model.m.nq, model.m.nv, model.m.nu, bool(cfg.use_imitation), int(cfg.task))
        if table is None:
            from open_duck_playground_amd import constants
            table = dict(np.load(constants.POLY_COEFFICIENTS, allow_pickle=False))
        self.ref, self._coeffs = refmotion_struct(table)
        self.fs = np.zeros(self.L.nfloat)
        self.is_ = np.zeros(self.L.nint, dtype=np.int32)
        self.obs = np.zeros(self.L.obs_size)
        self.priv = np.zeros(self.L.priv_size)

    def reset(self, seed: int, env_id: int = 0):
        lib().oracle_env_reset(self.model.ptr, C.byref(self.cfg), C.byref(self.ref), seed, env_id, _dp(self.fs),
                               _ip(self.is_), _dp(self.obs), _dp(self.priv))
        return self.obs.copy(), self.priv.copy()

    def step(self, action, data: Optional[OracleData] = None):
        a = np.ascontiguousarray(action, dtype=np.float64)
        rew = np.zeros(1)
        done = np.zeros(1)
        lib().oracle_env_step(self.model.ptr, C.byref(self.cfg), C.byref(self.ref), _dp(self.fs), _ip(self.is_),
                              _dp(a), _dp(self.obs), _dp(self.priv), _dp(rew), _dp(done),
                              C.byref(data) if data is not None else None)
        return self.obs.copy(), self.priv.copy(), float(rew[0]), float(done[0])


class OracleBatch:
    """SoA batch of envs on the oracle with OpenMP (CPU baseline)."""

    def __init__(self, models, cfg: DuckEnvConfig, n_envs: int, table=None):
        self.models = models if isinstance(models, list) else [models]
        self.cfg = cfg
        self.n = n_envs
        m = self.models[0].m
        self.L = layout(m.nq, m.nv, m.nu, bool(cfg.use_imitation), int(cfg.task))
        if table is None:
            from open_duck_playground_amd import constants
            table = dict(np.load(constants.POLY_COEFFICIENTS, allow_pickle=False))
        self.ref, self._coeffs = refmotion_struct(table)
        self.fs = np.zeros(self.L.nfloat * n_envs)
        self.is_ = np.zeros(self.L.nint * n_envs, dtype=np.int32)
        self.obs = np.zeros((n_envs, self.L.obs_size))
        self.priv = np.zeros((n_envs, self.L.priv_size))
        self.rew = np.zeros(n_envs)
        self.done = np.zeros(n_envs)
        self._ptrs = (C.c_void_p * len(self.models))(*[mm.ptr for mm in self.models])

    def reset(self, seed: int, env_offset: int = 0, threads: int = 0):
        lib().oracle_batch_reset(self._ptrs, len(self.models), C.byref(self.cfg), C.byref(self.ref), self.n, seed,
                                 env_offset, _dp(self.fs), _ip(self.is_), _dp(self.obs), _dp(self.priv), threads)

    def step(self, actions, threads: int = 0):
        a = np.ascontiguousarray(actions, dtype=np.float64)
        lib().oracle_batch_step(self._ptrs, len(self.models), C.byref(self.cfg), C.byref(self.ref), self.n,
                                _dp(self.fs), _ip(self.is_), _dp(a), _dp(self.obs), _dp(self.priv), _dp(self.rew),
                                _dp(self.done), threads)
