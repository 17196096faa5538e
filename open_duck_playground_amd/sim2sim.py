"""Single-robot 50 Hz control loop with an ONNX policy in the loop (mirror of
playground/open_duck_mini_v2/mujoco_infer.py:16-241 and mujoco_infer_base.py:7-285).

The reference steps CPU MuJoCo (``mujoco.mj_step``) at 500 Hz in a viewer loop and runs the ONNX
policy every ``decimation`` = 10 steps. Here the physics of one control period (10 substeps) is one
``duck_physics_step`` launch of the HIP kernels for a single env, the policy runs on the host
(``onnx_infer.OnnxInfer``), and the viewer / keyboard / wall-clock pacing are replaced by an explicit
``run(n_periods, command)`` (``realtime=True`` sleeps like the reference's loop).

Observation (mujoco_infer.py:67-103), 101 values: gyro, accelerometer with +1.3 added to x (this
script applies it; the training env's obs does not, joystick.py:502), command[7], actuator joint
angles - default, 0.05 * joint velocities, the last three actions, motor targets, foot contacts
(any penetrating contact between a foot and the floor, mujoco_infer_base.py:259-282), imitation
phase (cos, sin) advanced by ``phase_frequency_factor`` per period (:184-205).

``FleetInfer`` is the same loop for N robots, resident on the device (include/duck_fleet.h): the question a
user has of an exported policy -- does it track commands over the whole command box, does it survive the
randomised models -- takes thousands of runs. ``python -m open_duck_playground_amd.sim2sim`` keeps the
reference's flags and adds ``--num_robots``, ``--periods``, ``--command_grid``, ``--randomize``, ``--out``.
"""

from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import constants
from .cabi import dr_layout
from .joystick import Joystick
from .onnx_infer import OnnxInfer

USE_MOTOR_SPEED_LIMITS = True  # mujoco_infer.py:14


class MjInfer:
    """MjInfer(model_path, reference_data, onnx_model_path, standing) on one MI355X env."""

    def __init__(self, model_path: str = "flat_terrain", reference_data: Optional[str] = None,
                 onnx_model_path: Optional[str] = None, standing: bool = False, device="cuda:0", policy=None):
        self.env = Joystick(model_path, num_envs=1, device=device, use_imitation=False)
        m = self.model = self.env.mj_model
        self.device = torch.device(device)
        self.sim_dt = 0.002   # mujoco_infer_base.py:15-18
        self.decimation = 10
        self.standing = standing
        self.head_control_mode = self.standing
        self.dof_vel_scale = 0.05
        self.action_scale = 0.25
        self.max_motor_velocity = 5.24
        self.phase_frequency_factor = 1.0
        self.num_dofs = m.nu
        self.policy = policy if policy is not None else OnnxInfer(onnx_model_path, awd=True)
        if not standing:
            table = np.load(reference_data or constants.POLY_COEFFICIENTS, allow_pickle=False)
            self.nb_steps_in_period = int(table["nb_steps_in_period"])
        self.actuator_qpos_addr = np.array([m.jnt_qposadr[j] for j in m.actuator_trnid])
        self.actuator_qvel_addr = np.array([m.jnt_dofadr[j] for j in m.actuator_trnid])
        names = m.names["sensor"]
        self.gyro_addr = int(m.sensor_adr[names.index("gyro")])
        self.accelerometer_addr = int(m.sensor_adr[names.index("accelerometer")])
        floor = m.id("geom", "floor")
        self._foot_slots = []
        for foot in constants.FEET_GEOMS:  # the pairs (floor, foot): 4 contact slots each
            g = m.id("geom", foot)
            p = [k for k in range(m.npair) if {int(m.pair_geom1[k]), int(m.pair_geom2[k])} == {floor, g}][0]
            self._foot_slots.append(slice(4 * p, 4 * p + 4))
        key = m.names["key"].index("home")
        self.default_actuator = m.key_ctrl[key].copy()
        self.motor_targets = self.default_actuator.copy()
        self.prev_motor_targets = self.default_actuator.copy()
        self.last_action = np.zeros(self.num_dofs)
        self.last_last_action = np.zeros(self.num_dofs)
        self.last_last_last_action = np.zeros(self.num_dofs)
        self.commands = [0.0] * 7
        self.imitation_i = 0.0
        self.imitation_phase = np.array([0.0, 0.0])
        self.saved_obs: List[np.ndarray] = []
        # MJInferBase.__init__: MjData at qpos0 with zero ctrl, one mj_step, then the home keyframe's
        # qpos and ctrl (the velocity of that first step is kept)
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)[:, None], device=self.device)  # noqa: E731
        self.qpos, self.qvel = t(m.qpos0), t(np.zeros(m.nv))
        self.warm, self.ctrl = t(np.zeros(m.nv)), t(np.zeros(m.nu))
        self.aux = torch.zeros(self.env.aux_size(), 1, dtype=torch.float32, device=self.device)
        self.env.physics_step(self.qpos, self.qvel, self.warm, self.ctrl, 1, self.aux)
        self.qpos.copy_(t(m.key_qpos[key]))
        self.ctrl.copy_(t(self.default_actuator))
        self._aux_np = None

    # --- one control period of physics (mj_step x decimation) ---------------------------------
    def _physics(self):
        self.env.physics_step(self.qpos, self.qvel, self.warm, self.ctrl, self.decimation, self.aux)
        torch.cuda.synchronize(self.device)
        self._aux_np = self.aux[:, 0].cpu().numpy().astype(np.float64)

    def _aux(self, name: str) -> np.ndarray:
        m = self.model
        sizes = [("qacc", m.nv), ("qacc_smooth", m.nv), ("qvel", m.nv), ("qfrc_smooth", m.nv),
                 ("actuator_force", m.nu), ("sensordata", m.nsensordata), ("con_dist", 4 * m.npair)]
        o = 0
        for k, n in sizes:
            if k == name:
                return self._aux_np[o:o + n]
            o += n
        raise KeyError(name)

    def get_gyro(self) -> np.ndarray:
        return self._aux("sensordata")[self.gyro_addr:self.gyro_addr + 3].copy()

    def get_accelerometer(self) -> np.ndarray:
        return self._aux("sensordata")[self.accelerometer_addr:self.accelerometer_addr + 3].copy()

    def get_feet_contacts(self):
        d = self._aux("con_dist")
        return tuple(bool((d[s] < 0).any()) for s in self._foot_slots)

    def get_obs(self, command: Sequence[float]) -> np.ndarray:
        """mujoco_infer.py:67-103 (state of the last mj_step of the period, sensors as mj_step left them)."""
        gyro = self.get_gyro()
        accelerometer = self.get_accelerometer()
        accelerometer[0] += 1.3
        qpos = self.qpos[:, 0].cpu().numpy().astype(np.float64)
        qvel = self.qvel[:, 0].cpu().numpy().astype(np.float64)
        joint_angles = qpos[self.actuator_qpos_addr]
        joint_vel = qvel[self.actuator_qvel_addr]
        contacts = np.array(self.get_feet_contacts(), dtype=np.float64)
        return np.concatenate([gyro, accelerometer, np.asarray(command, dtype=np.float64),
                               joint_angles - self.default_actuator, joint_vel * self.dof_vel_scale,
                               self.last_action, self.last_last_action, self.last_last_last_action,
                               self.motor_targets, contacts, self.imitation_phase])

    def control_step(self):
        """One policy period of mujoco_infer.py:175-241: decimation substeps, then obs -> action -> ctrl."""
        self._physics()
        if not self.standing:
            self.imitation_i += 1.0 * self.phase_frequency_factor
            self.imitation_i = self.imitation_i % self.nb_steps_in_period
            ph = self.imitation_i / self.nb_steps_in_period * 2 * np.pi
            self.imitation_phase = np.array([np.cos(ph), np.sin(ph)])
        obs = self.get_obs(self.commands)
        self.saved_obs.append(obs)
        action = np.asarray(self.policy.infer(obs), dtype=np.float64)
        self.last_last_last_action = self.last_last_action.copy()
        self.last_last_action = self.last_action.copy()
        self.last_action = action.copy()
        self.motor_targets = self.default_actuator + action * self.action_scale
        if USE_MOTOR_SPEED_LIMITS:
            lim = self.max_motor_velocity * (self.sim_dt * self.decimation)
            self.motor_targets = np.clip(self.motor_targets, self.prev_motor_targets - lim,
                                         self.prev_motor_targets + lim)
            self.prev_motor_targets = self.motor_targets.copy()
        self.ctrl.copy_(torch.tensor(self.motor_targets.astype(np.float32)[:, None], device=self.device))
        return obs, action

    def run(self, n_periods: int, command: Optional[Sequence[float]] = None, realtime: bool = False):
        if command is not None:
            self.commands = list(command)
        period = self.sim_dt * self.decimation
        for _ in range(n_periods):
            t0 = time.time()
            self.control_step()
            if realtime:
                time.sleep(max(0.0, period - (time.time() - t0)))
        return self.saved_obs


# --- the same loop for N robots, resident on the device ----------------------------------------

COMMANDS_RANGE_X = (-0.15, 0.15)      # mujoco_infer.py:40-42
COMMANDS_RANGE_Y = (-0.2, 0.2)
COMMANDS_RANGE_THETA = (-1.0, 1.0)


def ctl_fields(nu: int) -> Dict[str, Tuple[int, int]]:
    """(first column, width) of each field of the per-robot control record (include/duck_fleet.h)."""
    return {"last_action": (0, nu), "last_last_action": (nu, nu), "last_last_last_action": (2 * nu, nu),
            "motor_targets": (3 * nu, nu), "prev_motor_targets": (4 * nu, nu), "command": (5 * nu, 7),
            "imitation_i": (5 * nu + 7, 1), "phase_frequency_factor": (5 * nu + 8, 1),
            "imitation_phase": (5 * nu + 9, 2)}


def fleet_desc(m, naux: int, nb_steps_in_period: int, standing: bool, speed_limits: bool = USE_MOTOR_SPEED_LIMITS):
    """duck_fleet_desc (include/duck_fleet.h) of a compiled model: where the deployment loop's sensors,
    actuated joints and foot contacts are, and the loop's constants (mujoco_infer.py:27-31, :58, :74)."""
    from .native import FLEET_MAX_NU, DuckError, DuckFleetDesc
    if m.nu > FLEET_MAX_NU:
        raise DuckError(f"the fleet kernels take at most {FLEET_MAX_NU} actuators, the model has {m.nu}")
    d = DuckFleetDesc()
    d.nq, d.nv, d.nu, d.naux = int(m.nq), int(m.nv), int(m.nu), int(naux)
    d.sens_off = 4 * m.nv + m.nu          # write_aux (csrc/duck_physics.h): qacc, qacc_smooth, qvel,
    d.con_off = d.sens_off + m.nsensordata  # qfrc_smooth, actuator_force, sensordata, con_dist
    names = m.names["sensor"]
    for field, sensor in (("gyro", constants.GYRO_SENSOR), ("accelerometer", constants.ACCELEROMETER_SENSOR),
                          ("upvector", constants.GRAVITY_SENSOR), ("local_linvel", constants.LOCAL_LINVEL_SENSOR)):
        setattr(d, field, int(m.sensor_adr[names.index(sensor)]))
    key = m.names["key"].index("home")
    for a, j in enumerate(m.actuator_trnid):
        d.act_qpos[a], d.act_dof[a] = int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j])
        d.act_default[a] = float(m.key_ctrl[key][a])
    floor = m.id("geom", "floor")
    for f, foot in enumerate(constants.FEET_GEOMS):   # the pairs (floor, foot): 4 contact slots each
        g = m.id("geom", foot)
        d.foot_con[f] = 4 * [k for k in range(m.npair) if {int(m.pair_geom1[k]), int(m.pair_geom2[k])} == {floor, g}][0]
    d.dof_vel_scale, d.action_scale, d.accel_x_offset = 0.05, 0.25, 1.3
    d.target_step = float(np.float32(5.24 * 0.002 * 10))
    d.nb_steps_in_period = int(nb_steps_in_period)
    d.standing, d.speed_limits = int(bool(standing)), int(bool(speed_limits))
    return d


class FleetInfer:
    """The deployment loop of ``MjInfer`` for ``num_robots`` robots at once, resident on the device: one
    control period is four launches on one stream -- duck_physics_step (10 substeps, with the aux record),
    duck_fleet_observe, duck_policy_act, duck_fleet_actuate (include/duck_fleet.h) -- with no host round
    trip. The exported ONNX policy is imported as dense layers (onnx_infer.dense_policy); one outside
    duck_policy_act's limits raises DuckError (there is no host fallback).

    Every robot starts as MJInferBase starts its one: a substep from qpos0 with zero ctrl, then the home
    keyframe's qpos and ctrl with that step's velocity kept. ``randomize=seed`` gives each robot its
    duck_randomize(seed) model for the whole run (before that first step); None runs the nominal model.
    Per robot, duck_fleet_observe accumulates the periods survived, the tracked velocity and the squared
    tracking errors until the robot falls (``report()``); fallen robots keep being simulated and controlled.

    The first ``run`` is eager; later ones replay a captured graph of ``CHUNK`` periods (one stream, a
    linear graph) and run the remainder eagerly."""

    CHUNK = 50   # control periods per captured graph (200 launches)

    def __init__(self, model_path: str = "flat_terrain", onnx_model_path: Optional[str] = None, num_robots: int = 1,
                 reference_data: Optional[str] = None, standing: bool = False, device="cuda:0",
                 randomize: Optional[int] = None):
        import ctypes as C

        from .native import DuckError, check
        from .onnx_infer import OnnxGraph, dense_policy
        from .ppo import POLICY_ACT_MAX_LAYERS, POLICY_ACT_MAX_WIDTH
        n = self.num_robots = int(num_robots)
        if n < 1:
            raise DuckError("num_robots must be >= 1")
        with open(onnx_model_path, "rb") as f:
            pol = dense_policy(OnnxGraph(f.read()))
        sizes = pol["sizes"]
        if len(pol["W"]) > POLICY_ACT_MAX_LAYERS or max(sizes) > POLICY_ACT_MAX_WIDTH:
            raise DuckError(f"policy layers {sizes} are outside duck_policy_act's limits (at most "
                            f"{POLICY_ACT_MAX_LAYERS} layers, at most {POLICY_ACT_MAX_WIDTH} wide); there is no host fallback")
        self.env = Joystick(model_path, num_envs=n, device=device, use_imitation=False)
        m = self.model = self.env.mj_model
        self.device = dev = torch.device(device)
        self.standing = bool(standing)
        self.decimation = 10
        self._lib, self._sim, self._check = self.env._lib, self.env._sim, check
        nb = 0
        if not standing:
            table = np.load(reference_data or constants.POLY_COEFFICIENTS, allow_pickle=False)
            nb = int(table["nb_steps_in_period"])
        self.nb_steps_in_period = nb
        naux = self.env.aux_size()
        self.desc = fleet_desc(m, naux, nb, standing)
        nu = self.num_dofs = int(m.nu)
        self.obs_size = 17 + 6 * nu

        # the policy's dense layers on the device, pointers in host arrays (duck_policy_act's arguments)
        if sizes[0] != self.obs_size or pol["action_size"] != nu:
            raise DuckError(f"policy maps {sizes[0]} -> {pol['action_size']}, the model's loop needs {self.obs_size} -> {nu}")
        up = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32, device=dev).contiguous()  # noqa: E731
        self._W, self._b = [up(w) for w in pol["W"]], [up(b) for b in pol["b"]]
        self._mean, self._istd = up(pol["mean"]), up(pol["istd"])
        self._policy_args = (len(sizes) - 1, (C.c_int * len(sizes))(*sizes),
                             (C.c_void_p * len(self._W))(*[w.data_ptr() for w in self._W]),
                             (C.c_void_p * len(self._b))(*[b.data_ptr() for b in self._b]),
                             None if self._mean is None else self._mean.data_ptr(),
                             None if self._istd is None else self._istd.data_ptr())

        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        self.qpos, self.qvel = z(m.nq, n), z(m.nv, n)
        self.warm, self.ctrl, self.aux = z(m.nv, n), z(nu, n), z(naux, n)
        self._scratch = z(n * m.nv * m.nv)
        self.fields = ctl_fields(nu)
        self.ctl, self.obs, self.action = z(n, 5 * nu + 11), z(n, self.obs_size), z(n, nu)
        self.acc, self.alive = z(n, 6), torch.ones(n, dtype=torch.float32, device=dev)
        self.dr = None
        if randomize is not None:
            self.dr = z(dr_layout(m.nbody, nu)["nfloat"] * n)
            check(self._lib.duck_randomize(self._sim, n, self.dr.data_ptr(), int(randomize) & 0xFFFFFFFFFFFFFFFF, 0,
                                           self._stream()), self._lib)
        self.default_actuator = np.asarray(m.key_ctrl[m.names["key"].index("home")], dtype=np.float32)
        self.calls, self.graph = 0, None
        self.restart()

    def restart(self) -> None:
        """Every robot back to the loop's start, with the randomisation record ``dr`` as it is now.
        MJInferBase.__init__: MjData at qpos0 with zero ctrl, one mj_step, then the home keyframe's qpos and
        ctrl (the velocity of that first step is kept); mujoco_infer.py:49-60 for the control record."""
        m, n = self.model, self.num_robots
        col = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)[:, None], device=self.device)  # noqa: E731
        key = m.names["key"].index("home")
        self.qpos.copy_(col(m.qpos0).expand(-1, n))
        for t in (self.qvel, self.warm, self.ctrl, self.ctl):
            t.zero_()
        self._physics(1)
        self.qpos.copy_(col(m.key_qpos[key]).expand(-1, n))
        self.ctrl.copy_(col(self.default_actuator).expand(-1, n))
        default = torch.tensor(self.default_actuator, device=self.device)
        self.ctl_field("motor_targets").copy_(default.expand(n, -1))
        self.ctl_field("prev_motor_targets").copy_(default.expand(n, -1))
        self.ctl_field("phase_frequency_factor").fill_(1.0)
        self.reset_report()

    # --- launches -----------------------------------------------------------------------------
    def _stream(self):
        import ctypes as C
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _physics(self, n_substeps: int):
        L = self._lib
        self._check(L.duck_physics_step(self._sim, self.num_robots, self.qpos.data_ptr(), self.qvel.data_ptr(),
                                        self.warm.data_ptr(), self.ctrl.data_ptr(),
                                        None if self.dr is None else self.dr.data_ptr(), int(n_substeps),
                                        self.aux.data_ptr(), self._scratch.data_ptr(), self._stream()), L)

    def observe(self):
        """duck_fleet_observe on the current state: phase, observation, bookkeeping."""
        import ctypes as C
        L = self._lib
        self._check(L.duck_fleet_observe(C.byref(self.desc), self.num_robots, self.qpos.data_ptr(),
                                         self.qvel.data_ptr(), self.aux.data_ptr(), self.ctl.data_ptr(),
                                         self.obs.data_ptr(), self.acc.data_ptr(), self.alive.data_ptr(),
                                         self._stream()), L)

    def act(self):
        """duck_policy_act on ``obs``, then duck_fleet_actuate: history, motor targets, ctrl."""
        import ctypes as C
        from .native import lib
        L, P = self._lib, lib()   # the policy kernel ships with libduck.so only, the rest with the model's library
        self._check(P.duck_policy_act(self.num_robots, *self._policy_args, self.obs.data_ptr(), None,
                                      self.action.data_ptr(), self._stream()), P)
        self._check(L.duck_fleet_actuate(C.byref(self.desc), self.num_robots, self.action.data_ptr(),
                                         self.ctl.data_ptr(), self.ctrl.data_ptr(), self._stream()), L)

    def _periods(self, k: int, rec: Optional[torch.Tensor] = None, t0: int = 0):
        for t in range(k):
            self._physics(self.decimation)
            self.observe()
            if rec is not None:
                rec[t0 + t].copy_(self.obs)
            self.act()

    @torch.no_grad()
    def run(self, n_periods: int, record: bool = False):
        """``n_periods`` control periods for every robot. ``record=True`` returns the observations
        [T][N][obs] the policy saw (a numpy array; such a run is eager)."""
        from .ppo import check_device_error
        n_periods = int(n_periods)
        rec = torch.empty(n_periods, self.num_robots, self.obs_size, device=self.device) if record else None
        self.calls += 1
        chunk = max(1, int(self.CHUNK))
        if record or self.calls == 1 or n_periods < chunk:
            self._periods(n_periods, rec)
        else:
            if self.graph is None or self.graph[1] != chunk:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):   # one capture stream: a linear graph
                    self._periods(chunk)
                # (capturing records the launches without running them)
                self.graph = (g, chunk)
            for _ in range(n_periods // chunk):
                self.graph[0].replay()
            self._periods(n_periods % chunk)
        torch.cuda.synchronize(self.device)
        check_device_error(self.env, "fleet run")   # a replayed graph never re-enters duck_physics_step's entry check
        return rec.cpu().numpy() if record else None

    # --- host interface -----------------------------------------------------------------------
    def ctl_field(self, name: str) -> torch.Tensor:
        """A view [N, width] of one field of the control record (``ctl_fields``)."""
        o, w = self.fields[name]
        return self.ctl[:, o:o + w]

    def set_commands(self, cmd) -> None:
        """``cmd`` [7] for every robot, or [N][7]."""
        from .native import DuckError
        c = torch.as_tensor(np.asarray(cmd, dtype=np.float32), device=self.device)
        if c.shape not in ((7,), (self.num_robots, 7)):
            raise DuckError(f"commands must be [7] or [{self.num_robots}][7], got {tuple(c.shape)}")
        self.ctl_field("command").copy_(c.expand(self.num_robots, 7))

    def state(self):
        """(qpos [N][nq], qvel [N][nv], ctrl [N][nu]) as numpy float32."""
        return tuple(t.t().contiguous().cpu().numpy() for t in (self.qpos, self.qvel, self.ctrl))

    def load_state(self, qpos=None, qvel=None, ctrl=None, qacc_warmstart=None, **ctl) -> None:
        """Overwrite physics state ([k] for every robot or [N][k]) and control-record fields by name."""
        def put(dst, a):   # dst [N, k] view
            a = torch.as_tensor(np.asarray(a, dtype=np.float32), device=self.device).reshape(-1, dst.shape[1])
            dst.copy_(a.expand(dst.shape[0], -1))
        for t, a in ((self.qpos, qpos), (self.qvel, qvel), (self.ctrl, ctrl), (self.warm, qacc_warmstart)):
            if a is not None:
                put(t.t(), a)
        for name, a in ctl.items():
            put(self.ctl_field(name), a)

    def reset_report(self) -> None:
        self.acc.zero_()
        self.alive.fill_(1.0)

    def report(self) -> Dict[str, np.ndarray]:
        """Per robot: periods survived, fell, mean vx / vy / wz while alive, rms linear and yaw tracking
        error while alive (NaN for a robot that survived no period)."""
        acc = self.acc.cpu().numpy().astype(np.float64)
        alive = self.alive.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = acc[:, 1:] / acc[:, :1]
        return {"periods": acc[:, 0], "fell": alive == 0, "mean_vx": mean[:, 0], "mean_vy": mean[:, 1],
                "mean_wz": mean[:, 2], "rms_lin_err": np.sqrt(mean[:, 3]), "rms_yaw_err": np.sqrt(mean[:, 4])}


def command_grid(spec: str) -> np.ndarray:
    """``NXxNYxNT`` -> the [NX * NY * NT][7] commands over the reference's COMMANDS_RANGE_X / Y / THETA
    (both ends included; a single point is the range's middle)."""
    try:
        nx, ny, nt = (int(v) for v in spec.lower().split("x"))
        assert min(nx, ny, nt) >= 1
    except Exception:
        raise ValueError(f"--command_grid wants NXxNYxNT with positive integers, got {spec!r}") from None
    axis = lambda r, k: np.linspace(r[0], r[1], k) if k > 1 else np.array([0.5 * (r[0] + r[1])])  # noqa: E731
    cells = [(x, y, t) for x in axis(COMMANDS_RANGE_X, nx) for y in axis(COMMANDS_RANGE_Y, ny)
             for t in axis(COMMANDS_RANGE_THETA, nt)]
    out = np.zeros((len(cells), 7), dtype=np.float32)
    out[:, :3] = cells
    return out


def grid_report(rep: Dict[str, np.ndarray], acc: np.ndarray, cells: np.ndarray, n_periods: int) -> list:
    """Per command cell (robot r belongs to cell r mod the number of cells): the count, the share that
    never fell, the mean tracked velocity and the rms errors over the cell's surviving periods."""
    out = []
    for c in range(len(cells)):
        a = acc[c::len(cells)].astype(np.float64)
        tot = a.sum(0)
        stat = (lambda v: float(v / tot[0])) if tot[0] > 0 else (lambda v: None)
        out.append({"command": [float(v) for v in cells[c][:3]], "count": int(len(a)),
                    "survival_rate": float(np.mean(~rep["fell"][c::len(cells)])) if len(a) else None,
                    "mean_periods": float(a[:, 0].mean()) if len(a) else None, "periods": int(n_periods),
                    "mean_vx": stat(tot[1]), "mean_vy": stat(tot[2]), "mean_wz": stat(tot[3]),
                    "rms_lin_err": None if stat(tot[4]) is None else float(np.sqrt(stat(tot[4]))),
                    "rms_yaw_err": None if stat(tot[5]) is None else float(np.sqrt(stat(tot[5])))})
    return out


def main(argv=None) -> int:
    import argparse
    import json
    p = argparse.ArgumentParser(description="Run an exported policy in the deployment loop for a fleet of robots")
    p.add_argument("-o", "--onnx_model_path", type=str, required=True)
    p.add_argument("--reference_data", type=str, default=None)
    p.add_argument("--model_path", type=str, default="flat_terrain")
    p.add_argument("--standing", action="store_true", default=False)
    p.add_argument("--num_robots", type=int, default=1024)
    p.add_argument("--periods", type=int, default=500)
    p.add_argument("--command_grid", type=str, default="1x1x1")
    p.add_argument("--randomize", type=int, default=None, metavar="SEED")
    p.add_argument("--out", type=str, default=None, metavar="report.json")
    p.add_argument("--device", type=str, default="cuda:0")
    args = p.parse_args(argv)
    cells = command_grid(args.command_grid)
    fleet = FleetInfer(args.model_path, args.onnx_model_path, args.num_robots, reference_data=args.reference_data,
                       standing=args.standing, device=args.device, randomize=args.randomize)
    fleet.set_commands(cells[np.arange(args.num_robots) % len(cells)])
    t0 = time.time()
    fleet.run(args.periods)
    dt = time.time() - t0
    rows = grid_report(fleet.report(), fleet.acc.cpu().numpy(), cells, args.periods)
    doc = {"model_path": args.model_path, "onnx_model_path": args.onnx_model_path, "num_robots": args.num_robots,
           "periods": args.periods, "randomize": args.randomize, "standing": args.standing,
           "robot_periods_per_s": args.num_robots * args.periods / max(dt, 1e-9), "cells": rows}
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for r in rows:
        print(json.dumps(r))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
