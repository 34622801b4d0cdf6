"""Host side of the surrogate legged env step (csrc/sim.hip, `dtc_sim_step`, `dtc_sim_step_tilt`, `dtc_sim_step_act`, `dtc_sim_step_fly`): the state the env kernels run
on when no simulator stands behind them.  One launch per env step stands where the reference calls Isaac Gym: `decimation` substeps
of the PD law of LeggedRobot._compute_torques (control type "P"), a kinematic quadruped that rides on its stance feet over the int16
terrain table, and the bookkeeping of post_physics_step up to the planner.  include/dtc_hip.h states every operation; it is a
surrogate, not physics (no attitude or contact dynamics, no "V" / "T" control, no heading yaw law; no free flight unless
`SimConfig.flight` is set; no contact with anything but the soles of the feet unless `SimConfig.contacts` is set, and then
forces that feed the rewards only).  By default the
base only yaws; `SimConfig.tilt` (opt-in) lets its roll and pitch follow the support points of the stance feet, still kinematically:
after a reset the identity quaternion then gives one step with a tilt-rate spike.  `SimConfig.actuator` (opt-in, an
`ActuatorConfig`) adds the two disturbances the reference trains under: the PD goal taken from a six-slot lag buffer of scaled
actions at a slot the host draws per substep, and random pushes -- here a kinematic slip velocity of the base with a chosen decay,
not a contact dynamics.  `SimConfig.flight` (opt-in, a `FlightConfig`) gives the base a vertical degree of freedom: a base whose support
falls away falls under gravity and lands when it reaches a support, and a support that rises by more than a climbable step is a
crash that ends the episode through the base contact force.  `SimConfig.contacts` (opt-in, a `ContactConfig`) adds a second launch,
`dtc_sim_contacts` (csrc/sim_contacts.hip), behind the step: contact forces of thighs and shanks that penetrate the terrain and of a
swing foot that flies into a riser, for the reward terms that read them.  Nothing is held back by those forces and nothing topples
unless `SimConfig.balance` (opt-in, a `BalanceConfig`) is set: a further launch, `dtc_sim_balance` (csrc/sim_balance.hip), between
the step and the contacts, a point-mass inverted pendulum about the edge of the support polygon of the stance feet whose lean is
laid over the base's attitude, height and angular velocity and, beyond `fall_angle`, ends the episode through the base's contact
force.  An overlay, not attitude dynamics: it rotates no link, knows no friction and takes no push.

`SimConfig` holds the constants (Lite3 DTC values), `leg_tables(config)` the three small tables computed once in float64 from a
two-link leg linearised at the default pose, and `SimStep` runs the launch on an env's own tensors (attribute names as in
LeggedRobotDTC).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _ffi

_RANGES = ("lin_vel_x", "lin_vel_y", "ang_vel_yaw", "heading")
# per-env tensors of the env that dtc_sim_step reads or writes: name -> (trailing shape given D, B, C; dtype)
_ENV_TENSORS = dict(Kp_factors=("D", torch.float32), Kd_factors=("D", torch.float32), motor_strengths=("D", torch.float32),
                    motor_offsets=("D", torch.float32), root_states=(13, torch.float32), base_ang_vel=(3, torch.float32),
                    commands=("C", torch.float32), episode_length_buf=((), torch.int64), last_contacts=(4, torch.bool),
                    rigid_body_state=("B", 13, torch.float32), contact_forces=("B", 3, torch.float32), torques=("D", torch.float32),
                    actions=("D", torch.float32), base_lin_vel=(3, torch.float32), last_base_ang_vel=(3, torch.float32),
                    projected_gravity=(3, torch.float32), base_pos=(3, torch.float32), base_quat=(4, torch.float32),
                    contact_filt=(4, torch.bool))
_RING_BUFFERS = dict(lin_vel_buffer=2, ang_vel_buffer=1, cmd_buffer="C")
TERMINATION_FORCE = 100.0       # N: the contact-force threshold of dtc_check_termination (legged_robot_dtc.py:229-248)


@dataclass
class ActuatorConfig:
    """Actuator lag and random pushes of `dtc_sim_step_act` (include/dtc_hip.h states the operations).  `lag`: the PD goal of substep
    `it` is the lag buffer's slot `choice[it]`, one host draw per substep for all envs from the inclusive range `lag_slots` (the
    reference: np.random.randint(1, 5), legged_robot.py:614); slot 5 is the current action.  `push`: every `push_interval_s`, on two
    consecutive env steps, the base's planar velocity is overwritten by a uniform draw in +- `max_push_vel_xy`
    (legged_robot.py:546-553, :673-678).  The surrogate has no momentum to carry that velocity, so the draw rides on the base twist
    as a slip velocity that decays with the time constant `push_decay_s` and is dropped below `push_floor` [m/s]: both are free
    constants of the surrogate, chosen, not fitted to anything."""
    lag: bool = True
    lag_slots: tuple = (1, 4)
    push: bool = True
    push_interval_s: float = 15.0
    max_push_vel_xy: float = 1.0
    push_decay_s: float = 0.2
    push_floor: float = 1e-6

    def validate(self):
        lo, hi = self.lag_slots
        if not (0 <= int(lo) <= int(hi) <= 5):
            raise ValueError(f"ActuatorConfig: lag_slots {self.lag_slots} outside 0..5")
        if not (self.push_interval_s > 0 and self.push_decay_s > 0 and self.max_push_vel_xy >= 0 and self.push_floor >= 0):
            raise ValueError("ActuatorConfig: push_interval_s and push_decay_s must be positive, max_push_vel_xy and push_floor not negative")


@dataclass
class FlightConfig:
    """Free flight, landing and wall crashes of `dtc_sim_step_fly` (include/dtc_hip.h states the operations).  A substep whose
    ballistic candidate (z velocity less `gravity` * sim_dt) stays more than contact_eps clear of the support is airborne; any other
    is grounded as without flight, and leaves the base the z velocity its stance legs give it.  A grounded substep whose support
    rises by more than `max_step_up` [m] is a crash: the base takes the contact force `crash_force` [N], which must exceed the
    termination threshold (100 N), so check_termination ends the episode as it ends a fall in the reference.  `max_step_up` and
    `crash_force` are free constants of the surrogate, chosen, not fitted to anything (and so is the take-off rule): 0.3 m lies
    above every stair (0.18 m) and obstacle (0.2 m) the terrain generator makes and below a gap or a deep pit wall; 200 N is
    twice the threshold."""
    gravity: float = 9.81
    max_step_up: float = 0.3
    crash_force: float = 200.0

    def validate(self):
        if not (self.gravity >= 0 and math.isfinite(self.gravity)):
            raise ValueError(f"FlightConfig: gravity {self.gravity} must be finite and not negative")
        if not (self.max_step_up > 0 and math.isfinite(self.max_step_up)):
            raise ValueError(f"FlightConfig: max_step_up {self.max_step_up} must be positive and finite")
        if not (self.crash_force > TERMINATION_FORCE and math.isfinite(self.crash_force)):
            raise ValueError(f"FlightConfig: crash_force {self.crash_force} must exceed the termination threshold of {TERMINATION_FORCE} N")


@dataclass
class ContactConfig:
    """Leg collisions and foot stumbles of `dtc_sim_contacts` (include/dtc_hip.h states the operations), a launch of its own behind
    the step.  Thigh and shank are capsules of `body_radius` sampled at three and four points; the deepest sample's penetration of
    the terrain gives the body a vertical contact force `stiffness` * depth, capped at `max_force`.  A foot faster than `min_speed`
    whose look-ahead point, `probe` ahead along its planar velocity, stands more than `stumble_height` above it has hit a riser:
    its horizontal contact force opposes the velocity with `wall_damping` * speed, capped at `max_force`.  `shanks`: the body rows
    of the four shanks, where the knee position is written.  The forces feed the rewards (collision, stumble, feet_stumble,
    foot_clearance) and nothing else: a colliding shank is not held back, a stumbling foot is not stopped (the support rule still
    lifts it onto the riser), nothing topples, and the torso has no contact of its own.  Every constant here is a free choice of
    the surrogate, chosen, not fitted to anything: 0.02 m is a slim leg link, 5000 N/m reaches the collision threshold of 0.1 N
    at 0.02 mm and the cap at 0.04 m, 0.05 m is one terrain cell, 0.03 m lies under every stair riser the generator makes."""
    shanks: tuple = (3, 7, 11, 15)           # body rows; the knee position is written there
    body_radius: float = 0.02                # m, capsule radius of thigh and shank
    stiffness: float = 5000.0                # N/m, penetration spring
    max_force: float = 200.0                 # N, cap of every force this kernel writes
    probe: float = 0.05                      # m, look-ahead of a moving foot (one terrain cell)
    stumble_height: float = 0.03             # m, a face this much above the foot point is a riser
    wall_damping: float = 200.0              # N s/m, horizontal force per foot speed at a riser
    min_speed: float = 0.05                  # m/s, below it a foot does not stumble

    def validate(self, sim: "SimConfig | None" = None):
        """The fields alone; with `sim`, the shank rows against its body layout as well."""
        for name in ("stiffness", "max_force", "probe", "wall_damping"):
            v = getattr(self, name)
            if not (v > 0 and math.isfinite(v)):
                raise ValueError(f"ContactConfig: {name} {v} must be positive and finite")
        for name in ("body_radius", "stumble_height", "min_speed"):
            v = getattr(self, name)
            if not (v >= 0 and math.isfinite(v)):
                raise ValueError(f"ContactConfig: {name} {v} must be finite and not negative")
        shanks = tuple(int(v) for v in self.shanks)
        if len(shanks) != 4 or len(set(shanks)) != 4:
            raise ValueError(f"ContactConfig: shanks {self.shanks} must be four different body rows")
        if sim is not None:
            taken = {0, *(int(v) for v in sim.feet), *(int(v) for v in sim.thighs)}
            for v in shanks:
                if not 0 <= v < int(sim.num_bodies) or v in taken:
                    raise ValueError(f"ContactConfig: shank row {v} is the base, a foot, a thigh or outside 0..{int(sim.num_bodies) - 1}")


@dataclass
class BalanceConfig:
    """Support-polygon balance and falls of `dtc_sim_balance` (include/dtc_hip.h states the operations B1..B9), a launch of its own
    behind the step and in front of `dtc_sim_contacts`.  A point-mass inverted pendulum about the edge of the support of the
    stance feet (four or three: the polygon in the order FL, FR, HR, HL; two: the segment; one: the point; none: no torque): a lean
    vector [rad, world frame] accelerates away from the support while the base's xy (plus `com_offset`, base frame) lies outside it,
    is restored while inside and lands at zero, and is laid over the attitude, height and angular velocity the step wrote.  A lean
    beyond `fall_angle` is a fall: the base takes the contact force `fall_force`, which must exceed the termination threshold
    (100 N), so check_termination ends the episode as it ends a fall in the reference.  The pendulum's length is the base's height
    over the highest stance foot, floored at `h_min`; a lean over its support shorter than `lean_eps` lands.  What it is not: the
    link positions are not rotated (planner and contacts see the un-leaned feet and hips; the contacts' knee turns with the leaned
    quaternion), pushes do not feed the lean rate, there is no friction and no slipping pivot, crossed feet are neglected.  Every constant is a free choice of the
    surrogate, fitted to nothing: 0.8 rad is past any attitude a quadruped recovers from, 200 N is twice the threshold, 0.05 m
    keeps a crouched base a pendulum of finite rate, 1e-3 rad is under every observation noise."""
    gravity: float = 9.81
    h_min: float = 0.05                      # m, floor of the pendulum's length
    lean_eps: float = 1e-3                   # rad, a lean over its support shorter than this lands
    fall_angle: float = 0.8                  # rad, a lean beyond it is a fall
    fall_force: float = 200.0                # N, the base's contact force of a fallen env
    com_offset: tuple = (0.0, 0.0)           # m, base frame: the centre of mass relative to the base's origin

    def validate(self):
        for name in ("h_min", "fall_angle", "fall_force"):
            v = getattr(self, name)
            if not (v > 0 and math.isfinite(v)):
                raise ValueError(f"BalanceConfig: {name} {v} must be positive and finite")
        if not self.fall_force > TERMINATION_FORCE:
            raise ValueError(f"BalanceConfig: fall_force {self.fall_force} must exceed the termination threshold of {TERMINATION_FORCE} N")
        for name in ("gravity", "lean_eps"):
            v = getattr(self, name)
            if not (v >= 0 and math.isfinite(v)):
                raise ValueError(f"BalanceConfig: {name} {v} must be finite and not negative")
        if len(self.com_offset) != 2 or not all(math.isfinite(v) for v in self.com_offset):
            raise ValueError(f"BalanceConfig: com_offset {self.com_offset} must be two finite numbers")


@dataclass
class SimConfig:
    """Constants of the surrogate step (names as in DtcSimCfg, include/dtc_hip.h); defaults: the Lite3 DTC values."""
    sim_dt: float = 0.005
    decimation: int = 4
    action_scale: float = 0.25
    clip_actions: float = 100.0
    stiffness: float = 25.0
    damping: float = 0.5
    torque_limit: float = 24.0
    joint_inertia: float = 0.05              # kg m^2 seen by every joint: the PD loop is well damped at sim_dt (kp / I = 500 s^-2)
    joint_range: float = 1.0                 # position limits: default +- joint_range (a full crouch sinks the base below 0.15 m)
    contact_eps: float = 0.005               # a foot within 5 mm of the ground under the support plane is in contact
    mass: float = 12.0
    gravity: float = 9.81
    r_min: float = 0.05                      # a stance whose feet lie within r_min of their centroid gives no yaw rate
    default_dof_pos: tuple = (0.0, -0.8, 1.6) * 4
    hip_offset: tuple = ((0.17, 0.1, 0.0), (0.17, -0.1, 0.0), (-0.17, 0.1, 0.0), (-0.17, -0.1, 0.0))       # FL, FR, HL, HR
    link_lengths: tuple = (0.2, 0.2)
    num_bodies: int = 17                     # base, then (hip, thigh, shank, foot) per leg
    feet: tuple = (4, 8, 12, 16)
    thighs: tuple = (2, 6, 10, 14)
    num_commands: int = 4
    heading_command: bool = False
    resampling_time: float = 10.0
    buffer_len: int = 10
    lin_vel_x: tuple = (-0.75, 0.75)
    lin_vel_y: tuple = (-0.75, 0.75)
    ang_vel_yaw: tuple = (-0.5, 0.5)
    heading: tuple = (-3.14, 3.14)
    border_size: float = 20.0
    horizontal_scale: float = 0.05
    vertical_scale: float = 0.005
    tilt: bool = False                       # roll and pitch from the stance feet (dtc_sim_step_tilt); off: dtc_sim_step, bit for bit
    max_slope: float = 1.0                   # the fitted plane's slopes are clamped to +- max_slope (45 degrees)
    # a stance keeps its tilt unless the determinant of its centred xy scatter exceeds min_det [m^4].  Three feet give
    # det = (2 A)^2 / 3 (A: the triangle's area), so 1e-6 asks for 2 A > 1.7e-3 m^2: a triangle with a base of r_min = 0.05 m and a
    # height of 0.035 m.  Any three feet of the default stance (0.34 m x 0.2 m) give 1.5e-3, fp32 rounding of a collinear stance
    # of that size 1e-10.
    min_det: float = 1e-6
    actuator: ActuatorConfig | None = None   # lag buffer and pushes (dtc_sim_step_act); None: the entry points above, bit for bit
    flight: FlightConfig | None = None       # free flight, landing, crashes (dtc_sim_step_fly); None: the entry points above, bit for bit
    contacts: ContactConfig | None = None    # leg collisions, foot stumbles (dtc_sim_contacts, a second launch); None: no such launch
    balance: BalanceConfig | None = None     # support-polygon balance, falls (dtc_sim_balance, a launch of its own); None: no such launch

    @property
    def dt(self) -> float:
        return self.sim_dt * self.decimation

    @property
    def resampling_steps(self) -> int:
        return int(self.resampling_time / self.dt)                      # legged_robot.py:534

    @property
    def push_interval(self) -> int:
        return int(math.ceil(self.actuator.push_interval_s / self.dt))  # legged_robot.py:1240

    @property
    def nominal_height(self) -> float:
        """Base height over flat ground at the default pose."""
        return -float(leg_tables(self)["foot_nominal"][0, 2])


def leg_tables(config: SimConfig) -> dict:
    """hip_offset [4,3], foot_nominal [4,3], leg_jacobian [4,3,3] (float64): a leg is an abduction joint about x followed by two
    pitch joints with links l1, l2; foot = hip + (xs, -zs sin(a), zs cos(a)) with xs = -l1 sin(t1) - l2 sin(t1 + t2),
    zs = -l1 cos(t1) - l2 cos(t1 + t2); the Jacobian is taken at the default pose."""
    l1, l2 = config.link_lengths
    hip = np.asarray(config.hip_offset, dtype=np.float64)
    q0 = np.asarray(config.default_dof_pos, dtype=np.float64).reshape(4, 3)
    nominal, jac = np.zeros((4, 3)), np.zeros((4, 3, 3))
    for l in range(4):
        a, t1, t2 = q0[l]
        xs = -l1 * math.sin(t1) - l2 * math.sin(t1 + t2)
        zs = -l1 * math.cos(t1) - l2 * math.cos(t1 + t2)
        dxs = (-l1 * math.cos(t1) - l2 * math.cos(t1 + t2), -l2 * math.cos(t1 + t2))
        dzs = (l1 * math.sin(t1) + l2 * math.sin(t1 + t2), l2 * math.sin(t1 + t2))
        nominal[l] = hip[l] + (xs, -zs * math.sin(a), zs * math.cos(a))
        jac[l, :, 0] = (0.0, -zs * math.cos(a), -zs * math.sin(a))
        for k in range(2):
            jac[l, :, 1 + k] = (dxs[k], -dzs[k] * math.sin(a), dzs[k] * math.cos(a))
    return dict(hip_offset=hip, foot_nominal=nominal, leg_jacobian=jac)


def knee_tables(config: SimConfig) -> dict:
    """knee_nominal [4,3], knee_jacobian [4,3,3] (float64): the knee of the leg of `leg_tables`,
    knee = hip + (-l1 sin(t1), l1 cos(t1) sin(a), -l1 cos(t1) cos(a)), with its Jacobian at the default pose (no t2 column)."""
    l1, _ = config.link_lengths
    hip = np.asarray(config.hip_offset, dtype=np.float64)
    q0 = np.asarray(config.default_dof_pos, dtype=np.float64).reshape(4, 3)
    nominal, jac = np.zeros((4, 3)), np.zeros((4, 3, 3))
    for l in range(4):
        a, t1, _ = q0[l]
        xs, zs = -l1 * math.sin(t1), -l1 * math.cos(t1)
        dxs, dzs = -l1 * math.cos(t1), l1 * math.sin(t1)
        nominal[l] = hip[l] + (xs, -zs * math.sin(a), zs * math.cos(a))
        jac[l, :, 0] = (0.0, -zs * math.cos(a), -zs * math.sin(a))
        jac[l, :, 1] = (dxs, -dzs * math.sin(a), dzs * math.cos(a))
    return dict(knee_nominal=nominal, knee_jacobian=jac)


def joint_tables(config: SimConfig) -> dict:
    """p_gains, d_gains, torque_limits, default_dof_pos [12] and dof_pos_limits [12,2] (float64)."""
    d = np.asarray(config.default_dof_pos, dtype=np.float64)
    return dict(p_gains=np.full(12, config.stiffness), d_gains=np.full(12, config.damping), torque_limits=np.full(12, config.torque_limit),
                default_dof_pos=d, dof_pos_limits=np.stack([d - config.joint_range, d + config.joint_range], axis=1))


def flat_table(rows: int = 1400, cols: int = 900, device="cpu") -> torch.Tensor:
    """The flat int16 terrain table."""
    return torch.zeros(rows, cols, dtype=torch.int16, device=device)


class SimStep:
    """`dtc_sim_step` (`dtc_sim_step_tilt` with `config.tilt`) for `num_envs` envs over the terrain table `height_samples` [rows, cols] int16.  Owns the small device tables
    (`tables`: float32 copies of `leg_tables` / `joint_tables`).  `step(env, actions, u_cmd=None)` runs one env step in place on the
    tensors of `env`; with `u_cmd` left out the kernel draws the command resamples itself (Philox, keyed by `seed` and a call
    counter).  With `config.actuator` the launch is `dtc_sim_step_act` on the env's `lag_state` [N,6,12] and `push_vel` [N,2] as
    well: `lag_choice` (`decimation` slots; left out: drawn from a RandomState(seed) this object owns, as the reference draws on
    the host), `push` (the env's flag: this step draws a new push) and `u_push` [N,2] (left out: the kernel's Philox).  With
    `config.flight` the launch is `dtc_sim_step_fly` (on whichever of the above the config asks for) and writes the env's `airborne`
    and `crashed` [N] uint8 as well."""

    def __init__(self, num_envs: int, device, config: SimConfig, height_samples: torch.Tensor, *, seed: int = 0, tables: dict | None = None):
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if num_envs < 1 or len(config.default_dof_pos) != 12:
            raise ValueError("SimStep: >= 1 env and four legs of three joints are supported")
        if height_samples.dtype != torch.int16 or height_samples.dim() != 2 or min(height_samples.shape) < 2:
            raise ValueError("SimStep: height_samples must be an int16 table of at least 2 x 2")
        self.N, self.device, self.cfg, self.seed, self.counter = int(num_envs), dev, config, int(seed), 0
        self.height_samples = height_samples.to(dev).contiguous()
        t = dict(leg_tables(config), **joint_tables(config)) if tables is None else tables
        self.tables = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32).to(dev).contiguous() for k, v in t.items()}
        if config.actuator is not None:
            config.actuator.validate()
            self._lag_rng = np.random.RandomState(self.seed)
        if config.flight is not None:
            config.flight.validate()
        if config.contacts is not None:
            config.contacts.validate(config)
            self.knee = {k: torch.as_tensor(v, dtype=torch.float32).to(dev).contiguous() for k, v in knee_tables(config).items()}
        if config.balance is not None:
            config.balance.validate()

    def cfg_struct(self) -> "_ffi.DtcSimCfg":
        k, c = self.cfg, _ffi.DtcSimCfg()
        c.num_dof, c.num_bodies, c.num_commands, c.decimation = 12, int(k.num_bodies), int(k.num_commands), int(k.decimation)
        c.heading_command, c.buffer_len, c.resampling_steps = int(k.heading_command), int(k.buffer_len), int(k.resampling_steps)
        for l in range(4):
            c.feet[l], c.thighs[l] = int(k.feet[l]), int(k.thighs[l])
        c.sim_dt, c.action_scale, c.clip_actions, c.joint_inertia = k.sim_dt, k.action_scale, k.clip_actions, k.joint_inertia
        c.contact_eps, c.weight, c.r_min = k.contact_eps, float(np.float32(k.mass * k.gravity)), k.r_min
        c.rows, c.cols = int(self.height_samples.shape[0]), int(self.height_samples.shape[1])
        c.border_size, c.horizontal_scale, c.vertical_scale = k.border_size, k.horizontal_scale, k.vertical_scale
        for name in _RANGES:
            lo, hi = getattr(k, name)
            getattr(c, name)[0], getattr(c, name)[1] = float(lo), float(hi)
        c.seed, c.counter = self.seed, self.counter
        return c

    def _check(self, name, t, tail, dtype):
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != dtype or tuple(t.shape) != tail or not t.is_contiguous():
            raise _ffi.DtcError(f"SimStep: {name} must be a contiguous {dtype} tensor of shape {tail} on {self.device}")

    def act_struct(self, lag_choice=None, push: bool = False) -> "_ffi.DtcSimActuator":
        """The by-value constants of dtc_sim_step_act (the three pointers are left NULL)."""
        k, a, act = self.cfg, self.cfg.actuator, _ffi.DtcSimActuator()
        if lag_choice is None:
            lag_choice = self._lag_rng.randint(int(a.lag_slots[0]), int(a.lag_slots[1]) + 1, size=int(k.decimation))
        lag_choice = [int(v) for v in lag_choice]
        if len(lag_choice) != int(k.decimation) or not all(0 <= v <= 5 for v in lag_choice):
            raise _ffi.DtcError(f"SimStep: lag_choice must be {int(k.decimation)} slots in 0..5, got {lag_choice}")
        for it, v in enumerate(lag_choice):
            act.lag_choice[it] = v
        act.lag, act.push, act.push_now = int(bool(a.lag)), int(bool(a.push)), int(bool(a.push) and bool(push))
        act.keep = float(np.float32(math.exp(-k.sim_dt / a.push_decay_s)))
        act.floor2 = float(np.float32(a.push_floor * a.push_floor))
        act.push_span, act.push_lo = float(np.float32(2.0 * a.max_push_vel_xy)), float(np.float32(-a.max_push_vel_xy))
        return act

    def step(self, env, actions: torch.Tensor, u_cmd: torch.Tensor | None = None, *, lag_choice=None, u_push: torch.Tensor | None = None,
             push: bool = False):
        k, N = self.cfg, self.N
        if k.actuator is None and (lag_choice is not None or u_push is not None or push):
            raise _ffi.DtcError("SimStep: lag_choice / u_push / push need config.actuator")
        dims = dict(D=12, B=int(k.num_bodies), C=int(k.num_commands))
        s = _ffi.DtcSimStep()
        self._check("actions", actions, (N, 12), torch.float32)
        s.actions_in = _ffi.ptr(actions)
        for name, (*tail, dtype) in _ENV_TENSORS.items():
            tail = tuple(v for t in tail for v in (t if isinstance(t, tuple) else (t,)))
            t = getattr(env, name)
            self._check(name, t, (N,) + tuple(dims.get(v, v) for v in tail), dtype)
            setattr(s, name, _ffi.ptr(t))
        for name, width in _RING_BUFFERS.items():
            t = getattr(env, name)
            self._check(name, t, (int(k.buffer_len), N, dims.get(width, width)), torch.float32)
            setattr(s, name, _ffi.ptr(t))
        for name in ("dof_pos", "dof_vel"):                              # the two interleaved views of dof_state [N,D,2], or dense
            t = getattr(env, name)
            if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.float32 or tuple(t.shape) != (N, 12):
                raise _ffi.DtcError(f"SimStep: {name} must be a float32 tensor of shape {(N, 12)} on {self.device}")
            setattr(s, name, _ffi.ptr(t))
            setattr(s, name + "_row_stride", t.stride(0))
            setattr(s, name + "_elem_stride", t.stride(1))
        if u_cmd is not None:
            self._check("u_cmd", u_cmd, (N, 3), torch.float32)
            s.u_cmd = _ffi.ptr(u_cmd)
        s.height_samples = _ffi.ptr(self.height_samples)
        for name, t in self.tables.items():
            setattr(s, name, _ffi.ptr(t))
        c = self.cfg_struct()
        tilt = _ffi.DtcSimTilt(float(k.max_slope), float(k.min_det)) if k.tilt else None
        drew_push = False
        act = None
        if k.actuator is not None:
            act = self.act_struct(lag_choice, push)
            self._check("lag_state", env.lag_state, (N, 6, 12), torch.float32)
            act.lag_state = _ffi.ptr(env.lag_state)
            if k.actuator.push:
                self._check("push_vel", env.push_vel, (N, 2), torch.float32)
                act.push_vel = _ffi.ptr(env.push_vel)
                if u_push is not None:
                    self._check("u_push", u_push, (N, 2), torch.float32)
                    act.u_push = _ffi.ptr(u_push)
                drew_push = bool(act.push_now) and u_push is None
        if k.flight is not None:
            f = k.flight
            fly = _ffi.DtcSimFlight(float(f.gravity), float(f.max_step_up), float(f.crash_force))
            for name in ("airborne", "crashed"):
                self._check(name, getattr(env, name), (N,), torch.uint8)
                setattr(fly, name, _ffi.ptr(getattr(env, name)))
            _ffi.check(_ffi.lib().dtc_sim_step_fly(s, c, tilt, act, fly, N, _ffi.stream()), "dtc_sim_step_fly")
        elif act is not None:
            _ffi.check(_ffi.lib().dtc_sim_step_act(s, c, tilt, act, N, _ffi.stream()), "dtc_sim_step_act")
        elif k.tilt:
            _ffi.check(_ffi.lib().dtc_sim_step_tilt(s, c, tilt, N, _ffi.stream()), "dtc_sim_step_tilt")
        else:
            _ffi.check(_ffi.lib().dtc_sim_step(s, c, N, _ffi.stream()), "dtc_sim_step")
        if u_cmd is None or drew_push:
            self.counter += 1

    def contacts(self, env):
        """`dtc_sim_contacts` on the tensors of `env`, as `step` just wrote them: the thigh, shank and foot-xy rows of
        `contact_forces`, the knee positions (shank rows of `rigid_body_state`), `leg_contact` [N,8] and `stumbled` [N,4] uint8.
        Needs `config.contacts`."""
        k, N = self.cfg, self.N
        if k.contacts is None:
            raise _ffi.DtcError("SimStep: contacts() needs config.contacts")
        B = int(k.num_bodies)
        s = _ffi.DtcSimStep()
        for name, tail in (("base_pos", (3,)), ("base_quat", (4,)), ("rigid_body_state", (B, 13)), ("contact_forces", (B, 3))):
            self._check(name, getattr(env, name), (N,) + tail, torch.float32)
            setattr(s, name, _ffi.ptr(getattr(env, name)))
        t = env.dof_pos                                                  # an interleaved view of dof_state [N,D,2], or dense
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.float32 or tuple(t.shape) != (N, 12):
            raise _ffi.DtcError(f"SimStep: dof_pos must be a float32 tensor of shape {(N, 12)} on {self.device}")
        s.dof_pos, s.dof_pos_row_stride, s.dof_pos_elem_stride = _ffi.ptr(t), t.stride(0), t.stride(1)
        s.default_dof_pos, s.height_samples = _ffi.ptr(self.tables["default_dof_pos"]), _ffi.ptr(self.height_samples)
        con = self.contact_struct()
        for name, width in (("leg_contact", 8), ("stumbled", 4)):
            self._check(name, getattr(env, name), (N, width), torch.uint8)
            setattr(con, name, _ffi.ptr(getattr(env, name)))
        _ffi.check(_ffi.lib().dtc_sim_contacts(s, self.cfg_struct(), con, N, _ffi.stream()), "dtc_sim_contacts")

    def balance(self, env):
        """`dtc_sim_balance` on the tensors of `env`, as `step` just wrote them: the env's `lean` [N,4] and `fallen` [N] uint8, and
        with a lean the base's attitude, height and angular velocity in `base_quat`, `root_states`, `base_pos`,
        `projected_gravity`, `base_lin_vel`, `base_ang_vel`, the base row of `rigid_body_state` and, for a fallen env, of
        `contact_forces`.  Needs `config.balance`."""
        k, N = self.cfg, self.N
        if k.balance is None:
            raise _ffi.DtcError("SimStep: balance() needs config.balance")
        B = int(k.num_bodies)
        s = _ffi.DtcSimStep()
        for name, tail, dtype in (("root_states", (13,), torch.float32), ("base_pos", (3,), torch.float32), ("base_quat", (4,), torch.float32),
                                  ("projected_gravity", (3,), torch.float32), ("base_lin_vel", (3,), torch.float32),
                                  ("base_ang_vel", (3,), torch.float32), ("rigid_body_state", (B, 13), torch.float32),
                                  ("contact_forces", (B, 3), torch.float32), ("contact_filt", (4,), torch.bool),
                                  ("episode_length_buf", (), torch.int64)):
            self._check(name, getattr(env, name), (N,) + tail, dtype)
            setattr(s, name, _ffi.ptr(getattr(env, name)))
        bal = self.balance_struct()
        for name, tail, dtype in (("lean", (4,), torch.float32), ("fallen", (), torch.uint8)):
            self._check(name, getattr(env, name), (N,) + tail, dtype)
            setattr(bal, name, _ffi.ptr(getattr(env, name)))
        _ffi.check(_ffi.lib().dtc_sim_balance(s, self.cfg_struct(), bal, N, _ffi.stream()), "dtc_sim_balance")

    def balance_struct(self) -> "_ffi.DtcSimBalance":
        """The constants of dtc_sim_balance (the two pointers are left NULL)."""
        k, b, bal = self.cfg, self.cfg.balance, _ffi.DtcSimBalance()
        for name in ("gravity", "h_min", "lean_eps", "fall_angle", "fall_force"):
            setattr(bal, name, float(getattr(b, name)))
        bal.dt = float(np.float32(float(k.sim_dt) * int(k.decimation)))
        bal.com_offset[0], bal.com_offset[1] = float(b.com_offset[0]), float(b.com_offset[1])
        return bal

    def contact_struct(self) -> "_ffi.DtcSimContacts":
        """The constants and the two knee tables of dtc_sim_contacts (the two flag pointers are left NULL)."""
        c, con = self.cfg.contacts, _ffi.DtcSimContacts()
        con.knee_nominal, con.knee_jacobian = _ffi.ptr(self.knee["knee_nominal"]), _ffi.ptr(self.knee["knee_jacobian"])
        for l in range(4):
            con.shanks[l] = int(c.shanks[l])
        for name in ("body_radius", "stiffness", "max_force", "probe", "stumble_height", "wall_damping", "min_speed"):
            setattr(con, name, float(getattr(c, name)))
        return con
