"""SurrogateLeggedEnv: a closed-loop legged env that lives entirely in device memory, with no simulator behind it.

`dtc_sim_step` (csrc/sim.hip) stands where LeggedRobotDTC calls Isaac Gym and fills the tensors the env-side kernels read; the rest
of `step()` is the reference's post_physics_step on those kernels: `EnvStep` (heights, planner, termination, foothold rewards,
observations), `EnvRewards`, `EnvReset` on `reset_buf`, `compute_observations(where=reset_buf)`, the step tail
(legged_robot_dtc.py:215-223) and the observation clip (legged_robot.py:118-121).  Nothing in `step()` reads the device or calls
`nonzero()`.  The env owns every tensor under the attribute name the reference env uses.

It is a surrogate, not physics (include/dtc_hip.h lists what is absent; `SimConfig.tilt` opts into a kinematic roll and pitch): it gives the kernels a state that is consistent, evolves,
responds to actions, terminates and resets, and a reward that depends on what the policy does.

`SimConfig.actuator` (opt-in, a `sim.ActuatorConfig`; None: the env above, bit for bit) adds the reference's two training
disturbances to the same launch: the PD goal lags behind the action by a host-drawn number of substeps (`lag_state`, and
`lag_buffer`, its six slots under the reference's name), and every `push_interval` steps, on two consecutive steps, a random planar
velocity is given to the base (`push_vel`; `common_step_counter` is a host integer).  The push is a kinematic slip velocity with a
chosen decay, not a contact dynamics.

`SurrogateConfig.terrain` (opt-in, a `terrain.TerrainConfig`; None: the env above, bit for bit) puts the env on the DTC curriculum
terrain generated on the device (`dtc_amd.terrain`): stairs, stepping stones, gaps, pits.  The env origins are then the sub-terrain
origins, `terrain_levels` / `terrain_types` are set as LeggedRobot._get_env_origins does (legged_robot.py:1205-1215) and the terrain
curriculum of reset_idx runs on state that evolves.  What this is NOT: the surrogate rides on its highest support, so a foot over a
hole is simply out of contact, and an env whose four feet are all over a gap drops to the gap floor kinematically and climbs the far
wall in one step -- there is no falling, no collision with a wall and no getting stuck; the terrain shapes the footholds, the height
scan, the rewards and the curriculum, not a contact dynamics.

`SimConfig.flight` (opt-in, a `sim.FlightConfig`; None: the env above, bit for bit, nothing new allocated) changes exactly that, in
the same launch (`dtc_sim_step_fly`): a base whose support falls away falls under gravity and lands when it reaches a support, and a
support that rises by more than `max_step_up` within a substep is a crash.  The env then owns `airborne` and `crashed` [N] uint8.
Nothing else in `step()` changes: a crash reaches `reset_buf` through the base's contact force and check_termination, as a fall does
in the reference, and a base that falls into a gap terminates through the existing base-height rule.  Still a surrogate: the
flight is a point mass on a parabola, `max_step_up`, `crash_force` and the take-off rule are choices, and nothing topples.

`SimConfig.contacts` (opt-in, a `sim.ContactConfig`; None: the env above, bit for bit, nothing new allocated or launched) runs
`dtc_sim_contacts` directly behind the surrogate step: thighs and shanks that penetrate the terrain and a swing foot that flies into
a riser get contact forces, so the reward terms `collision`, `stumble`, `feet_stumble` and `foot_clearance` see non-zero inputs
through the tensors they already read (`CONTACT_SCALES` holds scales for the first two; `reward_scales` stays the caller's).  The
env then owns `leg_contact` [N,8] and `stumbled` [N,4] uint8.  The forces feed the rewards and nothing else: a colliding shank is
not held back, a stumbling foot is not stopped but lifted onto the riser as before, nothing topples, the torso has no contact of
its own, and every constant is a choice.

`SimConfig.balance` (opt-in, a `sim.BalanceConfig`; None: the env above, bit for bit, nothing new allocated or launched) runs
`dtc_sim_balance` between the surrogate step and `dtc_sim_contacts`: a point-mass inverted pendulum about the edge of the support
polygon of the stance feet.  A base whose xy leaves the support of its stance feet leans, faster the further it leans; over its
support a lean is restored and lands.  The lean is laid over `base_quat`, `root_states`, `projected_gravity`, `base_lin_vel`,
`base_ang_vel`, `base_pos` and the base row of `rigid_body_state`, so the `orientation`, `ang_vel_xy` and base-height terms see it
(`BALANCE_SCALES` holds scales for a caller to add), and a lean beyond `fall_angle` ends the episode through the base's contact
force and check_termination.  The env then owns `lean` [N,4] float32 (cleared by a reset) and `fallen` [N] uint8, and
`extras["episode"]["fall_rate"]` is the share of envs that fell in the step (a device scalar).  Still a surrogate: the link
positions are not rotated (planner and contacts see the un-leaned feet and hips), pushes do not feed the lean rate, there
is no friction and no slipping pivot, crossed feet are neglected, and every constant is a choice.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from .. import foothold, reset, rewards, sim
from ..terrain import Terrain, TerrainConfig
from .vec_env import VecEnv

# raw reward scales (multiplied by dt, as the reference does): a Lite3-style set in which every term reads surrogate state
_SCALES = dict(action_rate=-0.01, ang_vel_xy=-0.005, dof_acc=-2.5e-8, dof_pos_limits=-10.0, feet_air_time=1.0, lin_vel_z=-0.2,
               smooth=-0.0015, torques=-1e-6, tracking_ang_vel=0.5, tracking_lin_vel=1.0, tracking_optimal_footholds=0.2)
# the two terms `SimConfig.contacts` gives an input to, for a caller to add to `reward_scales` (the default set is not touched):
# collision is the Lite3 DTC value (lite3_dtc_config.py:161), stumble is a choice of this project
CONTACT_SCALES = dict(collision=-1.5, stumble=-0.5)
# the two terms that read what `SimConfig.balance` writes, likewise for a caller to add: the Lite3 DTC values
# (lite3_dtc_config.py:150, :162); the default set is not touched
BALANCE_SCALES = dict(orientation=-0.5, termination=-0.1)


@dataclass
class SurrogateConfig:
    """Defaults: the Lite3 DTC values (53 / 1389 / 12, the 33 x 21 grid, decimation 4, dt 0.005, Kp 25, Kd 0.5, action scale 0.25)."""
    sim: sim.SimConfig = field(default_factory=sim.SimConfig)
    obs: foothold.ObsConfig = field(default_factory=foothold.ObsConfig)
    grid: foothold.GridConfig = field(default_factory=foothold.GridConfig)
    reward_scales: dict = field(default_factory=lambda: dict(_SCALES))
    episode_length_s: float = 20.0
    num_observation_history: int = 5
    clip_observations: float = 100.0
    randomize_motor_strength: bool = True
    add_noise: bool = True                   # observation noise (legged_robot_dtc.py:284-288) when the draws are not given
    noise_scales: dict = field(default_factory=lambda: dict(ang_vel=0.2, gravity=0.05, dof_pos=0.01, dof_vel=1.5))
    contain_nonfinite: bool = True           # an env whose dofs or root state are not finite after the surrogate step is reset at once
    env_spacing: float = 1.0                 # env origins: rows of 32 envs, this far apart, inside the terrain table
    terrain: TerrainConfig | None = None     # opt-in: the DTC curriculum terrain, generated on the device (None: the tables above)

    @property
    def max_episode_length(self) -> int:
        return int(math.ceil(self.episode_length_s / self.sim.dt))                      # legged_robot.py:_parse_cfg

    def reward_config(self) -> rewards.RewardConfig:
        dt = self.sim.dt
        scales = {k: float(np.float32(v * dt)) for k, v in sorted(self.reward_scales.items()) if v != 0}
        return rewards.RewardConfig(scales=scales, dt=dt, base_height_target=self.obs.base_height_target,
                                    lin_vel_x_max=self.sim.lin_vel_x[1], ang_vel_yaw_max=self.sim.ang_vel_yaw[1],
                                    points_x=tuple(self.grid.points_x), points_y=tuple(self.grid.points_y))

    def reset_config(self) -> reset.ResetConfig:
        s = self.sim
        init = (0.0, 0.0, s.nominal_height, 0.0, 0.0, 0.0, 1.0) + (0.0,) * 6
        t = self.terrain
        if t is not None:
            return reset.ResetConfig(terrain_curriculum=bool(t.curriculum), custom_origins=True, max_terrain_level=int(t.num_rows),
                                     env_length=float(t.terrain_length), heading_command=s.heading_command,
                                     randomize_motor_strength=self.randomize_motor_strength, max_episode_length_s=self.episode_length_s,
                                     lin_vel_x=s.lin_vel_x, lin_vel_y=s.lin_vel_y, ang_vel_yaw=s.ang_vel_yaw, heading=s.heading,
                                     base_init_state=init)
        return reset.ResetConfig(terrain_curriculum=False, custom_origins=False, heading_command=s.heading_command,
                                 randomize_motor_strength=self.randomize_motor_strength, max_episode_length_s=self.episode_length_s,
                                 lin_vel_x=s.lin_vel_x, lin_vel_y=s.lin_vel_y, ang_vel_yaw=s.ang_vel_yaw, heading=s.heading,
                                 base_init_state=init)


class _Cfg:
    """The two config attributes HistoryWrapper and the runner read from an env."""

    def __init__(self, c: SurrogateConfig):
        self.env = type("env", (), dict(num_observation_history=c.num_observation_history, episode_length_s=c.episode_length_s))
        self.surrogate = c


class SurrogateLeggedEnv(VecEnv):
    """`num_envs` kinematic quadrupeds over the int16 terrain table `height_samples` (default: flat; `synthetic.reward_table()` is
    the rough one).  `step(actions, draws=None)`: `draws` is the parity mode -- a dict with any of u_cmd [N,3], u_reset [N,26],
    u_obs [N,53], u_heights [N,693] (uniform [0,1)), height_noise (float) and, with `config.sim.actuator`, lag_choice (`decimation`
    slots in 0..5, a host sequence) and u_push [N,2]; what it leaves out is drawn on the device from `seed`
    (command and reset draws by the kernels' Philox streams, the two observation noises by a seeded device generator); the reset's
    height_noise is the reference's host draw, np.random.normal(0, 0.02), from a seeded RandomState.

    With `config.terrain` set the table is the generated DTC terrain (`self.terrain`, a `dtc_amd.terrain.Terrain`; passing
    `height_samples` as well is an error), `terrain_levels` is drawn in [0, max_init_terrain_level] from the env's seeded device
    generator unless given, the first `reset()` leaves the levels alone (init_done, legged_robot.py:693-695), later resets move
    them, `draws` may carry level_draw [N] int64 next to u_reset, and `extras["episode"]["terrain_level"]` is the mean level
    (a device scalar).  `regenerate_terrain(seed)` lays the terrain out anew in place."""

    def __init__(self, num_envs: int, device="cuda", config: SurrogateConfig | None = None, height_samples: torch.Tensor | None = None,
                 seed: int = 0, terrain_levels: torch.Tensor | None = None):
        c = self.config = config or SurrogateConfig()
        tc = c.terrain
        if tc is not None:
            if height_samples is not None:
                raise ValueError("SurrogateLeggedEnv: config.terrain generates the table; height_samples cannot be given as well")
            tc.validate()
            for name in ("horizontal_scale", "vertical_scale", "border_size"):
                if float(getattr(tc, name)) != float(getattr(c.sim, name)):
                    raise ValueError(f"SurrogateLeggedEnv: terrain.{name} {getattr(tc, name)} != sim.{name} {getattr(c.sim, name)}")
            max_init = int(tc.max_init_terrain_level) if tc.curriculum else tc.num_rows - 1          # legged_robot.py:1209-1210
            if not 0 <= max_init < tc.num_rows:
                raise ValueError(f"SurrogateLeggedEnv: max_init_terrain_level {max_init} outside 0..{tc.num_rows - 1}")
        elif terrain_levels is not None:
            raise ValueError("SurrogateLeggedEnv: terrain_levels needs config.terrain")
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        s = c.sim
        N, D, B, C, P, T = int(num_envs), 12, int(s.num_bodies), int(s.num_commands), c.grid.num_points, int(s.buffer_len)
        self.cfg, self.device, self.num_envs, self.num_dof, self.num_bodies, self.num_actions = _Cfg(c), dev, N, D, B, D
        self.num_obs, self.num_privileged_obs = 9 + 3 * D + c.obs.num_foothold_obs, 2 * P + 3
        self.num_obs_history = c.num_observation_history * self.num_obs
        self.max_episode_length, self.dt = c.max_episode_length, s.dt
        self.terrain = Terrain(tc, dev) if tc is not None else None
        if self.terrain is not None:
            self.height_samples = self.terrain.height_field_raw
        else:
            self.height_samples = (sim.flat_table() if height_samples is None else height_samples).to(dev).contiguous()
        self.sim = sim.SimStep(N, dev, s, self.height_samples, seed=seed)
        f = dict(dtype=torch.float32, device=dev)
        z = lambda *shape: torch.zeros(*shape, **f)                                      # noqa: E731
        t = self.sim.tables
        self.default_dof_pos, self.dof_pos_limits, self.torque_limits = t["default_dof_pos"].view(1, D), t["dof_pos_limits"], t["torque_limits"]
        self.p_gains, self.d_gains, self.dof_vel_limits = t["p_gains"], t["d_gains"], torch.full((D,), 30.0, **f)
        self.feet_indices = torch.tensor(s.feet, dtype=torch.int64, device=dev)
        self.thigh_indices = torch.tensor(s.thighs, dtype=torch.int64, device=dev)
        self.termination_contact_indices = torch.tensor([0], dtype=torch.int64, device=dev)
        self.penalised_contact_indices = torch.tensor([b for l in range(4) for b in (s.thighs[l], s.thighs[l] + 1)], dtype=torch.int64, device=dev)
        self.hip_indices = torch.tensor([0, 3, 6, 9], dtype=torch.int64, device=dev)
        self.command_ranges = {k: list(getattr(s, k)) for k in ("lin_vel_x", "lin_vel_y", "ang_vel_yaw", "heading")}
        # state
        self.dof_state = z(N, D, 2)
        self.dof_pos, self.dof_vel = self.dof_state[..., 0], self.dof_state[..., 1]
        self.root_states, self.rigid_body_state, self.contact_forces = z(N, 13), z(N, B, 13), z(N, B, 3)
        self.torques, self.actions, self.last_actions, self.last_actions_2, self.last_dof_vel = z(N, D), z(N, D), z(N, D), z(N, D), z(N, D)
        self.last_root_vel, self.last_foot_velocities = z(N, 6), z(N, 4, 3)
        self.base_lin_vel, self.base_ang_vel, self.last_base_ang_vel, self.projected_gravity = z(N, 3), z(N, 3), z(N, 3), z(N, 3)
        self.base_ang_vel_last, self.base_lin_vel_last, self.base_pos, self.base_quat = z(N, 3), z(N, 3), z(N, 3), z(N, 4)
        self.commands, self.forces, self.height_noise_offset = z(N, C), z(N, B, 3), z(N, P)
        self.lin_vel_buffer, self.ang_vel_buffer, self.cmd_buffer = z(T, N, 2), z(T, N, 1), z(T, N, C)
        self.Kp_factors, self.Kd_factors, self.motor_strengths, self.motor_offsets = 1 + z(N, D), 1 + z(N, D), 1 + z(N, D), z(N, D)
        self.episode_length_buf = torch.zeros(N, dtype=torch.int64, device=dev)
        self._actuator_rows = ()
        if s.actuator is not None:                                                       # legged_robot.py:827, :546-553
            self.lag_state, self.push_vel, self.common_step_counter = z(N, 6, D), z(N, 2), 0
            self.lag_buffer = [self.lag_state[:, i] for i in range(6)]
            self._actuator_rows = (self.lag_state, self.push_vel)
        if s.flight is not None:
            self.airborne, self.crashed = torch.zeros(N, dtype=torch.uint8, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev)
        self._contact_flags = ()
        if s.contacts is not None:
            self.leg_contact, self.stumbled = torch.zeros(N, 8, dtype=torch.uint8, device=dev), torch.zeros(N, 4, dtype=torch.uint8, device=dev)
            self._contact_flags = (self.leg_contact, self.stumbled)
        self._balance_rows = ()
        if s.balance is not None:
            self.lean, self.fallen = z(N, 4), torch.zeros(N, dtype=torch.uint8, device=dev)
            self._balance_rows = (self.lean,)
        self.last_contacts = torch.zeros(N, 4, dtype=torch.bool, device=dev)
        self.contact_filt = torch.zeros(N, 4, dtype=torch.bool, device=dev)
        self.robot_mass = torch.full((N,), float(s.mass), **f)
        self.terrain_levels = torch.zeros(N, dtype=torch.int64, device=dev)
        i = torch.arange(N, device=dev)
        self.env_origins = torch.stack([(i % 32) * c.env_spacing, (i // 32 % 24) * c.env_spacing, torch.zeros_like(i)], dim=1).float().contiguous()
        self.noise_scale_vec = z(self.num_obs)                                           # _get_noise_scale_vec, noise level 1
        ns, ob = c.noise_scales, c.obs
        self.noise_scale_vec[0:3], self.noise_scale_vec[3:6] = ns["ang_vel"] * ob.ang_vel, ns["gravity"]
        self.noise_scale_vec[9:9 + D], self.noise_scale_vec[9 + D:9 + 2 * D] = ns["dof_pos"] * ob.dof_pos, ns["dof_vel"] * ob.dof_vel
        self.rew_buf = z(N)
        self.extras = {}
        self.nonfinite_act_envs = None            # OnPolicyRunner.learn hands the policy-step containment's mask over here
        # the env-side kernels
        self.env_step = foothold.EnvStep(N, dev, c.grid, c.obs)
        self.env_rewards = rewards.EnvRewards(N, dev, c.reward_config(), feet_indices=self.feet_indices,
                                              penalised_contact_indices=self.penalised_contact_indices, hip_indices=self.hip_indices, num_dof=D)
        self.feet_air_time, self.pitch_est = self.env_rewards.feet_air_time, self.env_rewards.pitch_est
        names = self.env_rewards.cfg.names
        self.episode_sums = {n: self.env_rewards.episode_sums[k] for k, n in enumerate(names)}
        self.env_reset = reset.EnvReset(N, dev, c.reset_config(), n_sums=len(names), num_dof=D, seed=seed)
        self._episode = {"rew_" + n: self.env_reset.episode_means[k] for k, n in enumerate(names)}
        self._height_noise = np.random.RandomState(seed)
        self._gen = torch.Generator(device=dev).manual_seed(seed) if dev.type == "cuda" else None
        self._out = self.env_step.out
        self.reset_buf, self.time_out_buf = self._out["reset_buf"], self._out["time_out_buf"]
        self.obs_buf, self.privileged_obs_buf = self._out["obs_buf"], self._out["privileged_obs_buf"]
        self.custom_origins, self.init_done = self.terrain is not None, self.terrain is None
        if self.terrain is not None:                                                     # _get_env_origins, legged_robot.py:1205-1215
            if terrain_levels is None:
                terrain_levels = torch.randint(0, max_init + 1, (N,), generator=self._gen, device=dev)
            elif tuple(terrain_levels.shape) != (N,) or terrain_levels.dtype != torch.int64:
                raise ValueError(f"SurrogateLeggedEnv: terrain_levels must be an int64 tensor of shape {(N,)}")
            self.terrain_levels = terrain_levels.to(dev).clone().contiguous()
            self.terrain_types = torch.div(torch.arange(N, device=dev), N / tc.num_cols, rounding_mode="floor").to(torch.long)
            self.max_terrain_level = tc.num_rows
            self.terrain_origins = self.terrain.env_origins
            self.env_origins = self.terrain_origins[self.terrain_levels, self.terrain_types].contiguous()
            if tc.curriculum:
                self._episode["terrain_level"] = self.env_reset.terrain_level_mean[0]   # legged_robot.py:257-259

    # ------------------------------------------------------------------ one env step
    def _observation_inputs(self, draws):
        if not draws:                            # production mode: seeded device draws, as the reference's two torch.rand_like
            draws = dict(u_heights=torch.rand(self.num_envs, self.config.grid.num_points, generator=self._gen, device=self.device))
            if self.config.add_noise:
                draws["u_obs"] = torch.rand(self.num_envs, self.num_obs, generator=self._gen, device=self.device)
        return dict(base_ang_vel=self.base_ang_vel, projected_gravity=self.projected_gravity, commands=self.commands, dof_pos=self.dof_pos,
                    default_dof_pos=self.default_dof_pos, dof_vel=self.dof_vel, actions=self.actions, forces=self.forces,
                    root_states=self.root_states, height_noise_offset=self.height_noise_offset, u_obs=draws.get("u_obs"),
                    noise_scale_vec=self.noise_scale_vec if draws.get("u_obs") is not None else None, u_heights=draws.get("u_heights"))

    def _reset_envs(self, draws):
        """reset_idx for the envs named in reset_buf (legged_robot.py:200-272), one dtc_env_reset call."""
        hn = draws.get("height_noise")
        on_terrain = {}
        if self.terrain is not None:
            on_terrain = dict(terrain_levels=self.terrain_levels, terrain_types=self.terrain_types, terrain_origins=self.terrain_origins,
                              level_draw=draws.get("level_draw"), init_done=self.init_done)
        self.env_reset(**on_terrain, reset_buf=self.reset_buf, root_states=self.root_states, env_origins=self.env_origins, commands=self.commands,
                       dof_pos=self.dof_pos, dof_vel=self.dof_vel, default_dof_pos=self.default_dof_pos.reshape(-1), forces=self.forces,
                       motor_strengths=self.motor_strengths, Kp_factors=self.Kp_factors, Kd_factors=self.Kd_factors,
                       height_noise_offset=self.height_noise_offset, episode_sums=self.env_rewards.episode_sums, stumble=self.env_rewards.stumble,
                       last_actions=self.last_actions, last_actions_2=self.last_actions_2, last_dof_vel=self.last_dof_vel,
                       feet_air_time=self.feet_air_time, pitch_est=self.pitch_est, base_ang_vel_last=self.base_ang_vel_last,
                       base_lin_vel_last=self.base_lin_vel_last, episode_length_buf=self.episode_length_buf, contact_filt=self.contact_filt,
                       last_contacts=self.last_contacts, lin_vel_buffer=self.lin_vel_buffer, ang_vel_buffer=self.ang_vel_buffer,
                       cmd_buffer=self.cmd_buffer, u=draws.get("u_reset"), command_ranges=self.command_ranges,
                       extra_rows=self._actuator_rows + self._balance_rows,
                       height_noise=float(self._height_noise.normal(0, 0.02)) if hn is None else float(hn))

    def step(self, actions: torch.Tensor, draws: dict | None = None):
        draws = draws or {}
        c, s = self.config, self.config.sim
        # 1. the surrogate's physics and the bookkeeping up to the planner
        if s.actuator is None:
            self.sim.step(self, actions.to(self.device, torch.float32).contiguous(), draws.get("u_cmd"))
        else:                                                                            # legged_robot.py:67, :673
            self.common_step_counter += 1
            push = s.actuator.push and self.common_step_counter % s.push_interval in (0, 1)
            self.sim.step(self, actions.to(self.device, torch.float32).contiguous(), draws.get("u_cmd"), lag_choice=draws.get("lag_choice"),
                          u_push=draws.get("u_push"), push=push)
        if s.balance is not None:                                                        # the lean over the support polygon, and falls
            self.sim.balance(self)
        if s.contacts is not None:                                                       # leg collisions and stumbles, on what the step wrote
            self.sim.contacts(self)
        if s.heading_command:                                                            # legged_robot.py:537-539
            if s.tilt:                                                                   # forward = quat_apply(q, (1, 0, 0))
                qx, qy, qz, qw = self.base_quat.unbind(dim=1)
                heading = torch.atan2(2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qy * qy + qz * qz))
            else:                                                                        # the same, for a yaw-only base
                heading = torch.atan2(2.0 * self.base_quat[:, 2] * self.base_quat[:, 3], 1.0 - 2.0 * self.base_quat[:, 2] * self.base_quat[:, 2])
            d = self.commands[:, 3] - heading
            d = torch.remainder(d + math.pi, 2 * math.pi) - math.pi                      # wrap_to_pi
            self.commands[:, 2] = torch.clip(0.5 * d, -1.5, 1.5)
        bad = None
        if c.contain_nonfinite:
            # a non-finite env (its own divergence, or NaN written into its state) would carry NaN into the rewards, the episode
            # sums and every later step: its rows are zeroed here, ahead of every consumer, and it is reset in this step
            bad = ~(torch.isfinite(self.dof_state).flatten(1).all(dim=1) & torch.isfinite(self.root_states).all(dim=1))
            for t in (self.dof_state, self.root_states, self.rigid_body_state, self.contact_forces, self.torques, self.base_lin_vel,
                      self.base_ang_vel, self.last_base_ang_vel, self.base_pos, self.base_quat) + self._actuator_rows + self._balance_rows:
                t.masked_fill_(bad.view(-1, *([1] * (t.dim() - 1))), 0.0)
            for t in (self.lin_vel_buffer, self.ang_vel_buffer, self.cmd_buffer):
                t.masked_fill_(bad.view(1, -1, 1), 0.0)
            for t in self._contact_flags:
                t.masked_fill_(bad.view(-1, 1), 0)
            if s.balance is not None:
                self.fallen.masked_fill_(bad, 0)
        self.foot_positions = self.rigid_body_state[:, self.feet_indices, 0:3]
        self.foot_velocities = self.rigid_body_state[:, self.feet_indices, 7:10]
        self.hip_positions = self.rigid_body_state[:, self.thigh_indices, 0:3]
        # 2. heights, planner, termination, foothold rewards, observations
        obs_in = self._observation_inputs(draws)
        o = self.env_step(thigh_pos=self.hip_positions, contact_forces=self.contact_forces,
                          termination_contact_indices=self.termination_contact_indices, episode_length_buf=self.episode_length_buf,
                          max_episode_length=self.max_episode_length, foot_positions=self.foot_positions, contact_filt=self.contact_filt,
                          height_samples=self.height_samples, border_size=s.border_size, horizontal_scale=s.horizontal_scale,
                          vertical_scale=s.vertical_scale, **obs_in)
        self.measured_heights, self.foothold_obs, self.optimal_footholds_world = o["measured_heights"], o["foothold_obs"], o["optimal_footholds_world"]
        if bad is not None:
            self.reset_buf |= bad.to(torch.uint8)
        if self.nonfinite_act_envs is not None:
            self.reset_buf |= self.nonfinite_act_envs                                    # envs whose policy step was repaired
        # 3. the reward terms
        self.env_rewards(last_contacts=self.last_contacts, out=self.rew_buf, height_samples=self.height_samples, border_size=s.border_size,
                         horizontal_scale=s.horizontal_scale, vertical_scale=s.vertical_scale, root_states=self.root_states,
                         base_lin_vel=self.base_lin_vel, base_ang_vel=self.base_ang_vel, projected_gravity=self.projected_gravity,
                         commands=self.commands, dof_pos=self.dof_pos, default_dof_pos=self.default_dof_pos.reshape(-1), dof_vel=self.dof_vel,
                         last_dof_vel=self.last_dof_vel, torques=self.torques, actions=self.actions, last_actions=self.last_actions,
                         last_actions_2=self.last_actions_2, contact_forces=self.contact_forces, foot_positions=self.foot_positions,
                         foot_velocities=self.foot_velocities, last_foot_velocities=self.last_foot_velocities,
                         optimal_footholds_world=self.optimal_footholds_world, contact_filt=self.contact_filt,
                         measured_heights=self.measured_heights, reset_buf=self.reset_buf, time_out_buf=self.time_out_buf,
                         robot_mass=self.robot_mass, terrain_levels=self.terrain_levels, dof_pos_limits=self.dof_pos_limits,
                         dof_vel_limits=self.dof_vel_limits, torque_limits=self.torque_limits, cmd_buffer=self.cmd_buffer,
                         lin_vel_buffer=self.lin_vel_buffer, ang_vel_buffer=self.ang_vel_buffer)
        # 4. reset, 5. the observation rows of the reset envs: their new dofs, root state and commands, the stale derived quantities
        self._reset_envs(draws)
        foothold.compute_observations(foothold_obs=self.foothold_obs, measured_heights=self.measured_heights, cfg=c.obs, where=self.reset_buf,
                                      out=self._out, **obs_in)
        # 6. the step tail (legged_robot_dtc.py:215-223)
        self.last_actions_2.copy_(self.last_actions)
        self.last_actions.copy_(self.actions)
        self.last_dof_vel.copy_(self.dof_vel)
        self.last_root_vel.copy_(self.root_states[:, 7:13])
        self.last_foot_velocities.copy_(self.foot_velocities)
        self.base_ang_vel_last.copy_(self.base_ang_vel)
        self.base_lin_vel_last.copy_(self.base_lin_vel)
        # 7. the observation clip (legged_robot.py:118-121)
        self.obs_buf = torch.clip(self._out["obs_buf"], -c.clip_observations, c.clip_observations)
        self.privileged_obs_buf = torch.clip(self._out["privileged_obs_buf"], -c.clip_observations, c.clip_observations)
        self.extras = {"time_outs": self.time_out_buf.bool(), "episode": dict(self._episode)}
        if s.balance is not None:
            self.extras["episode"]["fall_rate"] = self.fallen.float().mean()
        return self.obs_buf, self.privileged_obs_buf, self.rew_buf, self.reset_buf.bool(), self.extras

    # ------------------------------------------------------------------ the rest of the env contract
    def reset(self, env_ids=None, draws: dict | None = None):
        """Reset every env, then one step with zero actions (base_task.py:115-119)."""
        self.reset_buf.fill_(1)
        self._reset_envs(draws or {})
        self.init_done = True                                                            # the initial reset moved no level; later ones do
        obs, _, _, _, _ = self.step(torch.zeros(self.num_envs, self.num_actions, device=self.device), draws)
        return obs

    def regenerate_terrain(self, seed: int):
        """A new layout from `seed`, in place: the table every kernel holds is refilled, and the env origins follow the new
        sub-terrain origins at the unchanged levels.  Robots stay where they are until their next reset."""
        if self.terrain is None:
            raise ValueError("SurrogateLeggedEnv.regenerate_terrain: the env has no config.terrain")
        self.terrain.generate(seed)
        self.env_origins.copy_(self.terrain_origins[self.terrain_levels, self.terrain_types])

    def get_observations(self):
        return self.obs_buf

    def get_privileged_observations(self):
        return self.privileged_obs_buf

    def get_base_vel(self):
        return self.base_lin_vel * self.config.obs.lin_vel                               # legged_robot.py:1429-1431

    def get_reward_buf(self):
        return self.rew_buf
