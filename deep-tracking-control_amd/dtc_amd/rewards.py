"""Host side of the fused env rewards (drop-in for LeggedRobot.compute_reward, legged_gym/envs/base/legged_robot.py:274-291).

`RewardConfig.from_cfg(env_cfg)` resolves the reward scales the way `_prepare_reward_function` does (legged_robot.py:929-952);
`EnvRewards` owns the reward state and the episode sums and runs every active `_reward_*` term of LeggedRobotDTC in ONE launch
(csrc/rewards.hip, `dtc_env_rewards`); `patch_env(env)` replaces an env's `compute_reward` by that launch on the env's own buffers.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _ffi
from .synthetic import MEASURED_POINTS_X, MEASURED_POINTS_Y

# the 34 `_reward_*` methods of LeggedRobotDTC, in the order of DTC_REW_* (include/dtc_hip.h): alphabetical
TERMS = tuple(sorted("""action_rate ang_vel_xy base_height big_pitch collision dof_acc dof_pos_limits dof_vel dof_vel_limits feet_air_time
feet_contact_forces feet_slip feet_stumble foot_acc foot_clearance foothold_miss hip_pos lin_vel_z orientation orientation_roll pos_acc
power powerchange smooth soft_tracking_ang_vel soft_tracking_lin_vel stand_still stumble termination torque_limits torques
tracking_ang_vel tracking_lin_vel tracking_optimal_footholds""".split()))
assert len(TERMS) == _ffi.REWARD_TERMS


def plane_rows(points_x, points_y) -> np.ndarray:
    """Rows 0, 1 of (A^T A)^-1 A^T, A = [x, y, 1] over the height grid (meshgrid indexing='ij', as _init_height_points): the
    constant part of get_plane_norm's batched least squares (legged_robot.py:1535-1557).  float64, from the fp32 coordinates."""
    x = np.asarray(points_x, dtype=np.float32).astype(np.float64)
    y = np.asarray(points_y, dtype=np.float32).astype(np.float64)
    gx, gy = np.meshgrid(x, y, indexing="ij")
    A = np.stack([gx.ravel(), gy.ravel(), np.ones(gx.size)], axis=1)
    return (np.linalg.inv(A.T @ A) @ A.T)[:2].copy()


@dataclass
class RewardConfig:
    """The active reward terms and their settings.  `scales`: {name: float32(scale * dt)} of the non-zero scales, in the
    reference's order (class_to_dict: alphabetical), termination included."""
    scales: dict
    dt: float = 0.02
    tracking_sigma: float = 0.25
    soft_dof_vel_limit: float = 1.0
    soft_torque_limit: float = 1.0
    base_height_target: float = 0.32
    max_contact_force: float = 100.0
    max_acc: float = 100.0
    only_positive_rewards: bool = False
    lin_vel_x_max: float = 0.75
    ang_vel_yaw_max: float = 0.5
    points_x: tuple = field(default_factory=lambda: tuple(MEASURED_POINTS_X))
    points_y: tuple = field(default_factory=lambda: tuple(MEASURED_POINTS_Y))

    @property
    def names(self) -> list:
        """Active terms in the reference's order: the keys of env.reward_scales / env.episode_sums."""
        return list(self.scales)

    @classmethod
    def from_cfg(cls, env_cfg) -> "RewardConfig":
        """From a LeggedRobotCfg-style config class or instance: cfg.rewards.scales read as class_to_dict reads it (dir() order,
        legged_gym/utils/helpers.py:11-26), zero scales dropped, the rest multiplied by dt = sim.dt * control.decimation in double
        precision and rounded to fp32 (legged_robot.py:929-938)."""
        r = env_cfg.rewards
        sc = r.scales
        dt = env_cfg.sim.dt * env_cfg.control.decimation
        scales = {}
        for k in dir(sc):
            if k.startswith("_"):
                continue
            v = getattr(sc, k)
            if v == 0:
                continue
            if k not in TERMS:
                raise ValueError(f"reward scale {k!r} has no _reward_{k} in LeggedRobotDTC")
            scales[k] = float(np.float32(v * dt))
        needs_acc = "foot_acc" in scales
        if needs_acc and not hasattr(r, "max_acc"):
            raise ValueError("foot_acc is on but cfg.rewards has no max_acc")
        ranges = env_cfg.commands.ranges
        return cls(scales=scales, dt=dt, tracking_sigma=r.tracking_sigma, soft_dof_vel_limit=r.soft_dof_vel_limit,
                   soft_torque_limit=r.soft_torque_limit, base_height_target=r.base_height_target,
                   max_contact_force=r.max_contact_force, max_acc=getattr(r, "max_acc", 0.0),
                   only_positive_rewards=bool(r.only_positive_rewards), lin_vel_x_max=ranges.lin_vel_x[1],
                   ang_vel_yaw_max=ranges.ang_vel_yaw[1], points_x=tuple(env_cfg.terrain.measured_points_x),
                   points_y=tuple(env_cfg.terrain.measured_points_y))


# inputs of dtc_env_rewards: name -> (shape given N, D, B, C; dtype); None entries are free
def _shapes(N, D, B, C, P):
    f, b = torch.float32, torch.bool
    return dict(root_states=((N, 13), f), base_lin_vel=((N, 3), f), base_ang_vel=((N, 3), f), projected_gravity=((N, 3), f),
                commands=((N, C), f), dof_pos=((N, D), f), default_dof_pos=((D,), f), dof_vel=((N, D), f), last_dof_vel=((N, D), f),
                torques=((N, D), f), actions=((N, D), f), last_actions=((N, D), f), last_actions_2=((N, D), f),
                contact_forces=((N, B, 3), f), foot_positions=((N, 4, 3), f), foot_velocities=((N, 4, 3), f),
                last_foot_velocities=((N, 4, 3), f), optimal_footholds_world=((N, 4, 3), f), contact_filt=((N, 4), b),
                measured_heights=((N, P), f), reset_buf=((N,), b), time_out_buf=((N,), b), robot_mass=((N,), f),
                terrain_levels=((N,), torch.int64), dof_pos_limits=((D, 2), f), dof_vel_limits=((D,), f), torque_limits=((D,), f),
                cmd_buffer=((10, N, C), f), lin_vel_buffer=((10, N, 2), f), ang_vel_buffer=((10, N, 1), f),
                measured_foot_clearance=((N, 4), f))


class EnvRewards:
    """`compute_reward` for `num_envs` envs as one launch.  Owns the reward state the reference keeps on the env -- feet_air_time
    [N,4], last_contacts [N,4] bool, the stumble history (uint8 [N,4], bit k = the mask of k steps ago), pitch_est [N] -- and the
    episode sums [n_active, N] (row i = reward_cfg.names[i]).  Index lists are the env's feet_indices / penalised_contact_indices
    (bodies of contact_forces) and hip_indices (columns of dof_pos)."""

    def __init__(self, num_envs: int, device, reward_cfg: RewardConfig, grid=None, *, feet_indices, penalised_contact_indices,
                 hip_indices, num_dof: int = 12):
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.N, self.device, self.cfg = int(num_envs), dev, reward_cfg
        # the height grid of the plane fit: grid= overrides the config's, on this instance only (the config is not changed)
        self.points_x, self.points_y = ((tuple(grid.points_x), tuple(grid.points_y)) if grid is not None else
                                        (tuple(reward_cfg.points_x), tuple(reward_cfg.points_y)))
        feet, pen, hips = ([int(i) for i in torch.as_tensor(t).reshape(-1).tolist()] for t in
                           (feet_indices, penalised_contact_indices, hip_indices))
        if len(feet) != 4 or len(pen) > 32 or len(hips) > 16 or not 1 <= num_dof <= 64:
            raise ValueError("EnvRewards: 4 feet, <= 32 penalised bodies, <= 16 hip dofs and 1..64 dofs are supported")
        self.num_dof, self.feet = num_dof, feet
        N, dev = self.N, self.device
        self.P = len(self.points_x) * len(self.points_y)
        self.plane = torch.from_numpy(plane_rows(self.points_x, self.points_y).astype(np.float32)).to(dev).contiguous()
        self.feet_air_time = torch.zeros(N, 4, device=dev)
        self.last_contacts = torch.zeros(N, 4, dtype=torch.bool, device=dev)
        self.stumble = torch.zeros(N, 4, dtype=torch.uint8, device=dev)
        self.pitch_est = torch.zeros(N, device=dev)
        self.episode_sums = torch.zeros(len(reward_cfg.names), N, device=dev)
        self.rew_buf = torch.zeros(N, device=dev)
        c = _ffi.DtcRewardCfg()
        for i in range(_ffi.REWARD_TERMS):
            c.row[i] = -1
        for r, name in enumerate(reward_cfg.names):
            i = TERMS.index(name)
            c.scale[i], c.row[i] = reward_cfg.scales[name], r
        for k in ("dt", "tracking_sigma", "soft_dof_vel_limit", "soft_torque_limit", "base_height_target", "max_contact_force",
                  "max_acc", "lin_vel_x_max", "ang_vel_yaw_max"):
            setattr(c, k, float(getattr(reward_cfg, k)))
        c.only_positive_rewards = int(reward_cfg.only_positive_rewards)
        c.num_dof, c.n_penalised, c.n_hip, c.num_points = num_dof, len(pen), len(hips), self.P
        for i, v in enumerate(feet):
            c.feet[i] = v
        for i, v in enumerate(pen):
            c.penalised[i] = v
        for i, v in enumerate(hips):
            c.hip[i] = v
        c.plane = self.plane.data_ptr() if dev.type == "cuda" else None
        self._c = c

    def set_command_ranges(self, lin_vel_x_max: float, ang_vel_yaw_max: float):
        """command_ranges["lin_vel_x"][1] / ["ang_vel_yaw"][1] (the command curriculum moves them)."""
        self._c.lin_vel_x_max, self._c.ang_vel_yaw_max = float(lin_vel_x_max), float(ang_vel_yaw_max)

    def __call__(self, *, last_contacts=None, height_samples=None, border_size=20.0, horizontal_scale=0.05, vertical_scale=0.005,
                 foot_clearance_out=None, per_term=False, out=None, **env):
        """Keyword tensors named as the env's attributes (see include/dtc_hip.h, DtcRewardStep), e.g. root_states=...,
        contact_forces=..., cmd_buffer=...; the inputs of inactive terms may be left out.  `last_contacts`: the env's tensor after
        _post_physics_step_callback (updated in place when feet_air_time is on; default: this object's).  The foot clearance comes
        from `measured_foot_clearance` [N,4] or, with `height_samples` (int16 table) + border / scales, is computed in the launch
        (and written to `foot_clearance_out` if given).  Returns rew_buf (`out` if given), and per_term [n_active, N] on request."""
        N, D = self.N, self.num_dof
        cmd = env.get("commands")
        cf = env.get("contact_forces")
        if cmd is None or cf is None or cmd.dim() != 2 or cf.dim() != 3:
            raise ValueError("EnvRewards: commands [N, C] and contact_forces [N, B, 3] are required")
        C, B = cmd.shape[1], cf.shape[1]
        shapes = _shapes(N, D, B, C, self.P)
        st = _ffi.DtcRewardStep()
        keep = []
        for k, t in env.items():
            if k not in shapes:
                raise ValueError(f"EnvRewards: unknown input {k!r}")
            if t is None:
                continue
            shape, dtype = shapes[k]
            if tuple(t.shape) != shape:
                raise ValueError(f"EnvRewards: {k} has shape {tuple(t.shape)}, expected {shape}")
            if t.device != self.device:
                raise ValueError(f"EnvRewards: {k} is on {t.device}, expected {self.device}")
            if dtype is torch.bool:
                t = t.contiguous()
                t = t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)
            elif t.dtype != dtype:
                t = t.to(dtype)
            t = t.contiguous()
            keep.append(t)
            setattr(st, "foot_clearance" if k == "measured_foot_clearance" else k, _ffi.ptr(t))
        lc = self.last_contacts if last_contacts is None else last_contacts
        if tuple(lc.shape) != (N, 4) or lc.dtype not in (torch.bool, torch.uint8) or not lc.is_contiguous():
            raise ValueError("EnvRewards: last_contacts must be a contiguous [N, 4] bool tensor (updated in place)")
        st.last_contacts = _ffi.ptr(lc)
        if height_samples is not None:
            if height_samples.dtype != torch.int16 or height_samples.dim() != 2:
                raise ValueError("EnvRewards: height_samples must be an int16 [rows, cols] table")
            hs = height_samples.contiguous()
            keep.append(hs)
            st.height_samples, st.rows, st.cols = _ffi.ptr(hs), hs.shape[0], hs.shape[1]
            st.border_size, st.horizontal_scale, st.vertical_scale = border_size, horizontal_scale, vertical_scale
            if env.get("measured_foot_clearance") is not None:
                raise ValueError("EnvRewards: pass either measured_foot_clearance or height_samples, not both")
            st.foot_clearance = None                       # with the table, foot_clearance is an output only
            if foot_clearance_out is not None:
                if tuple(foot_clearance_out.shape) != (N, 4) or foot_clearance_out.dtype != torch.float32 or \
                        not foot_clearance_out.is_contiguous():
                    raise ValueError("EnvRewards: foot_clearance_out must be a contiguous fp32 [N, 4] tensor")
                st.foot_clearance = _ffi.ptr(foot_clearance_out)
        rew = self.rew_buf if out is None else out
        if tuple(rew.shape) != (N,) or rew.dtype != torch.float32 or not rew.is_contiguous():
            raise ValueError("EnvRewards: out must be a contiguous fp32 [N] tensor")
        pt = torch.empty(len(self.cfg.names), N, device=self.device) if per_term else None
        st.feet_air_time, st.stumble, st.pitch_est = _ffi.ptr(self.feet_air_time), _ffi.ptr(self.stumble), _ffi.ptr(self.pitch_est)
        st.rew_buf, st.episode_sums, st.per_term = _ffi.ptr(rew), _ffi.ptr(self.episode_sums), _ffi.ptr(pt)
        st.num_bodies, st.num_commands = B, C
        _ffi.check(_ffi.lib().dtc_env_rewards(st, self._c, N, _ffi.stream()), "dtc_env_rewards")
        return (rew, pt) if per_term else rew


def patch_env(env, grid=None) -> EnvRewards:
    """Replace `env.compute_reward` by one `dtc_env_rewards` launch on the env's own buffers.  `env.episode_sums` becomes a dict
    of row views into the kernel's [n_active, N] tensor and `env.feet_air_time` / `env.pitch_est` the tensors the kernel updates
    in place, so `reset_idx` (which zeroes their rows) and its logging run unchanged; `env.reset_idx` additionally clears the
    kernel's stumble history of the reset envs, as the reference clears its 5-list (legged_robot.py:250-251)."""
    cfg = RewardConfig.from_cfg(env.cfg)
    R = EnvRewards(env.num_envs, env.device, cfg, grid, feet_indices=env.feet_indices,
                   penalised_contact_indices=env.penalised_contact_indices, hip_indices=env.hip_indices, num_dof=env.num_dof)
    old = getattr(env, "episode_sums", None) or {}
    for i, name in enumerate(cfg.names):
        if name in old:
            R.episode_sums[i].copy_(old[name])
    env.episode_sums = {name: R.episode_sums[i] for i, name in enumerate(cfg.names)}
    R.feet_air_time.copy_(env.feet_air_time)
    R.pitch_est.copy_(env.pitch_est)
    env.feet_air_time, env.pitch_est = R.feet_air_time, R.pitch_est
    hist = getattr(env, "stumb_buffer", None)
    if hist is not None:                  # the 5-list, oldest first -> bit k = the mask pushed k steps ago
        R.stumble.copy_(sum(hist[len(hist) - 1 - k].to(torch.uint8) << k for k in range(min(5, len(hist)))))
    names = ("root_states", "base_lin_vel", "base_ang_vel", "projected_gravity", "commands", "dof_pos", "dof_vel", "last_dof_vel",
             "torques", "actions", "last_actions", "last_actions_2", "contact_forces", "foot_positions", "foot_velocities",
             "last_foot_velocities", "optimal_footholds_world", "contact_filt", "measured_heights", "reset_buf", "time_out_buf",
             "robot_mass", "terrain_levels", "dof_pos_limits", "dof_vel_limits", "torque_limits", "cmd_buffer", "lin_vel_buffer",
             "ang_vel_buffer", "measured_foot_clearance")

    def compute_reward():
        """legged_robot.py:274-291 in one launch (reads the env's tensors as they are at this point of post_physics_step)."""
        R.set_command_ranges(env.command_ranges["lin_vel_x"][1], env.command_ranges["ang_vel_yaw"][1])
        inputs = {k: getattr(env, k, None) for k in names}
        inputs["default_dof_pos"] = env.default_dof_pos.reshape(-1)
        R(last_contacts=env.last_contacts, out=env.rew_buf, **inputs)
        return env.rew_buf

    orig_reset = env.reset_idx

    def reset_idx(env_ids):
        orig_reset(env_ids)
        if len(env_ids) > 0:
            R.stumble[env_ids] = 0

    env.compute_reward = compute_reward
    env.reset_idx = reset_idx
    env.env_rewards = R
    return R
