"""Host side of the on-device env reset (drop-in for LeggedRobot.reset_idx, legged_gym/envs/base/legged_robot.py:200-272, with
_update_terrain_curriculum, _reset_dofs, LeggedRobotDTC._reset_root_states, _resample_commands, _randomize_dof_props, the buffer
clears and the extras["episode"] means).

`ResetConfig.from_cfg(env_cfg)` reads the flags and ranges the reference reads from cfg.terrain / cfg.commands / cfg.domain_rand /
cfg.env / cfg.init_state; `EnvReset` runs the whole reset of the envs whose `reset_buf` is set as two launches (csrc/reset.hip,
`dtc_env_reset`) -- no `nonzero()`, no host read, the same launches whatever the mask; `patch_env(env)` replaces an env's
`reset_idx` by that call on the env's own tensors.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _ffi

# tensors whose row n is zeroed ([N, ...], legged_robot.py:233-247, :267-268) and the time-major ring buffers (:270-272)
ROW_ITEMS = ("last_actions", "last_actions_2", "last_dof_vel", "feet_air_time", "feet_contact_time", "last_scale_actions",
             "last_scale_actions2", "pitch_est", "base_ang_vel_last", "base_lin_vel_last", "episode_length_buf", "contact_filt",
             "last_contacts", "stumble")
ROW_LISTS = ("lag_buffer", "stumb_buffer")
TIME_ITEMS = ("lin_vel_buffer", "ang_vel_buffer", "cmd_buffer")
_RANGES = ("lin_vel_x", "lin_vel_y", "ang_vel_yaw", "heading")


@dataclass
class ResetConfig:
    """The flags, ranges and constants of reset_idx and its callees (names as in DtcResetCfg, include/dtc_hip.h)."""
    terrain_curriculum: bool = True
    init_done: bool = True
    custom_origins: bool = True
    heading_command: bool = True
    play_command: bool = False
    randomize_motor_strength: bool = True
    randomize_kp: bool = False
    randomize_kd: bool = False
    max_terrain_level: int = 6
    env_length: float = 8.0
    max_episode_length_s: float = 20.0
    origin_xy: tuple = (-0.5, 0.5)
    lin_vel_x: tuple = (-0.75, 0.75)
    lin_vel_y: tuple = (-0.75, 0.75)
    ang_vel_yaw: tuple = (-0.5, 0.5)
    heading: tuple = (-3.14, 3.14)
    motor_strength: tuple = (0.9, 1.1)
    kp_range: tuple = (0.95, 1.05)
    kd_range: tuple = (0.95, 1.05)
    base_init_state: tuple = field(default_factory=lambda: (0.0, 0.0, 0.4, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0))
    commands_curriculum: bool = False
    send_timeouts: bool = True

    @classmethod
    def from_cfg(cls, env_cfg, *, custom_origins=None, init_done: bool = True, origin_xy=(-0.5, 0.5)) -> "ResetConfig":
        """From a LeggedRobotCfg-style config class or instance.  Terrain curriculum and custom origins exist only on a heightfield /
        trimesh terrain (legged_robot.py:1205-1219); `origin_xy` is the xy spread of LeggedRobotDTC._reset_root_states
        (legged_robot_dtc.py:303; LeggedRobot uses (-1, 1), legged_robot.py:659)."""
        t, c, d, e, i = env_cfg.terrain, env_cfg.commands, env_cfg.domain_rand, env_cfg.env, env_cfg.init_state
        meshed = t.mesh_type in ("heightfield", "trimesh")
        r = c.ranges
        return cls(terrain_curriculum=bool(t.curriculum) and meshed, init_done=init_done,
                   custom_origins=meshed if custom_origins is None else bool(custom_origins), heading_command=bool(c.heading_command),
                   play_command=bool(getattr(e, "play_commond", False)), randomize_motor_strength=bool(d.randomize_motor_strength),
                   randomize_kp=bool(d.randomize_Kp_factor), randomize_kd=bool(d.randomize_Kd_factor), max_terrain_level=int(t.num_rows),
                   env_length=float(t.terrain_length), max_episode_length_s=float(e.episode_length_s), origin_xy=tuple(origin_xy),
                   lin_vel_x=tuple(r.lin_vel_x), lin_vel_y=tuple(r.lin_vel_y), ang_vel_yaw=tuple(r.ang_vel_yaw), heading=tuple(r.heading),
                   motor_strength=tuple(d.motor_strength), kp_range=tuple(d.kp_range), kd_range=tuple(d.kd_range),
                   base_init_state=tuple(float(v) for v in list(i.pos) + list(i.rot) + list(i.lin_vel) + list(i.ang_vel)),
                   commands_curriculum=bool(c.curriculum), send_timeouts=bool(getattr(e, "send_timeouts", True)))


# tensor arguments of dtc_env_reset: name -> (shape given N, D, B, C, P, n_sums; dtype; written in place)
def _shapes(N, D, B, C, P, R):
    f, i64 = torch.float32, torch.int64
    return dict(reset_buf=((N,), torch.bool, False), terrain_types=((N,), i64, False), default_dof_pos=((D,), f, False),
                terrain_levels=((N,), i64, True), env_origins=((N, 3), f, True), root_states=((N, 13), f, True),
                commands=((N, C), f, True), forces=((N, B, 3), f, True),
                motor_strengths=((N, D), f, True), Kp_factors=((N, D), f, True), Kd_factors=((N, D), f, True),
                height_noise_offset=((N, P), f, True), episode_sums=((R, N), f, True), u=((N, D + _ffi.RESET_FIXED_DRAWS), f, False),
                level_draw=((N,), i64, False))


class EnvReset:
    """`reset_idx` for `num_envs` envs, driven by `reset_buf`.  Owns the outputs -- env_ids [N] int32 (ascending, entries [0, count)),
    count [1] int32, episode_means [n_sums] (row i = the i-th episode sum / max_episode_length_s), terrain_level_mean [1] -- and the
    workspace.  With `u` / `level_draw` left out the kernel draws its own (Philox, keyed by `seed` and a call counter: torch's
    distribution, not torch's bits)."""

    def __init__(self, num_envs: int, device, config: ResetConfig, *, n_sums: int, num_dof: int = 12, seed: int = 0):
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if not 1 <= num_dof <= 64 or not 0 <= n_sums <= _ffi.RESET_MAX_SUMS or num_envs < 1:
            raise ValueError(f"EnvReset: 1..64 dofs, at most {_ffi.RESET_MAX_SUMS} episode sums and >= 1 env are supported")
        self.N, self.device, self.cfg, self.num_dof, self.n_sums = int(num_envs), dev, config, int(num_dof), int(n_sums)
        self.seed, self.counter = int(seed), 0
        self.env_ids = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.episode_means = torch.zeros(max(self.n_sums, 1), device=dev)[:self.n_sums]
        self.terrain_level_mean = torch.zeros(1, device=dev)
        ws = _ffi.lib().dtc_env_reset_workspace(self.N, self.n_sums) if dev.type == "cuda" else 8
        self.workspace = torch.zeros(ws // 8, dtype=torch.float64, device=dev)

    def _cfg_struct(self, height_noise, B, C, P, rows, cols, command_ranges, init_done) -> "_ffi.DtcResetCfg":
        k, c = self.cfg, _ffi.DtcResetCfg()
        c.num_dof, c.num_bodies, c.num_commands, c.num_points = self.num_dof, B, C, P
        c.terrain_curriculum, c.init_done, c.custom_origins = int(k.terrain_curriculum), int(init_done), int(k.custom_origins)
        c.heading_command, c.play_command = int(k.heading_command), int(k.play_command)
        c.randomize_motor_strength, c.randomize_kp, c.randomize_kd = int(k.randomize_motor_strength), int(k.randomize_kp), int(k.randomize_kd)
        c.max_terrain_level, c.terrain_rows, c.terrain_cols = int(k.max_terrain_level), rows, cols
        c.move_up_distance = float(np.float32(k.env_length * 0.6))
        c.max_episode_length_s = float(k.max_episode_length_s)
        for i, v in enumerate(k.base_init_state):
            c.base_init_state[i] = v
        c.height_noise = float(np.float32(height_noise))
        for name in ("origin_xy",) + _RANGES + ("motor_strength", "kp_range", "kd_range"):
            lo, hi = command_ranges[name] if name in command_ranges else getattr(k, name)
            getattr(c, name)[0], getattr(c, name)[1] = float(lo), float(hi)
        c.seed, c.counter = self.seed, self.counter
        return c

    def _rows(self, what, t, lead):
        """(pointer, bytes per env row) of a tensor cleared in place: dense, on the device, env axis at position `lead`."""
        if not isinstance(t, torch.Tensor) or t.dim() <= lead or t.shape[lead] != self.N:
            raise ValueError(f"EnvReset: {what} must be a tensor with {self.N} envs on axis {lead}")
        if t.device != self.device:
            raise ValueError(f"EnvReset: {what} is on {t.device}, expected {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"EnvReset: {what} must be contiguous (it is cleared in place)")
        rb = t.element_size()
        for s in t.shape[lead + 1:]:
            rb *= s
        if rb <= 0 or rb > (1 << 20):
            raise ValueError(f"EnvReset: {what} has {rb} bytes per env row")
        return _ffi.ptr(t), rb

    def _strided(self, name, t):
        """dof_pos / dof_vel: fp32 [N, D] on the device, dense or a strided view such as dof_state.view(N, D, 2)[..., 0]
        (legged_robot.py:774-775); written in place through its strides."""
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (self.N, self.num_dof):
            raise ValueError(f"EnvReset: {name} has shape {tuple(getattr(t, 'shape', ()))}, expected {(self.N, self.num_dof)}")
        if t.device != self.device:
            raise ValueError(f"EnvReset: {name} is on {t.device}, expected {self.device}")
        if t.dtype != torch.float32:
            raise ValueError(f"EnvReset: {name} is {t.dtype}, expected {torch.float32}")
        rs, es = t.stride()
        if es < 1 or (self.N > 1 and rs < (self.num_dof - 1) * es + 1):
            raise ValueError(f"EnvReset: {name} has strides {(rs, es)}: needs a positive element stride and a row stride beyond one row's span")
        return _ffi.ptr(t), max(rs, (self.num_dof - 1) * es + 1), es

    def __call__(self, *, height_noise=None, command_ranges=None, init_done=None, extra_rows=(), extra_time_rows=(), **env):
        """Keyword tensors named as the env's attributes (see include/dtc_hip.h, DtcResetStep): reset_buf, root_states, env_origins,
        commands, dof_pos, dof_vel, default_dof_pos, terrain_levels / terrain_types / terrain_origins (terrain curriculum), forces,
        motor_strengths / Kp_factors / Kd_factors (the ones whose flag is on), height_noise_offset, episode_sums [n_sums, N]; the
        tensors to clear -- any of ROW_ITEMS, the lists lag_buffer / stumb_buffer (or `stumble`, the bits of EnvRewards), any of
        TIME_ITEMS, plus `extra_rows` / `extra_time_rows`; optionally the draws u [N, D + 14] and level_draw [N].  Everything is
        updated in place, so dtype, device and contiguity must be exact; dof_pos / dof_vel alone may be strided views (the
        reference's are the two halves of dof_state [N, D, 2]).  `height_noise`: the np.random.normal(0, 0.02) of
        legged_robot.py:230 (drawn here when None); `command_ranges` / `init_done`: the env's as they are now, for this call only
        (default: the config's; the config object is not changed).
        Returns (env_ids, count, episode_means, terrain_level_mean), device tensors; nothing is read back."""
        N, D, k = self.N, self.num_dof, self.cfg
        for name in ("reset_buf", "root_states", "env_origins", "commands", "dof_pos", "dof_vel", "default_dof_pos"):
            if env.get(name) is None:
                raise ValueError(f"EnvReset: {name} is required")
        cmd = env["commands"]
        if cmd.dim() != 2:
            raise ValueError("EnvReset: commands must be [N, C]")
        C = cmd.shape[1]
        if C < (4 if k.heading_command else 3):
            raise ValueError(f"EnvReset: commands has {C} columns")
        forces, hno = env.get("forces"), env.get("height_noise_offset")
        B = forces.shape[1] if forces is not None and forces.dim() == 3 else 0
        P = hno.shape[1] if hno is not None and hno.dim() == 2 else 0
        shapes = _shapes(N, D, B, C, P, self.n_sums)
        st = _ffi.DtcResetStep()
        keep = []
        rows, time_rows = [], []
        for name, t in env.items():
            if t is None:
                continue
            if name in ROW_ITEMS:
                rows.append(self._rows(name, t, 0))
            elif name in ROW_LISTS:
                rows.extend(self._rows(f"{name}[{j}]", b, 0) for j, b in enumerate(t))
            elif name in TIME_ITEMS:
                time_rows.append(self._rows(name, t, 1) + (t.shape[0],))
            elif name == "terrain_origins":
                if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                    raise ValueError("EnvReset: terrain_origins must be a contiguous fp32 [rows, cols, 3] tensor on the device")
                st.terrain_origins = _ffi.ptr(t)
            elif name in ("dof_pos", "dof_vel"):
                ptr, rs, es = self._strided(name, t)
                setattr(st, name, ptr)
                setattr(st, name + "_row_stride", rs)
                setattr(st, name + "_elem_stride", es)
            elif name in shapes:
                shape, dtype, inplace = shapes[name]
                if tuple(t.shape) != shape:
                    raise ValueError(f"EnvReset: {name} has shape {tuple(t.shape)}, expected {shape}")
                if t.device != self.device:
                    raise ValueError(f"EnvReset: {name} is on {t.device}, expected {self.device}")
                if t.dtype != dtype and not (dtype is torch.bool and t.dtype == torch.uint8):
                    raise ValueError(f"EnvReset: {name} is {t.dtype}, expected {dtype}")
                if not t.is_contiguous():
                    raise ValueError(f"EnvReset: {name} must be contiguous" + (" (it is updated in place)" if inplace else ""))
                setattr(st, name, _ffi.ptr(t))
            else:
                raise ValueError(f"EnvReset: unknown input {name!r}")
            keep.append(t)
        rows.extend(self._rows(f"extra_rows[{j}]", t, 0) for j, t in enumerate(extra_rows))
        time_rows.extend(self._rows(f"extra_time_rows[{j}]", t, 1) + (t.shape[0],) for j, t in enumerate(extra_time_rows))
        if len(rows) > _ffi.RESET_MAX_ROWS or len(time_rows) > _ffi.RESET_MAX_TIME_ROWS:
            raise ValueError(f"EnvReset: {len(rows)} row items / {len(time_rows)} time-major items; at most {_ffi.RESET_MAX_ROWS} / "
                             f"{_ffi.RESET_MAX_TIME_ROWS} fit one call")
        if self.n_sums and env.get("episode_sums") is None:
            raise ValueError("EnvReset: episode_sums [n_sums, N] is required")
        if k.terrain_curriculum and (env.get("terrain_levels") is None or
                                     ((k.init_done if init_done is None else init_done) and (env.get("terrain_types") is None or env.get("terrain_origins") is None))):
            raise ValueError("EnvReset: the terrain curriculum needs terrain_levels, terrain_types and terrain_origins")
        for flag, name in ((k.randomize_motor_strength, "motor_strengths"), (k.randomize_kp, "Kp_factors"), (k.randomize_kd, "Kd_factors")):
            if flag and env.get(name) is None:
                raise ValueError(f"EnvReset: {name} is required (its randomisation is on)")
        for j, (p, rb) in enumerate(rows):
            st.rows[j].ptr, st.rows[j].row_bytes = p, rb
        for j, (p, rb, T) in enumerate(time_rows):
            st.time_rows[j].ptr, st.time_rows[j].row_bytes, st.time_rows[j].T = p, rb, T
        st.n_sums, st.n_rows, st.n_time_rows = self.n_sums, len(rows), len(time_rows)
        st.env_ids, st.count, st.workspace = _ffi.ptr(self.env_ids), _ffi.ptr(self.count), _ffi.ptr(self.workspace)
        st.episode_means = _ffi.ptr(self.episode_means) if self.n_sums else None
        st.terrain_level_mean = _ffi.ptr(self.terrain_level_mean)
        to = env.get("terrain_origins")
        trows, tcols = (to.shape[0], to.shape[1]) if to is not None else (0, 0)
        if height_noise is None:
            height_noise = np.random.normal(0, 0.02)
        ranges = {n: command_ranges[n] for n in _RANGES if n in command_ranges} if command_ranges is not None else {}
        c = self._cfg_struct(height_noise, B, C, P, trows, tcols, ranges, k.init_done if init_done is None else init_done)
        self.counter += 1
        _ffi.check(_ffi.lib().dtc_env_reset(st, c, N, _ffi.stream()), "dtc_env_reset")
        return self.env_ids, self.count, self.episode_means, self.terrain_level_mean


_ENV_TENSORS = ("reset_buf", "root_states", "env_origins", "commands", "dof_pos", "dof_vel", "terrain_levels", "terrain_types",
                "terrain_origins", "forces", "motor_strengths", "Kp_factors", "Kd_factors", "height_noise_offset")


def patch_env(env, rewards=None, *, seed: int = 0, hand_over=None) -> EnvReset:
    """Replace `env.reset_idx` by one `dtc_env_reset` call on the env's own tensors.  The `env_ids` argument of the new `reset_idx`
    is IGNORED: the envs whose `env.reset_buf` is set are reset (what post_physics_step passes, legged_robot_dtc.py:205-206) -- so
    the caller drops its `reset_buf.nonzero()` as well.  Apply `rewards.patch_env(env)` FIRST when both are used (pass its result as
    `rewards`, or leave it to `env.env_rewards`): the episode sums are then the kernel's [n_active, N] tensor and the stumble history
    its bit array; otherwise `env.episode_sums` is rebound to row views of one [n_sums, N] tensor and the env's `stumb_buffer` list
    is cleared.  `env.extras["episode"]` becomes a dict of views into the device means (no `.item()`); after a call in which no env
    reset, the views still hold the last means (the reference leaves the dict alone; before the first reset they read 0).
    `env.command_ranges` is re-read on every call, and `update_command_curriculum` (legged_robot.py:717-726), a host decision taken
    once per max_episode_length steps, runs after the launch on the same means and only if an env reset (count and mean come in one
    host read).  The reference widens the range BEFORE `_resample_commands`, so it applies to the same reset; here it applies from
    the next reset on.  The dof tensors may be the env's strided views of `dof_state`: the kernel writes through their strides.
    `hand_over(env_ids, count)`, if given, is called after the launch: the place for the simulator's indexed setters."""
    cfg = ResetConfig.from_cfg(env.cfg, custom_origins=getattr(env, "custom_origins", None), init_done=bool(getattr(env, "init_done", True)))
    rewards = rewards if rewards is not None else getattr(env, "env_rewards", None)
    if rewards is not None:
        names, sums = list(rewards.cfg.names), rewards.episode_sums
    else:
        names = list(env.episode_sums)
        sums = torch.zeros(len(names), env.num_envs, device=env.device)
        for i, n in enumerate(names):
            sums[i].copy_(env.episode_sums[n])
        env.episode_sums = {n: sums[i] for i, n in enumerate(names)}
    E = EnvReset(env.num_envs, env.device, cfg, n_sums=len(names), num_dof=env.num_dof, seed=seed)
    episode = {"rew_" + n: E.episode_means[i] for i, n in enumerate(names)}
    if cfg.terrain_curriculum:
        episode["terrain_level"] = E.terrain_level_mean[0]

    def reset_idx(env_ids=None, *, u=None, level_draw=None, height_noise=None):
        """legged_robot.py:200-272 for the envs with reset_buf set (`env_ids` is ignored).  u / level_draw / height_noise: the
        draws, for parity runs (default: drawn by the kernel / here)."""
        inputs = {k: getattr(env, k, None) for k in _ENV_TENSORS + ROW_ITEMS[:-1] + TIME_ITEMS}
        inputs["default_dof_pos"] = env.default_dof_pos.reshape(-1)
        inputs["lag_buffer"] = getattr(env, "lag_buffer", None)
        if rewards is not None:
            inputs["stumble"] = rewards.stumble
        else:
            inputs["stumb_buffer"] = getattr(env, "stumb_buffer", None)
        E(episode_sums=sums, command_ranges=env.command_ranges, init_done=bool(getattr(env, "init_done", True)), u=u,
          level_draw=level_draw, height_noise=height_noise, **inputs)
        if hasattr(env, "rb_positions"):
            env.force_positions = env.rb_positions.clone()                         # :593
        env.extras["episode"] = dict(episode)
        if cfg.commands_curriculum:
            env.extras["episode"]["max_command_x"] = env.command_ranges["lin_vel_x"][1]
            if env.common_step_counter % env.max_episode_length == 0 and "tracking_lin_vel" in names:
                # update_command_curriculum (:717-726): mean(episode_sums) / max_episode_length > 0.8 * scale.  One host read per
                # max_episode_length steps, count and mean together; nothing happens when no env reset (:210-211)
                i = names.index("tracking_lin_vel")
                count, mean = torch.cat((E.count.float(), E.episode_means[i:i + 1])).tolist()
                if count > 0 and mean * cfg.max_episode_length_s / env.max_episode_length > 0.8 * env.reward_scales["tracking_lin_vel"]:
                    r, m = env.command_ranges["lin_vel_x"], env.cfg.commands.max_curriculum
                    r[0], r[1] = float(np.clip(r[0] - 0.5, -m, 0.0)), float(np.clip(r[1] + 0.5, 0.0, m))
        if cfg.send_timeouts and hasattr(env, "time_out_buf"):
            env.extras["time_outs"] = env.time_out_buf
        if hand_over is not None:
            hand_over(E.env_ids, E.count)

    env.reset_idx = reset_idx
    env.env_reset = E
    return E
