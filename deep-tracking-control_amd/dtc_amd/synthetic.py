"""Deterministic synthetic inputs for the hot path.

Isaac Gym physics is out of scope, so both parity tests and `bench.py` run on synthetic /
pre-recorded rollout buffers.  Everything here is a pure function of (shape, seed) on a
`torch.Generator`, so the CPU oracle and the HIP path can be fed identical numbers.
"""
from __future__ import annotations

import math

import torch

NUM_OBS, NUM_PRIV, NUM_HIST, NUM_ACT, N_POINTS = 53, 1389, 265, 12, 693

# Lite3DTCCfg.terrain (legged_gym/envs/lite3/lite3_dtc_config.py:32-36)
MEASURED_POINTS_X = [round(-0.8 + 0.05 * i, 2) for i in range(33)]
MEASURED_POINTS_Y = [round(-0.5 + 0.05 * i, 2) for i in range(21)]


def _gen(seed: int, device="cpu") -> torch.Generator:
    return torch.Generator(device=device).manual_seed(seed)


def rollout(num_envs: int, num_steps: int = 24, seed: int = 4, device="cpu") -> dict:
    """A filled `[T, N, d]` rollout (field names = RolloutStorage attributes,
    rsl_rl/rsl_rl/storage/rollout_storage.py:57-97) + `last_values`."""
    g = _gen(seed, device)
    T, N = num_steps, num_envs
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    obs_seq = rn(T + 1, N, NUM_OBS)
    out = dict(
        observations=obs_seq[:T].contiguous(),
        next_observations=obs_seq[1:].contiguous(),
        privileged_observations=rn(T, N, NUM_PRIV).clamp_(-5.0, 5.0),
        observation_histories=rn(T, N, NUM_HIST),
        base_vel=rn(T, N, 3),
        rewards=0.1 * rn(T, N, 1),
        dones=(torch.rand(T, N, 1, generator=g, device=device) < 0.02).to(torch.uint8),
        mu=0.01 * rn(T, N, NUM_ACT),
        sigma=torch.ones(T, N, NUM_ACT, device=device),
        values=0.01 * rn(T, N, 1),
    )
    out["actions"] = out["mu"] + out["sigma"] * rn(T, N, NUM_ACT)
    a, m, s = out["actions"], out["mu"], out["sigma"]
    logp = -((a - m) ** 2) / (2 * s * s) - s.log() - math.log(math.sqrt(2 * math.pi))
    out["actions_log_prob"] = logp.sum(-1, keepdim=True)
    out["last_values"] = torch.zeros(N, 1, device=device)
    return out


def update_noise(num_envs: int, num_steps: int = 24, num_mini_batches: int = 4, num_epochs: int = 5,
                 seed: int = 123, device="cpu"):
    """The random draws one `PPO.update` consumes: the mini-batch permutation (one per update,
    rollout_storage.py:165) and the two reparameterisation noises per mini-batch
    (actor_critic_decoder.py:283)."""
    g = _gen(seed, device)
    mb = (num_envs * num_steps) // num_mini_batches
    steps = num_mini_batches * num_epochs
    perm = torch.randperm(num_mini_batches * mb, generator=g, device=device)
    eps1 = torch.randn(steps, mb, 16, generator=g, device=device)
    eps2 = torch.randn(steps, mb, 16, generator=g, device=device)
    return perm, eps1, eps2


def height_points() -> torch.Tensor:
    """[693, 3] base-frame sample grid, flat index i = ix*21 + iy
    (legged_gym/envs/base/legged_robot.py:1263-1277)."""
    x = torch.tensor(MEASURED_POINTS_X)
    y = torch.tensor(MEASURED_POINTS_Y)
    gx, gy = torch.meshgrid(x, y, indexing="ij")
    pts = torch.zeros(N_POINTS, 3)
    pts[:, 0] = gx.flatten()
    pts[:, 1] = gy.flatten()
    return pts


def scorer_inputs(num_envs: int, seed: int = 7, device="cpu") -> dict:
    """Mock env state for the foothold planner: root_states [N,13] (pos, quat
    xyzw, lin vel, ang vel), thigh positions [N,4,3] (FL,FR,HL,HR), commands [N,4],
    measured_heights [N,693] (stepping-stone-like, quantised to vertical_scale = 0.005)."""
    g = _gen(seed, device)
    N = num_envs
    ru = lambda *s: torch.rand(*s, generator=g, device=device)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    root = torch.zeros(N, 13, device=device)
    root[:, 0] = 20.0 + 40.0 * ru(N)
    root[:, 1] = 20.0 + 10.0 * ru(N)
    root[:, 2] = 0.3 + 0.3 * ru(N)
    yaw = (2 * ru(N) - 1) * math.pi
    q = torch.stack([0.05 * rn(N), 0.05 * rn(N), torch.sin(yaw / 2), torch.cos(yaw / 2)], dim=1)
    root[:, 3:7] = q / q.norm(dim=1, keepdim=True)
    root[:, 7:13] = 0.5 * rn(N, 6)
    commands = 0.5 * rn(N, 4)
    off = torch.tensor([[0.17, 0.1, 0.0], [0.17, -0.1, 0.0], [-0.17, 0.1, 0.0], [-0.17, -0.1, 0.0]],
                       device=device)
    c, s = torch.cos(yaw), torch.sin(yaw)
    thigh = torch.empty(N, 4, 3, device=device)
    thigh[:, :, 0] = root[:, None, 0] + c[:, None] * off[None, :, 0] - s[:, None] * off[None, :, 1]
    thigh[:, :, 1] = root[:, None, 1] + s[:, None] * off[None, :, 0] + c[:, None] * off[None, :, 1]
    thigh[:, :, 2] = root[:, None, 2]
    flat = ru(N, N_POINTS) < 0.7
    steps = torch.randint(-400, 20, (N, N_POINTS), generator=g, device=device).float() * 0.005
    heights = (root[:, 2:3] - 0.32) + torch.where(flat, torch.zeros_like(steps), steps)
    return dict(root_states=root, thigh_pos=thigh.contiguous(), commands=commands,
                measured_heights=heights.contiguous())


def env_state(num_envs: int, seed: int = 13, device="cpu") -> dict:
    """Mock env state consumed by compute_observations / check_termination (legged_robot_dtc.py:229-288):
    the scorer inputs of `scorer_inputs(seed)` plus joint state, actions, contacts, forces and the uniform draws
    the reference takes from torch.rand_like (inputs here, so that both sides use the same numbers)."""
    d = scorer_inputs(num_envs, seed=seed, device=device)
    g = _gen(seed + 1000, device)
    N = num_envs
    ru = lambda *s: torch.rand(*s, generator=g, device=device)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    grav = torch.stack([0.1 * rn(N), 0.1 * rn(N), -1.0 + 0.05 * rn(N).abs()], dim=1)
    grav[: N // 32, 2] = 0.3                                   # fallen over -> terminated by the gravity test
    d.update(base_ang_vel=0.5 * rn(N, 3), projected_gravity=grav, dof_pos=0.3 * rn(N, 12),
             default_dof_pos=torch.tensor([0.0, -0.8, 1.6] * 4, device=device), dof_vel=2.0 * rn(N, 12),
             actions=rn(N, 12), foothold_obs=0.5 * rn(N, 8), forces=10.0 * rn(N, 17, 3),
             height_noise_offset=0.02 * rn(N, 1).expand(N, N_POINTS).contiguous(),
             u_obs=ru(N, 53), u_heights=ru(N, N_POINTS),
             noise_scale_vec=torch.cat([0.05 * ru(45), torch.zeros(8, device=device)]),
             contact_forces=40.0 * rn(N, 17, 3), episode_length_buf=torch.randint(0, 1100, (N,), generator=g, device=device),
             termination_contact_indices=torch.tensor([0, 1, 5, 9, 13], device=device))
    # a few robots sunk into the terrain -> the base-height termination test fires
    d["root_states"][N // 32: N // 16, 2] -= 0.25
    return d


# body layout of the reward inputs: base, then (hip, thigh, shank, foot) per leg -- 17 bodies as the Lite3 URDF
REWARD_FEET = (4, 8, 12, 16)
REWARD_PENALISED = (0, 2, 3, 6, 7, 10, 11, 14, 15)
REWARD_HIPS = (0, 3, 6, 9)
# command-range maxima the margins below are kept for (Lite3DTCCfg: 0.75 / 0.5, LeggedRobotCfg and X30DTCCfg: 1.0 / 1.0)
REWARD_RANGE_MAXIMA = ((0.75, 0.5), (1.0, 1.0))


def _away(x, th, rel=2e-3):
    """x moved at least rel * |th| away from the threshold th (keeping its side; exact hits go up)."""
    gap = rel * abs(th) if th != 0 else rel
    lo, hi = th - gap, th + gap
    return torch.where((x > lo) & (x < hi), torch.where(x < th, torch.full_like(x, lo), torch.full_like(x, hi)), x)


def reward_state(num_envs: int, seed: int = 31, device="cpu") -> dict:
    """Mock env state for `compute_reward` (legged_robot.py:274-291, the 34 terms of LeggedRobotDTC): the inputs, ring
    buffers and reward state of `dtc_amd.rewards.EnvRewards`, keyed by the env's attribute names (bool tensors as the env
    holds them).  Every thresholded quantity is kept >= 1e-3 (relative) away from its threshold -- contact fz > 1, the
    collision norm > 0.1, the 3 / 4 / 5 |fz| stumble tests, the clearance cuts 0.03 / 0.18, |g_x| > 0.6, the command norm
    0.1, the 0.15 yaw tolerance (for the ranges of REWARD_RANGE_MAXIMA) and the +-0.1 pitch / roll clip of the plane fit --
    except the rows of `threshold_rows`, which sit exactly on a threshold on purpose."""
    g = _gen(seed, device)
    N, D = num_envs, 12
    ru = lambda *s: torch.rand(*s, generator=g, device=device)          # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=g, device=device)         # noqa: E731
    root = torch.zeros(N, 13, device=device)
    root[:, 0] = 21.0 + 30.0 * ru(N)
    root[:, 1] = 21.0 + 15.0 * ru(N)
    root[:, 2] = 0.25 + 0.15 * ru(N)
    root[:, 6] = 1.0
    root[:, 7:13] = 0.5 * rn(N, 6)
    cmd = 0.6 * rn(N, 4)
    still = ru(N) < 0.15                                                    # standing commands: norm well below 0.1
    cmd[still, :2] *= 0.05
    nrm = cmd[:, :2].norm(dim=1, keepdim=True)
    cmd[:, :2] *= _away(nrm, 0.1) / nrm.clamp(min=1e-12)
    grav = torch.stack([0.35 * rn(N), 0.2 * rn(N), -0.9 + 0.05 * ru(N)], dim=1)
    grav[:, 0] = torch.sign(grav[:, 0]) * _away(grav[:, 0].abs(), 0.6)
    default = torch.tensor([0.0, -0.8, 1.6] * 4, device=device)
    ang_vel = 0.5 * rn(N, 3)
    ang_vel[:, 2] = cmd[:, 2] + 0.12 * rn(N)                             # the yaw rate enters the ring buffer (0.15 tolerance)
    for _, ymax in REWARD_RANGE_MAXIMA:
        e = (cmd[:, 2] - ang_vel[:, 2]) / ymax
        ang_vel[:, 2] = cmd[:, 2] - ymax * torch.sign(e) * _away(e.abs(), 0.15)
    d = dict(root_states=root, base_lin_vel=0.5 * rn(N, 3), base_ang_vel=ang_vel, projected_gravity=grav, commands=cmd,
             dof_pos=default + 0.3 * rn(N, D), default_dof_pos=default.clone(), dof_vel=2.0 * rn(N, D), last_dof_vel=2.0 * rn(N, D),
             torques=6.0 * rn(N, D), actions=rn(N, D), last_actions=rn(N, D), last_actions_2=rn(N, D))
    # contact forces [N, 17, 3]: feet in / out of contact, with horizontal / vertical ratios spread over the stumble tests
    cf = 5.0 * rn(N, 17, 3) * (ru(N, 17, 1) < 0.5)
    fz = torch.where(ru(N, 4) < 0.6, 5.0 + 60.0 * ru(N, 4), 0.9 * ru(N, 4))
    fz = _away(fz, 1.0)
    ratio = 7.0 * ru(N, 4)
    for th in (3.0, 4.0, 5.0):
        ratio = _away(ratio, th)
    ang = 2 * math.pi * ru(N, 4)
    cf[:, REWARD_FEET, 0] = ratio * fz * torch.cos(ang)
    cf[:, REWARD_FEET, 1] = ratio * fz * torch.sin(ang)
    cf[:, REWARD_FEET, 2] = fz * torch.where(ru(N, 4) < 0.9, 1.0, -1.0)
    bn = cf.norm(dim=-1, keepdim=True)
    cf = torch.where(bn > 0, cf * _away(bn, 0.1) / bn.clamp(min=1e-12), cf)
    d["contact_forces"] = cf
    fp = torch.empty(N, 4, 3, device=device)
    fp[:, :, :2] = root[:, None, :2] + 0.25 * rn(N, 4, 2)
    fp[:, :, 2] = _away(0.2 * ru(N, 4) - 0.03, 0.0, rel=1e-3)
    fv = 1.5 * rn(N, 4, 3)
    d.update(foot_positions=fp, foot_velocities=fv, last_foot_velocities=fv + 2.0 * rn(N, 4, 3),
             optimal_footholds_world=fp + 0.15 * rn(N, 4, 3), contact_filt=ru(N, 4) < 0.6,
             measured_foot_clearance=_away(_away(0.45 * ru(N, 4) - 0.05, 0.03), 0.18))
    # measured heights: a tilted plane + roughness, its fitted pitch / roll kept off the +-0.1 clip
    pts = height_points().to(device)
    slope = 0.25 * rn(N, 2)
    h = (root[:, 2:3] - 0.3) + slope[:, :1] * pts[None, :, 0] + slope[:, 1:] * pts[None, :, 1] + 0.01 * rn(N, N_POINTS)
    h64 = h.double()
    x64, y64 = pts[:, 0].double(), pts[:, 1].double()
    A = torch.stack([x64, y64, torch.ones_like(x64)], dim=1)
    M = torch.linalg.inv(A.t() @ A) @ A.t()
    for _ in range(3):
        ax, by = h64 @ M[0], h64 @ M[1]
        n = torch.sqrt(ax * ax + by * by + 1.0)
        pitch, roll = torch.atan(-ax / n), torch.atan(by / n)
        # target angles off the clip; the shift of the slope moves the fitted plane exactly (M @ x = e0, M @ y = e1)
        tp = torch.sign(pitch) * _away(pitch.abs(), 0.1, rel=4e-3)
        tr = torch.sign(roll) * _away(roll.abs(), 0.1, rel=4e-3)
        u, w = torch.tan(tp), torch.tan(tr)                                 # tan(pitch) = -ax / n, tan(roll) = by / n
        n2 = 1.0 / torch.sqrt(1.0 - u * u - w * w)
        ax2, by2 = -u * n2, w * n2
        h64 = h64 + (ax2 - ax)[:, None] * x64[None] + (by2 - by)[:, None] * y64[None]
    d["measured_heights"] = h64.float()
    # ring buffers [10, N, .]: the yaw-rate errors of the last 4 rows kept off the 0.15 tolerance for every range in use
    cmd_buf = 0.6 * rn(10, N, 4)
    ang_buf = cmd_buf[:, :, 2:3] + 0.12 * rn(10, N, 1)
    for _, ymax in REWARD_RANGE_MAXIMA:
        e = (cmd_buf[:, :, 2:3] - ang_buf) / ymax
        ang_buf = cmd_buf[:, :, 2:3] - ymax * torch.sign(e) * _away(e.abs(), 0.15)
    d.update(cmd_buffer=cmd_buf, lin_vel_buffer=cmd_buf[:, :, :2] + 0.2 * rn(10, N, 2), ang_vel_buffer=ang_buf,
             reset_buf=ru(N) < 0.1, time_out_buf=ru(N) < 0.03, robot_mass=9.0 + 3.0 * ru(N),
             terrain_levels=torch.randint(0, 10, (N,), generator=g, device=device))
    d["dof_pos_limits"] = torch.stack([default - 0.45, default + 0.45], dim=1)
    d["dof_vel_limits"] = torch.full((D,), 2.5, device=device)
    d["torque_limits"] = torch.full((D,), 7.5, device=device)
    # reward state
    air = 0.6 * ru(N, 4) * (ru(N, 4) < 0.7)
    d.update(feet_air_time=air, last_contacts=ru(N, 4) < 0.5,
             stumble=torch.randint(0, 32, (N, 4), generator=g, device=device).to(torch.uint8) * (ru(N, 4) < 0.3),
             pitch_est=0.1 * rn(N))
    threshold_rows(d)
    return d


def threshold_rows(d: dict) -> dict:
    """Rows that sit EXACTLY on a threshold (all comparisons of the reference are strict or fp32-exact here):
      row 0: foot 0 fz == 1        -> not in contact (fz > 1 is false);
      row 1: command xy == (0.1, 0) -> neither standing (< 0.1) nor moving (> 0.1);
      row 2: |g_x| == 0.6           -> no big_pitch (> 0.6 is false);
      row 3: foot 1 clearance == 0.18 -> not counted by foot_clearance (> 0.18 is false);
      row 4: the lowest foot at z == 0 -> no foothold_miss (< 0 is false);
      row 5: terrain level == 5     -> foot_acc mask 1.0 (> 5 is false);
      row 6: foot 0 |f_xy| == 3 |fz| -> feet_stumble not triggered (> is false), and 4 / 5 |fz| neither."""
    N = d["root_states"].shape[0]
    F0, F1 = REWARD_FEET[0], REWARD_FEET[1]
    if N > 0:
        d["contact_forces"][0, F0] = torch.tensor([0.0, 0.0, 1.0])
    if N > 1:
        d["commands"][1, :2] = torch.tensor([0.1, 0.0])
    if N > 2:
        d["projected_gravity"][2, 0] = 0.6
    if N > 3:
        d["measured_foot_clearance"][3, 1] = 0.18
    if N > 4:
        d["foot_positions"][4, :, 2] = torch.tensor([0.0, 0.05, 0.1, 0.12])
    if N > 5:
        d["terrain_levels"][5] = 5
    if N > 6:
        d["contact_forces"][6, F0] = torch.tensor([6.0, 0.0, 2.0])
        d["contact_forces"][6, F1] = torch.tensor([0.0, 0.0, 2.0])
    return d


def reward_table(rows: int = 1400, cols: int = 900, seed: int = 37, device="cpu") -> torch.Tensor:
    """int16 terrain table (horizontal 0.05 m, vertical 0.005 m, 20 m border) under the feet of `reward_state`."""
    g = _gen(seed, device)
    return torch.randint(-200, 200, (rows, cols), generator=g, device=device).to(torch.int16)


# tensors of a LeggedRobotDTC env that reset_idx clears row-wise ([N, ...]) and the time-major ring buffers ([10, N, C])
RESET_ROW_ITEMS = ("last_actions", "last_actions_2", "last_dof_vel", "feet_air_time", "feet_contact_time", "last_scale_actions",
                   "last_scale_actions2", "pitch_est", "base_ang_vel_last", "base_lin_vel_last", "episode_length_buf", "contact_filt",
                   "last_contacts")
RESET_TIME_ITEMS = ("lin_vel_buffer", "ang_vel_buffer", "cmd_buffer")


def reset_state(num_envs: int, seed: int = 41, device="cpu", *, terrain_rows: int = 6, terrain_cols: int = 2, n_sums: int = 24,
                reset: str = "some", env_length: float = 8.0, episode_length_s: float = 20.0) -> dict:
    """Mock env state for `reset_idx` (legged_robot.py:200-272): every tensor it and its callees read or write, keyed by the env's
    attribute names (`lag_buffer` / `stumb_buffer` are lists, `episode_sums` is [n_sums, N]).  About one env in eight is reset
    (`reset` = "some"; "all" / "none" set every / no flag).  The terrain curriculum (legged_robot.py:690-711) meets all its branches:
    levels are weighted towards 0 and terrain_rows - 1, and the walked distance is drawn beyond env_length * 0.6 (move up), below
    |commands_xy| * episode_length_s * 0.5 (move down) or between, each >= 2e-3 (relative) away from its threshold.  A few envs
    that are NOT reset hold NaN rows, so that an untouched row is provable."""
    g = _gen(seed, device)
    N, D, B = num_envs, 12, 17
    ru = lambda *s: torch.rand(*s, generator=g, device=device)          # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=g, device=device)         # noqa: E731
    ri = lambda hi, *s: torch.randint(0, hi, s, generator=g, device=device)          # noqa: E731
    flag = {"some": ru(N) < 0.125, "all": torch.ones(N, dtype=torch.bool, device=device),
            "none": torch.zeros(N, dtype=torch.bool, device=device)}[reset]
    R, Ct = terrain_rows, terrain_cols
    origins = torch.zeros(R, Ct, 3, device=device)
    origins[:, :, 0] = 24.0 + 8.0 * torch.arange(R, device=device, dtype=torch.float32)[:, None]
    origins[:, :, 1] = 24.0 + 8.0 * torch.arange(Ct, device=device, dtype=torch.float32)[None, :]
    origins[:, :, 2] = 0.1 * rn(R, Ct)
    types = (torch.arange(N, device=device) * Ct) // max(N, 1)
    edge = ru(N)
    levels = torch.where(edge < 0.3, torch.zeros(N, dtype=torch.int64, device=device),
                         torch.where(edge < 0.6, torch.full((N,), R - 1, dtype=torch.int64, device=device), ri(R, N)))
    env_origins = origins[levels, types].clone()
    cmd = 0.6 * rn(N, 4)
    still = ru(N) < 0.15
    cmd[still, :2] *= 0.05
    cn = cmd[:, :2].norm(dim=1)
    half = cn * (episode_length_s * 0.5)
    up_at = env_length * 0.6
    kind = ru(N)
    dist = torch.where(kind < 0.4, up_at * 1.01 + 3.0 * ru(N),
                       torch.where(kind < 0.85, 0.95 * ru(N) * torch.minimum(half, torch.full_like(half, up_at * 0.98)),
                                   _away(half * 1.1, up_at)))
    ang = 2 * math.pi * ru(N)
    root = torch.zeros(N, 13, device=device)
    root[:, 0] = env_origins[:, 0] + dist * torch.cos(ang)
    root[:, 1] = env_origins[:, 1] + dist * torch.sin(ang)
    root[:, 2] = env_origins[:, 2] + 0.3 + 0.1 * ru(N)
    q = rn(N, 4)
    root[:, 3:7] = q / q.norm(dim=1, keepdim=True)
    root[:, 7:13] = 0.5 * rn(N, 6)
    default = torch.tensor([0.1, -0.8, 1.6, -0.1, -0.8, 1.6] * 2, device=device)
    d = dict(reset_buf=flag, root_states=root, env_origins=env_origins, commands=cmd, terrain_levels=levels, terrain_types=types,
             terrain_origins=origins, default_dof_pos=default, dof_pos=default + 0.3 * rn(N, D), dof_vel=2.0 * rn(N, D),
             forces=10.0 * rn(N, B, 3), motor_strengths=0.9 + 0.2 * ru(N, D), Kp_factors=0.95 + 0.1 * ru(N, D),
             Kd_factors=0.95 + 0.1 * ru(N, D), height_noise_offset=(0.02 * rn(N, 1)).expand(N, N_POINTS).contiguous(),
             base_init_state=torch.tensor([0.0, 0.0, 0.4, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], device=device),
             episode_sums=5.0 * rn(n_sums, N),
             last_actions=rn(N, D), last_actions_2=rn(N, D), last_dof_vel=2.0 * rn(N, D), feet_air_time=0.6 * ru(N, 4),
             feet_contact_time=0.6 * ru(N, 4), last_scale_actions=0.25 * rn(N, D), last_scale_actions2=0.25 * rn(N, D),
             pitch_est=0.1 * rn(N), base_ang_vel_last=0.5 * rn(N, 3), base_lin_vel_last=0.5 * rn(N, 3),
             episode_length_buf=1 + ri(1000, N), contact_filt=ru(N, 4) < 0.6, last_contacts=ru(N, 4) < 0.5,
             lag_buffer=[0.25 * rn(N, D) for _ in range(6)], stumb_buffer=[ru(N, 4) < 0.3 for _ in range(5)],
             lin_vel_buffer=0.5 * rn(10, N, 2), ang_vel_buffer=0.5 * rn(10, N, 1), cmd_buffer=0.6 * rn(10, N, 4))
    # NaN rows in envs that are not reset (every 7th of them): they must come out bit-identical
    keep = torch.nonzero(~flag).flatten()[::7]
    for k in ("dof_pos", "dof_vel", "last_actions", "height_noise_offset", "motor_strengths", "feet_air_time", "forces"):
        d[k][keep] = float("nan")
    d["root_states"][keep, 7:] = float("nan")
    d["commands"][keep, 2:] = float("nan")
    d["episode_sums"][:, keep] = float("nan")
    d["cmd_buffer"][:, keep] = float("nan")
    return d


def reset_draws(num_envs: int, seed: int = 43, device="cpu", *, num_dof: int = 12, max_terrain_level: int = 6):
    """The draws one `reset_idx` call may consume, one row per env (include/dtc_hip.h, dtc_env_reset): u [N, num_dof + 14] in [0, 1)
    and level_draw [N] int64 in [0, max_terrain_level)."""
    g = _gen(seed, device)
    u = torch.rand(num_envs, num_dof + 14, generator=g, device=device)
    return u, torch.randint(0, max_terrain_level, (num_envs,), generator=g, device=device)
