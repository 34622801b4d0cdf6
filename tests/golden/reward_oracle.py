"""Float64 numpy restatement of LeggedRobot.compute_reward and the 34 `_reward_*` terms of LeggedRobotDTC
(legged_gym/envs/base/legged_robot.py:274-291, :1321-1622; legged_gym/envs/base/legged_robot_dtc.py:522-586).

Used by tests/test_reward_oracle.py (against the reference-captured tests/golden/rewards.npz) and by
tests/test_hip_rewards.py (as the yardstick of csrc/rewards.hip).  Thresholds are compared against their fp32 values, as
torch compares an fp32 tensor with a Python scalar; the integer table gather of `_get_foot_clearance` is done in fp32 as the
reference does, so that it can be matched exactly.

Inputs `s`: dict of numpy arrays keyed by the env's attribute names.  State `st` (read and written):
feet_air_time [N,4], last_contacts [N,4] bool, stumble [N,4] uint8 (bit k = the stumble mask pushed k steps ago;
the 5-deep list of :1485), pitch_est [N].

`term` / `compute_reward` take a working precision `wp`: float64 (the default: the yardstick) or float32, whose distance from
the float64 run on the same inputs is the yardstick's own fp32 rounding error (tests/reward_cases.py builds the bound of every
comparison from it).  `state(s, wp)` hands out the state in that precision.
"""
import itertools

import numpy as np

NAMES = sorted("""action_rate ang_vel_xy base_height big_pitch collision dof_acc dof_pos_limits dof_vel dof_vel_limits feet_air_time
feet_contact_forces feet_slip feet_stumble foot_acc foot_clearance foothold_miss hip_pos lin_vel_z orientation orientation_roll pos_acc
power powerchange smooth soft_tracking_ang_vel soft_tracking_lin_vel stand_still stumble termination torque_limits torques
tracking_ang_vel tracking_lin_vel tracking_optimal_footholds""".split())
assert len(NAMES) == 34

# terms whose value is a count / indicator (compared exactly, as term = per_term / scale); the rest are continuous
DISCRETE = {"big_pitch", "collision", "feet_stumble", "foot_clearance", "foothold_miss", "stumble", "termination"}


def f32(x):
    """A Python threshold as torch sees it next to an fp32 tensor."""
    return float(np.float32(x))


def plane_rows(points_x, points_y):
    """Rows 0, 1 of (A^T A)^-1 A^T for A = [x, y, 1] over the height grid (legged_robot.py:1535-1557, _init_height_points
    meshgrid indexing='ij'): the least-squares slopes of a height row are M @ h.  float64 from the fp32 grid coordinates."""
    x = np.asarray(points_x, dtype=np.float32).astype(np.float64)
    y = np.asarray(points_y, dtype=np.float32).astype(np.float64)
    gx, gy = np.meshgrid(x, y, indexing="ij")
    A = np.stack([gx.ravel(), gy.ravel(), np.ones(gx.size)], axis=1)
    M = np.linalg.inv(A.T @ A) @ A.T
    return M[:2].copy()


def foot_clearance_from_table(foot_positions, height_samples, border_size, horizontal_scale, vertical_scale):
    """_get_foot_clearance (legged_robot.py:1443-1472) in the reference's fp32 arithmetic: max of 10 samples, indices
    truncated toward zero and clipped to [1, dim-3]."""
    p = foot_positions.astype(np.float32)
    pts = (p[:, :, :2] + np.float32(border_size)) / np.float32(horizontal_scale)
    # .long() as on the GPU: NaN -> 0, +-inf saturate; then clip(1, dim - 3).  Index -1 (px - 2 at px == 1) wraps to the last row /
    # column, as torch (and numpy) indexing does
    pts = np.clip(np.nan_to_num(pts.astype(np.float64), nan=0.0, posinf=2.0 ** 62, neginf=-2.0 ** 62), -2.0 ** 62, 2.0 ** 62)
    px = np.clip(np.trunc(pts[:, :, 0]).astype(np.int64), 1, height_samples.shape[0] - 3)
    py = np.clip(np.trunc(pts[:, :, 1]).astype(np.int64), 1, height_samples.shape[1] - 3)
    offs = [(0, 0), (1, 0), (0, 1), (2, 0), (0, 2), (1, 1), (-1, 0), (0, -1), (-2, 0), (0, -2)]
    h = np.max(np.stack([height_samples[px + dx, py + dy] for dx, dy in offs]), axis=0)
    return p[:, :, 2] - h.astype(np.float32) * np.float32(vertical_scale)


def _norm(v):
    return np.sqrt(np.sum(v * v, axis=-1))


def _quat_from_euler_xyz(roll, pitch, yaw):
    cy, sy = np.cos(yaw * 0.5), np.sin(yaw * 0.5)
    cr, sr = np.cos(roll * 0.5), np.sin(roll * 0.5)
    cp, sp = np.cos(pitch * 0.5), np.sin(pitch * 0.5)
    return np.stack([cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp, sy * cr * cp - cy * sr * sp,
                     cy * cr * cp + sy * sr * sp], axis=-1)


def _quat_rotate_inverse(q, v):
    w, qv = q[:, 3:4], q[:, :3]
    return v * (2.0 * w * w - 1.0) - np.cross(qv, v) * w * 2.0 + qv * np.sum(qv * v, axis=-1, keepdims=True) * 2.0


def _orientation(s, cfg, st, wp=np.float64):
    """Shared part of _reward_orientation / _reward_orientation_roll (legged_robot.py:1559-1596): updates pitch_est and
    returns the gravity direction of the fitted plane in the estimated base frame."""
    h = s["measured_heights"].astype(wp)
    plane = np.asarray(cfg["plane"], dtype=wp)
    ax, by = h @ plane[0], h @ plane[1]
    n = np.sqrt(ax * ax + by * by + 1.0)
    pitch, roll = np.arctan(-ax / n), -np.arctan(-by / n)          # p_norm = -plane_vector
    lim = f32(0.1)
    pitch_c = np.where((pitch >= -lim) & (pitch <= lim), wp(0.0), pitch)
    roll_c = np.where((roll >= -lim) & (roll <= lim), wp(0.0), roll)
    st["pitch_est"] = st["pitch_est"] * f32(0.2) + f32(0.8) * pitch_c
    q = _quat_from_euler_xyz(roll_c, st["pitch_est"], np.zeros_like(roll_c))
    grav = np.tile(np.array([0.0, 0.0, -1.0], dtype=wp), (len(q), 1))
    return _quat_rotate_inverse(q, grav)


def state(s, wp=np.float64):
    """Copies of the reward state of `s` for `term` / `compute_reward`, the float items in working precision `wp`.  `term`
    advances feet_air_time and pitch_est in the dtype they come in: handed the env's own fp32 arrays, a float64 run does those
    updates in fp32."""
    return {k: (s[k].astype(wp) if s[k].dtype.kind == "f" else s[k].copy()) for k in STATE}


def term(name, s, cfg, st, wp=np.float64):
    """Value of `_reward_<name>` (before the scale), `wp` [N]; updates `st` as the reference updates the env.  `wp` is the
    working precision: float64 (the yardstick) or float32 (the yardstick's own rounding error: every input, constant and
    intermediate in fp32, summed in numpy's order).  Constants enter as Python floats rounded to `wp`, which leave an array's
    dtype alone."""
    k = lambda x: float(wp(x))                                               # noqa: E731
    F = cfg["feet_indices"]
    cf = s["contact_forces"].astype(wp)
    cff = cf[:, F]
    cmd = s["commands"].astype(wp)
    cmd_norm = _norm(cmd[:, :2])
    dt = k(cfg["dt"])
    g = lambda key: s[key].astype(wp)                                        # noqa: E731
    if name == "lin_vel_z":                                                  # :1321
        return g("base_lin_vel")[:, 2] ** 2
    if name == "ang_vel_xy":                                                 # :1325
        return np.sum(g("base_ang_vel")[:, :2] ** 2, axis=1)
    if name == "torques":                                                    # :1334
        return np.sum(g("torques") ** 2, axis=1)
    if name == "dof_vel":                                                    # :1338
        return np.sum(g("dof_vel") ** 2, axis=1)
    if name == "dof_acc":                                                    # :1342
        return np.sum(((g("last_dof_vel") - g("dof_vel")) / dt) ** 2, axis=1)
    if name == "action_rate":                                                # :1620 (= :1346)
        return np.sum((g("last_actions") - g("actions")) ** 2, axis=1)
    if name == "collision":                                                  # :1350
        return np.sum(_norm(cf[:, cfg["penalised_contact_indices"]]) > f32(0.1), axis=1).astype(wp)
    if name == "termination":                                                # :1354
        return (s["reset_buf"].astype(bool) & ~s["time_out_buf"].astype(bool)).astype(wp)
    if name == "dof_pos_limits":                                             # :1358
        q, lim = g("dof_pos"), g("dof_pos_limits")
        return np.sum(-np.minimum(q - lim[:, 0], 0.0) + np.maximum(q - lim[:, 1], 0.0), axis=1)
    if name == "dof_vel_limits":                                             # :1364
        return np.sum(np.clip(np.abs(g("dof_vel")) - g("dof_vel_limits") * k(cfg["soft_dof_vel_limit"]), 0.0, 1.0), axis=1)
    if name == "torque_limits":                                              # :1369
        return np.sum(np.maximum(np.abs(g("torques")) - g("torque_limits") * k(cfg["soft_torque_limit"]), 0.0), axis=1)
    if name == "tracking_lin_vel":                                           # :1373
        e = np.sum(((cmd[:, :2] - g("base_lin_vel")[:, :2]) / k(cfg["lin_vel_x_max"])) ** 2, axis=1)
        return np.exp(-e / k(cfg["tracking_sigma"]))
    if name == "tracking_ang_vel":                                           # legged_robot_dtc.py:571 (= :1380)
        return np.exp(-(cmd[:, 2] - g("base_ang_vel")[:, 2]) ** 2 / k(cfg["tracking_sigma"]))
    if name == "feet_air_time":                                              # :1386-1412
        contact = cff[:, :, 2] > 1.0
        cfilt = contact | st["last_contacts"]
        st["last_contacts"] = contact
        first = (st["feet_air_time"] > 0.0) & cfilt
        st["feet_air_time"] = st["feet_air_time"] + dt
        rew = np.sum((st["feet_air_time"] - 0.5) * first, axis=1) * (cmd_norm > f32(0.1))
        st["feet_air_time"] = st["feet_air_time"] * ~cfilt
        return rew
    if name in ("stumble", "feet_stumble"):                                  # :1417 / legged_robot_dtc.py:526
        m = 5.0 if name == "stumble" else 3.0
        return np.any(_norm(cff[:, :, :2]) > m * np.abs(cff[:, :, 2]), axis=1).astype(wp)
    if name == "stand_still":                                                # :1422
        return np.sum(np.abs(g("dof_pos") - g("default_dof_pos").reshape(1, -1)), axis=1) * (cmd_norm < f32(0.1))
    if name == "feet_contact_forces":                                        # :1426
        return np.sum(np.maximum(_norm(cff) - k(cfg["max_contact_force"]), 0.0), axis=1)
    if name == "power":                                                      # :1435
        return np.sum(np.maximum(g("torques") * g("dof_vel"), 0.0), axis=1)
    if name == "smooth":                                                     # :1440
        return np.sum((g("actions") - 2 * g("last_actions") + g("last_actions_2")) ** 2, axis=1)
    if name == "foot_clearance":                                             # :1474-1492
        stumb = _norm(cff[:, :, :2]) > 4 * np.abs(cff[:, :, 2])
        st["stumble"] = ((st["stumble"].astype(np.uint8) << 1) | stumb.astype(np.uint8)) & np.uint8(0x1F)
        flag = st["stumble"] != 0
        return np.sum(~flag & (g("measured_foot_clearance") > f32(0.18)), axis=1).astype(wp)
    if name == "feet_slip":                                                  # :1494
        cfilt = (cff[:, :, 2] > 1.0) | st["last_contacts"]
        return np.sum(cfilt * np.sum(g("foot_velocities")[:, :, :2] ** 2, axis=-1), axis=1)
    if name == "hip_pos":                                                    # :1504
        return np.sum(g("dof_pos")[:, cfg["hip_indices"]] ** 2, axis=1)
    if name == "powerchange":                                                # :1613 (= :1507)
        smooth_co = np.maximum(cmd[:, 0], 1.0)
        return (np.sum(np.maximum(g("torques") * g("dof_vel"), 0.0), axis=1) / (g("robot_mass") * k(9.815) * smooth_co)) ** 2
    if name == "pos_acc":                                                    # :1600 (the later definition: half-extents / 2)
        pts = (np.array(list(itertools.product([-1, 1], repeat=3))) * [0.3, 0.2, 0.15] / 2.0).astype(np.float32).astype(wp)
        v = g("base_lin_vel")[:, None, :] + np.cross(g("base_ang_vel")[:, None, :], pts[None])
        return np.sum(np.sum(v * v, axis=-1), axis=1)
    if name == "foot_acc":                                                   # :1525
        mask = np.where(s["terrain_levels"] > 5, f32(0.2), 1.0).astype(wp)
        a = _norm((g("last_foot_velocities") - g("foot_velocities")) / dt)
        return np.sum(np.maximum(mask[:, None] * (a - k(cfg["max_acc"])), 0.0), axis=1)
    if name == "orientation":                                                # :1559
        p = _orientation(s, cfg, st, wp)
        return (g("projected_gravity")[:, 0] - p[:, 0]) ** 2
    if name == "orientation_roll":                                           # :1579
        p = _orientation(s, cfg, st, wp)
        return np.abs(g("projected_gravity")[:, 1] - p[:, 1])
    if name == "big_pitch":                                                  # legged_robot_dtc.py:522
        return (np.abs(g("projected_gravity")[:, 0]) > f32(0.6)).astype(wp)
    if name == "base_height":                                                # legged_robot_dtc.py:531
        fp = g("foot_positions")
        return (g("root_states")[:, 2] - np.mean(fp[:, :, 2], axis=-1) - k(cfg["base_height_target"])) ** 2
    if name == "foothold_miss":                                              # legged_robot_dtc.py:536
        return (np.min(g("foot_positions")[:, :, 2], axis=-1) < 0).astype(wp)
    if name == "soft_tracking_lin_vel":                                      # legged_robot_dtc.py:542 (sic: ONE velocity row)
        d = (g("cmd_buffer")[-3:, :, :2] - g("lin_vel_buffer")[-3, :, :2]) / k(cfg["lin_vel_x_max"])
        return np.mean(np.exp(-np.sum(d * d, axis=-1) / k(cfg["tracking_sigma"])), axis=0)
    if name == "soft_tracking_ang_vel":                                      # legged_robot_dtc.py:555
        d = ((g("cmd_buffer")[-4:, :, 2] - g("ang_vel_buffer")[-4:, :, 0]) / k(cfg["ang_vel_yaw_max"])) ** 2
        d = np.where(d <= f32(0.15 ** 2), 0.0, 1.0).astype(wp)
        return np.mean(np.exp(-d / k(cfg["tracking_sigma"])), axis=0)
    if name == "tracking_optimal_footholds":                                 # legged_robot_dtc.py:577
        fp, opt = g("foot_positions"), g("optimal_footholds_world")
        r = -np.log(k(0.8) + _norm(fp[:, :, :2] - opt[:, :, :2]))
        return np.sum(np.where(s["contact_filt"].astype(bool), r, wp(0.0)), axis=-1)
    raise KeyError(name)


def compute_reward(s, cfg, st, episode_sums, wp=np.float64):
    """legged_robot.py:274-291.  cfg["scales"]: {name: fp32(scale * dt)} of the active terms in the reference's order
    (termination included).  Updates `st` and `episode_sums` ({name: `wp` [N]}); returns (rew_buf, {name: term * scale}), all
    in the working precision `wp` (see `term`)."""
    N = s["root_states"].shape[0]
    rew = np.zeros(N, dtype=wp)
    per = {}
    for name, scale in cfg["scales"].items():
        if name == "termination":
            continue
        per[name] = term(name, s, cfg, st, wp) * float(wp(scale))
        rew = rew + per[name]
        episode_sums[name] = episode_sums[name] + per[name]
    if cfg["only_positive_rewards"]:
        rew = np.maximum(rew, 0.0)
    if "termination" in cfg["scales"]:
        per["termination"] = term("termination", s, cfg, st, wp) * float(wp(cfg["scales"]["termination"]))
        rew = rew + per["termination"]
        episode_sums["termination"] = episode_sums["termination"] + per["termination"]
    return rew, per


def config(scales, rewards, commands_ranges, dt, feet_indices, penalised_contact_indices, hip_indices, points_x, points_y):
    """Oracle config from plain values.  `scales`: {name: fp32 scale*dt} in the reference's order."""
    return dict(scales=dict(scales), dt=float(np.float32(dt)), tracking_sigma=rewards["tracking_sigma"],
                soft_dof_vel_limit=rewards["soft_dof_vel_limit"], soft_torque_limit=rewards["soft_torque_limit"],
                base_height_target=rewards["base_height_target"], max_contact_force=rewards["max_contact_force"],
                max_acc=rewards["max_acc"], only_positive_rewards=bool(rewards["only_positive_rewards"]),
                lin_vel_x_max=commands_ranges["lin_vel_x"][1], ang_vel_yaw_max=commands_ranges["ang_vel_yaw"][1],
                feet_indices=list(feet_indices), penalised_contact_indices=list(penalised_contact_indices),
                hip_indices=list(hip_indices), plane=plane_rows(points_x, points_y))


# ---------------------------------------------------------------------------------------------------------------- sequences
# A multi-step run of compute_reward as LeggedRobotDTC.post_physics_step drives it (legged_robot_dtc.py:60-223): fresh env
# quantities every step, the velocity / command ring-buffer roll (:76-81), the contact update of _post_physics_step_callback
# (legged_robot.py:561-564), compute_reward, reset_idx on the rows it zeroes (legged_robot.py:233-272) and the last_* roll
# (legged_robot_dtc.py:213-217).  The env is a dict of numpy arrays; `state` names what compute_reward itself updates.
CARRIED = ("last_dof_vel", "last_actions", "last_actions_2", "last_foot_velocities", "cmd_buffer", "lin_vel_buffer", "ang_vel_buffer",
           "contact_filt")
STATE = ("feet_air_time", "last_contacts", "stumble", "pitch_est")


def np_state(d):
    return {k: (v.numpy().copy() if hasattr(v, "numpy") else np.array(v)) for k, v in d.items()}


def seq_begin(d0, feet_indices):
    env = np_state(d0)
    seq_callback(env, feet_indices)
    return env


def seq_callback(env, feet_indices):
    contact = env["contact_forces"][:, feet_indices, 2] > np.float32(1.0)
    env["contact_filt"] = contact | env["last_contacts"]
    env["last_contacts"] = contact


def seq_reset(env, episode_sums):
    """reset_idx for the envs with reset_buf set; returns their indices."""
    ids = np.nonzero(env["reset_buf"])[0]
    for k in ("last_actions", "last_actions_2", "last_dof_vel", "feet_air_time", "pitch_est", "stumble", "contact_filt", "last_contacts"):
        env[k][ids] = 0
    for k in ("lin_vel_buffer", "ang_vel_buffer", "cmd_buffer"):
        env[k][:, ids] = 0
    for v in episode_sums.values():
        v[ids] = 0
    return ids


def seq_next(env, fresh, feet_indices):
    """last_* roll of the finished step, then the next step's fresh quantities, buffer roll and contact update."""
    env["last_actions_2"] = env["last_actions"].copy()
    env["last_actions"] = env["actions"].copy()
    env["last_dof_vel"] = env["dof_vel"].copy()
    env["last_foot_velocities"] = env["foot_velocities"].copy()
    for k, v in np_state(fresh).items():
        if k not in CARRIED and k not in STATE:
            env[k] = v
    for k, new in (("lin_vel_buffer", env["base_lin_vel"][:, :2]), ("ang_vel_buffer", env["base_ang_vel"][:, 2:3]),
                   ("cmd_buffer", env["commands"])):
        env[k] = np.concatenate([env[k][1:], new[None]], axis=0)
    seq_callback(env, feet_indices)
