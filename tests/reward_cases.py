"""Shared by tests/test_reward_oracle.py (CPU) and tests/test_hip_rewards.py (GPU): the per-term measure of a reward term against the
float64 oracle (tests/golden/reward_oracle.py), its bound from the oracle's own fp32 run, and the cases both files run.

Measure of a continuous term with reference vector `ref` over the rows of a case:

    err = max_i |got_i - ref_i| / max(|ref_i|, 1e-2 * max_j |ref_j|)           (max_j |ref_j| == 0: got must be exactly zero)

Bound: max(2^-20, 8 * e32), e32 = the same measure of the oracle run in float32 working precision on the same inputs against its
float64 run (the factor 8 is the one of tests/test_hip_recurrence_bptt.py: it covers a different summation order and the device
expf / logf / atanf / sinf / cosf next to numpy's).  The inputs are chosen so that 8 * e32 <= CAP for every continuous term of every
case -- a condition on the inputs, asserted on the CPU (test_reward_oracle.py), not a measurement of the kernel.
"""
import dataclasses
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import reward_oracle as O  # noqa: E402
from dtc_amd import synthetic as S  # noqa: E402
from dtc_amd.rewards import RewardConfig, TERMS  # noqa: E402

FLOOR, FACTOR, CAP = 2.0 ** -20, 8.0, 5e-4
OLD_BOUND = 4e-6                                   # the bound of the measure this one replaces (old_err)
CONTINUOUS = tuple(n for n in TERMS if n not in O.DISCRETE)
# the carried state a term advances; every other term must leave it bit-unchanged
OWNS = {"feet_air_time": ("feet_air_time", "last_contacts"), "foot_clearance": ("stumble",), "orientation": ("pitch_est",),
        "orientation_roll": ("pitch_est",)}
SCALE = float(np.float32(-0.37 * 0.02))            # the scale of a term run alone (an fp32 value that is no power of two)
SETS = (("feet_air_time", "feet_slip"), ("feet_slip",), ("orientation", "orientation_roll"),
        ("foot_clearance", "stumble", "feet_stumble"))


def term_err(got, ref):
    """The measure above; inf where `ref` is all zero and `got` is not, NaN where `got` holds one."""
    ref = np.asarray(ref, dtype=np.float64).ravel()
    got = np.asarray(got, dtype=np.float64).ravel()
    if ref.size == 0:
        return 0.0
    top = float(np.max(np.abs(ref)))
    if top == 0.0:
        return 0.0 if np.all(got == 0.0) else float("inf")
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-2 * top)))


def old_err(got, ref):
    """|got - ref| / max(1, |ref|): the measure the tests used before; kept to pin what it could not see."""
    ref = np.asarray(ref, dtype=np.float64)
    e = np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    return float(np.max(e)) if e.size else 0.0


def bound(e32):
    return max(FLOOR, FACTOR * e32)


@dataclasses.dataclass(frozen=True)
class Layout:
    """The robot the inputs describe: dofs, bodies, command width and the index lists of EnvRewards."""
    num_dof: int = 12
    num_bodies: int = 17
    num_commands: int = 4
    feet: tuple = S.REWARD_FEET
    penalised: tuple = S.REWARD_PENALISED
    hips: tuple = S.REWARD_HIPS


LITE3 = Layout()


def oracle_cfg(rc: RewardConfig, layout: Layout = LITE3):
    r = dict(tracking_sigma=rc.tracking_sigma, soft_dof_vel_limit=rc.soft_dof_vel_limit, soft_torque_limit=rc.soft_torque_limit,
             base_height_target=rc.base_height_target, max_contact_force=rc.max_contact_force, max_acc=rc.max_acc,
             only_positive_rewards=rc.only_positive_rewards)
    ranges = dict(lin_vel_x=[-rc.lin_vel_x_max, rc.lin_vel_x_max], ang_vel_yaw=[-rc.ang_vel_yaw_max, rc.ang_vel_yaw_max])
    return O.config(rc.scales, r, ranges, rc.dt, layout.feet, layout.penalised, layout.hips, rc.points_x, rc.points_y)


def run_oracle(env, cfg, sums0, wp):
    """One compute_reward of the oracle in working precision `wp` from the state and the episode sums `sums0` ([n_active, N])."""
    st = O.state(env, wp)
    sums = {n: np.asarray(sums0[i]).astype(wp) for i, n in enumerate(cfg["scales"])}
    rew, per = O.compute_reward(env, cfg, st, sums, wp)
    return dict(rew=rew, per=per, st=st, sums=sums)


def e32_of(r32, r64):
    """e32 per continuous term, of rew and of the two float state items, from the two oracle runs."""
    e = {n: term_err(r32["per"][n], r64["per"][n]) for n in r64["per"] if n not in O.DISCRETE}
    e["rew"] = term_err(r32["rew"], r64["rew"])
    e["air"] = term_err(r32["st"]["feet_air_time"], r64["st"]["feet_air_time"])
    e["pitch"] = term_err(r32["st"]["pitch_est"], r64["st"]["pitch_est"])
    return e


def reference(env, cfg, sums0):
    """-> (the float64 run, e32 per checked quantity)."""
    r64 = run_oracle(env, cfg, sums0, np.float64)
    return r64, e32_of(run_oracle(env, cfg, sums0, np.float32), r64)


# ------------------------------------------------------------------------------------------------------------------- cases
def cfg_from_fixture(z, tag):
    """A LeggedRobotCfg-shaped config holding the raw scale attributes and reward settings the fixture recorded."""
    raw = dict(zip([str(n) for n in z[f"{tag}_raw_names"]], [float(v) for v in z[f"{tag}_raw_values"]]))
    p = z[f"{tag}_params"]
    rewards = type("rewards", (), dict(scales=type("scales", (), raw), tracking_sigma=p[1], soft_dof_vel_limit=p[2],
                                       soft_torque_limit=p[3], base_height_target=p[4], max_contact_force=p[5], max_acc=p[6],
                                       only_positive_rewards=bool(p[7])))
    ranges = type("ranges", (), dict(lin_vel_x=[-p[8], p[8]], ang_vel_yaw=[-p[9], p[9]]))
    return type("cfg", (), dict(rewards=rewards, sim=type("sim", (), dict(dt=0.005)), control=type("control", (), dict(decimation=4)),
                                commands=type("commands", (), dict(ranges=ranges)),
                                terrain=type("terrain", (), dict(measured_points_x=S.MEASURED_POINTS_X,
                                                                 measured_points_y=S.MEASURED_POINTS_Y))))


def fixture_rc(fx, tag, only_positive=None):
    rc = RewardConfig.from_cfg(cfg_from_fixture(fx, tag))
    if only_positive is not None:
        rc.only_positive_rewards = only_positive
    return rc


EVERY_TERM_N = (1, 64, 1024, 4099)
_STATES = {}


def lite3_state(N, seed):
    """synthetic.reward_state as numpy arrays; drawn once per (N, seed) and handed out as copies."""
    if (N, seed) not in _STATES:
        _STATES[N, seed] = O.np_state(S.reward_state(N, seed=seed))
    return {k: v.copy() for k, v in _STATES[N, seed].items()}


def linspace_sums(n_terms, N):
    return np.linspace(-1.0, 1.0, n_terms * N, dtype=np.float64).astype(np.float32).reshape(n_terms, N)


def alone(name, termination):
    """The config of one term as the only active one (plus termination on request), in the reference's order."""
    names = sorted({name, "termination"} if termination else {name})
    return RewardConfig(scales={n: SCALE for n in names})


def term_set(names):
    return RewardConfig(scales={n: SCALE for n in sorted(names)})


ALONE_N, ALONE_SEED = 67, 4067
ALONE_CASES = tuple((n, t) for n in TERMS for t in (False, True) if not (n == "termination" and t))

# (num_dof, num_bodies, num_commands, feet, n_penalised, hips, grid points x / y as slices of the Lite3 grid coordinates)
_X, _Y = tuple(S.MEASURED_POINTS_X), tuple(S.MEASURED_POINTS_Y)
SHAPES = {
    "dof1-body5-cmd3-grid2x2": (1, 5, 3, (3, 0, 4, 1), 0, (), (_X[0], _X[-1]), (_Y[0], _Y[-1])),
    "dof1-body5-cmd5-grid11x7": (1, 5, 5, (3, 0, 4, 1), 1, (0,), _X[:11], _Y[:7]),
    "dof13-body40-cmd3-grid13x5": (13, 40, 3, (39, 0, 17, 5), 32, (12,), _X[10:23], _Y[8:13]),
    "dof64-body40-cmd5-grid33x21": (64, 40, 5, (3, 0, 4, 1), 32, tuple(range(63, -1, -4)), _X, _Y),
    "dof64-body5-cmd3-grid11x7": (64, 5, 3, (4, 2, 0, 1), 1, tuple(range(1, 64, 4)), _X[:11], _Y[:7]),
    "dof13-body5-cmd5-grid13x5": (13, 5, 5, (1, 4, 3, 0), 0, (0, 3, 6, 9), _X[:13], _Y[:5]),
    # Lite3 itself on the 77-point grid, which the GPU test hands to EnvRewards as grid= next to a config of 693 points
    "dof12-body17-cmd4-grid11x7": (12, 17, 4, S.REWARD_FEET, len(S.REWARD_PENALISED), S.REWARD_HIPS, _X[:11], _Y[:7]),
}
GRID_ARGUMENT = "dof12-body17-cmd4-grid11x7"
SHAPE_N = (5, 67)


def shape_case(key, rc_all):
    """-> (layout, the `all` config on this shape's height grid)."""
    D, B, C, feet, n_pen, hips, px, py = SHAPES[key]
    others = [b for b in range(B) if b not in feet]
    pen = tuple(others[::-1][:n_pen])                        # the non-foot bodies from the last one down
    assert len(pen) == n_pen and len(hips) in (0, 1, 4, 16) and all(0 <= h < D for h in hips)
    return Layout(D, B, C, tuple(feet), pen, tuple(hips)), dataclasses.replace(rc_all, points_x=tuple(px), points_y=tuple(py))


def _away(x, th, rel=2e-3):
    """synthetic._away on numpy arrays: x at least rel * |th| away from the threshold th, on its side (exact hits go up)."""
    gap = rel * abs(th) if th != 0 else rel
    lo, hi = th - gap, th + gap
    return np.where((x > lo) & (x < hi), np.where(x < th, lo, hi), x)


def shaped_state(N, layout: Layout, points_x, points_y, seed):
    """The inputs and state of synthetic.reward_state, its value ranges and its distance from every threshold, for any number of
    dofs, bodies, command columns and height points.  numpy default_rng; float32 arrays as the env holds them."""
    g = np.random.default_rng(seed)
    D, B, C, F = layout.num_dof, layout.num_bodies, layout.num_commands, list(layout.feet)
    ru, rn = (lambda *s: g.random(s)), (lambda *s: g.standard_normal(s))
    root = np.zeros((N, 13))
    root[:, 0], root[:, 1], root[:, 2], root[:, 6] = 21.0 + 30.0 * ru(N), 21.0 + 15.0 * ru(N), 0.25 + 0.15 * ru(N), 1.0
    root[:, 7:13] = 0.5 * rn(N, 6)
    cmd = 0.6 * rn(N, C)
    cmd[ru(N) < 0.15, :2] *= 0.05
    nrm = np.linalg.norm(cmd[:, :2], axis=1, keepdims=True)
    cmd[:, :2] *= _away(nrm, 0.1) / np.maximum(nrm, 1e-12)
    grav = np.stack([0.35 * rn(N), 0.2 * rn(N), -0.9 + 0.05 * ru(N)], axis=1)
    grav[:, 0] = np.sign(grav[:, 0]) * _away(np.abs(grav[:, 0]), 0.6)
    default = np.tile([0.0, -0.8, 1.6], (D + 2) // 3)[:D]
    ang_vel = 0.5 * rn(N, 3)
    ang_vel[:, 2] = cmd[:, 2] + 0.12 * rn(N)

    def off_tolerance(c, a):
        for _, ymax in S.REWARD_RANGE_MAXIMA:
            e = (c - a) / ymax
            a = c - ymax * np.sign(e) * _away(np.abs(e), 0.15)
        return a
    ang_vel[:, 2] = off_tolerance(cmd[:, 2], ang_vel[:, 2])
    d = dict(root_states=root, base_lin_vel=0.5 * rn(N, 3), base_ang_vel=ang_vel, projected_gravity=grav, commands=cmd,
             dof_pos=default + 0.3 * rn(N, D), default_dof_pos=default.copy(), dof_vel=2.0 * rn(N, D), last_dof_vel=2.0 * rn(N, D),
             torques=6.0 * rn(N, D), actions=rn(N, D), last_actions=rn(N, D), last_actions_2=rn(N, D))
    cf = 5.0 * rn(N, B, 3) * (ru(N, B, 1) < 0.5)
    fz = _away(np.where(ru(N, 4) < 0.6, 5.0 + 60.0 * ru(N, 4), 0.9 * ru(N, 4)), 1.0)
    ratio = 7.0 * ru(N, 4)
    for th in (3.0, 4.0, 5.0):
        ratio = _away(ratio, th)
    ang = 2 * np.pi * ru(N, 4)
    cf[:, F, 0], cf[:, F, 1] = ratio * fz * np.cos(ang), ratio * fz * np.sin(ang)
    cf[:, F, 2] = fz * np.where(ru(N, 4) < 0.9, 1.0, -1.0)
    bn = np.linalg.norm(cf, axis=-1, keepdims=True)
    d["contact_forces"] = np.where(bn > 0, cf * _away(bn, 0.1) / np.maximum(bn, 1e-12), cf)
    fp = np.empty((N, 4, 3))
    fp[:, :, :2] = root[:, None, :2] + 0.25 * rn(N, 4, 2)
    fp[:, :, 2] = _away(0.2 * ru(N, 4) - 0.03, 0.0, rel=1e-3)
    fv = 1.5 * rn(N, 4, 3)
    d.update(foot_positions=fp, foot_velocities=fv, last_foot_velocities=fv + 2.0 * rn(N, 4, 3),
             optimal_footholds_world=fp + 0.15 * rn(N, 4, 3),
             measured_foot_clearance=_away(_away(0.45 * ru(N, 4) - 0.05, 0.03), 0.18))
    # measured heights: a tilted plane + roughness, the fitted pitch / roll moved off the +-0.1 clip (M @ x = e0, M @ y = e1)
    x = np.asarray(points_x, dtype=np.float32).astype(np.float64)
    y = np.asarray(points_y, dtype=np.float32).astype(np.float64)
    gx, gy = (a.ravel() for a in np.meshgrid(x, y, indexing="ij"))
    M = O.plane_rows(points_x, points_y)
    slope = 0.25 * rn(N, 2)
    h = (root[:, 2:3] - 0.3) + slope[:, :1] * gx[None] + slope[:, 1:] * gy[None] + 0.01 * rn(N, gx.size)
    for _ in range(3):
        ax, by = h @ M[0], h @ M[1]
        n = np.sqrt(ax * ax + by * by + 1.0)
        pitch, roll = np.arctan(-ax / n), np.arctan(by / n)
        u = np.tan(np.sign(pitch) * _away(np.abs(pitch), 0.1, rel=4e-3))
        w = np.tan(np.sign(roll) * _away(np.abs(roll), 0.1, rel=4e-3))
        n2 = 1.0 / np.sqrt(1.0 - u * u - w * w)
        h = h + (-u * n2 - ax)[:, None] * gx[None] + (w * n2 - by)[:, None] * gy[None]
    d["measured_heights"] = h
    cmd_buf = 0.6 * rn(10, N, C)
    ang_buf = off_tolerance(cmd_buf[:, :, 2:3], cmd_buf[:, :, 2:3] + 0.12 * rn(10, N, 1))
    d.update(cmd_buffer=cmd_buf, lin_vel_buffer=cmd_buf[:, :, :2] + 0.2 * rn(10, N, 2), ang_vel_buffer=ang_buf,
             robot_mass=9.0 + 3.0 * ru(N), dof_pos_limits=np.stack([default - 0.45, default + 0.45], axis=1),
             dof_vel_limits=np.full(D, 2.5), torque_limits=np.full(D, 7.5), feet_air_time=0.6 * ru(N, 4) * (ru(N, 4) < 0.7),
             pitch_est=0.1 * rn(N))
    d = {k: v.astype(np.float32) for k, v in d.items()}
    d.update(contact_filt=ru(N, 4) < 0.6, reset_buf=ru(N) < 0.1, time_out_buf=ru(N) < 0.03, terrain_levels=g.integers(0, 10, N),
             last_contacts=ru(N, 4) < 0.5, stumble=(g.integers(0, 32, (N, 4)) * (ru(N, 4) < 0.3)).astype(np.uint8))
    # the fp32 rounding of the heights may not move a fitted angle back onto the clip
    ab = d["measured_heights"].astype(np.float64) @ M.T
    angles = np.arctan(ab / np.sqrt(np.sum(ab * ab, axis=1, keepdims=True) + 1.0))
    assert np.all(np.abs(np.abs(angles) - 0.1) > 2e-4) and d["measured_heights"].shape == (N, gx.size)
    return d


TAGS = ("lite3", "x30", "all")
TWENTY = dict(N=1024, steps=20, seed=900, tags=("lite3", "all"))


def every_term_case(fx, tag, N, only_positive):
    rc = fixture_rc(fx, tag, only_positive)
    return rc, LITE3, lite3_state(N, 11 + N), linspace_sums(len(rc.names), N)


def alone_case(name, termination):
    rc = alone(name, termination)
    return rc, LITE3, lite3_state(ALONE_N, ALONE_SEED), np.zeros((len(rc.names), ALONE_N), dtype=np.float32)


def set_case(names):
    rc = term_set(names)
    return rc, LITE3, lite3_state(ALONE_N, ALONE_SEED), np.zeros((len(rc.names), ALONE_N), dtype=np.float32)


def shaped_case(fx, key, N):
    layout, rc = shape_case(key, fixture_rc(fx, "all"))
    env = shaped_state(N, layout, rc.points_x, rc.points_y, seed=7000 + 10 * sorted(SHAPES).index(key) + N)
    return rc, layout, env, linspace_sums(len(rc.names), N)


def single_step_cases(fx):
    """Every one-launch case of tests/test_hip_rewards.py: (label, config, layout, inputs and state, episode sums before)."""
    for tag in TAGS:
        for N in EVERY_TERM_N:
            for op in (False, True):
                yield (f"{tag} N={N} only_positive={op}",) + every_term_case(fx, tag, N, op)
    for name, t in ALONE_CASES:
        yield (f"alone {name}{' +termination' if t else ''}",) + alone_case(name, t)
    for names in SETS:
        yield ("set " + "+".join(names),) + set_case(names)
    for key in SHAPES:
        for N in SHAPE_N:
            yield (f"{key} N={N}",) + shaped_case(fx, key, N)


# ---------------------------------------------------------------------------------------------- spoiled outputs (CPU proof)
def drop_one(name, env, st, layout: Layout = LITE3):
    """Inputs / state changed so that ONE dof, foot or component no longer contributes to term `name`; False where the term
    is no sum (or its elements cannot be taken out through the inputs)."""
    D0 = (slice(None), 0)
    if name == "action_rate":
        env["actions"][D0] = env["last_actions"][D0]
    elif name == "ang_vel_xy":
        env["base_ang_vel"][D0] = 0
    elif name == "base_height":
        env["foot_positions"][:, 0, 2] = 0
    elif name == "dof_acc":
        env["last_dof_vel"][D0] = env["dof_vel"][D0]
    elif name in ("dof_pos_limits", "stand_still"):
        env["dof_pos"][D0] = env["default_dof_pos"][0]
    elif name in ("dof_vel", "dof_vel_limits"):
        env["dof_vel"][D0] = 0
    elif name == "feet_air_time":
        st["feet_air_time"][D0] = 0
    elif name == "feet_contact_forces":
        env["contact_forces"][:, layout.feet[0]] = 0
    elif name == "feet_slip":
        env["foot_velocities"][D0] = 0
    elif name == "foot_acc":
        env["last_foot_velocities"][D0] = env["foot_velocities"][D0]
    elif name == "hip_pos":
        env["dof_pos"][:, layout.hips[0]] = 0
    elif name in ("power", "powerchange", "torque_limits", "torques"):
        env["torques"][D0] = 0
    elif name == "smooth":
        for k in ("actions", "last_actions", "last_actions_2"):
            env[k][D0] = 0
    elif name == "tracking_lin_vel":
        env["base_lin_vel"][:, 1] = env["commands"][:, 1]
    elif name == "tracking_optimal_footholds":
        env["contact_filt"][D0] = False
    else:
        return False
    return True
