"""First closed-loop measurements: `OnPolicyRunner.learn` on `SurrogateLeggedEnv`, PPO with default arithmetic and with
`gemm_passes=1`, fixed seeds.  Nothing here has a target.

    python deep-tracking-control_amd/tools/closed_loop.py [--envs 4096] [--iters 10] [--out profiles/closed_loop.txt]
    python deep-tracking-control_amd/tools/closed_loop.py --signal        # + the learning-signal run: 256 envs, 30 iterations
    python deep-tracking-control_amd/tools/closed_loop.py --tilt [--out profiles/closed_loop_tilt.txt]
                                                                          # the yaw-only env beside the tilt env (SimConfig.tilt), timing only
    python deep-tracking-control_amd/tools/closed_loop.py --terrain [--out profiles/closed_loop_terrain.txt]
                                                                          # the rough table beside the generated DTC terrain
    python deep-tracking-control_amd/tools/closed_loop.py --actuator [--out profiles/closed_loop_actuator.txt]
                                                                          # the env beside the env with actuator lag and pushes
    python deep-tracking-control_amd/tools/closed_loop.py --flight [--out profiles/closed_loop_flight.txt]
                                                                          # the terrain env beside the one with free flight and crashes
    python deep-tracking-control_amd/tools/closed_loop.py --contacts [--out profiles/closed_loop_contacts.txt]
                                                                          # the terrain env beside the one with leg collisions and stumbles
    python deep-tracking-control_amd/tools/closed_loop.py --balance [--out profiles/closed_loop_balance.txt]
                                                                          # the terrain env beside the one with support-polygon balance and falls

Per run and iteration: the mean step reward (mean of rew_buf over the iteration's 24 steps and all envs), the mean episode length
(the runner's tracker: the last <= 100 finished episodes; "-" before the first one ends) and the mean length of the episodes in flight.
Timing, three interleaved rounds (default, one pass, default, ...), each figure with its spread (min .. max of the three):
  * env-steps/s of the whole loop: host-clock window around learn(iters), closed by one device synchronise, nothing inside it;
  * time per iteration of env.step(), alg.act() and alg.update(): a second learn(iters) in which each of the three calls is a
    host-clock window that ends in a device synchronise (so the three do not overlap, and their sum exceeds the whole loop's time);
  * dtc_sim_step beside the torch restatement of the same step (below: the same arithmetic as torch ops on the same tensors, checked
    against the kernel to 1e-5 before it is timed), alternating, median of --calls windows each.
With --tilt the two runs are the yaw-only env and the tilt env, both over the rough table `synthetic.reward_table()` (on the flat one
the tilt stays level), default arithmetic: the same three interleaved rounds, and dtc_sim_step beside dtc_sim_step_tilt, alternating.
With --terrain the two runs are the env over the rough table and the env on the generated DTC terrain (`SurrogateConfig.terrain`, the
Lite3 grid), default arithmetic, the same three interleaved rounds; then dtc_terrain_generate at the Lite3 grid (6 x 2, 1760 x 1120
cells) and at 10 x 20 beside the numpy restatement tests/terrain_oracle.py on the host, and, on a 6 x 9 grid that holds every family
as one column, the mean terrain level and the share of envs reset per step per family over 200 steps of an untrained policy.
With --actuator the two runs are the yaw-only env over the rough table without and with `SimConfig(actuator=ActuatorConfig())` (the
reference's lag range and push schedule), default arithmetic, the same three interleaved rounds; dtc_sim_step beside
dtc_sim_step_act, alternating; and the mean step reward per iteration of both, for which nothing was tuned.
With --flight the two runs are the env on the generated DTC terrain (the Lite3 grid) without and with
`SimConfig(flight=FlightConfig())`, default arithmetic, the same three interleaved rounds; dtc_sim_step beside dtc_sim_step_fly on
that terrain, alternating; and, on a 6 x 9 grid that holds every family as one column, the share of envs airborne, crashed and
reset per step per family over 200 steps of an untrained policy.  Nothing is asserted and nothing was tuned.
With --contacts the two runs are the env on the generated DTC terrain (the Lite3 grid) without and with
`SimConfig(contacts=ContactConfig())`, default arithmetic and the default reward scales, the same three interleaved rounds;
dtc_sim_step beside dtc_sim_contacts, the launch behind it, on that terrain; on the 6 x 9 one-family-per-column grid the share of
env steps with any leg_contact and with any stumbled per family over 200 steps of an untrained policy; and the learning signal: 256
envs, 30 iterations on a stairs-only terrain with CONTACT_SCALES added to the default scales, the share of env steps with a leg
collision in iterations 1-5 and in iterations 26-30.  Nothing is asserted and nothing was tuned.
With --balance the two runs are the env on the generated DTC terrain (the Lite3 grid) without and with
`SimConfig(balance=BalanceConfig())`, default arithmetic and the default reward scales, the same three interleaved rounds;
dtc_sim_step beside dtc_sim_balance, the launch behind it, on that terrain; on the 6 x 9 one-family-per-column grid the share of
env steps that lean, that end fallen and that end in a reset per family over 200 steps of an untrained policy; and the learning
signal: 256 envs, 30 iterations on the Lite3 terrain with BALANCE_SCALES added to the default scales, the share of env steps
that end fallen in iterations 1-5 and in iterations 26-30.  Nothing is asserted and nothing was tuned.
"""
import argparse
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from dtc_amd import sim as SIM, synthetic  # noqa: E402
from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv  # noqa: E402
from dtc_amd.env.surrogate import _SCALES, BALANCE_SCALES, CONTACT_SCALES  # noqa: E402
from dtc_amd.runners import OnPolicyRunner  # noqa: E402
from dtc_amd.runners.on_policy_runner import _EpisodeTracker  # noqa: E402
from dtc_amd.terrain import FAMILIES, Terrain, TerrainConfig  # noqa: E402

DEV = "cuda"
STEPS = 24
RUNS = (("default", {}), ("gemm_passes=1", dict(gemm_passes=1)))


def rough_env(num_envs, tilt, actuator=None):
    return SurrogateLeggedEnv(num_envs, DEV, SurrogateConfig(sim=SIM.SimConfig(tilt=tilt, actuator=actuator)), synthetic.reward_table(), seed=5)


def make(num_envs, algo, seed=11, tilt=None, terrain=None, steps=STEPS, actuator=None, flight=None, contacts=None, scales=None, balance=None):
    """`tilt` None: the default env on the flat table; False / True: the yaw-only / the tilt env on the rough table (`actuator`, an
    ActuatorConfig: with lag and pushes); `terrain`, a TerrainConfig: the env on the generated terrain (`flight`, a FlightConfig: with
    free flight, landing and crashes; `contacts`, a ContactConfig: with leg collisions and stumbles; `balance`, a BalanceConfig: with
    the support-polygon lean and falls; `scales`: reward scales in place of the default set)."""
    torch.manual_seed(seed)
    if terrain is not None:
        kw = {} if scales is None else dict(reward_scales=dict(scales))
        env = SurrogateLeggedEnv(num_envs, DEV, SurrogateConfig(sim=SIM.SimConfig(flight=flight, contacts=contacts, balance=balance), terrain=terrain, **kw), seed=5)
    else:
        env = SurrogateLeggedEnv(num_envs, DEV, SurrogateConfig(), seed=5) if tilt is None else rough_env(num_envs, tilt, actuator)
    runner = dict(policy_class_name="ActorCriticDecoder", algorithm_class_name="PPO", num_steps_per_env=steps, save_interval=10 ** 9)
    return OnPolicyRunner(env, dict(runner=runner, algorithm=dict(algo), policy=dict()), log_dir=None, device=DEV), env


class Watch:
    """Wraps env.step of a runner: per-iteration reward and episode statistics on the device, no host read inside an iteration."""

    def __init__(self, r, env):
        self.env, self.tracker = env, _EpisodeTracker(env.num_envs, DEV)
        self.sum, self.rows = torch.zeros((), dtype=torch.float64, device=DEV), []
        inner = r.env.step

        def step(actions):
            out = inner(actions)
            self.sum += out[1].double().mean()
            self.tracker.step(out[1], out[2])
            return out
        object.__setattr__(r.env, "step", step)              # on the wrapper itself: its __setattr__ would hand it to the env

    def close_iteration(self):
        m = self.tracker.means()
        self.rows.append((float(self.sum) / STEPS, None if m is None else m[1], float(self.env.episode_length_buf.float().mean())))
        self.sum.zero_()


def learning_curve(num_envs, iters, algo, **kw):
    r, env = make(num_envs, algo, **kw)
    w = Watch(r, env)
    for _ in range(iters):
        r.learn(1)
        w.close_iteration()
    return w.rows


def timed(fn, acc):
    def f(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a, **k)
        torch.cuda.synchronize()
        acc.append(time.perf_counter() - t0)
        return out
    return f


def timing_round(num_envs, iters, algo, tilt=None, terrain=None, actuator=None, flight=None, contacts=None, balance=None):
    r, env = make(num_envs, algo, tilt=tilt, terrain=terrain, actuator=actuator, flight=flight, contacts=contacts, balance=balance)
    r.learn(2)                                                # warm-up: allocations, first launches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r.learn(iters)
    torch.cuda.synchronize()
    whole = time.perf_counter() - t0
    t_env, t_act, t_upd = [], [], []
    object.__setattr__(r.env, "step", timed(r.env.step, t_env))
    r.alg.act, r.alg.update = timed(r.alg.act, t_act), timed(r.alg.update, t_upd)
    r.learn(iters)
    return dict(steps_per_s=num_envs * STEPS * iters / whole, env_ms=1e3 * sum(t_env) / iters, act_ms=1e3 * sum(t_act) / iters,
                update_ms=1e3 * sum(t_upd) / iters)


def torch_sim_step(env, actions, u_cmd):
    """dtc_sim_step as torch ops (include/dtc_hip.h states the arithmetic), in place on the env's tensors."""
    c, t = env.config.sim, env.sim.tables
    N, dt = env.num_envs, c.sim_dt
    lo, hi, dflt = t["dof_pos_limits"][:, 0], t["dof_pos_limits"][:, 1], t["default_dof_pos"]
    J, nom, hip = t["leg_jacobian"], t["foot_nominal"], t["hip_offset"]
    a = torch.clip(actions, -c.clip_actions, c.clip_actions)
    goal = torch.clip(a * c.action_scale + dflt, lo, hi)
    q, qd = env.dof_pos.clone(), env.dof_vel.clone()
    x, y, z, qz, qw = (env.root_states[:, i].clone() for i in (0, 1, 2, 5, 6))
    kp, kd = t["p_gains"] * env.Kp_factors, t["d_gains"] * env.Kd_factors
    hs = env.height_samples
    for _ in range(c.decimation):
        tau = torch.clip((kp * (goal - q + env.motor_offsets) - kd * qd) * env.motor_strengths, -t["torque_limits"], t["torque_limits"])
        qd = qd + tau / c.joint_inertia * dt
        q = q + qd * dt
        out = (q < lo) | (q > hi)
        q, qd = torch.clip(q, lo, hi), torch.where(out, torch.zeros_like(qd), qd)
        p = nom + torch.einsum("lik,nlk->nli", J, (q - dflt).view(N, 4, 3))
        u = torch.einsum("lik,nlk->nli", J, qd.view(N, 4, 3))
        cs, sn = 1 - 2 * qz * qz, 2 * qz * qw
        fx = x[:, None] + cs[:, None] * p[..., 0] - sn[:, None] * p[..., 1]
        fy = y[:, None] + sn[:, None] * p[..., 0] + cs[:, None] * p[..., 1]
        ix = ((fx + c.border_size) / c.horizontal_scale).long().clip(0, hs.shape[0] - 2)
        iy = ((fy + c.border_size) / c.horizontal_scale).long().clip(0, hs.shape[1] - 2)
        h = torch.min(torch.min(hs[ix, iy], hs[ix + 1, iy]), hs[ix, iy + 1]).float() * c.vertical_scale
        bz = (h - p[..., 2]).max(dim=1).values
        ct = (bz[:, None] + p[..., 2] - h) <= c.contact_eps
        m = ct.float()
        nc = m.sum(1)
        pm = (p[..., :2] * m[..., None]).sum(1) / nc[:, None]
        um = (u[..., :2] * m[..., None]).sum(1) / nc[:, None]
        dp, du = p[..., :2] - pm[:, None], u[..., :2] - um[:, None]
        num = ((dp[..., 0] * du[..., 1] - dp[..., 1] * du[..., 0]) * m).sum(1)
        den = ((dp * dp).sum(-1) * m).sum(1)
        w = torch.where(den > c.r_min ** 2, -num / den.clamp_min(1e-30), torch.zeros_like(den))
        vbx, vby = -um[:, 0] + w * pm[:, 1], -um[:, 1] - w * pm[:, 0]
        x, y = x + (cs * vbx - sn * vby) * dt, y + (sn * vbx + cs * vby) * dt
        vz, z = (bz - z) / dt, bz
        zn, wn = qz + 0.5 * dt * w * qw, qw - 0.5 * dt * w * qz
        r = torch.sqrt(zn * zn + wn * wn)
        qz, qw = zn / r, wn / r
    cs, sn = 1 - 2 * qz * qz, 2 * qz * qw
    Vx, Vy = cs * vbx - sn * vby, sn * vbx + cs * vby
    zero = torch.zeros_like(x)
    env.dof_pos.copy_(q), env.dof_vel.copy_(qd), env.torques.copy_(tau), env.actions.copy_(a)
    env.root_states.copy_(torch.stack([x, y, z, zero, zero, qz, qw, Vx, Vy, vz, zero, zero, w], dim=1))
    env.last_base_ang_vel.copy_(env.base_ang_vel)
    env.base_lin_vel.copy_(torch.stack([vbx, vby, vz], dim=1)), env.base_ang_vel.copy_(torch.stack([zero, zero, w], dim=1))
    env.projected_gravity.copy_(torch.stack([zero, zero, zero - 1], dim=1))
    env.base_quat.copy_(torch.stack([zero, zero, qz, qw], dim=1)), env.base_pos.copy_(torch.stack([x, y, z], dim=1))
    rot = lambda vx, vy: (cs[:, None] * vx - sn[:, None] * vy, sn[:, None] * vx + cs[:, None] * vy)         # noqa: E731
    fx, fy = rot(p[..., 0], p[..., 1])
    gx, gy = rot(u[..., 0] - w[:, None] * p[..., 1], u[..., 1] + w[:, None] * p[..., 0])
    env.rigid_body_state[:, env.feet_indices, 0:3] = torch.stack([x[:, None] + fx, y[:, None] + fy, z[:, None] + p[..., 2]], dim=-1)
    env.rigid_body_state[:, env.feet_indices, 7:10] = torch.stack([Vx[:, None] + gx, Vy[:, None] + gy, vz[:, None] + u[..., 2]], dim=-1)
    tx, ty = rot(hip[None, :, 0], hip[None, :, 1])
    env.rigid_body_state[:, env.thigh_indices, 0:3] = torch.stack([x[:, None] + tx, y[:, None] + ty, z[:, None] + hip[None, :, 2]], dim=-1)
    env.contact_forces.zero_()
    env.contact_forces[:, env.feet_indices, 2] = m * (c.mass * c.gravity / nc)[:, None]
    env.episode_length_buf += 1
    for buf, new in ((env.lin_vel_buffer, torch.stack([vbx, vby], dim=1)), (env.ang_vel_buffer, w[:, None]), (env.cmd_buffer, env.commands)):
        buf[:-1] = buf[1:].clone()
        buf[-1] = new
    ids = (env.episode_length_buf % c.resampling_steps == 0).nonzero(as_tuple=False).flatten()             # as the reference: a host read
    if len(ids):
        span = lambda r, v: (r[1] - r[0]) * v + r[0]                                                         # noqa: E731
        env.commands[ids, 0], env.commands[ids, 1] = span(c.lin_vel_x, u_cmd[ids, 0]), span(c.lin_vel_y, u_cmd[ids, 1])
        env.commands[ids, 3 if c.heading_command else 2] = span(c.heading if c.heading_command else c.ang_vel_yaw, u_cmd[ids, 2])
        env.commands[ids, :2] *= (torch.norm(env.commands[ids, :2], dim=1) > 0.1).unsqueeze(1)
    contact = env.contact_forces[:, env.feet_indices, 2] > 1.
    env.contact_filt.copy_(contact | env.last_contacts)
    env.last_contacts.copy_(contact)


CHECKED = ("dof_state", "root_states", "torques", "base_lin_vel", "base_ang_vel", "rigid_body_state", "contact_forces", "commands",
           "lin_vel_buffer", "cmd_buffer", "contact_filt", "episode_length_buf")


def sim_step_probe(num_envs, calls):
    envs = [SurrogateLeggedEnv(num_envs, DEV, SurrogateConfig(), seed=5) for _ in range(2)]
    g = torch.Generator(device=DEV).manual_seed(3)
    for e in envs:
        e.reset()
    worst = 0.0
    for _ in range(5):                                         # same steps both ways, compared
        a, u = torch.randn(num_envs, 12, generator=g, device=DEV), torch.rand(num_envs, 3, generator=g, device=DEV)
        envs[0].sim.step(envs[0], a, u)
        torch_sim_step(envs[1], a, u)
        for name in CHECKED:
            x, y = getattr(envs[0], name).double(), getattr(envs[1], name).double()
            worst = max(worst, float(((x - y).abs() / (1 + y.abs())).max()))
        for name in CHECKED:                                   # keep the two on one trajectory
            getattr(envs[1], name).copy_(getattr(envs[0], name))
    assert worst <= 1e-5, f"the torch restatement differs from dtc_sim_step by {worst:.2e}"
    t_k, t_t = [], []
    for i in range(calls + 20):
        a, u = torch.randn(num_envs, 12, generator=g, device=DEV), torch.rand(num_envs, 3, generator=g, device=DEV)
        for acc, fn, e in ((t_k, lambda: envs[0].sim.step(envs[0], a, u), 0), (t_t, lambda: torch_sim_step(envs[1], a, u), 1)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 20:
                acc.append(1e6 * (time.perf_counter() - t0))
    return statistics.median(t_k), statistics.median(t_t), worst


def tilt_probe(num_envs, calls):
    """dtc_sim_step beside dtc_sim_step_tilt on the rough table, same actions, alternating: us per call (median)."""
    envs = [rough_env(num_envs, tilt) for tilt in (False, True)]
    g = torch.Generator(device=DEV).manual_seed(3)
    for e in envs:
        e.reset()
    acc = ([], [])
    for i in range(calls + 20):
        a, u = torch.randn(num_envs, 12, generator=g, device=DEV), torch.rand(num_envs, 3, generator=g, device=DEV)
        for t, e in zip(acc, envs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.sim.step(e, a, u)
            torch.cuda.synchronize()
            if i >= 20:
                t.append(1e6 * (time.perf_counter() - t0))
    tilted = float((envs[1].projected_gravity[:, :2].abs().amax(dim=1) > 0.01).float().mean())
    return statistics.median(acc[0]), statistics.median(acc[1]), tilted


def tilt_report(args):
    runs = (("yaw only", False), ("tilt", True))
    rounds = {tag: [] for tag, _ in runs}
    for _ in range(3):
        for tag, tilt in runs:
            rounds[tag].append(timing_round(args.envs, args.iters, {}, tilt=tilt))
    lines = [f"closed loop on SurrogateLeggedEnv over the rough table, yaw-only base beside SimConfig(tilt=True): {args.envs} envs x {STEPS} steps "
             f"per iteration, {args.iters} iterations, PPO, default arithmetic, fixed seeds",
             "", "three interleaved rounds, median (min .. max):"]
    for tag, _ in runs:
        rs = rounds[tag]
        lines.append(f"  {tag:9s} env-steps/s, whole loop {spread([r['steps_per_s'] for r in rs], '{:.0f}')}")
        lines.append(f"  {'':9s} ms per iteration, each call closed by a synchronise: env.step x{STEPS} {spread([r['env_ms'] for r in rs], '{:.2f}')}"
                     f" | act() x{STEPS} {spread([r['act_ms'] for r in rs], '{:.2f}')} | update() {spread([r['update_ms'] for r in rs], '{:.2f}')}")
    probes = [tilt_probe(args.envs, args.calls) for _ in range(3)]
    lines += ["", f"one surrogate step at {args.envs} envs, us per call (host clock, closed by a synchronise), alternating, three rounds:",
              f"  dtc_sim_step (yaw only)  {spread([p[0] for p in probes])}",
              f"  dtc_sim_step_tilt        {spread([p[1] for p in probes])}   (envs tilted by more than 0.01 at the end: "
              f"{100 * statistics.mean(p[2] for p in probes):.0f} %)"]
    return lines


def actuator_probe(num_envs, calls):
    """dtc_sim_step beside dtc_sim_step_act on the rough table, same actions, alternating: us per call (median).  The lag slots are
    drawn on the host as in production; a push is drawn on two of every three calls (far more often than the reference's schedule),
    so that a push is pending in every call."""
    envs = [rough_env(num_envs, False, act) for act in (None, SIM.ActuatorConfig())]
    g = torch.Generator(device=DEV).manual_seed(3)
    for e in envs:
        e.reset()
    acc = ([], [])
    for i in range(calls + 20):
        a, u = torch.randn(num_envs, 12, generator=g, device=DEV), torch.rand(num_envs, 3, generator=g, device=DEV)
        for t, e, kw in zip(acc, envs, ({}, dict(push=i % 3 in (0, 1)))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.sim.step(e, a, u, **kw)
            torch.cuda.synchronize()
            if i >= 20:
                t.append(1e6 * (time.perf_counter() - t0))
    return statistics.median(acc[0]), statistics.median(acc[1])


def actuator_report(args):
    runs = (("no actuator", None), ("actuator", SIM.ActuatorConfig()))
    rounds = {tag: [] for tag, _ in runs}
    for _ in range(3):
        for tag, act in runs:
            rounds[tag].append(timing_round(args.envs, args.iters, {}, tilt=False, actuator=act))
    lines = [f"closed loop on SurrogateLeggedEnv over the rough table, without and with SimConfig(actuator=ActuatorConfig()) (lag slots 1..4, a "
             f"push of up to 1 m/s every 15 s on two consecutive steps, decay 0.2 s): {args.envs} envs x {STEPS} steps per iteration, "
             f"{args.iters} iterations, PPO, default arithmetic, fixed seeds",
             "", "three interleaved rounds, median (min .. max):"]
    for tag, _ in runs:
        rs = rounds[tag]
        lines.append(f"  {tag:11s} env-steps/s, whole loop {spread([r['steps_per_s'] for r in rs], '{:.0f}')}")
        lines.append(f"  {'':11s} ms per iteration, each call closed by a synchronise: env.step x{STEPS} {spread([r['env_ms'] for r in rs], '{:.2f}')}"
                     f" | act() x{STEPS} {spread([r['act_ms'] for r in rs], '{:.2f}')} | update() {spread([r['update_ms'] for r in rs], '{:.2f}')}")
    probes = [actuator_probe(args.envs, args.calls) for _ in range(3)]
    lines += ["", f"one surrogate step at {args.envs} envs, us per call (host clock, closed by a synchronise), alternating, three rounds:",
              f"  dtc_sim_step      {spread([p[0] for p in probes])}",
              f"  dtc_sim_step_act  {spread([p[1] for p in probes])}   (a new push on two of every three calls, one pending in every call; the host's lag draws included)",
              "", f"mean step reward per iteration, {args.iters} iterations (the reference's schedule: pushes at env steps 1, 750, 751, 1500, ..., so in a "
              f"short run the lag is what acts); nothing was tuned for the disturbances:"]
    for tag, act in runs:
        rows = learning_curve(args.envs, args.iters, {}, tilt=False, actuator=act)
        lines.append(f"  {tag:11s} " + " ".join(f"{r[0]:+.5f}" for r in rows))
    lines += ["", "bench.py runs no env step: its headline is not re-measured here."]
    return lines


def flight_probe(num_envs, calls):
    """dtc_sim_step beside dtc_sim_step_fly on the generated Lite3 terrain, same actions, alternating: us per call (median), and the
    share of envs the flight env has in the air at the end."""
    envs = [SurrogateLeggedEnv(num_envs, DEV, SurrogateConfig(sim=SIM.SimConfig(flight=f), terrain=TerrainConfig(seed=1)), seed=5)
            for f in (None, SIM.FlightConfig())]
    g = torch.Generator(device=DEV).manual_seed(3)
    for e in envs:
        e.reset()
    acc = ([], [])
    for i in range(calls + 20):
        a, u = torch.randn(num_envs, 12, generator=g, device=DEV), torch.rand(num_envs, 3, generator=g, device=DEV)
        for t, e in zip(acc, envs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.sim.step(e, a, u)
            torch.cuda.synchronize()
            if i >= 20:
                t.append(1e6 * (time.perf_counter() - t0))
    return statistics.median(acc[0]), statistics.median(acc[1]), float(envs[1].airborne.float().mean())


def flight_family_probe(num_envs, steps=200, rollout=25):
    """An untrained policy on a 6 x 9 grid whose column j is family j, with flight: per family the share of its envs airborne (at the
    end of the step), crashed and reset per step, and the mean terrain level at the start and at the end.  Rollouts without updates;
    everything is summed on the device and read once."""
    cfg = TerrainConfig(num_rows=6, num_cols=9, terrain_proportions=tuple([1 / 9] * 9), seed=1)
    r, env = make(num_envs, {}, terrain=cfg, steps=rollout, flight=SIM.FlightConfig())
    types = env.terrain_types
    count = torch.bincount(types, minlength=9).double()
    level0 = torch.zeros(9, dtype=torch.float64, device=DEV).index_add_(0, types, env.terrain_levels.double()) / count
    sums = torch.zeros(3, 9, dtype=torch.float64, device=DEV)
    inner = r.env.step

    def step(actions):
        out = inner(actions)
        for row, flag in zip(sums, (env.airborne, env.crashed, out[2])):
            row.index_add_(0, types, flag.double())
        return out
    object.__setattr__(r.env, "step", step)
    state = dict(obs_dict=r.env.get_observations(), rew_buf=r.env.get_reward_buf())
    for _ in range(steps // rollout):
        r._collect(state, None, [])
        r.alg.storage.clear()
    level1 = torch.zeros(9, dtype=torch.float64, device=DEV).index_add_(0, types, env.terrain_levels.double()) / count
    return (sums / count / (steps // rollout * rollout)).tolist(), level0.tolist(), level1.tolist(), count.tolist()


def flight_report(args):
    lite3 = TerrainConfig(seed=1)
    runs = (("no flight", None), ("flight", SIM.FlightConfig()))
    rounds = {tag: [] for tag, _ in runs}
    for _ in range(3):
        for tag, f in runs:
            rounds[tag].append(timing_round(args.envs, args.iters, {}, terrain=lite3, flight=f))
    lines = [f"closed loop on SurrogateLeggedEnv on the generated DTC terrain (the Lite3 grid), without and with SimConfig(flight=FlightConfig()) "
             f"(gravity 9.81, max_step_up 0.3 m, crash_force 200 N): {args.envs} envs x {STEPS} steps per iteration, {args.iters} iterations, PPO, "
             f"default arithmetic, fixed seeds",
             "", "three interleaved rounds, median (min .. max):"]
    for tag, _ in runs:
        rs = rounds[tag]
        lines.append(f"  {tag:11s} env-steps/s, whole loop {spread([r['steps_per_s'] for r in rs], '{:.0f}')}")
        lines.append(f"  {'':11s} ms per iteration, each call closed by a synchronise: env.step x{STEPS} {spread([r['env_ms'] for r in rs], '{:.2f}')}"
                     f" | act() x{STEPS} {spread([r['act_ms'] for r in rs], '{:.2f}')} | update() {spread([r['update_ms'] for r in rs], '{:.2f}')}")
    probes = [flight_probe(args.envs, args.calls) for _ in range(3)]
    lines += ["", f"one surrogate step at {args.envs} envs on that terrain, us per call (host clock, closed by a synchronise), alternating, three rounds:",
              f"  dtc_sim_step      {spread([p[0] for p in probes])}",
              f"  dtc_sim_step_fly  {spread([p[1] for p in probes])}   (envs in the air at the end, under random actions: "
              f"{100 * statistics.mean(p[2] for p in probes):.1f} %)"]
    share, level0, level1, count = flight_family_probe(args.envs)
    lines += ["", f"an untrained policy with flight, {args.envs} envs on a 6 x 9 grid (column j = family j, max_init_terrain_level 5), 200 steps, no update;",
              "per step, the share of a family's envs that end it airborne, that crashed in it, and that were reset in it:",
              "  family              envs   airborne   crashed   reset     mean terrain_level start -> end"]
    for j, name in enumerate(FAMILIES):
        lines.append(f"  {name:19s} {int(count[j]):5d}   {100 * share[0][j]:6.2f} %   {100 * share[1][j]:5.2f} %   {100 * share[2][j]:5.2f} %   "
                     f"{level0[j]:.3f} -> {level1[j]:.3f}")
    lines += ["", "bench.py runs no env step: its headline is not re-measured here."]
    return lines


def contacts_probe(num_envs, calls):
    """dtc_sim_step, then dtc_sim_contacts on what it wrote, on the generated Lite3 terrain under random actions: us per call of each
    (median), and the share of envs with any leg contact and with any stumble at the end."""
    env = SurrogateLeggedEnv(num_envs, DEV, SurrogateConfig(sim=SIM.SimConfig(contacts=SIM.ContactConfig()), terrain=TerrainConfig(seed=1)), seed=5)
    g = torch.Generator(device=DEV).manual_seed(3)
    env.reset()
    acc = ([], [])
    for i in range(calls + 20):
        a, u = torch.randn(num_envs, 12, generator=g, device=DEV), torch.rand(num_envs, 3, generator=g, device=DEV)
        for t, fn in zip(acc, (lambda: env.sim.step(env, a, u), lambda: env.sim.contacts(env))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 20:
                t.append(1e6 * (time.perf_counter() - t0))
    return (statistics.median(acc[0]), statistics.median(acc[1]), float(env.leg_contact.any(dim=1).float().mean()),
            float(env.stumbled.any(dim=1).float().mean()))


def contacts_family_probe(num_envs, steps=200, rollout=25):
    """An untrained policy on a 6 x 9 grid whose column j is family j, with contacts: per family the share of env steps with any
    leg_contact, with any stumbled, and with a reset.  Rollouts without updates; everything is summed on the device and read once."""
    cfg = TerrainConfig(num_rows=6, num_cols=9, terrain_proportions=tuple([1 / 9] * 9), seed=1)
    r, env = make(num_envs, {}, terrain=cfg, steps=rollout, contacts=SIM.ContactConfig())
    types = env.terrain_types
    count = torch.bincount(types, minlength=9).double()
    sums = torch.zeros(3, 9, dtype=torch.float64, device=DEV)
    inner = r.env.step

    def step(actions):
        out = inner(actions)
        for row, flag in zip(sums, (env.leg_contact.any(dim=1), env.stumbled.any(dim=1), out[2])):
            row.index_add_(0, types, flag.double())
        return out
    object.__setattr__(r.env, "step", step)
    state = dict(obs_dict=r.env.get_observations(), rew_buf=r.env.get_reward_buf())
    for _ in range(steps // rollout):
        r._collect(state, None, [])
        r.alg.storage.clear()
    return (sums / count / (steps // rollout * rollout)).tolist(), count.tolist()


STAIRS_ONLY = (0.0, 0.0, 0.5, 0.5)                            # column 0: stairs down, column 1: stairs up


def collision_curve(num_envs=256, iters=30):
    """The learning signal of the collision term: PPO on a stairs-only terrain (the Lite3 grid) with CONTACT_SCALES added to the
    default scales.  Per iteration: the share of env steps with any leg_contact, with any stumbled, and the mean step reward."""
    r, env = make(num_envs, {}, terrain=TerrainConfig(terrain_proportions=STAIRS_ONLY, seed=1), contacts=SIM.ContactConfig(),
                  scales=dict(_SCALES, **CONTACT_SCALES))
    sums, rows = torch.zeros(3, dtype=torch.float64, device=DEV), []
    inner = r.env.step

    def step(actions):
        out = inner(actions)
        sums[0] += env.leg_contact.any(dim=1).double().mean()
        sums[1] += env.stumbled.any(dim=1).double().mean()
        sums[2] += out[1].double().mean()
        return out
    object.__setattr__(r.env, "step", step)
    for _ in range(iters):
        r.learn(1)
        rows.append(tuple((sums / STEPS).tolist()))
        sums.zero_()
    return rows


def contacts_report(args):
    lite3 = TerrainConfig(seed=1)
    runs = (("no contacts", None), ("contacts", SIM.ContactConfig()))
    rounds = {tag: [] for tag, _ in runs}
    for _ in range(3):
        for tag, c in runs:
            rounds[tag].append(timing_round(args.envs, args.iters, {}, terrain=lite3, contacts=c))
    c = SIM.ContactConfig()
    lines = [f"closed loop on SurrogateLeggedEnv on the generated DTC terrain (the Lite3 grid), without and with SimConfig(contacts=ContactConfig()) "
             f"(body_radius {c.body_radius} m, stiffness {c.stiffness:.0f} N/m, max_force {c.max_force:.0f} N, probe {c.probe} m, stumble_height "
             f"{c.stumble_height} m, wall_damping {c.wall_damping:.0f} N s/m, min_speed {c.min_speed} m/s): {args.envs} envs x {STEPS} steps per "
             f"iteration, {args.iters} iterations, PPO, default arithmetic, the default reward scales, fixed seeds",
             "", "three interleaved rounds, median (min .. max):"]
    for tag, _ in runs:
        rs = rounds[tag]
        lines.append(f"  {tag:11s} env-steps/s, whole loop {spread([r['steps_per_s'] for r in rs], '{:.0f}')}")
        lines.append(f"  {'':11s} ms per iteration, each call closed by a synchronise: env.step x{STEPS} {spread([r['env_ms'] for r in rs], '{:.2f}')}"
                     f" | act() x{STEPS} {spread([r['act_ms'] for r in rs], '{:.2f}')} | update() {spread([r['update_ms'] for r in rs], '{:.2f}')}")
    probes = [contacts_probe(args.envs, args.calls) for _ in range(3)]
    lines += ["", f"one surrogate step and the contact launch behind it at {args.envs} envs on that terrain, us per call (host clock, each closed by a "
              "synchronise), three rounds:",
              f"  dtc_sim_step      {spread([p[0] for p in probes])}",
              f"  dtc_sim_contacts  {spread([p[1] for p in probes])}   (envs with any leg contact / any stumble at the end, under random actions: "
              f"{100 * statistics.mean(p[2] for p in probes):.1f} % / {100 * statistics.mean(p[3] for p in probes):.1f} %)"]
    share, count = contacts_family_probe(args.envs)
    lines += ["", f"an untrained policy with contacts, {args.envs} envs on a 6 x 9 grid (column j = family j, max_init_terrain_level 5), 200 steps, no update;",
              "the share of a family's env steps with any leg_contact, with any stumbled, and with a reset:",
              "  family              envs   leg_contact   stumbled   reset"]
    for j, name in enumerate(FAMILIES):
        lines.append(f"  {name:19s} {int(count[j]):5d}   {100 * share[0][j]:8.2f} %   {100 * share[1][j]:6.2f} %   {100 * share[2][j]:5.2f} %")
    rows = collision_curve()
    first, last = statistics.mean(r[0] for r in rows[:5]), statistics.mean(r[0] for r in rows[25:30])
    lines += ["", "learning signal: 256 envs, 30 iterations, PPO, a stairs-only terrain (the Lite3 grid, stairs down and stairs up), the default scales "
              f"plus CONTACT_SCALES {CONTACT_SCALES}; per iteration the share of env steps with any leg_contact:",
              "  " + " ".join(f"{100 * r[0]:.2f}" for r in rows) + "   [%]",
              "  with any stumbled:",
              "  " + " ".join(f"{100 * r[1]:.2f}" for r in rows) + "   [%]",
              "  mean step reward:",
              "  " + " ".join(f"{r[2]:+.5f}" for r in rows),
              f"  leg collisions, iterations 1-5: {100 * first:.3f} %   iterations 26-30: {100 * last:.3f} %   difference: {100 * (last - first):+.3f} points"]
    lines += ["", "bench.py runs no env step: its headline is not re-measured here."]
    return lines


def balance_probe(num_envs, calls):
    """dtc_sim_step, then dtc_sim_balance on what it wrote, on the generated Lite3 terrain under random actions: us per call of each
    (median), and the share of envs that lean and that are fallen at the end."""
    env = SurrogateLeggedEnv(num_envs, DEV, SurrogateConfig(sim=SIM.SimConfig(balance=SIM.BalanceConfig()), terrain=TerrainConfig(seed=1)), seed=5)
    g = torch.Generator(device=DEV).manual_seed(3)
    env.reset()
    acc = ([], [])
    for i in range(calls + 20):
        a, u = torch.randn(num_envs, 12, generator=g, device=DEV), torch.rand(num_envs, 3, generator=g, device=DEV)
        for t, fn in zip(acc, (lambda: env.sim.step(env, a, u), lambda: env.sim.balance(env))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 20:
                t.append(1e6 * (time.perf_counter() - t0))
    return (statistics.median(acc[0]), statistics.median(acc[1]), float(env.lean[:, :2].any(dim=1).float().mean()), float(env.fallen.float().mean()))


def balance_family_probe(num_envs, steps=200, rollout=25):
    """An untrained policy on a 6 x 9 grid whose column j is family j, with balance: per family the share of env steps that lean,
    that end fallen, and that end in a reset.  Rollouts without updates; everything is summed on the device and read once."""
    cfg = TerrainConfig(num_rows=6, num_cols=9, terrain_proportions=tuple([1 / 9] * 9), seed=1)
    r, env = make(num_envs, {}, terrain=cfg, steps=rollout, balance=SIM.BalanceConfig())
    types = env.terrain_types
    count = torch.bincount(types, minlength=9).double()
    sums = torch.zeros(3, 9, dtype=torch.float64, device=DEV)
    inner, leaning = r.env.step, [None]
    balance = env.sim.balance

    def launch(e):                                            # the lean as the launch leaves it: the reset behind it clears a fallen env's
        balance(e)
        leaning[0] = e.lean[:, :2].any(dim=1)
    env.sim.balance = launch

    def step(actions):
        out = inner(actions)
        for row, flag in zip(sums, (leaning[0], env.fallen, out[2])):
            row.index_add_(0, types, flag.double())
        return out
    object.__setattr__(r.env, "step", step)
    state = dict(obs_dict=r.env.get_observations(), rew_buf=r.env.get_reward_buf())
    for _ in range(steps // rollout):
        r._collect(state, None, [])
        r.alg.storage.clear()
    return (sums / count / (steps // rollout * rollout)).tolist(), count.tolist()


def fall_curve(num_envs=256, iters=30):
    """The learning signal of a fall: PPO on the Lite3 terrain with BALANCE_SCALES added to the default scales.  Per iteration:
    the share of env steps that end fallen (the mean of extras["episode"]["fall_rate"] over the rollout), that end in a reset, and
    the mean step reward."""
    r, env = make(num_envs, {}, terrain=TerrainConfig(seed=1), balance=SIM.BalanceConfig(), scales=dict(_SCALES, **BALANCE_SCALES))
    sums, rows = torch.zeros(3, dtype=torch.float64, device=DEV), []
    inner = r.env.step

    def step(actions):
        out = inner(actions)
        sums[0] += out[3]["episode"]["fall_rate"].double()
        sums[1] += out[2].double().mean()
        sums[2] += out[1].double().mean()
        return out
    object.__setattr__(r.env, "step", step)
    for _ in range(iters):
        r.learn(1)
        rows.append(tuple((sums / STEPS).tolist()))
        sums.zero_()
    return rows


def balance_report(args):
    lite3 = TerrainConfig(seed=1)
    runs = (("no balance", None), ("balance", SIM.BalanceConfig()))
    rounds = {tag: [] for tag, _ in runs}
    for _ in range(3):
        for tag, b in runs:
            rounds[tag].append(timing_round(args.envs, args.iters, {}, terrain=lite3, balance=b))
    b = SIM.BalanceConfig()
    lines = [f"closed loop on SurrogateLeggedEnv on the generated DTC terrain (the Lite3 grid), without and with SimConfig(balance=BalanceConfig()) "
             f"(gravity {b.gravity} m/s^2, h_min {b.h_min} m, lean_eps {b.lean_eps} rad, fall_angle {b.fall_angle} rad, fall_force {b.fall_force:.0f} N, "
             f"com_offset {b.com_offset}): {args.envs} envs x {STEPS} steps per iteration, {args.iters} iterations, PPO, default arithmetic, the "
             "default reward scales, fixed seeds", "", "three interleaved rounds, median (min .. max):"]
    for tag, _ in runs:
        rs = rounds[tag]
        lines.append(f"  {tag:11s} env-steps/s, whole loop {spread([r['steps_per_s'] for r in rs], '{:.0f}')}")
        lines.append(f"  {'':11s} ms per iteration, each call closed by a synchronise: env.step x{STEPS} {spread([r['env_ms'] for r in rs], '{:.2f}')}"
                     f" | act() x{STEPS} {spread([r['act_ms'] for r in rs], '{:.2f}')} | update() {spread([r['update_ms'] for r in rs], '{:.2f}')}")
    probes = [balance_probe(args.envs, args.calls) for _ in range(3)]
    lines += ["", f"one surrogate step and the balance launch behind it at {args.envs} envs on that terrain, us per call (host clock, each closed by a "
              "synchronise), three rounds:",
              f"  dtc_sim_step     {spread([p[0] for p in probes])}",
              f"  dtc_sim_balance  {spread([p[1] for p in probes])}   (envs that lean / are fallen at the end, under random actions with no reset between: "
              f"{100 * statistics.mean(p[2] for p in probes):.1f} % / {100 * statistics.mean(p[3] for p in probes):.1f} %)"]
    share, count = balance_family_probe(args.envs)
    lines += ["", f"an untrained policy with balance, {args.envs} envs on a 6 x 9 grid (column j = family j, max_init_terrain_level 5), 200 steps, no update;",
              "the share of a family's env steps that lean, that end fallen, and that end in a reset:",
              "  family              envs   leaning    fallen    reset"]
    for j, name in enumerate(FAMILIES):
        lines.append(f"  {name:19s} {int(count[j]):5d}   {100 * share[0][j]:6.2f} %   {100 * share[1][j]:5.2f} %   {100 * share[2][j]:5.2f} %")
    rows = fall_curve()
    first, last = statistics.mean(r[0] for r in rows[:5]), statistics.mean(r[0] for r in rows[25:30])
    lines += ["", "learning signal: 256 envs, 30 iterations, PPO, the Lite3 terrain, the default scales "
              f"plus BALANCE_SCALES {BALANCE_SCALES}; per iteration the share of env steps that end fallen (fall_rate):",
              "  " + " ".join(f"{100 * r[0]:.2f}" for r in rows) + "   [%]",
              "  that end in a reset:",
              "  " + " ".join(f"{100 * r[1]:.2f}" for r in rows) + "   [%]",
              "  mean step reward:",
              "  " + " ".join(f"{r[2]:+.5f}" for r in rows),
              f"  fall_rate, iterations 1-5: {100 * first:.3f} %   iterations 26-30: {100 * last:.3f} %   difference: {100 * (last - first):+.3f} points"]
    lines += ["", "bench.py runs no env step: its headline is not re-measured here."]
    return lines


ALL_FAMILIES = (0.1, 0.1, 0.1, 0.1, 0.15, 0.15, 0.1, 0.1, 0.1)


def generation_probe(cfg, calls):
    """dtc_terrain_generate in place, us per call (host clock, closed by a synchronise; median), and the numpy restatement's seconds for one table."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))
    import terrain_oracle as O
    t = Terrain(cfg, DEV)
    acc = []
    for i in range(calls + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.generate(seed=i)
        torch.cuda.synchronize()
        if i >= 5:
            acc.append(1e6 * (time.perf_counter() - t0))
    k = O.config(horizontal_scale=cfg.horizontal_scale, vertical_scale=cfg.vertical_scale, border_size=cfg.border_size,
                 curriculum=cfg.curriculum, terrain_length=cfg.terrain_length, terrain_width=cfg.terrain_width, num_rows=cfg.num_rows,
                 num_cols=cfg.num_cols, terrain_proportions=cfg.terrain_proportions, seed=calls + 4)
    t0 = time.perf_counter()
    want = O.generate(k)
    host = time.perf_counter() - t0
    same = bool((t.height_field_raw.cpu().numpy() == want["table"]).all())
    return statistics.median(acc), host, same, (t.tot_rows, t.tot_cols)


def family_probe(num_envs, steps=200, rollout=25):
    """An untrained policy on a 6 x 9 grid whose column j is family j: per family the mean terrain level at the start and at the end
    and the share of its envs reset per step.  Rollouts without updates; everything is summed on the device and read once."""
    cfg = TerrainConfig(num_rows=6, num_cols=9, terrain_proportions=tuple([1 / 9] * 9), seed=1)
    r, env = make(num_envs, {}, terrain=cfg, steps=rollout)
    types = env.terrain_types
    count = torch.bincount(types, minlength=9).double()
    level0 = torch.zeros(9, dtype=torch.float64, device=DEV).index_add_(0, types, env.terrain_levels.double()) / count
    resets = torch.zeros(9, dtype=torch.float64, device=DEV)
    inner = r.env.step

    def step(actions):
        out = inner(actions)
        resets.index_add_(0, types, out[2].double())
        return out
    object.__setattr__(r.env, "step", step)
    state = dict(obs_dict=r.env.get_observations(), rew_buf=r.env.get_reward_buf())
    for _ in range(steps // rollout):
        r._collect(state, None, [])
        r.alg.storage.clear()
    level1 = torch.zeros(9, dtype=torch.float64, device=DEV).index_add_(0, types, env.terrain_levels.double()) / count
    return level0.tolist(), level1.tolist(), (resets / count / (steps // rollout * rollout)).tolist(), count.tolist()


def terrain_report(args):
    lite3 = TerrainConfig(seed=1)
    runs = (("rough table", dict(tilt=False)), ("terrain", dict(terrain=lite3)))
    rounds = {tag: [] for tag, _ in runs}
    for _ in range(3):
        for tag, kw in runs:
            rounds[tag].append(timing_round(args.envs, args.iters, {}, **kw))
    lines = [f"closed loop on SurrogateLeggedEnv over the rough table beside SurrogateConfig(terrain=TerrainConfig()), the Lite3 grid: "
             f"{args.envs} envs x {STEPS} steps per iteration, {args.iters} iterations, PPO, default arithmetic, fixed seeds",
             "", "three interleaved rounds, median (min .. max):"]
    for tag, _ in runs:
        rs = rounds[tag]
        lines.append(f"  {tag:11s} env-steps/s, whole loop {spread([r['steps_per_s'] for r in rs], '{:.0f}')}")
        lines.append(f"  {'':11s} ms per iteration, each call closed by a synchronise: env.step x{STEPS} {spread([r['env_ms'] for r in rs], '{:.2f}')}"
                     f" | act() x{STEPS} {spread([r['act_ms'] for r in rs], '{:.2f}')} | update() {spread([r['update_ms'] for r in rs], '{:.2f}')}")
    lines += ["", "dtc_terrain_generate in place, us per call (host clock, closed by a synchronise), three rounds; the numpy restatement "
              "(tests/terrain_oracle.py) on the host, ms:"]
    for tag, cfg in (("Lite3 6 x 2", lite3), ("10 x 20", TerrainConfig(num_rows=10, num_cols=20, terrain_proportions=ALL_FAMILIES, seed=1))):
        probes = [generation_probe(cfg, args.calls) for _ in range(3)]
        rows, cols = probes[0][3]
        lines.append(f"  {tag:11s} {rows} x {cols} cells: kernel {spread([p[0] for p in probes])} us | numpy {spread([1e3 * p[1] for p in probes])} ms"
                     f" | tables equal: {all(p[2] for p in probes)}")
    level0, level1, share, count = family_probe(args.envs)
    lines += ["", f"an untrained policy, {args.envs} envs on a 6 x 9 grid (column j = family j, max_init_terrain_level 5), 200 steps, no update:",
              "  family              envs   mean terrain_level start -> end   envs reset per step"]
    for j, name in enumerate(FAMILIES):
        lines.append(f"  {name:19s} {int(count[j]):5d}   {level0[j]:.3f} -> {level1[j]:.3f}                     {100 * share[j]:.2f} %")
    return lines


def spread(vals, fmt="{:.1f}"):
    return f"{fmt.format(statistics.median(vals))} ({fmt.format(min(vals))} .. {fmt.format(max(vals))})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--signal", action="store_true")
    ap.add_argument("--tilt", action="store_true")
    ap.add_argument("--terrain", action="store_true")
    ap.add_argument("--actuator", action="store_true")
    ap.add_argument("--flight", action="store_true")
    ap.add_argument("--contacts", action="store_true")
    ap.add_argument("--balance", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.tilt or args.terrain or args.actuator or args.flight or args.contacts or args.balance:
        report = (tilt_report if args.tilt else terrain_report if args.terrain else actuator_report if args.actuator else
                  flight_report if args.flight else contacts_report if args.contacts else balance_report)
        text = "\n".join(report(args)) + "\n"
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text)
        return
    lines = [f"closed loop on SurrogateLeggedEnv: {args.envs} envs x {STEPS} steps per iteration, {args.iters} iterations, PPO, fixed seeds",
             "", "iteration: mean step reward | mean episode length (finished, last <= 100) | mean length in flight"]
    for tag, algo in RUNS:
        lines.append(f"  {tag}")
        for i, (rw, ln, fl) in enumerate(learning_curve(args.envs, args.iters, algo), 1):
            lines.append(f"    {i:3d}  {rw:+.6f} | {'-' if ln is None else f'{ln:.1f}'} | {fl:.1f}")
    rounds = {tag: [] for tag, _ in RUNS}
    for _ in range(3):
        for tag, algo in RUNS:
            rounds[tag].append(timing_round(args.envs, args.iters, algo))
    lines += ["", "three interleaved rounds, median (min .. max):"]
    for tag, _ in RUNS:
        rs = rounds[tag]
        lines.append(f"  {tag:14s} env-steps/s, whole loop {spread([r['steps_per_s'] for r in rs], '{:.0f}')}")
        lines.append(f"  {'':14s} ms per iteration, each call closed by a synchronise: env.step x{STEPS} {spread([r['env_ms'] for r in rs], '{:.2f}')}"
                     f" | act() x{STEPS} {spread([r['act_ms'] for r in rs], '{:.2f}')} | update() {spread([r['update_ms'] for r in rs], '{:.2f}')}")
    probes = [sim_step_probe(args.envs, args.calls) for _ in range(3)]
    lines += ["", f"one surrogate step at {args.envs} envs, us per call (host clock, closed by a synchronise), three rounds:",
              f"  dtc_sim_step (one launch)      {spread([p[0] for p in probes])}",
              f"  torch restatement of the step  {spread([p[1] for p in probes])}   (largest difference to the kernel: {max(p[2] for p in probes):.1e})"]
    if args.signal:
        rows = learning_curve(256, 30, {})
        first, last = statistics.mean(r[0] for r in rows[:5]), statistics.mean(r[0] for r in rows[25:30])
        lines += ["", "learning signal: 256 envs, 30 iterations, default arithmetic, mean step reward per iteration:",
                  "  " + " ".join(f"{r[0]:+.5f}" for r in rows),
                  f"  iterations 1-5: {first:+.6f}   iterations 26-30: {last:+.6f}   difference: {last - first:+.6f}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
