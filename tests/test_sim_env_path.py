"""SurrogateLeggedEnv on the GPU: 16 envs x 40 steps with a 12-step episode limit, every draw an input.  After every step the
tensors dtc_sim_step writes are compared bit for bit with tests/sim_oracle.py run on the env's own state before the step (so the
surrogate is checked on state that evolves and resets), the env-side bookkeeping is checked against its definition, and time-out
resets, base-height terminations and command resamples are all seen.  One step runs under torch's sync debug mode "error"."""
import numpy as np
import pytest
import torch

import sim_oracle as O

pytestmark = pytest.mark.gpu
N, STEPS, MAX_LEN = 16, 40, 12
SIM_WRITES = ("root_states", "base_ang_vel", "episode_length_buf", "last_contacts", "lin_vel_buffer", "ang_vel_buffer", "cmd_buffer",
              "rigid_body_state", "contact_forces", "torques", "actions", "base_lin_vel", "last_base_ang_vel", "projected_gravity",
              "base_pos", "base_quat", "contact_filt")


def _env(rough=False, **sim_kw):
    from dtc_amd import sim as SIM, synthetic as S
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    s = SIM.SimConfig(resampling_time=7 * 0.02 + 1e-9, **sim_kw)
    cfg = SurrogateConfig(sim=s, episode_length_s=MAX_LEN * s.dt)
    table = S.reward_table() if rough else None
    return SurrogateLeggedEnv(N, "cuda", cfg, table, seed=3), cfg


def _draws(i, dev, n=N):
    g = torch.Generator().manual_seed(100 + i)
    return dict(u_cmd=torch.rand(n, 3, generator=g).to(dev), u_reset=torch.rand(n, 26, generator=g).to(dev),
                u_heights=torch.rand(n, 693, generator=g).to(dev), height_noise=0.01)


def _actions(i, dev):
    """Env n crouches harder the larger n is (the knee folds, the thigh swings back): the upper envs sink under the 0.15 m limit."""
    g = torch.Generator().manual_seed(200 + i)
    a = 0.3 * torch.randn(N, 12, generator=g)
    depth = torch.linspace(0.0, 4.0, N)[:, None]
    a += depth * torch.tensor([0.0, -2.0, 2.4] * 4)
    return a.to(dev)


def _state(env):
    st = {k: getattr(env, k).detach().cpu().numpy().copy() for k in O.STATE + O.INPUTS}
    return st


@pytest.mark.parametrize("rough", [False, True], ids=["flat", "rough"])
def test_env_steps_on_evolving_state(rough):
    from dtc_amd import sim as SIM
    env, cfg = _env(rough)
    dev = env.device
    assert cfg.max_episode_length == MAX_LEN and (env.num_obs, env.num_privileged_obs, env.num_actions, env.num_obs_history) == (53, 1389, 12, 265)
    tables = {k: v.cpu().numpy() for k, v in env.sim.tables.items()}
    hs = env.height_samples.cpu().numpy()
    k = O.config_dict(cfg.sim, hs.shape[0], hs.shape[1])
    env.reset(draws=_draws(-1, dev))
    seen = dict(time_out=0, height=0, resample=0, reset=0)
    for i in range(STEPS):
        before = _state(env)
        last_actions = env.last_actions.clone()
        a, d = _actions(i, dev), _draws(i, dev)
        obs, priv, rew, dones, extras = env.step(a, d)
        # --- dtc_sim_step on the state the env was in: equal bits wherever no reset has rewritten the row since
        want = O.sim_step(before, k, tables, a.cpu().numpy(), hs, d["u_cmd"].cpu().numpy())
        done = dones.cpu().numpy()
        assert dones.dtype == torch.bool and np.array_equal(done, env.reset_buf.cpu().numpy() != 0)
        keep = ~done
        for name in SIM_WRITES:
            got, exp = getattr(env, name).cpu().numpy(), want[name]
            if name.endswith("_buffer"):
                got, exp = got[:, keep], exp[:, keep]
            elif name in ("root_states", "episode_length_buf", "last_contacts", "contact_filt"):          # rows that reset_idx rewrites
                got, exp = got[keep], exp[keep]
            assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(exp).view(np.uint8)), f"step {i}: {name}"
        for name in ("dof_pos", "dof_vel", "commands"):
            assert np.array_equal(getattr(env, name).cpu().numpy()[keep].view(np.int32), np.ascontiguousarray(want[name][keep]).view(np.int32)), name
        # --- the env side: termination rule, reset rows, step tail, observation layout and clip, extras
        t_out = want["episode_length_buf"] > MAX_LEN
        assert np.array_equal(extras["time_outs"].cpu().numpy(), t_out) and (done | ~t_out).all()
        mh = env.measured_heights.cpu().numpy()
        mean = (want["root_states"][:, 2:3] - np.maximum(mh[:, 210:483], 0)).mean(1)
        clear = np.abs(mean - 0.15) > 1e-4
        assert np.array_equal(done[clear], (t_out | (mean < 0.15))[clear])
        assert (env.episode_length_buf.cpu().numpy()[done] == 0).all() and (env.dof_vel.cpu().numpy()[done] == 0).all()
        assert (env.lin_vel_buffer.cpu().numpy()[:, done] == 0).all() and (env.last_actions_2.cpu().numpy()[keep] == last_actions.cpu().numpy()[keep]).all()
        assert (env.last_actions_2.cpu().numpy()[done] == 0).all() and torch.equal(env.last_actions, env.actions)
        assert torch.equal(env.last_dof_vel, env.dof_vel) and torch.equal(env.last_root_vel, env.root_states[:, 7:13])
        assert torch.equal(env.base_lin_vel_last, env.base_lin_vel) and torch.equal(env.last_foot_velocities, env.foot_velocities)
        assert obs.shape == (N, 53) and priv.shape == (N, 1389) and bool(torch.isfinite(obs).all()) and bool(torch.isfinite(priv).all())
        assert torch.equal(obs[:, 0:3], env.base_ang_vel * cfg.obs.ang_vel) and torch.equal(obs[:, 33:45], env.actions)
        assert torch.equal(obs[:, 9:21], (env.dof_pos - env.default_dof_pos) * cfg.obs.dof_pos)          # reset rows: the NEW dof_pos
        assert float(obs.abs().max()) <= cfg.clip_observations and bool(torch.isfinite(rew).all())
        assert set(extras["episode"]) == {"rew_" + n for n in env.env_rewards.cfg.names}
        due = want["episode_length_buf"] % cfg.sim.resampling_steps == 0
        seen["time_out"] += int(t_out.sum()); seen["height"] += int((done & ~t_out).sum())
        seen["resample"] += int((due & keep).sum()); seen["reset"] += int(done.sum())
    assert seen["time_out"] > 0 and seen["height"] > 0 and seen["resample"] > 0 and seen["reset"] < N * STEPS // 2, seen


def test_heading_command_follows_the_float64_rule():
    """commands[:, 2] = clip(0.5 * wrap_to_pi(commands[:, 3] - heading), -1.5, 1.5) (legged_robot.py:537-539) in float64 from the
    env's own quaternion and heading command, within 1e-6: eight fp32 ulps at the clip bound 1.5."""
    env, cfg = _env(heading_command=True)
    dev = env.device
    env.reset(draws=_draws(-1, dev))
    for i in range(8):
        env.step(_actions(i, dev), _draws(i, dev))
        q, c = env.base_quat.double().cpu().numpy(), env.commands.double().cpu().numpy()
        heading = np.arctan2(2 * q[:, 2] * q[:, 3], 1 - 2 * q[:, 2] ** 2)
        d = (c[:, 3] - heading) % (2 * np.pi)
        d -= 2 * np.pi * (d > np.pi)
        keep = ~(env.reset_buf.cpu().numpy() != 0)                                       # a reset redraws column 3 after the rule ran
        assert np.abs(c[:, 2] - np.clip(0.5 * d, -1.5, 1.5))[keep].max() <= 1e-6


def test_a_step_synchronises_nothing():
    env, _ = _env()
    dev = env.device
    env.reset(draws=_draws(-1, dev))
    a, d = _actions(0, dev), _draws(0, dev)
    env.step(a, d)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        env.step(a, d)
        env.step(a)                                                                      # the seeded draws of the production mode too
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the composition of the oracles
def _snapshot(env):
    """Every tensor the oracles need, as the env holds it before a step."""
    st = _state(env)
    for k in ("last_actions", "last_actions_2", "last_dof_vel", "last_foot_velocities", "feet_air_time", "pitch_est", "height_noise_offset",
              "motor_strengths", "env_origins", "forces", "robot_mass", "terrain_levels", "base_ang_vel_last", "base_lin_vel_last"):
        st[k] = getattr(env, k).detach().cpu().numpy().copy()
    st["stumble"] = env.env_rewards.stumble.cpu().numpy().copy()
    st["episode_sums"] = env.env_rewards.episode_sums.cpu().numpy().copy()
    return st


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("rough", [False, True], ids=["flat", "rough"])
def test_env_equals_the_composition_of_the_oracles(rough):
    """After every step, every public tensor against tests/sim_oracle.py -> oracle/heights.py -> oracle/foothold.py ->
    oracle/observations.py (check_termination) -> tests/golden/reward_oracle.py -> tests/golden/reset_oracle.py ->
    oracle/observations.py (compute_observations) -> the step tail, each oracle fed by the one before it and by the env's state
    before the step.  Bit for bit, except where the reward oracle documents a tolerance: rew_buf, the episode sums and feet_air_time
    are held to tests/reward_cases.py's bound, max(2^-20, 8 * e32) with e32 from the oracle's own float32 run on the same inputs
    (the bound of tests/test_hip_rewards.py for the same quantities: K.bound, K.term_err); the episode means of the extras, float64
    sums of those fp32 episode sums, to the largest of the terms' bounds."""
    import dataclasses
    import reward_cases as K
    import reset_oracle as RO
    from oracle import foothold as OF, heights as OH, observations as OB
    env, cfg = _env(rough)
    dev, s = env.device, cfg.sim
    tables = {k: v.cpu().numpy() for k, v in env.sim.tables.items()}
    hs = env.height_samples.cpu().numpy()
    k = O.config_dict(s, hs.shape[0], hs.shape[1])
    px, py = cfg.grid.points_x, cfg.grid.points_y
    feet, thighs = list(s.feet), list(s.thighs)
    rc = env.env_rewards.cfg
    layout = dataclasses.replace(K.LITE3, feet=tuple(feet), penalised=tuple(env.penalised_contact_indices.tolist()), hips=(0, 3, 6, 9))
    rcfg = K.oracle_cfg(rc, layout)
    reset_cfg = RO.config(terrain_curriculum=False, custom_origins=False, heading_command=False, randomize_motor_strength=True,
                          max_episode_length_s=cfg.episode_length_s)
    base_init = np.array(cfg.reset_config().base_init_state, dtype=np.float32)
    env.reset(draws=_draws(-1, dev))
    resets = 0
    for i in range(STEPS):
        B = _snapshot(env)
        a, d = _actions(i, dev), _draws(i, dev)
        obs, priv, rew, dones, extras = env.step(a, d)
        # 1. the surrogate step
        W = O.sim_step(B, k, tables, a.cpu().numpy(), hs, d["u_cmd"].cpu().numpy())
        # 2. heights, 3. planner
        mh = OH.get_heights(hs, W["root_states"], px, py, s.border_size, s.horizontal_scale, s.vertical_scale)
        assert np.array_equal(_bits(env.measured_heights.cpu().numpy()), _bits(mh)), f"step {i}: measured_heights"
        thigh = np.ascontiguousarray(W["rigid_body_state"][:, thighs, 0:3])
        plan = OF.plan(mh, W["root_states"], thigh, W["commands"], px, py, t_stance=s.dt)
        for name, key in (("foothold_obs", "foothold_obs"), ("optimal_footholds_world", "optimal_footholds_world")):
            assert np.array_equal(_bits(getattr(env, name).cpu().numpy()), _bits(plan[key].astype(np.float32))), f"step {i}: {name}"
        # 4. termination
        term_in = dict(contact_forces=W["contact_forces"], termination_contact_indices=[0], episode_length_buf=W["episode_length_buf"],
                       projected_gravity=W["projected_gravity"], root_states=W["root_states"], measured_heights=mh)
        reset_ref, time_out, _ = OB.check_termination(term_in, MAX_LEN)
        assert np.array_equal(dones.cpu().numpy(), reset_ref) and np.array_equal(extras["time_outs"].cpu().numpy(), time_out), f"step {i}"
        keep = ~reset_ref
        resets += int(reset_ref.sum())
        # 5. rewards (float64 oracle; the bound of tests/test_hip_rewards.py, K.bound(e32), per quantity)
        R = dict(W)
        R.update(default_dof_pos=tables["default_dof_pos"], last_dof_vel=B["last_dof_vel"], last_actions=B["last_actions"],
                 last_actions_2=B["last_actions_2"], last_foot_velocities=B["last_foot_velocities"],
                 foot_positions=np.ascontiguousarray(W["rigid_body_state"][:, feet, 0:3]),
                 foot_velocities=np.ascontiguousarray(W["rigid_body_state"][:, feet, 7:10]),
                 optimal_footholds_world=plan["optimal_footholds_world"].astype(np.float32), measured_heights=mh, reset_buf=reset_ref,
                 time_out_buf=time_out, robot_mass=B["robot_mass"], terrain_levels=B["terrain_levels"],
                 dof_pos_limits=tables["dof_pos_limits"], dof_vel_limits=env.dof_vel_limits.cpu().numpy(), torque_limits=tables["torque_limits"],
                 feet_air_time=B["feet_air_time"], stumble=B["stumble"], pitch_est=B["pitch_est"])
        r64, e32 = K.reference(R, rcfg, B["episode_sums"])
        err = K.term_err(rew.cpu().numpy(), r64["rew"])
        assert err <= K.bound(e32["rew"]), f"step {i}: rew_buf {err:.2e} over {K.bound(e32['rew']):.2e}"
        worst = K.bound(e32["rew"])
        sums = env.env_rewards.episode_sums.cpu().numpy()
        for j, name in enumerate(rc.names):
            b = K.bound(e32[name])
            worst = max(worst, b)
            # the sum is the fp32 sum before plus the term: the term's bound at the size of the larger of the two
            ref = r64["sums"][name][keep]
            size = np.maximum(np.abs(ref), np.abs(r64["per"][name][keep]))
            assert (np.abs(sums[j][keep] - ref) <= b * np.maximum(size, 1e-2 * (size.max() if size.size else 0)) + 1e-30).all(), f"step {i}: sum of {name}"
            assert (sums[j][reset_ref] == 0).all()
        air = env.feet_air_time.cpu().numpy()
        assert K.term_err(air[keep], r64["st"]["feet_air_time"][keep]) <= K.bound(e32["air"]) and (air[reset_ref] == 0).all(), f"step {i}: feet_air_time"
        # 6. reset (bit for bit on every row it rewrites; the episode means within the largest term bound)
        E = dict(W)
        E.update(reset_buf=reset_ref, default_dof_pos=tables["default_dof_pos"], base_init_state=base_init, env_origins=B["env_origins"],
                 forces=B["forces"], motor_strengths=B["motor_strengths"], height_noise_offset=B["height_noise_offset"],
                 last_actions=B["last_actions"], last_actions_2=B["last_actions_2"], last_dof_vel=B["last_dof_vel"],
                 feet_air_time=air.copy(), pitch_est=env.pitch_est.cpu().numpy().copy(), base_ang_vel_last=B["base_ang_vel_last"],
                 base_lin_vel_last=B["base_lin_vel_last"], lag_buffer=[], stumble=env.env_rewards.stumble.cpu().numpy().copy(),
                 episode_sums=np.stack([r64["sums"][n] for n in rc.names]))
        E = {key: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for key, v in E.items()}
        for name in ("feet_contact_time", "last_scale_actions", "last_scale_actions2"):            # rows the reference clears; not in this env
            E[name] = np.zeros((N, 1), dtype=np.float32)
        out = RO.reset_idx(E, reset_cfg, d["u_reset"].cpu().numpy(), np.zeros(N, dtype=np.int64), d["height_noise"])
        for name in ("dof_pos", "dof_vel", "root_states", "commands", "motor_strengths", "height_noise_offset", "episode_length_buf",
                     "contact_filt", "last_contacts", "lin_vel_buffer", "ang_vel_buffer", "cmd_buffer", "forces"):
            got = getattr(env, name).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(E[name].astype(got.dtype))), f"step {i}: {name} after the reset"
        if out["count"]:
            means = np.array([float(extras["episode"]["rew_" + n]) for n in rc.names])
            assert np.allclose(means, out["episode_means"], rtol=worst, atol=worst * np.abs(out["episode_means"]).max()), f"step {i}: episode means"
        # 7. observations: the rows of the reset envs from their new state, every row equal to the oracle
        S_ = dict(base_ang_vel=W["base_ang_vel"], projected_gravity=W["projected_gravity"], commands=E["commands"], dof_pos=E["dof_pos"],
                  default_dof_pos=tables["default_dof_pos"], dof_vel=E["dof_vel"], actions=W["actions"], foothold_obs=plan["foothold_obs"],
                  root_states=E["root_states"], measured_heights=mh, u_heights=d["u_heights"].cpu().numpy(),
                  height_noise_offset=E["height_noise_offset"], forces=E["forces"])
        # the rows the first observation pass wrote (envs not reset) used the offsets before the reset: the same values for those rows
        o_ref, p_ref, _ = OB.compute_observations(S_, add_noise=False)
        clip = np.float32(cfg.clip_observations)
        assert np.array_equal(_bits(obs.cpu().numpy()), _bits(np.clip(o_ref, -clip, clip))), f"step {i}: obs_buf"
        assert np.array_equal(_bits(priv.cpu().numpy()), _bits(np.clip(p_ref, -clip, clip))), f"step {i}: privileged_obs_buf"
        # 8. the step tail
        tail = dict(last_actions=W["actions"], last_actions_2=np.where(reset_ref[:, None], np.float32(0), B["last_actions"]),
                    last_dof_vel=E["dof_vel"], last_root_vel=E["root_states"][:, 7:13], last_foot_velocities=R["foot_velocities"],
                    base_ang_vel_last=W["base_ang_vel"], base_lin_vel_last=W["base_lin_vel"])
        for name, ref in tail.items():
            assert np.array_equal(_bits(getattr(env, name).cpu().numpy()), _bits(ref.astype(np.float32))), f"step {i}: {name}"
    assert 0 < resets < N * STEPS // 2
