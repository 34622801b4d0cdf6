"""SurrogateLeggedEnv with `tilt=True` on the GPU, on the terms of tests/test_sim_env_path.py: 16 envs x 12 steps over the rough
table, every draw an input, with and without the heading command, reward scales that include `orientation` and `ang_vel_xy`.  After
every step every public tensor is compared with the composition tests/sim_tilt_oracle.py -> oracle/heights.py -> oracle/foothold.py
-> oracle/observations.py -> tests/golden/reward_oracle.py -> tests/golden/reset_oracle.py -> the step tail: bit for bit, the reward
sums to the reward tests' own bound.  Then PPO and RecurrentDecoderPPO learn on the tilt env."""
import dataclasses

import numpy as np
import pytest
import torch

import sim_tilt_oracle as TO
import test_sim_env_path as E

pytestmark = pytest.mark.gpu
N, STEPS, MAX_LEN = 16, 12, 6


def _env(heading, n=N, max_len=MAX_LEN):
    from dtc_amd import sim as SIM, synthetic as S
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    from dtc_amd.env.surrogate import _SCALES
    s = SIM.SimConfig(resampling_time=5 * 0.02 + 1e-9, tilt=True, heading_command=heading)
    cfg = SurrogateConfig(sim=s, episode_length_s=max_len * s.dt, reward_scales=dict(_SCALES, orientation=-0.2, orientation_roll=-0.1))
    assert cfg.reward_scales["ang_vel_xy"] != 0
    return SurrogateLeggedEnv(n, "cuda", cfg, S.reward_table(), seed=3), cfg


def _heading_rule(q, target):
    """clip(0.5 * wrap_to_pi(target - heading), -1.5, 1.5) with heading = the yaw of quat_apply(q, (1, 0, 0)), float64."""
    q = q.astype(np.float64)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    heading = np.arctan2(2 * (x * y + w * z), 1 - 2 * (y * y + z * z))
    d = (target.astype(np.float64) - heading) % (2 * np.pi)
    d -= 2 * np.pi * (d > np.pi)
    return np.clip(0.5 * d, -1.5, 1.5)


@pytest.mark.parametrize("heading", [False, True], ids=["yaw_rate", "heading"])
def test_tilt_env_equals_the_composition_of_the_oracles(heading):
    import reward_cases as K
    import reset_oracle as RO
    from oracle import foothold as OF, heights as OH, observations as OB
    env, cfg = _env(heading)
    dev, s = env.device, cfg.sim
    assert cfg.max_episode_length == MAX_LEN
    tables = {k: v.cpu().numpy() for k, v in env.sim.tables.items()}
    hs = env.height_samples.cpu().numpy()
    k = TO.config_dict(s, hs.shape[0], hs.shape[1])
    px, py = cfg.grid.points_x, cfg.grid.points_y
    feet, thighs = list(s.feet), list(s.thighs)
    rc = env.env_rewards.cfg
    assert {"orientation", "orientation_roll", "ang_vel_xy"} <= set(rc.names)
    layout = dataclasses.replace(K.LITE3, feet=tuple(feet), penalised=tuple(env.penalised_contact_indices.tolist()), hips=(0, 3, 6, 9))
    rcfg = K.oracle_cfg(rc, layout)
    reset_cfg = RO.config(terrain_curriculum=False, custom_origins=False, heading_command=heading, randomize_motor_strength=True,
                          max_episode_length_s=cfg.episode_length_s)
    base_init = np.array(cfg.reset_config().base_init_state, dtype=np.float32)
    # the commands as the env-side kernels see them: after the heading law, which runs between dtc_sim_step_tilt and them
    seen, inner = {}, env.env_step

    def env_step(**kw):
        seen["commands"] = env.commands.detach().clone()
        return inner(**kw)
    env.env_step = env_step
    env.reset(draws=E._draws(-1, dev))
    resets, tilted, turning, ang_sum = 0, 0.0, 0.0, 0.0
    for i in range(STEPS):
        B = E._snapshot(env)
        a, d = E._actions(i, dev), E._draws(i, dev)
        obs, priv, rew, dones, extras = env.step(a, d)
        # 1. the surrogate step with tilt, then the heading law (float64 rule within 1e-6, as tests/test_sim_env_path.py holds it)
        W = TO.sim_step(B, k, tables, a.cpu().numpy(), hs, d["u_cmd"].cpu().numpy())
        for name in E.SIM_WRITES:
            if name not in ("root_states", "episode_length_buf", "last_contacts", "contact_filt") and not name.endswith("_buffer"):
                assert np.array_equal(E._bits(getattr(env, name).cpu().numpy()), E._bits(W[name])), f"step {i}: {name}"
        cmd = seen["commands"].cpu().numpy()
        if heading:
            assert np.abs(cmd[:, 2] - _heading_rule(W["base_quat"], W["commands"][:, 3])).max() <= 1e-6, f"step {i}: heading law"
            W["commands"][:, 2] = cmd[:, 2]
        assert np.array_equal(E._bits(cmd), E._bits(W["commands"])), f"step {i}: commands"
        tilted = max(tilted, float(np.abs(W["projected_gravity"][:, :2]).max()))
        turning = max(turning, float(np.abs(W["base_ang_vel"][:, :2]).max()))
        # 2. heights, 3. planner
        mh = OH.get_heights(hs, W["root_states"], px, py, s.border_size, s.horizontal_scale, s.vertical_scale)
        assert np.array_equal(E._bits(env.measured_heights.cpu().numpy()), E._bits(mh)), f"step {i}: measured_heights"
        thigh = np.ascontiguousarray(W["rigid_body_state"][:, thighs, 0:3])
        plan = OF.plan(mh, W["root_states"], thigh, W["commands"], px, py, t_stance=s.dt)
        for name in ("foothold_obs", "optimal_footholds_world"):
            assert np.array_equal(E._bits(getattr(env, name).cpu().numpy()), E._bits(plan[name].astype(np.float32))), f"step {i}: {name}"
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
            ref = r64["sums"][name][keep]
            size = np.maximum(np.abs(ref), np.abs(r64["per"][name][keep]))
            assert (np.abs(sums[j][keep] - ref) <= b * np.maximum(size, 1e-2 * (size.max() if size.size else 0)) + 1e-30).all(), f"step {i}: sum of {name}"
            assert (sums[j][reset_ref] == 0).all()
            if name == "ang_vel_xy":
                ang_sum = max(ang_sum, float(np.abs(sums[j]).max()))
        air = env.feet_air_time.cpu().numpy()
        assert K.term_err(air[keep], r64["st"]["feet_air_time"][keep]) <= K.bound(e32["air"]) and (air[reset_ref] == 0).all(), f"step {i}: feet_air_time"
        # 6. reset (bit for bit on every row it rewrites; the episode means within the largest term bound)
        Z = dict(W)
        Z.update(reset_buf=reset_ref, default_dof_pos=tables["default_dof_pos"], base_init_state=base_init, env_origins=B["env_origins"],
                 forces=B["forces"], motor_strengths=B["motor_strengths"], height_noise_offset=B["height_noise_offset"],
                 last_actions=B["last_actions"], last_actions_2=B["last_actions_2"], last_dof_vel=B["last_dof_vel"],
                 feet_air_time=air.copy(), pitch_est=env.pitch_est.cpu().numpy().copy(), base_ang_vel_last=B["base_ang_vel_last"],
                 base_lin_vel_last=B["base_lin_vel_last"], lag_buffer=[], stumble=env.env_rewards.stumble.cpu().numpy().copy(),
                 episode_sums=np.stack([r64["sums"][n] for n in rc.names]))
        Z = {key: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for key, v in Z.items()}
        for name in ("feet_contact_time", "last_scale_actions", "last_scale_actions2"):            # rows the reference clears; not in this env
            Z[name] = np.zeros((N, 1), dtype=np.float32)
        out = RO.reset_idx(Z, reset_cfg, d["u_reset"].cpu().numpy(), np.zeros(N, dtype=np.int64), d["height_noise"])
        for name in ("dof_pos", "dof_vel", "root_states", "commands", "motor_strengths", "height_noise_offset", "episode_length_buf",
                     "contact_filt", "last_contacts", "lin_vel_buffer", "ang_vel_buffer", "cmd_buffer", "forces"):
            got = getattr(env, name).cpu().numpy()
            assert np.array_equal(E._bits(got), E._bits(Z[name].astype(got.dtype))), f"step {i}: {name} after the reset"
        if out["count"]:
            means = np.array([float(extras["episode"]["rew_" + n]) for n in rc.names])
            assert np.allclose(means, out["episode_means"], rtol=worst, atol=worst * np.abs(out["episode_means"]).max()), f"step {i}: episode means"
        # 7. observations: the rows of the reset envs from their new state, every row equal to the oracle
        S_ = dict(base_ang_vel=W["base_ang_vel"], projected_gravity=W["projected_gravity"], commands=Z["commands"], dof_pos=Z["dof_pos"],
                  default_dof_pos=tables["default_dof_pos"], dof_vel=Z["dof_vel"], actions=W["actions"], foothold_obs=plan["foothold_obs"],
                  root_states=Z["root_states"], measured_heights=mh, u_heights=d["u_heights"].cpu().numpy(),
                  height_noise_offset=Z["height_noise_offset"], forces=Z["forces"])
        o_ref, p_ref, _ = OB.compute_observations(S_, add_noise=False)
        clip = np.float32(cfg.clip_observations)
        assert np.array_equal(E._bits(obs.cpu().numpy()), E._bits(np.clip(o_ref, -clip, clip))), f"step {i}: obs_buf"
        assert np.array_equal(E._bits(priv.cpu().numpy()), E._bits(np.clip(p_ref, -clip, clip))), f"step {i}: privileged_obs_buf"
        # 8. the step tail
        tail = dict(last_actions=W["actions"], last_actions_2=np.where(reset_ref[:, None], np.float32(0), B["last_actions"]),
                    last_dof_vel=Z["dof_vel"], last_root_vel=Z["root_states"][:, 7:13], last_foot_velocities=R["foot_velocities"],
                    base_ang_vel_last=W["base_ang_vel"], base_lin_vel_last=W["base_lin_vel"])
        for name, ref in tail.items():
            assert np.array_equal(E._bits(getattr(env, name).cpu().numpy()), E._bits(ref.astype(np.float32))), f"step {i}: {name}"
    assert 0 < resets < N * STEPS
    # the attitude is no longer trivial: three observation entries, the ang_vel_xy term and the orientation terms see it
    assert tilted > 0.01 and turning > 0.01 and ang_sum > 0, (tilted, turning, ang_sum)


def test_tilt_adds_no_attribute_to_the_env_or_its_step():
    from dtc_amd import sim as SIM
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    plain = SurrogateLeggedEnv(N, "cuda", SurrogateConfig(), seed=3)
    tilt = SurrogateLeggedEnv(N, "cuda", SurrogateConfig(sim=SIM.SimConfig(tilt=True)), seed=3)
    assert set(vars(plain)) == set(vars(tilt)) and set(vars(plain.sim)) == set(vars(tilt.sim))            # no new attribute either way


@pytest.mark.parametrize("model", ["ppo", "rdppo"])
def test_trainers_learn_on_the_tilt_env(model):
    """Three learn() iterations at 16 envs x 24 steps on the rough table with tilt: finite weights, a tilted base in the rollout,
    and an env step that reads nothing back."""
    from dtc_amd.runners import OnPolicyRunner
    import test_sim_runner_path as RP
    torch.manual_seed(11)
    env, cfg = _env(False, max_len=30)
    runner = dict(num_steps_per_env=24, save_interval=1000, **RP.MODELS[model])
    r = OnPolicyRunner(env, dict(runner=runner, algorithm=dict(num_learning_epochs=2), policy=dict()), log_dir=None, device="cuda")
    r.learn(3)
    torch.cuda.synchronize()
    ac = r.alg.actor_critic
    assert bool(torch.isfinite(ac.arena.flat).all()) if hasattr(ac, "arena") else all(bool(torch.isfinite(p).all()) for p in ac.parameters())
    assert bool(torch.isfinite(env.obs_buf).all()) and bool(torch.isfinite(env.rew_buf).all())
    assert float(env.projected_gravity[:, :2].abs().max()) > 0
    a = torch.zeros(N, 12, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        env.step(a)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
