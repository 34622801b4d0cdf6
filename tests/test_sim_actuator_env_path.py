"""SurrogateLeggedEnv with `SimConfig.actuator` on the GPU, on the terms of tests/test_sim_env_path.py: 16 envs x 30 steps, a push
every third step (on two consecutive steps), every draw an input, with the yaw-only base, with tilt, and once on a small generated
terrain.  The compositions of tests/test_sim_env_path.py / tests/test_sim_tilt_env_path.py run unchanged, to their own bounds, with
tests/sim_actuator_oracle.py standing where they call the surrogate step's oracle; lag_state and push_vel are compared bit for bit
after every step and are zero in the rows of every env reset in it.  Then the trainers learn on the env, and the policy-step
containment keeps a NaN env away from the others' lag buffers."""
import types

import numpy as np
import pytest
import torch

import sim_actuator_oracle as AO
import sim_oracle as O
import test_sim_env_path as E
import test_sim_tilt_env_path as T

pytestmark = pytest.mark.gpu
N, STEPS, INTERVAL_S = 16, 30, 0.06


def _actuator():
    from dtc_amd import sim as SIM
    return SIM.ActuatorConfig(push_interval_s=INTERVAL_S)


def _env(tilt, max_len, terrain=None, n=N, **sim_kw):
    from dtc_amd import sim as SIM, synthetic as S
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    from dtc_amd.env.surrogate import _SCALES
    s = SIM.SimConfig(resampling_time=(5 if tilt else 7) * 0.02 + 1e-9, tilt=tilt, actuator=_actuator(), **sim_kw)
    scales = dict(_SCALES, orientation=-0.2, orientation_roll=-0.1) if tilt else dict(_SCALES)
    cfg = SurrogateConfig(sim=s, episode_length_s=max_len * s.dt, reward_scales=scales, terrain=terrain)
    assert s.push_interval == 3
    table = None if terrain is not None else S.reward_table()
    return SurrogateLeggedEnv(n, "cuda", cfg, table, seed=3), cfg


def _patch(monkeypatch, env, cfg, tilt, max_len):
    """Hand the actuator env to the imported composition: its draws gain lag_choice and u_push, its snapshot the two new tensors, and
    the oracle it calls for the surrogate step is tests/sim_actuator_oracle.py, which also checks the two new tensors."""
    last, seen = {}, dict(pushes=0, steps=0, resets=0, pending=0, lagged=0)
    inner_draws, inner_snapshot = E._draws, E._snapshot
    dec = cfg.sim.decimation

    def draws(i, dev, n=N):
        d = inner_draws(i, dev, n)
        g = torch.Generator().manual_seed(400 + i)
        d["lag_choice"] = [int(v) for v in torch.randint(1, 5, (dec,), generator=g)]
        d["u_push"] = torch.rand(n, 2, generator=g).to(dev)
        last["draws"] = d
        return d

    def snapshot(e):
        B = inner_snapshot(e)
        B["lag_state"], B["push_vel"] = e.lag_state.cpu().numpy().copy(), e.push_vel.cpu().numpy().copy()
        last["push"] = (e.common_step_counter + 1) % cfg.sim.push_interval in (0, 1)
        last["B"] = B
        return B

    def sim_step(B, k, tables, a, hs, u_cmd):
        d = last["draws"]
        trace = []
        W = AO.sim_step(B, k, tables, a, hs, u_cmd, trace=trace, tilt=tilt, lag_choice=d["lag_choice"], u_push=d["u_push"].cpu().numpy(),
                        push=last["push"])
        done = env.reset_buf.cpu().numpy() != 0
        for name in ("lag_state", "push_vel"):
            got = getattr(env, name).cpu().numpy()
            assert np.array_equal(E._bits(got[~done]), E._bits(W[name][~done])), f"{name} of the envs that went on"
            assert (got[done] == 0).all(), f"{name} of the reset envs"
        assert all(torch.equal(env.lag_buffer[i], env.lag_state[:, i]) for i in range(6))
        seen["steps"] += 1
        seen["pushes"] += int(last["push"])
        seen["resets"] += int(done.sum())
        seen["pending"] += int(np.stack([s["pushed"] for s in trace]).sum())
        clipped = np.minimum(np.maximum(a, -np.float32(cfg.sim.clip_actions)), np.float32(cfg.sim.clip_actions))
        seen["lagged"] += int(any((s["goal"] != np.minimum(np.maximum(clipped * np.float32(cfg.sim.action_scale) + tables["default_dof_pos"],
                                                                     tables["dof_pos_limits"][:, 0]), tables["dof_pos_limits"][:, 1])).any()
                                  for s in trace))
        return W

    shim = types.SimpleNamespace(STATE=O.STATE, INPUTS=O.INPUTS, config_dict=AO.config_dict, sim_step=sim_step)
    monkeypatch.setattr(E, "O", shim)
    monkeypatch.setattr(T, "TO", shim)
    for mod in (E, T):
        monkeypatch.setattr(mod, "N", env.num_envs)
        monkeypatch.setattr(mod, "STEPS", STEPS)
        monkeypatch.setattr(mod, "MAX_LEN", max_len)
    monkeypatch.setattr(E, "_draws", draws)
    monkeypatch.setattr(E, "_snapshot", snapshot)
    monkeypatch.setattr(E, "_env", lambda rough=False, **kw: (env, cfg))
    monkeypatch.setattr(T, "_env", lambda heading=False, **kw: (env, cfg))
    return seen


def _seen_enough(seen):
    # a push on two of every three steps (the step inside reset() is the first of a pair), pending pushes through the substeps, the
    # lag at work in every step, and resets that cleared rows
    assert seen["steps"] == STEPS and seen["pushes"] == 2 * STEPS // 3 and seen["lagged"] == STEPS, seen
    assert seen["pending"] > N * STEPS and 0 < seen["resets"] < N * STEPS, seen


def test_env_equals_the_composition_of_the_oracles(monkeypatch):
    env, cfg = _env(False, E.MAX_LEN)
    seen = _patch(monkeypatch, env, cfg, False, E.MAX_LEN)
    E.test_env_equals_the_composition_of_the_oracles(True)
    _seen_enough(seen)
    assert env.common_step_counter == STEPS + 1


def test_tilt_env_equals_the_composition_of_the_oracles(monkeypatch):
    env, cfg = _env(True, T.MAX_LEN)
    seen = _patch(monkeypatch, env, cfg, True, T.MAX_LEN)
    T.test_tilt_env_equals_the_composition_of_the_oracles(False)
    _seen_enough(seen)


def test_env_equals_the_composition_of_the_oracles_on_a_generated_terrain(monkeypatch):
    import test_terrain_env_path as TP
    from dtc_amd import sim as SIM
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    monkeypatch.setattr(TP, "N", N)
    s = SIM.SimConfig(resampling_time=7 * 0.02 + 1e-9, border_size=TP.BORDER, actuator=_actuator())
    cfg = SurrogateConfig(sim=s, episode_length_s=E.MAX_LEN * s.dt, terrain=TP._terrain_cfg(7))
    env = SurrogateLeggedEnv(N, "cuda", cfg, seed=3)
    on_terrain = TP._patch_harness(monkeypatch, env, cfg, E.MAX_LEN)
    seen = _patch(monkeypatch, env, cfg, False, E.MAX_LEN)
    E.test_env_equals_the_composition_of_the_oracles(True)
    _seen_enough(seen)
    assert on_terrain["resets"] > 0 and env.height_samples.cpu().numpy().any()


def test_without_an_actuator_the_env_has_none_of_the_new_attributes():
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    plain = SurrogateLeggedEnv(N, "cuda", SurrogateConfig(), seed=3)
    assert not any(hasattr(plain, name) for name in ("lag_state", "push_vel", "lag_buffer", "common_step_counter"))
    env, _ = _env(False, 12)
    assert set(vars(env)) - set(vars(plain)) == {"lag_state", "push_vel", "lag_buffer", "common_step_counter"}
    assert env.lag_state.shape == (N, 6, 12) and env.push_vel.shape == (N, 2) and len(env.lag_buffer) == 6


def test_a_step_synchronises_nothing():
    env, _ = _env(True, 12)
    dev = env.device
    env.reset()
    a = torch.zeros(N, 12, device=dev)
    env.step(a)
    env.step(a)                                                                          # a push step and one without were both warmed up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):                                                               # the seeded draws of the production mode
            env.step(a)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(env.push_vel.any()) and bool(env.lag_state.isfinite().all())


@pytest.mark.parametrize("model", ["ppo", "rdppo"])
def test_trainers_learn_on_the_actuator_env(model):
    """Two learn() iterations at 16 envs x 24 steps on the rough table with tilt, lag and pushes: finite weights and observations,
    pushes that were drawn, a lag buffer that holds scaled actions."""
    from dtc_amd.runners import OnPolicyRunner
    import test_sim_runner_path as RP
    torch.manual_seed(11)
    env, cfg = _env(True, 30)
    runner = dict(num_steps_per_env=24, save_interval=1000, **RP.MODELS[model])
    r = OnPolicyRunner(env, dict(runner=runner, algorithm=dict(num_learning_epochs=2), policy=dict()), log_dir=None, device="cuda")
    r.learn(2)
    torch.cuda.synchronize()
    ac = r.alg.actor_critic
    assert bool(torch.isfinite(ac.arena.flat).all()) if hasattr(ac, "arena") else all(bool(torch.isfinite(p).all()) for p in ac.parameters())
    assert bool(torch.isfinite(env.obs_buf).all()) and bool(torch.isfinite(env.rew_buf).all())
    assert env.common_step_counter >= 48 and bool(env.push_vel.any()) and bool(env.lag_state.any())
    assert bool(torch.isfinite(env.lag_state).all()) and float(env.push_vel.abs().max()) <= 1.0


def test_a_nan_observation_in_one_env_leaves_the_other_lag_buffers_alone():
    """contain_nonfinite_act=True: env 7 is handed a NaN observation ahead of a rollout.  Its policy step is repaired and it is reset;
    lag_state and push_vel of the other envs after the rollout equal a clean run's bit for bit, and its own rows are finite.

    The trainer is RecurrentPPO on ActorCriticRecurrent (GRU): its policy step keeps every row to itself under this flag
    (ops.rows_to_themselves), so the other envs are given the clean run's actions and whatever differed would be the env's doing.
    The decoder policies cannot serve here: their CE-net latent replaces outliers by a 2-sigma rule on the statistics of the whole
    batch (actor_critic_decoder.py:274-302), so one env's NaN observation changes the other envs' actions by the reference's own design
    (seen with PPO on this fixture: 6 of the other 15 envs act differently in the very step of the NaN)."""
    from dtc_amd.runners import OnPolicyRunner
    bad, out = 7, []
    policy = dict(actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu", rnn_type="gru", rnn_hidden_size=128,
                  rnn_num_layers=1)
    for dirty in (False, True):
        torch.manual_seed(11)
        env, cfg = _env(False, 30)
        runner = dict(num_steps_per_env=24, save_interval=1000, policy_class_name="ActorCriticRecurrent", algorithm_class_name="RecurrentPPO")
        algo = dict(num_learning_epochs=2, contain_nonfinite_act=True, contain_nonfinite_envs=True)
        r = OnPolicyRunner(env, dict(runner=runner, algorithm=algo, policy=dict(policy)), log_dir=None, device="cuda")
        r.learn(1)
        if dirty:
            with torch.inference_mode():                                                 # the rollout left an inference tensor behind
                env.obs_buf[bad, 3] = float("nan")
        r.learn(1)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(p).all()) for p in r.alg.actor_critic.parameters())
        out.append((env.lag_state.clone(), env.push_vel.clone(), int(r.alg.last_nonfinite_act)))
    others = torch.arange(N, device="cuda") != bad
    assert out[0][2] == 0 and out[1][2] >= 1
    for clean, dirt in zip(out[0][:2], out[1][:2]):
        assert torch.equal(clean[others].view(torch.uint8), dirt[others].view(torch.uint8))
        assert bool(torch.isfinite(dirt).all())
    assert bool(out[0][0].any())
