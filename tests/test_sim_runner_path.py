"""OnPolicyRunner.learn() end to end on the surrogate env: the first closed-loop iterations of this project on one GPU."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
N = 64
MODELS = dict(ppo=dict(policy_class_name="ActorCriticDecoder", algorithm_class_name="PPO"),
              rdppo=dict(policy_class_name="ActorCriticDecoderRecurrent", algorithm_class_name="RecurrentDecoderPPO"))


def _learn(model, iters, tmp_path=None, tag="a"):
    from dtc_amd import sim as SIM
    from dtc_amd.env import HistoryWrapper, SurrogateConfig, SurrogateLeggedEnv
    from dtc_amd.runners import OnPolicyRunner
    torch.manual_seed(11)
    cfg = SurrogateConfig(sim=SIM.SimConfig(), episode_length_s=30 * 0.02)
    env = SurrogateLeggedEnv(N, "cuda", cfg, seed=5)
    runner = dict(num_steps_per_env=24, save_interval=1000, **MODELS[model])
    log_dir = None if tmp_path is None else str(tmp_path / tag)
    if log_dir is not None:
        os.makedirs(log_dir)
    r = OnPolicyRunner(env, dict(runner=runner, algorithm=dict(num_learning_epochs=2), policy=dict()), log_dir=log_dir, device="cuda")
    assert isinstance(r.env, HistoryWrapper) and r.env.env is env
    r.learn(iters)
    torch.cuda.synchronize()
    return r, env


def test_ppo_learns_three_iterations_reproducibly(tmp_path):
    r1, env1 = _learn("ppo", 3, tmp_path, "a")
    flat = r1.alg.actor_critic.arena.flat
    assert bool(torch.isfinite(flat).all())
    means = r1.tracker.means()                                                           # episodes finished and were logged
    assert means is not None and means[1] > 0 and means[1] <= env1.max_episode_length + 1
    assert int(r1.tracker.finished) >= N and bool(torch.isfinite(env1.rew_buf).all())                 # 72 steps, 30-step episodes: every env finished one
    ep = env1.extras["episode"]
    assert set(ep) == {"rew_" + n for n in env1.env_rewards.cfg.names} and all(bool(torch.isfinite(v)) for v in ep.values())
    assert float(ep["rew_tracking_lin_vel"]) > 0                                           # means of the last reset reached the extras
    r2, env2 = _learn("ppo", 3, tmp_path, "b")
    assert torch.equal(flat, r2.alg.actor_critic.arena.flat)
    assert torch.equal(env1.root_states, env2.root_states) and torch.equal(env1.obs_buf, env2.obs_buf)


def test_recurrent_decoder_ppo_learns_one_iteration():
    r, env = _learn("rdppo", 1)
    assert all(bool(torch.isfinite(p).all()) for p in r.alg.actor_critic.parameters())
    assert bool(torch.isfinite(env.obs_buf).all())


def _per_env_tensors(env):
    """Every tensor the env owns that has an env axis: name -> (tensor, env axis)."""
    out = {}
    for name, t in list(vars(env).items()) + list(env.env_step.out.items()) + [("episode_sums", env.env_rewards.episode_sums),
                                                                             ("stumble", env.env_rewards.stumble)]:
        if isinstance(t, torch.Tensor) and t.dim() >= 1:
            axis = 1 if name.endswith("_buffer") or name == "episode_sums" else 0
            if t.dim() > axis and t.shape[axis] == N:
                out[name] = (t, axis)
    return out


def test_a_nan_env_is_reset_in_the_same_step_and_the_other_envs_do_not_notice():
    """A NaN written into one env's dof_state before a step: that env is reset in the same step, everything it owns is finite
    again after the step, and every tensor row of the other 63 envs equals a clean run bit for bit, in that step and after."""
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    bad = 7
    envs = [SurrogateLeggedEnv(N, "cuda", SurrogateConfig(episode_length_s=30 * 0.02), seed=5) for _ in range(2)]
    for e in envs:
        e.reset()
    g = torch.Generator().manual_seed(21)
    others = torch.arange(N, device="cuda") != bad
    for k in range(8):
        a = torch.randn(N, 12, generator=g).cuda()
        if k == 2:
            envs[1].dof_state[bad, 3, 0] = float("nan")
        outs = [e.step(a) for e in envs]
        clean, dirty = _per_env_tensors(envs[0]), _per_env_tensors(envs[1])
        assert set(clean) == set(dirty) and len(clean) > 50
        for name, (t, axis) in clean.items():
            sel = (slice(None),) * axis + (others,)
            assert torch.equal(t[sel].contiguous().view(torch.uint8), dirty[name][0][sel].contiguous().view(torch.uint8)), f"step {k}: {name}"
        if k == 2:
            assert bool(outs[1][3][bad]) and not bool(outs[0][3][bad]) and int(envs[1].episode_length_buf[bad]) == 0
        if k >= 2:
            for name, (t, axis) in dirty.items():
                if t.is_floating_point():
                    assert bool(torch.isfinite(t.select(axis, bad)).all()), f"step {k}: {name} of the repaired env"
            assert all(bool(torch.isfinite(v).all()) for v in envs[1].extras["episode"].values())


def test_learn_goes_on_through_a_nan_env_with_both_containments():
    from dtc_amd import sim as SIM
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    from dtc_amd.runners import OnPolicyRunner
    torch.manual_seed(11)
    env = SurrogateLeggedEnv(N, "cuda", SurrogateConfig(sim=SIM.SimConfig(), episode_length_s=30 * 0.02), seed=5)
    runner = dict(num_steps_per_env=24, save_interval=1000, **MODELS["ppo"])
    algo = dict(num_learning_epochs=2, contain_nonfinite_act=True, contain_nonfinite_envs=True)
    r = OnPolicyRunner(env, dict(runner=runner, algorithm=algo, policy=dict()), log_dir=None, device="cuda")
    r.learn(1)
    assert env.nonfinite_act_envs is r.alg.nonfinite_act_envs                            # the runner's hook reached the env
    env.dof_state[7, 3, 0] = float("nan")
    r.learn(1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(r.alg.actor_critic.arena.flat).all())
    assert all(bool(torch.isfinite(t).all()) for t, _ in _per_env_tensors(env).values() if t.is_floating_point())
