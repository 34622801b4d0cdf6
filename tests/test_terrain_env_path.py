"""SurrogateLeggedEnv on the generated DTC terrain (`SurrogateConfig.terrain`), on the GPU: 64 envs on a 3 x 9 grid of 4 m sub-terrains
with all nine families, tilt off and on.  The placement after reset(), 30 steps through the composition of the oracles of
tests/test_sim_env_path.py / tests/test_sim_tilt_env_path.py (imported, not edited: their env, draws and reset oracle are replaced by
ones that know the terrain, the curriculum tensors and `level_draw`), the curriculum moves against the reset oracle, the logged mean
level, regeneration in place, two trainers, and the opt-out."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import reset_oracle as RO  # noqa: E402
import terrain_oracle as TO  # noqa: E402
import test_sim_env_path as E  # noqa: E402
import test_sim_tilt_env_path as T  # noqa: E402

pytestmark = pytest.mark.gpu
N, R, C, LENGTH, BORDER = 64, 3, 9, 4.0, 1.0
NINE = tuple([1 / 9] * 9)
_HARNESS_DRAWS = E._draws


def _terrain_cfg(seed=7):
    from dtc_amd.terrain import TerrainConfig
    return TerrainConfig(terrain_length=LENGTH, terrain_width=LENGTH, border_size=BORDER, num_rows=R, num_cols=C, terrain_proportions=NINE,
                         max_init_terrain_level=R - 1, seed=seed)


def _oracle_table(seed):
    return TO.generate(TO.config(border_size=BORDER, terrain_length=LENGTH, terrain_width=LENGTH, num_rows=R, num_cols=C,
                                 terrain_proportions=NINE, seed=seed))


def _env(max_len, tilt=False, heading=False, resampling_time=7 * 0.02 + 1e-9, levels=None, n=N, reward_scales=None, seed=7):
    from dtc_amd import sim as SIM
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    s = SIM.SimConfig(resampling_time=resampling_time, border_size=BORDER, tilt=tilt, heading_command=heading)
    kw = {} if reward_scales is None else dict(reward_scales=reward_scales)
    cfg = SurrogateConfig(sim=s, episode_length_s=max_len * s.dt, terrain=_terrain_cfg(seed), **kw)
    return SurrogateLeggedEnv(n, "cuda", cfg, seed=3, terrain_levels=levels), cfg


def _draws(i, dev, n=N):
    d = _HARNESS_DRAWS(i, dev, n)
    d["level_draw"] = torch.randint(0, R, (n,), generator=torch.Generator().manual_seed(300 + i)).to(dev)
    return d


# ------------------------------------------------------------------------------------------------ placement
@pytest.mark.parametrize("tilt", [False, True], ids=["level", "tilt"])
def test_reset_places_the_envs_on_their_sub_terrains(tilt):
    env, cfg = _env(12, tilt=tilt)
    want = _oracle_table(7)
    assert env.custom_origins and env.max_terrain_level == R and env.height_samples is env.terrain.height_field_raw
    assert np.array_equal(env.height_samples.cpu().numpy(), want["table"])
    assert np.array_equal(env.terrain_origins.cpu().numpy().view(np.int32), want["origins"].view(np.int32))
    types, levels = env.terrain_types.cpu().numpy(), env.terrain_levels.cpu().numpy()
    assert env.terrain_types.dtype == torch.int64 and np.array_equal(types, np.floor(np.arange(N) / (N / C)).astype(np.int64))
    assert levels.min() >= 0 and levels.max() <= R - 1 and len(set(levels.tolist())) == R
    before = env.terrain_levels.clone()
    d = _draws(-1, env.device)
    origin = want["origins"][levels, types]
    assert np.array_equal(env.env_origins.cpu().numpy(), origin)
    # the rows as the reset writes them (reset() goes on with one env step)
    env.reset_buf.fill_(1)
    env._reset_envs(d)
    root = env.root_states.cpu().numpy()
    xy = RO.rand_float(-0.5, 0.5, d["u_reset"].cpu().numpy()[:, 12 + RO.ORIGIN:12 + RO.ORIGIN + 2])
    assert np.abs(root[:, :2] - origin[:, :2]).max() <= 0.5 + 1e-6 and np.array_equal(root[:, :2], origin[:, :2] + xy)
    assert np.array_equal(root[:, 2], np.float32(cfg.sim.nominal_height) + origin[:, 2])
    assert not env.init_done
    env.reset(draws=d)
    assert torch.equal(env.terrain_levels, before) and env.init_done                      # the initial reset moves no level
    assert np.array_equal(env.env_origins.cpu().numpy(), origin)


# ------------------------------------------------------------------------------------------------ the composition of the oracles
def _patch_harness(monkeypatch, env, cfg, max_len):
    """Hand the terrain env, its draws and a reset oracle that knows the curriculum to the imported composition."""
    last = {}
    types, origins = env.terrain_types.cpu().numpy(), env.terrain_origins.cpu().numpy()
    real_config, real_reset, real_snapshot = RO.config, RO.reset_idx, E._snapshot
    seen = dict(up=0, down=0, randint=0, resets=0)

    def draws(i, dev, n=N):
        last["draws"] = _draws(i, dev, n)
        return last["draws"]

    def snapshot(e):
        last["B"] = real_snapshot(e)
        return last["B"]

    def config(**kw):
        kw.update(terrain_curriculum=True, custom_origins=True, max_terrain_level=R, env_length=LENGTH)
        return real_config(**kw)

    def reset_idx(Z, k, u, _level_draw, height_noise):
        Z["terrain_levels"], Z["terrain_types"], Z["terrain_origins"] = last["B"]["terrain_levels"].copy(), types, origins
        out = real_reset(Z, k, u, last["draws"]["level_draw"].cpu().numpy(), height_noise)
        assert np.array_equal(env.terrain_levels.cpu().numpy(), Z["terrain_levels"]), "terrain_levels after the reset"
        assert np.array_equal(env.env_origins.cpu().numpy().view(np.int32), Z["env_origins"].view(np.int32)), "env_origins after the reset"
        if out["count"]:
            level = env.extras["episode"]["terrain_level"]
            assert level.dtype == torch.float32 and float(level) == float(out["terrain_level_mean"]) == float(np.float32(Z["terrain_levels"].mean()))
            for key in ("up", "down", "randint"):
                seen[key] += out["branches"]["move_" + key if key != "randint" else key]
            seen["resets"] += out["count"]
        return out

    for mod in (E, T):
        monkeypatch.setattr(mod, "N", N)
        monkeypatch.setattr(mod, "STEPS", 30)
        monkeypatch.setattr(mod, "MAX_LEN", max_len)
    monkeypatch.setattr(E, "_draws", draws)
    monkeypatch.setattr(E, "_snapshot", snapshot)
    monkeypatch.setattr(RO, "config", config)
    monkeypatch.setattr(RO, "reset_idx", reset_idx)
    monkeypatch.setattr(E, "_env", lambda rough=False, **kw: (env, cfg))
    monkeypatch.setattr(T, "_env", lambda heading=False, **kw: (env, cfg))
    return seen


def test_env_equals_the_composition_of_the_oracles_on_the_terrain(monkeypatch):
    """tests/test_sim_env_path.py's composition, step by step and bit for bit (the reward sums to that file's own bound), with the
    generated table under it and the curriculum tensors and level_draw handed to the reset oracle."""
    env, cfg = _env(E.MAX_LEN)
    seen = _patch_harness(monkeypatch, env, cfg, E.MAX_LEN)
    E.test_env_equals_the_composition_of_the_oracles(True)
    assert seen["resets"] > 0, seen
    assert env.height_samples.cpu().numpy().any()


def test_tilt_env_equals_the_composition_of_the_oracles_on_the_terrain(monkeypatch):
    from dtc_amd.env.surrogate import _SCALES
    env, cfg = _env(T.MAX_LEN, tilt=True, resampling_time=5 * 0.02 + 1e-9, reward_scales=dict(_SCALES, orientation=-0.2, orientation_roll=-0.1))
    seen = _patch_harness(monkeypatch, env, cfg, T.MAX_LEN)
    T.test_tilt_env_equals_the_composition_of_the_oracles(False)
    assert seen["resets"] > 0, seen


# ------------------------------------------------------------------------------------------------ the curriculum
@pytest.mark.parametrize("tilt", [False, True], ids=["level", "tilt"])
def test_curriculum_moves(tilt):
    """Episodes of 8 steps.  Before the step that ends them, the envs of kind 0 are placed beyond 0.6 * env_length from their origin,
    those of kind 1 get a large command and have not moved, those of kind 2 neither.  Against the reset oracle on the kernel's own
    inputs, and against the rule: up one level with the new level's origin (from level R - 1: level_draw), down one level (level 0
    stays), unchanged."""
    n = np.arange(N)
    levels0 = torch.from_numpy(n % R)
    kind = (n // R) % 3
    env, cfg = _env(8, tilt=tilt, resampling_time=10.0, levels=levels0)
    dev = env.device
    assert cfg.max_episode_length == 8
    still = torch.full((N, 26), 0.5)                                                      # default pose, no origin offset, no velocity, no command

    def draws(i):
        return dict(_draws(i, dev), u_reset=still.to(dev))
    zero = torch.zeros(N, 12, device=dev)
    env.reset(draws=draws(-1))
    captured, inner = {}, env.env_reset

    def env_reset(**kw):
        for key in ("root_states", "env_origins", "commands", "terrain_levels", "reset_buf"):
            captured[key] = kw[key].detach().cpu().numpy().copy()
        return inner(**kw)
    for i in range(16):
        if int(env.episode_length_buf.max()) == 8:
            break
        env.step(zero, draws(i))
    else:
        raise AssertionError("no env reached the end of its episode")
    before = env.terrain_levels.cpu().numpy().copy()
    env.root_states[torch.from_numpy(kind == 0).to(dev), 0] += 0.7 * LENGTH
    env.commands[torch.from_numpy(kind == 1).to(dev), :2] = 3.0
    env.env_reset = env_reset
    d = draws(99)
    _, _, _, dones, extras = env.step(zero, d)
    env.env_reset = inner
    # envs on ground below zero (stairs down, pits) end every step on the base-height rule; one of them moved off such ground is not reset
    done = captured["reset_buf"] != 0
    assert np.array_equal(done, dones.cpu().numpy()) and done.sum() >= N // 2 and np.array_equal(before, levels0.numpy())
    draw = d["level_draw"].cpu().numpy()
    dist = np.linalg.norm(captured["root_states"][:, :2] - captured["env_origins"][:, :2], axis=1)
    assert (dist[kind == 0] > 0.6 * LENGTH + 0.1).all() and (dist[kind != 0] < 0.2).all()
    want = np.where(kind == 0, np.where(before + 1 >= R, draw, before + 1), np.where(kind == 1, np.maximum(before - 1, 0), before))
    want = np.where(done, want, before)
    got = env.terrain_levels.cpu().numpy()
    assert np.array_equal(got, want)
    assert (done & (kind == 0) & (before == R - 1)).any() and (done & (kind == 1) & (before == 0)).any() and (want != before).sum() > N // 4
    origins, types = env.terrain_origins.cpu().numpy(), env.terrain_types.cpu().numpy()
    assert np.array_equal(env.env_origins.cpu().numpy(), origins[want, types])
    # the reset oracle on the kernel's inputs
    f = np.float32
    Z = dict(reset_buf=captured["reset_buf"] != 0, root_states=captured["root_states"], env_origins=captured["env_origins"],
             commands=captured["commands"], terrain_levels=captured["terrain_levels"], terrain_types=types, terrain_origins=origins,
             dof_pos=np.zeros((N, 12), f), dof_vel=np.zeros((N, 12), f), default_dof_pos=env.default_dof_pos.cpu().numpy().reshape(-1),
             base_init_state=np.array(cfg.reset_config().base_init_state, dtype=f), forces=np.zeros((N, 17, 3), f),
             motor_strengths=np.zeros((N, 12), f), height_noise_offset=np.zeros((N, 693), f), lag_buffer=[],
             episode_sums=np.zeros((1, N), f))
    for name in RO.ROW_ITEMS + RO.TIME_ITEMS:
        Z[name] = np.zeros((N, 1), f) if name in RO.ROW_ITEMS else np.zeros((1, N, 1), f)
    k = RO.config(terrain_curriculum=True, custom_origins=True, heading_command=False, max_terrain_level=R, env_length=LENGTH,
                  max_episode_length_s=cfg.episode_length_s)
    out = RO.reset_idx(Z, k, d["u_reset"].cpu().numpy(), draw, 0.0)
    assert np.array_equal(Z["terrain_levels"], got) and np.array_equal(Z["env_origins"], env.env_origins.cpu().numpy())
    assert np.array_equal(Z["root_states"].view(np.int32), env.root_states.cpu().numpy().view(np.int32))
    assert out["branches"]["move_up"] == (done & (kind == 0)).sum() and out["branches"]["move_down"] == (done & (kind == 1)).sum()
    level = extras["episode"]["terrain_level"]
    assert isinstance(level, torch.Tensor) and level.is_cuda and level.dtype == torch.float32
    assert float(level) == float(np.float32(got.astype(np.float32).mean())) == float(out["terrain_level_mean"])


# ------------------------------------------------------------------------------------------------ regeneration
def test_regenerate_terrain_in_place():
    env, _ = _env(12)
    env.reset(draws=_draws(-1, env.device))
    levels, table = env.terrain_levels.clone(), env.height_samples
    env.env_origins[:, 2] = 123.0                                                         # whatever stood there, the new origins replace it
    holder = env.sim.height_samples
    env.regenerate_terrain(8)
    want = _oracle_table(8)
    assert env.height_samples is table and holder.data_ptr() == table.data_ptr()
    assert np.array_equal(table.cpu().numpy(), want["table"]) and not np.array_equal(want["table"], _oracle_table(7)["table"])
    assert torch.equal(env.terrain_levels, levels)
    origin = want["origins"][levels.cpu().numpy(), env.terrain_types.cpu().numpy()]
    assert np.array_equal(env.env_origins.cpu().numpy(), origin)
    env.step(torch.zeros(N, 12, device=env.device), _draws(0, env.device))                 # the kernels stand on the new table
    assert bool(torch.isfinite(env.obs_buf).all())


# ------------------------------------------------------------------------------------------------ trainers
@pytest.mark.parametrize("model", ["ppo", "rdppo"])
def test_trainers_learn_on_the_terrain(model, tmp_path):
    from dtc_amd.runners import OnPolicyRunner
    import test_sim_runner_path as RP
    torch.manual_seed(11)
    env, cfg = _env(30, n=16)
    runner = dict(num_steps_per_env=24, save_interval=1000, **RP.MODELS[model])
    r = OnPolicyRunner(env, dict(runner=runner, algorithm=dict(num_learning_epochs=2), policy=dict()), log_dir=str(tmp_path),
                       device="cuda")
    logged, log = [], r.log
    r.log = lambda *a, **k: logged.append(log(*a, **k)) or logged[-1]
    r.learn(2)
    torch.cuda.synchronize()
    ac = r.alg.actor_critic
    assert bool(torch.isfinite(ac.arena.flat).all()) if hasattr(ac, "arena") else all(bool(torch.isfinite(p).all()) for p in ac.parameters())
    assert len(logged) == 2 and all("Episode/terrain_level" in s and 0 <= s["Episode/terrain_level"] <= R - 1 for s in logged)
    assert float(env.terrain_levels.float().mean()) >= 0 and bool(torch.isfinite(env.obs_buf).all())


# ------------------------------------------------------------------------------------------------ the opt-out
def test_without_a_terrain_the_env_is_the_one_built_the_old_way():
    from dtc_amd import sim as SIM, synthetic as S
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    table = S.reward_table()
    a = SurrogateLeggedEnv(16, "cuda", SurrogateConfig(terrain=None), table, seed=3)
    b = SurrogateLeggedEnv(16, "cuda", SurrogateConfig(), table, seed=3)
    assert a.terrain is None and not a.custom_origins and "terrain_level" not in a._episode
    i = torch.arange(16, device=a.device)
    old_origins = torch.stack([(i % 32) * 1.0, (i // 32 % 24) * 1.0, torch.zeros_like(i)], dim=1).float()
    assert torch.equal(a.env_origins, old_origins) and torch.equal(a.height_samples.cpu(), table) and not a.terrain_levels.any()
    flat = SurrogateLeggedEnv(16, "cuda", SurrogateConfig(), seed=3)
    assert torch.equal(flat.height_samples.cpu(), SIM.flat_table())
    a.reset(), b.reset()
    for step in range(3):
        act = E._actions(step, a.device)
        oa, ob = a.step(act), b.step(act)
        for x, y in zip(oa[:4], ob[:4]):
            assert torch.equal(x, y)
        assert set(oa[4]["episode"]) == set(ob[4]["episode"]) == {"rew_" + n for n in a.env_rewards.cfg.names}
    with pytest.raises(ValueError):
        a.regenerate_terrain(1)
