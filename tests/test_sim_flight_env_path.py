"""SurrogateLeggedEnv with `SimConfig.flight` on the GPU, on the terms of tests/test_sim_env_path.py: 16 envs x 30 steps on a small
generated terrain (gap and pit families only, 2 x 2 sub-terrains of 4 m), every draw an input, with the yaw-only base, with tilt and
with the actuator.  The compositions of tests/test_sim_env_path.py / tests/test_sim_tilt_env_path.py run unchanged, to their own
bounds, in the terrain harness of tests/test_terrain_env_path.py, with tests/sim_flight_oracle.py standing where they call the
surrogate step's oracle; airborne and crashed are compared bit for bit after every step.  After the first reset two envs are lifted
by 0.5 m (they fall and land) and one is sunk by 0.5 m (its support lies more than max_step_up above it: a crash), so that every
branch is on the path whatever the terrain seed gives.  Then the curriculum effect of a crash against a run without flight, the
trainers, and the default path."""
import types

import numpy as np
import pytest
import torch

import sim_flight_oracle as FO
import sim_oracle as O
import test_sim_actuator_env_path as AE
import test_sim_env_path as E
import test_sim_tilt_env_path as T
import test_terrain_env_path as TP

pytestmark = pytest.mark.gpu
N, STEPS, R, C = 16, 30, 2, 2
LIFTED, SUNK = (3, 4), 5
GAP_AND_PIT = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.5)


def _terrain_cfg(seed=7):
    from dtc_amd.terrain import TerrainConfig
    return TerrainConfig(terrain_length=TP.LENGTH, terrain_width=TP.LENGTH, border_size=TP.BORDER, num_rows=R, num_cols=C,
                         terrain_proportions=GAP_AND_PIT, max_init_terrain_level=R - 1, seed=seed)


def _env(tilt, act, max_len, flight=True, levels=None, resampling_time=None, intervene=True):
    from dtc_amd import sim as SIM
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    from dtc_amd.env.surrogate import _SCALES
    rt = (5 if tilt else 7) * 0.02 + 1e-9 if resampling_time is None else resampling_time
    s = SIM.SimConfig(resampling_time=rt, border_size=TP.BORDER, tilt=tilt, actuator=AE._actuator() if act else None,
                      flight=SIM.FlightConfig() if flight else None)
    scales = dict(_SCALES, orientation=-0.2, orientation_roll=-0.1) if tilt else dict(_SCALES)
    cfg = SurrogateConfig(sim=s, episode_length_s=max_len * s.dt, reward_scales=scales, terrain=_terrain_cfg())
    env = SurrogateLeggedEnv(N, "cuda", cfg, seed=3, terrain_levels=levels)
    if intervene:
        inner = env.reset

        def reset(env_ids=None, draws=None):
            obs = inner(env_ids, draws)
            env.root_states[list(LIFTED), 2] += 0.5
            env.root_states[SUNK, 2] -= 0.5
            return obs
        env.reset = reset
    return env, cfg


def _patch(monkeypatch, env, cfg, tilt, act, max_len):
    """The terrain harness of tests/test_terrain_env_path.py at this file's sizes, then: the draws gain the actuator's, the snapshot
    the new tensors, and the oracle the compositions call for the surrogate step is tests/sim_flight_oracle.py, which also checks
    airborne and crashed (and the actuator's two tensors)."""
    for name, v in (("N", N), ("R", R), ("C", C)):
        monkeypatch.setattr(TP, name, v)
    on_terrain = TP._patch_harness(monkeypatch, env, cfg, max_len)
    last, seen = {}, dict(steps=0, airborne=0, landings=0, crashes=0, resets=0, crash_resets=0, flags=0)
    inner_draws, inner_snapshot = E._draws, E._snapshot
    dec = cfg.sim.decimation

    def draws(i, dev, n=N):
        d = inner_draws(i, dev, n)
        if act:
            g = torch.Generator().manual_seed(400 + i)
            d["lag_choice"] = [int(v) for v in torch.randint(1, 5, (dec,), generator=g)]
            d["u_push"] = torch.rand(n, 2, generator=g).to(dev)
        last["draws"] = d
        return d

    def snapshot(e):
        B = inner_snapshot(e)
        for name in FO.FLAGS + (("lag_state", "push_vel") if act else ()):
            B[name] = getattr(e, name).cpu().numpy().copy()
        last["push"] = act and (e.common_step_counter + 1) % cfg.sim.push_interval in (0, 1)
        return B

    def sim_step(B, k, tables, a, hs, u_cmd):
        d, trace = last["draws"], []
        kw = dict(lag_choice=d["lag_choice"], u_push=d["u_push"].cpu().numpy(), push=last["push"]) if act else {}
        W = FO.sim_step(B, k, tables, a, hs, u_cmd, trace=trace, tilt=tilt, act=act, **kw)
        done = env.reset_buf.cpu().numpy() != 0
        for name in FO.FLAGS:                                             # a reset leaves the flags of the step that caused it
            got = getattr(env, name).cpu().numpy()
            assert got.dtype == np.uint8 and np.array_equal(got, W[name]), name
        for name in (("lag_state", "push_vel") if act else ()):
            got = getattr(env, name).cpu().numpy()
            assert np.array_equal(E._bits(got[~done]), E._bits(W[name][~done])), f"{name} of the envs that went on"
            assert (got[done] == 0).all(), f"{name} of the reset envs"
        air = np.stack([s["air"] for s in trace])
        seen["steps"] += 1
        seen["airborne"] += int(air.sum())
        seen["landings"] += int((air[:-1] & ~air[1:]).sum() + (~air[0] & (B["airborne"] == 1)).sum())
        seen["crashes"] += int(W["crashed"].sum())
        seen["resets"] += int(done.sum())
        seen["crash_resets"] += int((done & (W["crashed"] == 1)).sum())
        seen["flags"] += int(W["airborne"].sum())
        assert (done | (W["crashed"] == 0)).all()                         # every crash ends its episode
        assert (W["contact_forces"][W["crashed"] == 1, 0, 2] == np.float32(cfg.sim.flight.crash_force)).all()
        return W

    shim = types.SimpleNamespace(STATE=O.STATE, INPUTS=O.INPUTS, config_dict=FO.config_dict, sim_step=sim_step)
    monkeypatch.setattr(E, "O", shim)
    monkeypatch.setattr(T, "TO", shim)
    for mod in (E, T):
        monkeypatch.setattr(mod, "N", N)
        monkeypatch.setattr(mod, "STEPS", STEPS)
    monkeypatch.setattr(E, "_draws", draws)
    monkeypatch.setattr(E, "_snapshot", snapshot)
    return seen, on_terrain


def _seen_enough(seen, on_terrain):
    assert seen["steps"] == STEPS and seen["airborne"] > 0 and seen["landings"] > 0 and seen["flags"] > 0, seen
    assert seen["crashes"] > 0 and seen["crash_resets"] == seen["crashes"] and seen["resets"] < N * STEPS // 2, seen
    assert on_terrain["resets"] > 0, on_terrain


@pytest.mark.parametrize("act", [False, True], ids=["plain", "actuator"])
def test_env_equals_the_composition_of_the_oracles(monkeypatch, act):
    env, cfg = _env(False, act, E.MAX_LEN)
    seen, on_terrain = _patch(monkeypatch, env, cfg, False, act, E.MAX_LEN)
    E.test_env_equals_the_composition_of_the_oracles(True)
    _seen_enough(seen, on_terrain)
    assert env.height_samples.cpu().numpy().any()


def test_tilt_env_equals_the_composition_of_the_oracles(monkeypatch):
    env, cfg = _env(True, False, T.MAX_LEN)
    seen, on_terrain = _patch(monkeypatch, env, cfg, True, False, T.MAX_LEN)
    T.test_tilt_env_equals_the_composition_of_the_oracles(False)
    _seen_enough(seen, on_terrain)


def test_a_crash_ends_the_episode_and_moves_the_terrain_level():
    """Two envs alike, with and without flight, on the same draws with zero actions.  After the reset and one step env SUNK is
    placed 0.5 m under its support and given a large command.  Against the oracle first: with flight the step crashes it and check_termination resets it;
    without flight the base is put back on its support and nothing resets it.  Then the envs: with flight it is reset in that
    step and, having walked less than half the commanded distance, its terrain level moves down from 1 to 0; without flight
    it is not reset in that step and its level stays."""
    from oracle import heights as OH, observations as OB
    import sim_tilt_oracle as TO
    levels = torch.ones(N, dtype=torch.int64)
    out = {}
    for flight in (True, False):
        env, cfg = _env(False, False, 12, flight=flight, levels=levels, resampling_time=10.0, intervene=False)
        dev, s = env.device, cfg.sim
        still = torch.full((N, 26), 0.5)

        def draws(i):
            d = TP._draws(i, dev, N)
            d["level_draw"] = d["level_draw"] % R
            return dict(d, u_reset=still.to(dev))
        zero = torch.zeros(N, 12, device=dev)
        env.reset(draws=draws(-1))
        env.step(zero, draws(0))
        env.root_states[SUNK, 2] -= 0.5
        env.commands[SUNK, :2] = 3.0                                      # a command it has not followed: a reset moves it down a level
        before = E._snapshot(env)
        for name in (FO.FLAGS if flight else ()):
            before[name] = getattr(env, name).cpu().numpy().copy()
        assert before["terrain_levels"][SUNK] == 1 and before["episode_length_buf"][SUNK] >= 1
        # the oracle first
        tables = {k: v.cpu().numpy() for k, v in env.sim.tables.items()}
        hs = env.height_samples.cpu().numpy()
        d = draws(1)
        if flight:
            W = FO.sim_step(before, FO.config_dict(s, hs.shape[0], hs.shape[1]), tables, zero.cpu().numpy(), hs, d["u_cmd"].cpu().numpy())
            assert W["crashed"][SUNK] == 1 and W["crashed"].sum() == 1
        else:
            W = O.sim_step(before, TO.config_dict(s, hs.shape[0], hs.shape[1]), tables, zero.cpu().numpy(), hs, d["u_cmd"].cpu().numpy())
        mh = OH.get_heights(hs, W["root_states"], cfg.grid.points_x, cfg.grid.points_y, s.border_size, s.horizontal_scale, s.vertical_scale)
        term_in = dict(contact_forces=W["contact_forces"], termination_contact_indices=[0], episode_length_buf=W["episode_length_buf"],
                       projected_gravity=W["projected_gravity"], root_states=W["root_states"], measured_heights=mh)
        want, _, _ = OB.check_termination(term_in, 12)
        assert bool(want[SUNK]) == flight
        # then the env
        _, _, _, dones, _ = env.step(zero, d)
        assert np.array_equal(dones.cpu().numpy(), want)
        out[flight] = (bool(dones[SUNK]), int(env.terrain_levels[SUNK]))
        if flight:
            assert int(env.crashed[SUNK]) == 1 and int(env.episode_length_buf[SUNK]) == 0
    assert out[True] == (True, 0) and out[False] == (False, 1), out


@pytest.mark.parametrize("model", ["ppo", "rdppo"])
def test_trainers_learn_on_the_flight_env(model):
    """One learn() iteration at 16 envs x 24 steps on the gap and pit terrain with tilt, actuator and flight: finite weights,
    observations and rewards, flags that are flags."""
    from dtc_amd.runners import OnPolicyRunner
    import test_sim_runner_path as RP
    torch.manual_seed(11)
    env, cfg = _env(True, True, 30)
    runner = dict(num_steps_per_env=24, save_interval=1000, **RP.MODELS[model])
    r = OnPolicyRunner(env, dict(runner=runner, algorithm=dict(num_learning_epochs=2), policy=dict()), log_dir=None, device="cuda")
    r.learn(1)
    torch.cuda.synchronize()
    ac = r.alg.actor_critic
    assert bool(torch.isfinite(ac.arena.flat).all()) if hasattr(ac, "arena") else all(bool(torch.isfinite(p).all()) for p in ac.parameters())
    assert bool(torch.isfinite(env.obs_buf).all()) and bool(torch.isfinite(env.rew_buf).all()) and bool(torch.isfinite(env.root_states).all())
    assert env.airborne.dtype == torch.uint8 and int(env.airborne.max()) <= 1 and int(env.crashed.max()) <= 1


def test_without_flight_the_env_is_the_one_built_before_and_never_calls_the_new_entry_point(monkeypatch):
    from dtc_amd import _ffi
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    plain = SurrogateLeggedEnv(N, "cuda", SurrogateConfig(), seed=3)
    assert plain.config.sim.flight is None and not hasattr(plain, "airborne") and not hasattr(plain, "crashed")
    env, _ = _env(False, False, 12, intervene=False)
    same, _ = _env(False, False, 12, flight=False, intervene=False)
    assert set(vars(env)) - set(vars(same)) == {"airborne", "crashed"} and set(vars(same)) <= set(vars(env))
    assert env.airborne.shape == (N,) and env.crashed.shape == (N,) and env.airborne.dtype == env.crashed.dtype == torch.uint8

    def refuse(*a, **kw):
        raise AssertionError("dtc_sim_step_fly called by an env without flight")
    lib = _ffi.lib()
    monkeypatch.setattr(lib, "dtc_sim_step_fly", refuse, raising=True)
    dev = plain.device
    plain.reset(draws=E._draws(-1, dev))
    for i in range(3):
        obs, _, rew, _, _ = plain.step(E._actions(i, dev), E._draws(i, dev))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(rew).all()) and int(plain.episode_length_buf.max()) >= 1
    with pytest.raises(AssertionError, match="dtc_sim_step_fly"):
        env.reset(draws=TP._draws(-1, dev, N))
