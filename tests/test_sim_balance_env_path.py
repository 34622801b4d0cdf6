"""SurrogateLeggedEnv with `SimConfig.balance` on the GPU, on the terms of tests/test_sim_env_path.py: 16 envs, every draw an input,
`BALANCE_SCALES` added to the reward scales.  The composition of tests/test_sim_tilt_env_path.py runs unchanged, bit for bit and
the reward sums to its own bound, with the surrogate step's oracle followed by tests/sim_balance_oracle.py (and, where the env has
contacts, by tests/sim_contact_oracle.py behind that) where it calls the step's oracle: once with tilt on the rough table, once with
tilt, actuator, flight and contacts on a generated stairs-and-stones terrain (the harness of tests/test_sim_flight_env_path.py).
lean and fallen are compared after every step.  Then an env that lifts three legs and falls, a NaN env, the trainers, and the
opt-out."""
import types

import numpy as np
import pytest
import torch

import sim_balance_oracle as BO
import sim_tilt_oracle as TO
import test_sim_contact_env_path as CE
import test_sim_env_path as E
import test_sim_flight_env_path as FE
import test_sim_tilt_env_path as T
import test_terrain_env_path as TP

pytestmark = pytest.mark.gpu
N, STEPS = 16, 12
PER_ENV = ("root_states", "dof_state", "base_pos", "base_quat", "projected_gravity", "base_lin_vel", "base_ang_vel", "rigid_body_state",
           "contact_forces", "commands", "rew_buf", "reset_buf", "obs_buf", "privileged_obs_buf", "episode_length_buf", "contact_filt")


def _scales():
    from dtc_amd.env.surrogate import _SCALES, BALANCE_SCALES
    return dict(_SCALES, orientation_roll=-0.1, **BALANCE_SCALES)


def _rough_env(max_len, n=N):
    from dtc_amd import sim as SIM, synthetic as S
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    s = SIM.SimConfig(resampling_time=5 * 0.02 + 1e-9, tilt=True, balance=SIM.BalanceConfig())
    cfg = SurrogateConfig(sim=s, episode_length_s=max_len * s.dt, reward_scales=_scales())
    return SurrogateLeggedEnv(n, "cuda", cfg, S.reward_table(), seed=3), cfg


def _terrain_env(max_len, n=N):
    from dtc_amd import sim as SIM
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    from dtc_amd.env.surrogate import CONTACT_SCALES
    from dtc_amd.terrain import TerrainConfig
    import test_sim_actuator_env_path as AE
    s = SIM.SimConfig(resampling_time=5 * 0.02 + 1e-9, border_size=TP.BORDER, tilt=True, actuator=AE._actuator(), flight=SIM.FlightConfig(),
                      contacts=SIM.ContactConfig(), balance=SIM.BalanceConfig())
    terrain = TerrainConfig(terrain_length=TP.LENGTH, terrain_width=TP.LENGTH, border_size=TP.BORDER, num_rows=FE.R, num_cols=FE.C,
                            terrain_proportions=CE.STAIRS_AND_STONES, max_init_terrain_level=FE.R - 1, seed=7)
    cfg = SurrogateConfig(sim=s, episode_length_s=max_len * s.dt, reward_scales=dict(_scales(), **CONTACT_SCALES), terrain=terrain)
    return SurrogateLeggedEnv(n, "cuda", cfg, seed=3), cfg


def _flat_env(max_len=200, n=N):
    """The yaw-only base on flat ground, long episodes, commands that stay: what happens is the actions' doing."""
    from dtc_amd import sim as SIM
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    s = SIM.SimConfig(balance=SIM.BalanceConfig())
    cfg = SurrogateConfig(sim=s, episode_length_s=max_len * s.dt, reward_scales=_scales())
    return SurrogateLeggedEnv(n, "cuda", cfg, seed=3), cfg


def _snapshot_with_lean(monkeypatch):
    inner = E._snapshot

    def snapshot(e):
        B = inner(e)
        B["lean"] = e.lean.cpu().numpy().copy()
        return B
    monkeypatch.setattr(E, "_snapshot", snapshot)


def _with_balance(env, cfg, shim):
    """A shim whose surrogate step is `shim`'s followed by the balance oracle; lean and fallen are checked after every step."""
    seen = dict(steps=0, leaning=0, fallen=0, fall_resets=0, stance_short=0)
    inner, s = shim.sim_step, cfg.sim
    bk, feet = BO.balance_dict(s.balance, s.sim_dt, s.decimation), list(s.feet)

    def sim_step(B, k, tables, a, hs, u_cmd):
        W = inner(B, k, tables, a, hs, u_cmd)
        trace = {}
        out = BO.balance(dict(W, lean=B["lean"]), feet, bk, trace=trace)
        done = env.reset_buf.cpu().numpy() != 0
        got = env.fallen.cpu().numpy()                                    # a reset leaves the flag of the step that caused it
        assert got.dtype == np.uint8 and np.array_equal(got, out["fallen"]), "fallen"
        lean = env.lean.cpu().numpy()
        assert np.array_equal(E._bits(lean[~done]), E._bits(out["lean"][~done])), "lean of the envs that went on"
        assert (lean[done] == 0).all(), "lean of the reset envs"
        assert abs(float(env.extras["episode"]["fall_rate"]) - out["fallen"].mean()) < 1e-6
        fell = out["fallen"] != 0
        seen["steps"] += 1
        seen["leaning"] += int(trace["on"].sum())
        seen["fallen"] += int(fell.sum())
        seen["fall_resets"] += int((fell & done).sum())
        seen["stance_short"] += int((trace["k"] < 3).sum())
        assert (done | ~fell).all()                                       # every fall ends its episode
        W = dict(W)
        for name in BO.WRITTEN:
            if name not in ("lean", "fallen"):
                W[name] = out[name]
        return W
    return types.SimpleNamespace(STATE=shim.STATE, INPUTS=shim.INPUTS, config_dict=shim.config_dict, sim_step=sim_step), seen


def test_env_equals_the_composition_of_the_oracles_with_tilt_on_the_rough_table(monkeypatch):
    env, cfg = _rough_env(T.MAX_LEN)
    assert {"orientation", "termination", "ang_vel_xy"} <= set(env.env_rewards.cfg.names)
    _snapshot_with_lean(monkeypatch)
    shim, seen = _with_balance(env, cfg, types.SimpleNamespace(STATE=TO.STATE, INPUTS=TO.INPUTS, config_dict=TO.config_dict, sim_step=TO.sim_step))
    import reward_cases as K
    reference = K.reference

    def with_termination(R, rcfg, sums):
        # termination is a flag times a scale, which the reward tests hold to equal flags and for which the oracle reports no float32
        # error of its own: an e32 of 0 holds its sum to the floor of the composition's bound, K.bound(0) = 2^-20 of its size
        r64, e32 = reference(R, rcfg, sums)
        e32.setdefault("termination", 0.0)
        return r64, e32
    monkeypatch.setattr(K, "reference", with_termination)
    monkeypatch.setattr(T, "TO", shim)
    monkeypatch.setattr(T, "_env", lambda heading, **kw: (env, cfg))
    assert (T.N, T.STEPS) == (N, STEPS)
    T.test_tilt_env_equals_the_composition_of_the_oracles(False)
    print(seen)
    assert seen["steps"] == STEPS and seen["leaning"] > 0 and seen["stance_short"] > 0, seen


def test_env_equals_the_composition_of_the_oracles_with_everything_on_stairs_and_stones(monkeypatch):
    assert FE.N == N
    env, cfg = _terrain_env(T.MAX_LEN)
    _snapshot_with_lean(monkeypatch)                                      # ahead of the flight harness, which wraps the snapshot it finds
    flight, on_terrain = FE._patch(monkeypatch, env, cfg, True, True, T.MAX_LEN)
    for mod in (E, T):
        monkeypatch.setattr(mod, "STEPS", STEPS)
    shim, seen = _with_balance(env, cfg, E.O)
    contacts = CE._with_contacts(monkeypatch, env, cfg, shim)
    T.test_tilt_env_equals_the_composition_of_the_oracles(False)
    print(seen, contacts, flight)
    assert seen["steps"] == contacts["steps"] == flight["steps"] == STEPS and seen["leaning"] > 0 and seen["stance_short"] > 0, seen
    assert env.height_samples.cpu().numpy().any() and set(env.terrain_types.cpu().numpy().tolist()) == {0, 1}


def _lift(n, legs, depth=3.0):
    """Zero actions, but env `n` folds the knees of `legs` (the crouch of tests/test_sim_env_path.py, for those legs alone)."""
    a = torch.zeros(N, 12)
    for l in legs:
        a[n, 3 * l:3 * l + 3] = depth * torch.tensor([0.0, -2.0, 2.4])
    return a


def _still_draws(i, dev):
    d = E._draws(i, dev, N)
    d["u_cmd"] = torch.full((N, 3), 0.5, device=dev)                      # the middle of every command range: xy under 0.1 are zeroed
    d["u_reset"] = torch.full((N, 26), 0.5, device=dev)                   # ... and of every reset range: the default pose, at rest
    return d


def test_an_env_that_lifts_three_legs_falls_and_is_reset_and_the_others_do_not_notice():
    """Env 6 folds three legs and stands on its front left foot: the support is a point 0.2 m from the base, the lean grows until
    `fall_angle`, `fallen` and `reset_buf` are set in the same step and the reset clears the lean.  The other fifteen envs stand
    still; they leave the bits of a run in which env 6 stood still too."""
    X, steps = 6, 40
    runs = []
    for lifting in (True, False):
        env, cfg = _flat_env()
        dev = env.device
        env.reset(draws=_still_draws(-1, dev))
        a = (_lift(X, (1, 2, 3)) if lifting else torch.zeros(N, 12)).to(dev)
        rec = []
        for i in range(steps):
            before = env.lean[X].cpu().numpy().copy()
            env.step(a, _still_draws(i, dev))
            rec.append(dict({name: getattr(env, name).cpu().numpy().copy() for name in PER_ENV + ("lean", "fallen")}, lean_before=before))
        runs.append(rec)
    fell, still = runs
    others = np.arange(N) != X
    when = [i for i, r in enumerate(fell) if r["fallen"][X]]
    assert when, "env 6 never fell"
    i = when[0]
    r = fell[i]
    fall_angle = cfg.sim.balance.fall_angle
    assert 5 < i < steps - 1 and r["reset_buf"][X] == 1 and (r["lean"][X] == 0).all() and r["episode_length_buf"][X] == 0
    assert 0 < np.hypot(*r["lean_before"][:2]) <= fall_angle and r["contact_forces"][X, 0, 2] == np.float32(cfg.sim.balance.fall_force)
    assert r["projected_gravity"][X, 2] > -np.cos(0.7) and abs(np.linalg.norm(r["base_quat"][X]) - 1) < 1e-6
    mags = [np.hypot(*q["lean"][X, :2]) for q in fell[:i]]
    assert mags[-1] > 0.5 and all(b >= a for a, b in zip(mags, mags[1:]))                  # it tipped steadily, towards the lifted legs
    assert not any(q["fallen"][others].any() or q["lean"][others].any() or q["reset_buf"][others].any() for q in fell)
    assert not fell[i + 1]["fallen"][X] and (fell[i + 1]["lean"][X] == 0).all()            # the step after the reset is exempt
    assert not any(q["fallen"].any() or q["lean"].any() for q in still)
    for j, (p, q) in enumerate(zip(fell, still)):
        for name in PER_ENV + ("lean", "fallen"):
            assert np.array_equal(E._bits(p[name][others]), E._bits(q[name][others])), f"step {j}: {name}"


def test_a_nan_env_is_contained_and_the_others_keep_their_bits():
    """Odd envs lift the two legs of their right side and lean; after three steps env 5 gets NaN joints.  In that step its lean and
    its flag are zero (the containment's rows), it is reset, and every other env leaves the clean run's bits."""
    bad = 5
    runs = []
    for poison in (False, True):
        env, cfg = _flat_env()
        dev = env.device
        env.reset(draws=_still_draws(-1, dev))
        a = sum(_lift(n, (1, 3), depth=1.0) for n in range(1, N, 2)).to(dev)
        for i in range(6):
            if poison and i == 4:
                env.dof_state[bad] = float("nan")
            env.step(a, _still_draws(i, dev))
            if i == 4:
                at = {name: getattr(env, name).cpu().numpy().copy() for name in ("lean", "fallen", "reset_buf", "contact_forces", "rew_buf", "obs_buf")}
        runs.append((at, {name: getattr(env, name).cpu().numpy().copy() for name in PER_ENV + ("lean", "fallen")}))
    (clean_at, clean), (hurt_at, hurt) = runs
    others = np.arange(N) != bad
    assert clean_at["lean"][bad].any() and clean["lean"][1::2].any(axis=1).all() and not clean["lean"][0::2].any()
    assert hurt_at["reset_buf"][bad] == 1 and not hurt_at["lean"][bad].any() and hurt_at["fallen"][bad] == 0
    assert not hurt_at["contact_forces"][bad].any() and np.isfinite(hurt_at["rew_buf"]).all() and np.isfinite(hurt_at["obs_buf"]).all()
    for name in clean:
        assert np.array_equal(E._bits(clean[name][others]), E._bits(hurt[name][others])), name
    assert np.isfinite(hurt["lean"]).all() and np.isfinite(hurt["root_states"]).all()


@pytest.mark.parametrize("model", ["ppo", "rdppo"])
def test_trainers_learn_on_the_balance_env(model, tmp_path, capsys):
    """Two learn() iterations at 16 envs x 24 steps on the stairs-and-stones terrain with tilt, actuator, flight, contacts and
    balance: finite weights, observations and rewards, a fall_rate entry in what the runner logs, and an env step that reads
    nothing back."""
    from dtc_amd.runners import OnPolicyRunner
    import test_sim_runner_path as RP
    torch.manual_seed(11)
    env, cfg = _terrain_env(30)
    runner = dict(num_steps_per_env=24, save_interval=1000, **RP.MODELS[model])
    r = OnPolicyRunner(env, dict(runner=runner, algorithm=dict(num_learning_epochs=2), policy=dict()), log_dir=str(tmp_path), device="cuda")
    logged, inner = [], r.log
    r.log = lambda *a, **kw: logged.append(inner(*a, **kw))
    r.learn(2)
    torch.cuda.synchronize()
    ac = r.alg.actor_critic
    assert bool(torch.isfinite(ac.arena.flat).all()) if hasattr(ac, "arena") else all(bool(torch.isfinite(p).all()) for p in ac.parameters())
    assert bool(torch.isfinite(env.obs_buf).all()) and bool(torch.isfinite(env.rew_buf).all()) and bool(torch.isfinite(env.lean).all())
    assert len(logged) == 2 and all(0.0 <= s["Episode/fall_rate"] <= 1.0 for s in logged), logged
    assert env.fallen.dtype == torch.uint8 and int(env.fallen.max()) <= 1
    a = torch.zeros(N, 12, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        env.step(a)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_without_balance_the_env_is_the_one_built_before(monkeypatch):
    """balance=None: the binding's dtc_sim_balance and `SimStep.balance` are replaced by functions that raise.  The bytes of the env
    as it was before the option existed are recorded first: a 24-step run from a SimConfig built without naming `balance`.  The
    same seed with `balance=None` spelled out then equals it, tensor for tensor and bit for bit, after every step, and
    tests/test_sim_env_path.py's own check of the surrogate step on evolving state passes, bit for bit with tests/sim_oracle.py as
    before.  With balance set the same call raises."""
    from dtc_amd import _ffi, sim as SIM
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv

    def refuse(*a, **kw):
        raise AssertionError("dtc_sim_balance called")
    monkeypatch.setattr(_ffi.lib(), "dtc_sim_balance", refuse, raising=True)
    monkeypatch.setattr(SIM.SimStep, "balance", refuse)
    runs = []
    for kw in ({}, dict(balance=None)):
        s = SIM.SimConfig(resampling_time=7 * 0.02 + 1e-9, tilt=True, **kw)
        env = SurrogateLeggedEnv(N, "cuda", SurrogateConfig(sim=s, episode_length_s=12 * s.dt, reward_scales=_scales()), seed=3)
        assert s.balance is None and not hasattr(env, "lean") and not hasattr(env, "fallen") and env._balance_rows == ()
        dev = env.device
        env.reset(draws=E._draws(-1, dev))
        rec = []
        for i in range(24):
            _, _, _, _, extras = env.step(E._actions(i, dev), E._draws(i, dev))
            assert "fall_rate" not in extras["episode"]
            rec.append({name: getattr(env, name).cpu().numpy().copy() for name in PER_ENV})
        runs.append(rec)
    for j, (p, q) in enumerate(zip(*runs)):
        for name in PER_ENV:
            assert np.array_equal(E._bits(p[name]), E._bits(q[name])), f"step {j}: {name}"
    assert any(r["reset_buf"].any() for r in runs[0])
    E.test_env_steps_on_evolving_state(True)
    on, _ = _flat_env()
    with pytest.raises(AssertionError, match="dtc_sim_balance called"):
        on.reset(draws=E._draws(-1, on.device))
