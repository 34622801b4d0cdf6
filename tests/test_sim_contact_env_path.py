"""SurrogateLeggedEnv with `SimConfig.contacts` on the GPU, on the terms of tests/test_sim_env_path.py: 33 envs x 12 steps, every
draw an input, `CONTACT_SCALES` added to the reward scales.  The compositions of tests/test_sim_env_path.py /
tests/test_sim_tilt_env_path.py run unchanged, bit for bit and the reward sums to their own bound, with the surrogate step's oracle
followed by tests/sim_contact_oracle.py where they call the step's oracle: once with the plain yaw base on the rough table, once
with tilt, actuator and flight on a generated stairs-and-stones terrain (the harness of tests/test_sim_flight_env_path.py).
leg_contact and stumbled are compared after every step, and in both configurations the collision and stumble terms are non-zero for
some env-step.  Then the opt-out, a NaN env, and the trainers."""
import types

import numpy as np
import pytest
import torch

import sim_contact_oracle as CO
import sim_oracle as O
import test_sim_env_path as E
import test_sim_flight_env_path as FE
import test_sim_tilt_env_path as T
import test_terrain_env_path as TP

pytestmark = pytest.mark.gpu
N, STEPS = 33, 12
STAIRS_AND_STONES = (0.0, 0.0, 0.25, 0.25, 0.0, 0.5)          # column 0: stairs down, column 1: stepping stones


def _scales(tilt):
    from dtc_amd.env.surrogate import _SCALES, CONTACT_SCALES
    extra = dict(orientation=-0.2, orientation_roll=-0.1) if tilt else {}
    return dict(_SCALES, **CONTACT_SCALES, **extra)


def _plain_env(max_len, contacts=True, n=N):
    from dtc_amd import sim as SIM, synthetic as S
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    s = SIM.SimConfig(resampling_time=7 * 0.02 + 1e-9, contacts=SIM.ContactConfig() if contacts else None)
    cfg = SurrogateConfig(sim=s, episode_length_s=max_len * s.dt, reward_scales=_scales(False))
    return SurrogateLeggedEnv(n, "cuda", cfg, S.reward_table(), seed=3), cfg


def _terrain_env(max_len, n=N):
    from dtc_amd import sim as SIM
    from dtc_amd.env import SurrogateConfig, SurrogateLeggedEnv
    from dtc_amd.terrain import TerrainConfig
    import test_sim_actuator_env_path as AE
    s = SIM.SimConfig(resampling_time=5 * 0.02 + 1e-9, border_size=TP.BORDER, tilt=True, actuator=AE._actuator(), flight=SIM.FlightConfig(),
                      contacts=SIM.ContactConfig())
    terrain = TerrainConfig(terrain_length=TP.LENGTH, terrain_width=TP.LENGTH, border_size=TP.BORDER, num_rows=FE.R, num_cols=FE.C,
                            terrain_proportions=STAIRS_AND_STONES, max_init_terrain_level=FE.R - 1, seed=7)
    cfg = SurrogateConfig(sim=s, episode_length_s=max_len * s.dt, reward_scales=_scales(True), terrain=terrain)
    return SurrogateLeggedEnv(n, "cuda", cfg, seed=3), cfg


def _with_contacts(monkeypatch, env, cfg, shim):
    """Put the contact oracle behind the surrogate step's oracle of `shim`, check the two flag tensors after every step, and count
    what the reward terms get to see (from the oracles' outputs and from the reward oracle's per-term values)."""
    import reward_cases as K
    seen = dict(steps=0, leg_contact=0, stumbled=0, collision_in=0, stumble_in=0, collision=0, stumble=0)
    inner, s = shim.sim_step, cfg.sim
    knee, ck = CO.knee_tables(s), CO.contact_dict(s.contacts)
    feet, pen = list(s.feet), env.penalised_contact_indices.tolist()

    def sim_step(B, k, tables, a, hs, u_cmd):
        W = inner(B, k, tables, a, hs, u_cmd)
        C = CO.contacts(W, k, ck, tables, knee, hs)
        done = env.reset_buf.cpu().numpy() != 0
        for name in CO.FLAGS:                                             # a reset leaves the flags of the step that caused it
            got = getattr(env, name).cpu().numpy()
            assert got.dtype == np.uint8 and np.array_equal(got, C[name]), name
        for name in ("contact_forces", "rigid_body_state"):               # nor does it touch these two
            assert np.array_equal(E._bits(getattr(env, name).cpu().numpy()), E._bits(C[name])), name
        W = dict(W, contact_forces=C["contact_forces"], rigid_body_state=C["rigid_body_state"])
        f = W["contact_forces"]
        seen["steps"] += 1
        seen["leg_contact"] += int(C["leg_contact"].any(axis=1).sum())
        seen["stumbled"] += int(C["stumbled"].any(axis=1).sum())
        seen["collision_in"] += int((np.linalg.norm(f[:, pen], axis=-1) > 0.1).any(axis=1).sum())
        seen["stumble_in"] += int((np.linalg.norm(f[:, feet, :2], axis=-1) > 5 * np.abs(f[:, feet, 2])).any(axis=1).sum())
        return W

    reference = K.reference

    def with_terms(R, rcfg, sums):
        r64, e32 = reference(R, rcfg, sums)
        for name in ("collision", "stumble"):
            seen[name] += int((r64["per"][name] != 0).sum())
        # the two terms are counts times a scale, which the reward tests hold to equal counts and for which the oracle reports no
        # float32 error of its own: an e32 of 0 holds their sums to the floor of the compositions' bound, K.bound(0) = 2^-20 of
        # their size, a thousandth of what one count more or less would change
        for name in r64["per"]:
            e32.setdefault(name, 0.0)
        return r64, e32

    wrapped = types.SimpleNamespace(STATE=shim.STATE, INPUTS=shim.INPUTS, config_dict=shim.config_dict, sim_step=sim_step)
    monkeypatch.setattr(E, "O", wrapped)
    monkeypatch.setattr(T, "TO", wrapped)
    monkeypatch.setattr(K, "reference", with_terms)
    return seen


def _seen_enough(seen):
    print(seen)
    assert seen["steps"] == STEPS and seen["leg_contact"] > 0 and seen["stumbled"] > 0, seen
    assert seen["collision_in"] > 0 and seen["stumble_in"] > 0 and seen["collision"] > 0 and seen["stumble"] > 0, seen


def test_env_equals_the_composition_of_the_oracles_on_the_rough_table(monkeypatch):
    env, cfg = _plain_env(E.MAX_LEN)
    assert {"collision", "stumble"} <= set(env.env_rewards.cfg.names)
    draws = E._draws
    for name, v in (("N", N), ("STEPS", STEPS)):
        monkeypatch.setattr(E, name, v)
    monkeypatch.setattr(E, "_draws", lambda i, dev, n=N: draws(i, dev, n))
    monkeypatch.setattr(E, "_env", lambda rough=False, **kw: (env, cfg))
    seen = _with_contacts(monkeypatch, env, cfg, types.SimpleNamespace(STATE=O.STATE, INPUTS=O.INPUTS, config_dict=O.config_dict, sim_step=O.sim_step))
    E.test_env_equals_the_composition_of_the_oracles(True)
    _seen_enough(seen)


def test_env_equals_the_composition_of_the_oracles_with_tilt_actuator_and_flight_on_stairs_and_stones(monkeypatch):
    monkeypatch.setattr(FE, "N", N)
    env, cfg = _terrain_env(T.MAX_LEN)
    assert {"collision", "stumble"} <= set(env.env_rewards.cfg.names)
    flight, on_terrain = FE._patch(monkeypatch, env, cfg, True, True, T.MAX_LEN)
    for mod in (E, T):
        monkeypatch.setattr(mod, "STEPS", STEPS)
    seen = _with_contacts(monkeypatch, env, cfg, E.O)
    T.test_tilt_env_equals_the_composition_of_the_oracles(False)
    _seen_enough(seen)
    assert flight["steps"] == STEPS and env.height_samples.cpu().numpy().any()
    types_ = env.terrain_types.cpu().numpy()
    assert set(types_.tolist()) == {0, 1}                                 # both families carry envs


def test_without_contacts_the_env_is_the_one_built_before(monkeypatch):
    """contacts=None: the binding's dtc_sim_contacts is replaced by a function that raises, and tests/test_sim_env_path.py's own check
    of the surrogate step on evolving state runs on the env, bit for bit with tests/sim_oracle.py as before; the rows the contact
    kernel would own stay zero.  With contacts set the same call raises."""
    from dtc_amd import _ffi

    def refuse(*a, **kw):
        raise AssertionError("dtc_sim_contacts called")
    monkeypatch.setattr(_ffi.lib(), "dtc_sim_contacts", refuse, raising=True)
    held = {}
    env_of = E._env

    def _env(rough=False, **kw):
        held["env"], cfg = env_of(rough, **kw)
        return held["env"], cfg
    monkeypatch.setattr(E, "_env", _env)
    E.test_env_steps_on_evolving_state(True)
    env = held["env"]
    s = env.config.sim
    assert s.contacts is None and not hasattr(env, "leg_contact") and not hasattr(env, "stumbled")
    f = env.contact_forces.cpu().numpy()
    assert not f[:, env.penalised_contact_indices.tolist()].any() and not f[:, list(s.feet), :2].any() and f[:, list(s.feet), 2].any()
    assert not env.rigid_body_state[:, [t + 1 for t in s.thighs]].any()
    on, _ = _plain_env(12, n=16)
    with pytest.raises(AssertionError, match="dtc_sim_contacts called"):
        on.reset(draws=E._draws(-1, on.device))


def test_a_nan_env_has_no_flags_and_no_forces_and_the_others_keep_their_bits():
    """Two envs alike; after three steps one gets NaN joints in env 5.  In that step its flags and its contact forces are zero (the
    containment's rows), it is reset, and every other env leaves the clean run's bits."""
    bad = 5
    runs = []
    for poison in (False, True):
        env, cfg = _plain_env(30, n=16)
        dev = env.device
        env.reset(draws=E._draws(-1, dev, 16))
        g = torch.Generator().manual_seed(9)
        for i in range(4):
            if poison and i == 3:
                env.dof_state[bad] = float("nan")
            env.step((0.5 * torch.randn(16, 12, generator=g)).to(dev), E._draws(i, dev, 16))
        runs.append({name: getattr(env, name).cpu().numpy().copy() for name in
                     ("contact_forces", "rigid_body_state", "leg_contact", "stumbled", "rew_buf", "reset_buf", "obs_buf", "root_states")})
    clean, hurt = runs
    others = np.arange(16) != bad
    assert clean["leg_contact"].any() and clean["stumbled"].any()         # there was something to keep
    assert hurt["reset_buf"][bad] == 1 and not hurt["leg_contact"][bad].any() and not hurt["stumbled"][bad].any()
    assert not hurt["contact_forces"][bad].any() and np.isfinite(hurt["rew_buf"]).all() and np.isfinite(hurt["obs_buf"]).all()
    for name in clean:
        assert np.array_equal(E._bits(clean[name][others]), E._bits(hurt[name][others])), name


@pytest.mark.parametrize("model", ["ppo", "rdppo"])
def test_trainers_learn_on_the_contact_env(model):
    """One learn() iteration at 16 envs x 24 steps on the stairs-and-stones terrain with tilt, actuator, flight and contacts: finite
    weights, observations and rewards, flags that are flags, and an env step that reads nothing back."""
    from dtc_amd.runners import OnPolicyRunner
    import test_sim_runner_path as RP
    torch.manual_seed(11)
    env, cfg = _terrain_env(30, n=16)
    runner = dict(num_steps_per_env=24, save_interval=1000, **RP.MODELS[model])
    r = OnPolicyRunner(env, dict(runner=runner, algorithm=dict(num_learning_epochs=2), policy=dict()), log_dir=None, device="cuda")
    r.learn(1)
    torch.cuda.synchronize()
    ac = r.alg.actor_critic
    assert bool(torch.isfinite(ac.arena.flat).all()) if hasattr(ac, "arena") else all(bool(torch.isfinite(p).all()) for p in ac.parameters())
    assert bool(torch.isfinite(env.obs_buf).all()) and bool(torch.isfinite(env.rew_buf).all()) and bool(torch.isfinite(env.contact_forces).all())
    assert env.leg_contact.dtype == env.stumbled.dtype == torch.uint8 and int(env.leg_contact.max()) <= 1 and int(env.stumbled.max()) <= 1
    a = torch.zeros(16, 12, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        env.step(a)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
