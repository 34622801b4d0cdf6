"""dtc_sim_step_act (csrc/sim.hip) through the C ABI against its numpy float32 restatement (tests/sim_actuator_oracle.py): equal bits
on every output tensor, on lag_state and push_vel, and on the guard bytes around each, in the harness of tests/test_hip_sim.py
(NaN-filled guarded buffers, the strided dof_state views), over six chained steps with lag choices that vary per substep and pushes
drawn in steps 2 and 3.  tests/test_sim_actuator_host.py shows on the CPU what the seeded fixture reaches.  GPU only."""
import numpy as np
import pytest
import torch

import sim_actuator_oracle as AO
import sim_cases as CASES
import sim_oracle as O
import sim_tilt_oracle as TO
import test_hip_sim as H

pytestmark = pytest.mark.gpu
NEW = ("lag_state", "push_vel")


class _Env(H._Env):
    """The env's tensors of tests/test_hip_sim.py plus the two of the actuator, guarded alike."""

    def __init__(self, st, dev):
        super().__init__(st, dev)
        for name in NEW:
            view, whole = H._guarded(st[name], dev, 0)
            setattr(self, name, view)
            self.buffers[name] = whole


def _run(N, decimation, tilt, rough=True, seed=0, **act):
    from dtc_amd import sim as SIM
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = AO.config(decimation, tilt, **act)
    env = _Env(AO.state(N, cfg), dev)
    before = {name: H._bytes(b) for name, b in env.buffers.items()}
    step = SIM.SimStep(N, dev, cfg, torch.from_numpy(CASES.terrain(rough)), seed=seed)
    return cfg, env, before, step


def _compare(env, before, new, where):
    want = env.expect(new)
    for name, whole in env.buffers.items():
        got = H._bytes(whole).reshape(-1)
        exp = before[name].reshape(-1) if want[name] is None else want[name]
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, f"{where}: {name} differs in {bad.size} bytes, first at byte {bad[0]} of {got.size}"


def _dev(a, dev):
    return None if a is None else torch.from_numpy(a).to(dev)


@pytest.mark.parametrize("tilt", [False, True], ids=["yaw", "tilt"])
@pytest.mark.parametrize("decimation", [1, 4])
@pytest.mark.parametrize("N", [1, 3, 5, 257])
def test_sim_step_act_matches_the_oracle_bit_for_bit(N, decimation, tilt):
    cfg, env, before, step = _run(N, decimation, tilt)
    ref = AO.run(N, cfg, True)
    assert [r[4] for r in ref] == [False, False, True, True, False, False]
    dev = step.device
    for i, (a, u, ch, up, push, new) in enumerate(ref):
        step.step(env, _dev(a, dev), _dev(u, dev), lag_choice=ch, u_push=_dev(up, dev), push=push)
        torch.cuda.synchronize()
        _compare(env, before, new, f"step {i}")
    assert step.counter == 0                                              # given draws do not advance the call counter


@pytest.mark.parametrize("tilt", [False, True], ids=["yaw", "tilt"])
def test_generated_push_and_command_draws(tilt):
    """u_cmd and u_push left out: the kernel's own Philox draws (words 0 and 1 of the counter), the oracle's bits for the same key
    and call counter on every tensor; the counter advances once per step.  Then u_cmd given and u_push left out: the counter
    advances on the push steps alone."""
    N, decimation = 257, 4
    cfg, env, before, step = _run(N, decimation, tilt, seed=1234)
    ref = AO.run(N, cfg, True, u_given=False, seed=1234)
    due = 0
    for i, (a, _, ch, _, push, new) in enumerate(ref):
        step.step(env, _dev(a, step.device), lag_choice=ch, push=push)
        torch.cuda.synchronize()
        _compare(env, before, new, f"step {i}")
        due += int((new["episode_length_buf"] % cfg.resampling_steps == 0).sum())
    assert step.counter == AO.STEPS and due > 50
    pv = np.stack([ref[i][5]["push_vel"] for i in AO.PUSH_STEPS])
    assert (np.abs(pv) <= 1).all() and pv.min() < -0.9 and pv.max() > 0.9 and not np.array_equal(pv[0], pv[1])
    # the push draws alone
    cfg, env, before, step = _run(N, decimation, tilt, seed=77)
    hs, t, st, counter = CASES.terrain(True), CASES.tables(cfg), AO.state(N, cfg), 0
    for i in range(4):
        a, u, ch, push = CASES.actions(N, cfg, i), CASES.draws(N, i), AO.choices(decimation, i), i in (1, 2)
        k = AO.config_dict(cfg, CASES.ROWS, CASES.COLS, seed=77, counter=counter)
        new = AO.sim_step(st, k, t, a, hs, u, tilt=tilt, lag_choice=ch, push=push)
        step.step(env, _dev(a, step.device), _dev(u, step.device), lag_choice=ch, push=push)
        torch.cuda.synchronize()
        _compare(env, before, new, f"given commands, step {i}")
        counter += int(push)
        assert step.counter == counter
        st = dict(st, **new)


@pytest.mark.parametrize("tilt", [False, True], ids=["yaw", "tilt"])
def test_every_choice_five_and_no_push_is_the_old_entry_point(tilt):
    """Identity: the lag on with every choice 5 (the current action), pushes configured but none pending or drawn -- the bits of
    dtc_sim_step / dtc_sim_step_tilt, run here on a second env, on every pre-existing tensor and its guard bytes."""
    from dtc_amd import sim as SIM
    N, decimation = 257, 4
    cfg, env, _, step = _run(N, decimation, tilt)
    env.push_vel.zero_()
    dev = step.device
    old_cfg = CASES.config(decimation, tilt=tilt)
    assert old_cfg.actuator is None
    old_env = H._Env(TO.state(N, old_cfg) if tilt else CASES.state(N, old_cfg), dev)
    old_env.episode_length_buf.copy_(env.episode_length_buf)             # the fixture's one change to the parents' state
    old = SIM.SimStep(N, dev, old_cfg, torch.from_numpy(CASES.terrain(True)))
    for i in range(3):
        a, u = _dev(CASES.actions(N, cfg, i), dev), _dev(CASES.draws(N, i), dev)
        step.step(env, a, u, lag_choice=[5] * decimation)
        old.step(old_env, a, u)
        torch.cuda.synchronize()
        for name, whole in old_env.buffers.items():
            assert np.array_equal(H._bytes(env.buffers[name]), H._bytes(whole)), f"step {i}: {name}"
        assert not env.push_vel.any()
    assert env.lag_state.abs().sum() > 0


def test_a_nan_action_in_one_env_leaves_the_others_alone():
    """Env 2 of 5 is given a NaN action over three steps, the second of which draws a push: the rows of the other four in every
    tensor, lag_state and push_vel included, and every guard byte, equal a clean run's bit for bit."""
    N, bad = 5, 2
    runs = []
    for dirty in (False, True):
        cfg, env, _, step = _run(N, 4, True)
        for i in range(3):
            a = CASES.actions(N, cfg, i)
            if dirty:
                a[bad, 4] = np.nan
            step.step(env, _dev(a, step.device), _dev(CASES.draws(N, i), step.device), lag_choice=AO.choices(4, i),
                      u_push=_dev(AO.push_u(N, i), step.device), push=(i == 1))
        torch.cuda.synchronize()
        runs.append({name: H._bytes(b) for name, b in env.buffers.items()})
    others = np.arange(N + 2 * H.GUARD) != bad + H.GUARD
    for name, clean in runs[0].items():
        dirty = runs[1][name]
        if name.endswith("_buffer"):                                      # [T + 2 GUARD, N, W] bytes: the env axis is the second
            assert np.array_equal(clean[:, np.arange(N) != bad], dirty[:, np.arange(N) != bad]), name
        else:
            assert np.array_equal(clean.reshape(N + 2 * H.GUARD, -1)[others], dirty.reshape(N + 2 * H.GUARD, -1)[others]), name
    for name in ("actions", "lag_state"):
        assert not np.array_equal(runs[0][name][bad + H.GUARD], runs[1][name][bad + H.GUARD]), name


def test_without_an_actuator_the_old_entry_point_runs_on_an_env_that_has_no_lag_state():
    from dtc_amd import sim as SIM
    N = 5
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = CASES.config(4)
    assert cfg.actuator is None
    st = CASES.state(N, cfg)
    env = H._Env(st, dev)
    assert not hasattr(env, "lag_state") and not hasattr(env, "push_vel")
    before = {name: H._bytes(b) for name, b in env.buffers.items()}
    step = SIM.SimStep(N, dev, cfg, torch.from_numpy(CASES.terrain(True)))
    a, u = CASES.actions(N, cfg, 0), CASES.draws(N, 0)
    step.step(env, _dev(a, dev), _dev(u, dev))
    torch.cuda.synchronize()
    _compare(env, before, O.sim_step(st, O.config_dict(cfg, CASES.ROWS, CASES.COLS), CASES.tables(cfg), a, CASES.terrain(True), u), "no actuator")
