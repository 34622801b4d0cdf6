"""The surrogate step with actuator lag and pushes, without a GPU: the properties of the model on its numpy float32 restatement
(tests/sim_actuator_oracle.py), which the kernel is held to bit for bit in tests/test_hip_sim_actuator.py, the conditions the GPU
fixture must meet, and the C ABI of dtc_sim_step_act as the binding sees it."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import sim_actuator_oracle as AO
import sim_cases as CASES
import sim_oracle as O
import sim_tilt_oracle as TO

F = np.float32
EPS = float(np.finfo(np.float32).eps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------------------------------------ the model, on the oracle
@pytest.mark.parametrize("tilt", [False, True], ids=["yaw", "tilt"])
@pytest.mark.parametrize("mode", ["lag off", "every choice 5"])
def test_without_lag_and_push_the_step_is_the_parents(tilt, mode):
    """N = 257, rough, six chained steps of the sim_cases fixture: with the lag off (whatever the choices), and with the lag on and
    every choice 5 (the current action), no push pending and none drawn, every pre-existing output equals sim_oracle.sim_step /
    sim_tilt_oracle.sim_step bit for bit; lag_state fills with the scaled actions all the same."""
    N = 257
    cfg = AO.config(4, tilt, lag=(mode != "lag off"))
    ref = TO.run(N, cfg, True, steps=6) if tilt else CASES.run(N, cfg, True, steps=6)
    st = TO.state(N, cfg) if tilt else CASES.state(N, cfg)                                # the parents' own initial state
    st["lag_state"], st["push_vel"] = AO.state(N, cfg)["lag_state"], np.zeros((N, 2), dtype=F)
    choice = (lambda i: AO.choices(4, i)) if mode == "lag off" else (lambda i: [5] * 4)
    got = AO.run(N, cfg, True, steps=6, st=st, lag_choice=choice, push_steps=())
    for i, ((a, _, new), (a2, _, _, _, push, mine)) in enumerate(zip(ref, got)):
        assert np.array_equal(a, a2) and not push
        for name in O.STATE:
            assert np.array_equal(_bits(mine[name]), _bits(new[name])), f"step {i}: {name}"
        assert (mine["push_vel"] == 0).all() and not np.signbit(mine["push_vel"]).any()
        scaled = np.minimum(np.maximum(a, -F(cfg.clip_actions)), F(cfg.clip_actions)) * F(cfg.action_scale)
        assert np.array_equal(mine["lag_state"][:, 2:], np.broadcast_to(scaled[:, None], (N, 4, 12)))      # four substeps of this action


def test_lag_a_step_change_of_the_action_arrives_after_five_minus_choice_substeps():
    """The action A is held until the buffer holds nothing else, then B is given: substep j of that step, with choice c, has the PD
    goal of B exactly when c >= 5 - j (slot 5 is written in substep 0, slot 4 holds it from substep 1 on, ...), else that of A."""
    N, dec = 3, 4
    cfg = AO.config(dec, False)
    t = CASES.tables(cfg)
    A, B = CASES.actions(N, cfg, 0), CASES.actions(N, cfg, 1)
    goal = lambda a: np.minimum(np.maximum(np.minimum(np.maximum(a, -F(3)), F(3)) * F(cfg.action_scale) + t["default_dof_pos"],     # noqa: E731
                                           t["dof_pos_limits"][:, 0]), t["dof_pos_limits"][:, 1])
    gA, gB = goal(A), goal(B)
    assert (gA != gB)[:-1].any(axis=1).all()                                              # (the last env is given the same action always)
    hs, k = CASES.terrain(False), AO.config_dict(cfg, CASES.ROWS, CASES.COLS)
    st = AO.state(N, cfg)
    for _ in range(2):                                                                     # 8 substeps of A: all six slots
        st = dict(st, **AO.sim_step(st, k, t, A, hs, CASES.draws(N, 0), lag_choice=[5] * dec))
    assert np.array_equal(st["lag_state"], np.broadcast_to((np.minimum(np.maximum(A, -F(3)), F(3)) * F(cfg.action_scale))[:, None], (N, 6, 12)))
    seen = set()
    for c in range(6):
        trace = []
        AO.sim_step(st, k, t, B, hs, CASES.draws(N, 0), trace=trace, lag_choice=[c] * dec)
        for j, sub in enumerate(trace):
            new = c >= 5 - j
            assert np.array_equal(sub["goal"], gB if new else gA), (c, j)
            seen.add(new)
    assert seen == {True, False}


def _rest(N, cfg):
    """Default pose at rest at the world origin, no motor offsets, an empty lag buffer: with zero actions no joint moves."""
    st, t = AO.state(N, cfg), CASES.tables(cfg)
    st["dof_pos"], st["dof_vel"] = np.tile(t["default_dof_pos"], (N, 1)), np.zeros((N, 12), dtype=F)
    st["motor_offsets"], st["lag_state"], st["push_vel"] = np.zeros((N, 12), dtype=F), np.zeros((N, 6, 12), dtype=F), np.zeros((N, 2), dtype=F)
    st["root_states"][:, 0:2] = 0
    if cfg.tilt:
        st["root_states"][:, 3:7] = TO.quaternion(np.linspace(-3, 3, N), np.zeros(N), np.zeros(N))
    return st


@pytest.mark.parametrize("tilt", [False, True], ids=["yaw", "tilt"])
def test_push_displacement_is_the_decaying_sum_and_the_push_ends(tilt):
    """Zero joint motion on the flat table, one push drawn in step 0 (max 1 m/s, decay 0.05 s, floor 1e-4 m/s).  The push acts from
    step 1 on: substep i moves the base by pv * sim_dt * keep^i in the world frame, so the whole displacement is
    pv * sim_dt / (1 - keep) less a tail below floor * sim_dt / (1 - keep).

    The bound, per component, over the n substeps the push lives (n <= ln(floor / |pv|) / ln(keep) + 1 < 110): each substep rotates
    the push into the yaw frame and back (two products and a sum each way, <= 8 eps relative to |pv|, times sim_dt) and adds to a
    position below 0.1 m (eps/2 * 0.1); the decayed push itself carries i roundings after i products (eps/2 * i * keep^i, summed:
    eps/2 * keep / (1 - keep)^2); keep is float32(exp(-sim_dt / decay)), taken as the kernel takes it."""
    N, dec = 5, 4
    cfg = AO.config(dec, tilt, push_decay_s=0.05, push_floor=1e-4, max_push_vel_xy=1.0)
    t, hs = CASES.tables(cfg), CASES.terrain(False)
    k = AO.config_dict(cfg, CASES.ROWS, CASES.COLS)
    keep, dt = float(k["keep"]), float(k["sim_dt"])
    st = _rest(N, cfg)
    zero, u0 = np.zeros((N, 12), dtype=F), CASES.draws(N, 0)
    up = AO.push_u(N, 0)
    new = AO.sim_step(st, k, t, zero, hs, u0, tilt=tilt, lag_choice=[1, 2, 3, 4], u_push=up, push=True)
    pv = new["push_vel"].astype(np.float64)
    assert np.array_equal(new["push_vel"], F(2) * up + F(-1)) and np.array_equal(new["root_states"][:, 7:9], new["push_vel"])
    assert np.array_equal(new["root_states"][:, 0:2], st["root_states"][:, 0:2]) and (new["base_lin_vel"][:, :2] == 0).all()
    start = new["root_states"][:, 0:2].astype(np.float64)
    st, trace = dict(st, **new), []
    for i in range(1, 30):
        new = AO.sim_step(st, k, t, zero, hs, u0, trace=trace, tilt=tilt, lag_choice=[1, 2, 3, 4])
        st = dict(st, **new)
    live = np.stack([s["pushed"] for s in trace])                                          # [substeps, N]
    n = live.sum(axis=0)
    assert (n > 20).all() and (n < 110).all() and (np.diff(live.astype(int), axis=0) <= 0).all()        # it ends, and stays ended
    assert (st["push_vel"] == 0).all() and not np.signbit(st["push_vel"]).any()
    assert np.array_equal(st["dof_pos"], np.tile(t["default_dof_pos"], (N, 1))) and (st["dof_vel"] == 0).all()
    moved = st["root_states"][:, 0:2].astype(np.float64) - start
    want = pv * dt / (1 - keep)
    vmax = np.abs(pv).max()
    bound = 110 * (8 * EPS * vmax * dt + 0.5 * EPS * 0.1) + 0.5 * EPS * vmax * dt * keep / (1 - keep) ** 2 + 1e-4 * dt / (1 - keep)
    err = np.abs(moved - want).max()
    print(f"push displacement {moved[0]} against {want[0]}: largest error {err:.3e}, bound {bound:.3e}")
    assert np.abs(st["root_states"][:, 0:2]).max() < 0.1 and err <= bound
    assert (np.abs(moved) > 1e-3).any()


@pytest.mark.parametrize("tilt", [False, True], ids=["yaw", "tilt"])
def test_after_the_push_ended_the_env_is_an_unpushed_env_bit_for_bit(tilt):
    """Moving envs on the rough table, a push drawn in step 0 with a short decay and a high floor: once push_vel is exactly zero,
    every further step (every choice 5) equals the parent oracle's step from the same state on every pre-existing output."""
    N, dec = 33, 4
    cfg = AO.config(dec, tilt, push_decay_s=0.02, push_floor=0.05)
    t, hs = CASES.tables(cfg), CASES.terrain(True)
    st = AO.state(N, cfg)
    parent = TO if tilt else O
    ended = 0
    for i in range(10):
        a, u = CASES.actions(N, cfg, i), CASES.draws(N, i)
        k = AO.config_dict(cfg, CASES.ROWS, CASES.COLS, counter=i)
        new = AO.sim_step(st, k, t, a, hs, u, tilt=tilt, lag_choice=[5] * dec, u_push=AO.push_u(N, i), push=(i == 0))
        if i >= 1 and (st["push_vel"] == 0).all():
            kk = parent.config_dict(cfg, CASES.ROWS, CASES.COLS, counter=i)
            ref = parent.sim_step({n: st[n] for n in O.STATE + O.INPUTS}, kk, t, a, hs, u)
            for name in O.STATE:
                assert np.array_equal(_bits(new[name]), _bits(ref[name])), f"step {i}: {name}"
            ended += 1
        elif i >= 1:
            assert (new["root_states"][:, 0:2] != st["root_states"][:, 0:2]).any()
        st = dict(st, **new)
    assert 3 <= ended <= 8                                                                 # pushed steps and ended steps were both seen


# ------------------------------------------------------------------------------------------------ the GPU fixture
@pytest.mark.parametrize("tilt", [False, True], ids=["yaw", "tilt"])
@pytest.mark.parametrize("decimation", [1, 4])
def test_the_gpu_fixture_reaches_what_it_is_meant_to(decimation, tilt):
    N = 257
    cfg = AO.config(decimation, tilt)
    trace = []
    ref = AO.run(N, cfg, True, trace=trace)
    t = CASES.tables(cfg)
    used = set()
    for i, (a, u, ch, up, push, new) in enumerate(ref):
        used |= set(ch)
        assert all(1 <= c <= 4 for c in ch)
        if i >= 1:                                                                         # the lag changes a PD goal in every step
            clipped = np.minimum(np.maximum(a, -F(cfg.clip_actions)), F(cfg.clip_actions))
            now = np.minimum(np.maximum(clipped * F(cfg.action_scale) + t["default_dof_pos"], t["dof_pos_limits"][:, 0]), t["dof_pos_limits"][:, 1])
            subs = trace[i * decimation:(i + 1) * decimation]
            assert any((s["goal"] != now).any() for s in subs), f"step {i}"
    assert used == {1, 2, 3, 4} and (decimation == 1 or len(set(ref[1][2])) > 1)
    pushes = [i for i, r in enumerate(ref) if r[4]]
    assert pushes == [2, 3]
    both = 0
    for i in pushes:
        a, u, ch, up, push, new = ref[i]
        assert (new["push_vel"] != 0).any(axis=1).all() and np.array_equal(new["root_states"][:, 7:9], new["push_vel"])
        due = new["episode_length_buf"] % cfg.resampling_steps == 0
        cx, cy = F(1.5) * u[:, 0] + F(-0.75), F(1.5) * u[:, 1] + F(-0.75)
        zeroed = due & (np.sqrt(cx * cx + cy * cy) <= F(0.1))
        assert (new["commands"][zeroed, :2] == 0).all()
        both += int(zeroed.sum())
    assert both >= 1                                                                       # a pushed env whose resample was zeroed
    # a push is pending while the substeps of steps 3 and 4 run, and the env that came with one has it from step 0
    assert all(s["pushed"].all() for s in trace[3 * decimation:5 * decimation]) and trace[0]["pushed"][N - 2] and not trace[0]["pushed"][0]


# ------------------------------------------------------------------------------------------------ host
def _good(decimation=4, tilt=False):
    """A DtcSimStep whose every required pointer is a dummy host address (no call below gets as far as a launch), a good DtcSimCfg
    and a good DtcSimActuator."""
    from dtc_amd import _ffi, sim as SIM
    cfg = SIM.SimConfig(decimation=decimation, tilt=tilt, actuator=SIM.ActuatorConfig())
    step = SIM.SimStep(4, "cpu", cfg, SIM.flat_table(8, 8))
    dummy = C.create_string_buffer(64)
    addr = C.addressof(dummy)
    s = _ffi.DtcSimStep()
    for name, kind in _ffi.DtcSimStep._fields_:
        setattr(s, name, addr if kind is C.c_void_p else (24 if "row" in name else 2))
    s.u_cmd = None
    act = step.act_struct([1, 2, 3, 4][:decimation], push=True)
    act.lag_state, act.push_vel = addr, addr
    return step, s, step.cfg_struct(), act, dummy


def test_abi_symbols_version_and_size_table():
    from dtc_amd import _ffi
    lib = _ffi.lib()
    for name in ("dtc_sim_step_act", "dtc_sim_act_abi_sizes"):
        assert name in _ffi.exported_symbols() and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "dtc_hip.h")).read()
    assert int(re.search(r"#define\s+DTC_ABI_VERSION\s+(\d+)", header).group(1)) == 25 == _ffi.ABI_VERSION == lib.dtc_version()
    sizes = (C.c_int64 * 32)()
    assert lib.dtc_sim_act_abi_sizes(sizes, 32) == 1 and sizes[0] == C.sizeof(_ffi.DtcSimActuator) == 120
    assert lib.dtc_sim_act_abi_sizes(None, 0) == 1
    for table, count in (("dtc_abi_sizes", 18), ("dtc_env_reset_abi_sizes", 3), ("dtc_sim_abi_sizes", 2), ("dtc_sim_tilt_abi_sizes", 1)):
        assert getattr(lib, table)(sizes, 32) == count, table
    assert C.sizeof(_ffi.DtcSimStep) == 312 and C.sizeof(_ffi.DtcSimTilt) == 8            # the older structs are as they were


def test_the_default_config_has_no_actuator_and_its_defaults_are_the_references():
    from dtc_amd import sim as SIM
    assert SIM.SimConfig().actuator is None
    a = SIM.ActuatorConfig()
    assert (a.lag, a.lag_slots, a.push, a.push_interval_s, a.max_push_vel_xy, a.push_decay_s, a.push_floor) == (True, (1, 4), True, 15.0, 1.0, 0.2, 1e-6)
    cfg = SIM.SimConfig(actuator=a)
    assert cfg.push_interval == 750 and SIM.SimConfig(actuator=SIM.ActuatorConfig(push_interval_s=0.06)).push_interval == 3
    step = SIM.SimStep(4, "cpu", cfg, SIM.flat_table(8, 8), seed=7)
    drawn = np.concatenate([np.asarray(step.act_struct().lag_choice[:4]) for _ in range(50)])
    assert set(drawn.tolist()) == {1, 2, 3, 4}
    again = SIM.SimStep(4, "cpu", cfg, SIM.flat_table(8, 8), seed=7)
    assert np.array_equal(drawn[:4], np.asarray(again.act_struct().lag_choice[:4]))
    act = step.act_struct([5, 0, 1, 2], push=True)
    assert (act.lag, act.push, act.push_now) == (1, 1, 1) and act.keep == float(F(math.exp(-0.005 / 0.2))) and act.floor2 == float(F(1e-12))
    assert (act.push_span, act.push_lo) == (2.0, -1.0)
    with pytest.raises(Exception):
        step.act_struct([1, 2, 3, 6])
    with pytest.raises(ValueError):
        SIM.SimStep(4, "cpu", SIM.SimConfig(actuator=SIM.ActuatorConfig(lag_slots=(1, 6))), SIM.flat_table(8, 8))


def test_bad_actuator_descriptors_are_refused_before_any_launch():
    from dtc_amd import _ffi
    lib = _ffi.lib()
    for tilt in (None, _ffi.DtcSimTilt(1.0, 1e-6)):
        step, s, c, act, keep_alive = _good(tilt=tilt is not None)
        assert lib.dtc_sim_step_act(s, c, tilt, None, 4, None) == -1 and b"DtcSimActuator" in lib.dtc_last_error()
        assert lib.dtc_sim_step_act(None, c, tilt, act, 4, None) == -1 and lib.dtc_sim_step_act(s, None, tilt, act, 4, None) == -1
        assert lib.dtc_sim_step_act(s, c, tilt, act, 0, None) == -1
        assert lib.dtc_sim_step_act(_ffi.DtcSimStep(), c, tilt, act, 4, None) == -1 and b"null" in lib.dtc_last_error()

        def refused(word, **fields):
            _, _, _, a, _ = _good(tilt=tilt is not None)
            for name, v in fields.items():
                if name.startswith("choice"):
                    a.lag_choice[int(name[6:])] = v
                else:
                    setattr(a, name, v)
            assert lib.dtc_sim_step_act(s, c, tilt, a, 4, None) == -1, fields
            assert word in lib.dtc_last_error(), (fields, lib.dtc_last_error())

        refused(b"lag_state", lag_state=None)
        refused(b"push_vel", push_vel=None)
        refused(b"lag_choice[0]", choice0=6)
        refused(b"lag_choice[3]", choice3=255)
        for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
            refused(b"keep", keep=bad)
        refused(b"floor", floor2=-1e-12)
        refused(b"span", push_span=-2.0)
        refused(b"floor", floor2=float("nan"))
    # a choice beyond `decimation` is not read: with decimation 1 only entry 0 counts, and the refusal that follows is another one
    step, s, c, act, keep_alive = _good(decimation=1)
    act.lag_choice[1], act.keep = 9, 2.0
    assert lib.dtc_sim_step_act(s, c, None, act, 4, None) == -1 and b"keep" in lib.dtc_last_error()


def test_step_on_cpu_tensors_fails_loudly_and_the_old_path_reads_no_new_attribute():
    import torch
    from dtc_amd import _ffi, sim as SIM
    step = SIM.SimStep(4, "cpu", SIM.SimConfig(actuator=SIM.ActuatorConfig()), SIM.flat_table(8, 8))
    with pytest.raises(_ffi.DtcError):
        step.step(object(), torch.zeros(4, 12))
    plain = SIM.SimStep(4, "cpu", SIM.SimConfig(), SIM.flat_table(8, 8))
    with pytest.raises(_ffi.DtcError, match="actuator"):
        plain.step(object(), torch.zeros(4, 12), push=True)
