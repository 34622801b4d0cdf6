"""dtc_sim_step_fly (csrc/sim.hip) through the C ABI against its numpy float32 restatement (tests/sim_flight_oracle.py): equal bits
on every output tensor, on airborne and crashed, and on the guard bytes around each, in the harness of tests/test_hip_sim.py
(NaN-filled guarded buffers, the strided dof_state views), for all four steps underneath, over six chained steps on a table with
holes, a ledge and a wall.  Every case asserts from the oracle's own flags that it takes each branch: airborne, landing, crash,
grounded.  tests/test_sim_flight_host.py shows on the CPU what the model does.  GPU only."""
import numpy as np
import pytest
import torch

import sim_actuator_oracle as AO
import sim_cases as CASES
import sim_flight_oracle as FO
import test_hip_sim as H

pytestmark = pytest.mark.gpu
_NP = {**H._NP, torch.uint8: np.uint8}
BASES = [(False, False), (True, False), (False, True), (True, True)]
IDS = ["yaw", "tilt", "yaw-act", "tilt-act"]


class _Env(H._Env):
    """The env's tensors of tests/test_hip_sim.py plus airborne and crashed (and the two of the actuator), guarded alike."""

    def __init__(self, st, dev, act):
        super().__init__(st, dev)
        for name in (("lag_state", "push_vel") if act else ()) + FO.FLAGS:
            view, whole = H._guarded(st[name], dev, 0)
            setattr(self, name, view)
            self.buffers[name] = whole

    def expect(self, new):
        out = {}
        for name, whole in self.buffers.items():
            a = np.stack([new["dof_pos"], new["dof_vel"]], axis=2) if name == "dof_state" else new.get(name)
            if a is None:                                                 # an input: unchanged
                out[name] = None
                continue
            e = np.full(whole.numel() * whole.element_size(), 0xFF, dtype=np.uint8)
            a = np.ascontiguousarray(a).astype(_NP[whole.dtype], copy=False)
            row = a[0].nbytes
            e[H.GUARD * row:H.GUARD * row + a.nbytes] = a.view(np.uint8).reshape(-1)
            out[name] = e
        return out


def _run(N, tilt, act, st=None, seed=0, **fly):
    from dtc_amd import sim as SIM
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = FO.config(4, tilt, act, **fly)
    env = _Env(FO.state(N, cfg) if st is None else st, dev, act)
    before = {name: H._bytes(b) for name, b in env.buffers.items()}
    step = SIM.SimStep(N, dev, cfg, torch.from_numpy(FO.terrain()), seed=seed)
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


def _step(step, env, r, dev):
    a, u, ch, up, push, _ = r
    if ch is None:
        step.step(env, _dev(a, dev), _dev(u, dev))
    else:
        step.step(env, _dev(a, dev), _dev(u, dev), lag_choice=ch, u_push=_dev(up, dev), push=push)
    torch.cuda.synchronize()


def _branches(trace):
    """From the oracle's flags, over the substeps of a run: envs in the air, landings, crashes, grounded substeps."""
    air, crashed = np.stack([s["air"] for s in trace]), np.stack([s["crashed"] for s in trace])
    return dict(airborne=int(air.sum()), landing=int((air[:-1] & ~air[1:]).sum()), crash=int(crashed.any(axis=0).sum()),
                grounded=int((~air).sum()))


@pytest.mark.parametrize("tilt,act", BASES, ids=IDS)
@pytest.mark.parametrize("N", [1, 3, 5, 257])
def test_sim_step_fly_matches_the_oracle_bit_for_bit(N, tilt, act):
    """N = 1, 3: a partial workgroup; 5: a full one and a tail; 257: 64 full ones and a tail (4 envs per workgroup)."""
    cfg, env, before, step = _run(N, tilt, act)
    trace = []
    ref = FO.run(N, cfg, trace=trace)
    seen = _branches(trace)
    assert all(v > 0 for v in seen.values()), seen
    for i, r in enumerate(ref):
        _step(step, env, r, step.device)
        _compare(env, before, r[5], f"step {i}")
    assert step.counter == 0                                              # given draws do not advance the call counter
    flags = np.stack([r[5]["airborne"] for r in ref]), np.stack([r[5]["crashed"] for r in ref])
    assert set(np.unique(flags[0])) <= {0, 1} and set(np.unique(flags[1])) <= {0, 1}
    if N >= 5:                                                            # both values of both flags among the steps' outputs
        assert flags[0].any() and not flags[0].all() and flags[1].any() and not flags[1].all()


@pytest.mark.parametrize("tilt", [False, True], ids=["yaw", "tilt"])
def test_a_push_drawn_in_the_air_is_the_planar_velocity_of_the_next_call(tilt):
    """Two calls in a row: the carried state goes through root_states.  Step 1 draws a push; for an env that is airborne at the end
    of step 1 and through step 2 the oracle's world velocity in every substep of step 2 is that push, bit for bit, and its x, y
    advance by it; the kernel leaves the oracle's bits after both steps."""
    N = 257
    cfg, env, before, step = _run(N, tilt, True)
    trace = []
    ref = FO.run(N, cfg, steps=3, trace=trace, push_steps=(1,))
    dec = cfg.decimation
    air2 = np.stack([s["air"] for s in trace[2 * dec:3 * dec]]).all(axis=0) & (ref[1][5]["airborne"] == 1)
    assert air2.sum() >= 10
    pv = ref[1][5]["push_vel"]
    assert np.array_equal(ref[1][5]["root_states"][:, 7:9], pv) and np.abs(pv[air2]).min() > 0
    for s in trace[2 * dec:3 * dec]:
        assert np.array_equal(s["Vw"][air2].view(np.uint32), pv[air2].view(np.uint32))
    moved = ref[2][5]["root_states"][air2, 0:2] - ref[1][5]["root_states"][air2, 0:2]
    assert np.abs(moved - pv[air2] * np.float32(dec * cfg.sim_dt)).max() < 1e-5
    assert np.array_equal(ref[2][5]["root_states"][air2, 7:9], pv[air2])
    for i, r in enumerate(ref):
        _step(step, env, r, step.device)
        _compare(env, before, r[5], f"step {i}")


def test_generated_draws_with_flight():
    """u_cmd and u_push left out: the kernel's own Philox draws under the flight instantiation, the oracle's bits."""
    N = 257
    cfg, env, before, step = _run(N, True, True, seed=1234)
    ref = FO.run(N, cfg, steps=3, u_given=False, seed=1234)
    for i, (a, _, ch, _, push, new) in enumerate(ref):
        step.step(env, _dev(a, step.device), lag_choice=ch, push=push)
        torch.cuda.synchronize()
        _compare(env, before, new, f"step {i}")
    assert step.counter == 3


def test_the_entry_point_refuses_a_null_flag_pointer_and_a_crash_force_at_the_threshold():
    from dtc_amd import _ffi
    N = 5
    cfg, env, before, step = _run(N, False, False)
    a, u = _dev(CASES.actions(N, cfg, 0), step.device), _dev(CASES.draws(N, 0), step.device)
    for force in (100.0, 99.0, float("nan")):
        step.cfg.flight.crash_force = force                               # past FlightConfig.validate(), which SimStep ran
        with pytest.raises(_ffi.DtcError, match="crash_force"):
            step.step(env, a, u)
    step.cfg.flight.crash_force = 200.0
    step.cfg.flight.max_step_up = 0.0
    with pytest.raises(_ffi.DtcError, match="max_step_up"):
        step.step(env, a, u)
    step.cfg.flight.max_step_up = 0.3
    check = step._check
    for name in FO.FLAGS:
        kept = getattr(env, name)
        setattr(env, name, None)
        step._check = lambda n, t, tail, dtype: None if t is None else check(n, t, tail, dtype)
        with pytest.raises(_ffi.DtcError, match="null airborne / crashed"):
            step.step(env, a, u)
        setattr(env, name, kept)
    step._check = check
    kept, env.airborne = env.airborne, env.airborne.to(torch.int32)
    with pytest.raises(_ffi.DtcError, match="airborne"):                  # and the host side refuses a tensor of the wrong dtype
        step.step(env, a, u)
    env.airborne = kept
    torch.cuda.synchronize()
    for name, whole in env.buffers.items():                               # nothing was launched
        assert np.array_equal(H._bytes(whole), before[name]), name
    k = FO.config_dict(cfg, CASES.ROWS, CASES.COLS)
    step.step(env, a, u)
    torch.cuda.synchronize()
    _compare(env, before, FO.sim_step(FO.state(N, cfg), k, CASES.tables(cfg), CASES.actions(N, cfg, 0), FO.terrain(), CASES.draws(N, 0)), "after")
