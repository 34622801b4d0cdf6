"""dtc_sim_balance (csrc/sim_balance.hip) through the C ABI against its numpy float32 restatement (tests/sim_balance_oracle.py):
equal bits on every output -- root_states, base_pos, base_quat, projected_gravity, base_lin_vel, base_ang_vel, the base rows of
rigid_body_state and contact_forces, lean and fallen -- on every byte the kernel does not own (the feet, hip and shank rows of
rigid_body_state, the non-base rows of contact_forces, contact_filt, episode_length_buf) and on the guard bytes around each tensor,
in the harness of tests/test_hip_sim.py.  The scenarios of tests/sim_balance_cases.py take every branch of the rule over
ceil(20 / N) launches of N envs; every case asserts that from the oracle's own branch record.  The kernel reads no joint tensor, so
there is no strided input to vary: every tensor it takes is dense.  tests/test_sim_balance_host.py shows on the CPU what the model
does.  GPU only."""
import types

import numpy as np
import pytest
import torch

import sim_balance_cases as BC
import sim_balance_oracle as BO
import test_hip_sim as H

pytestmark = pytest.mark.gpu


def _config(tilted):
    from dtc_amd import sim as SIM
    return SIM.SimConfig(balance=SIM.BalanceConfig(com_offset=(0.02, 0.0) if tilted else (0.0, 0.0)))


def _run(N, tilted, round_=0, nan_rows=()):
    """The env's tensors inside guarded buffers, the step object, the bytes before the launch, the oracle's outputs and trace."""
    from dtc_amd import sim as SIM
    dev = torch.device("cuda", torch.cuda.current_device())
    st = BC.state(N, tilted, round_, nan_rows)
    env, buffers = types.SimpleNamespace(), {}
    for name, a in st.items():
        view, buffers[name] = H._guarded(a, dev, 0)
        setattr(env, name, view)
    view, buffers["fallen"] = H._guarded(np.full(N, 0xAB, dtype=np.uint8), dev, 0)
    env.fallen = view
    before = {name: H._bytes(b).copy() for name, b in buffers.items()}
    step = SIM.SimStep(N, dev, _config(tilted), SIM.flat_table(4, 4))
    want, trace = BC.expected(st, tilted)
    return st, env, buffers, before, step, want, trace


def _compare(buffers, before, want, where):
    for name, whole in buffers.items():
        got = H._bytes(whole).reshape(-1)
        exp = before[name].reshape(-1).copy()
        if name in BO.WRITTEN:
            a = np.ascontiguousarray(want[name])
            row = a[0].nbytes
            exp[H.GUARD * row:H.GUARD * row + a.nbytes] = a.view(np.uint8).reshape(-1)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, f"{where}: {name} differs in {bad.size} bytes, first at byte {bad[0]} of {got.size}"


@pytest.mark.parametrize("tilted", [False, True], ids=["level", "tilted"])
@pytest.mark.parametrize("N", [1, 3, 5, 257])
def test_sim_balance_matches_the_oracle_bit_for_bit(N, tilted):
    """N = 1, 3, 5: a partial workgroup; 257: four full ones and a tail (64 envs per workgroup)."""
    seen = dict.fromkeys(BO.BRANCHES, 0)
    for r in range(BC.rounds(N)):
        st, env, buffers, before, step, want, trace = _run(N, tilted, r)
        for name, v in BO.branches(trace).items():
            seen[name] += v
        step.balance(env)
        torch.cuda.synchronize()
        _compare(buffers, before, want, f"N = {N}, round {r}")
        # what the comparison above covers, said once more on the oracle's own arrays: the rows the kernel does not own kept their values
        assert np.array_equal(H._bytes(torch.from_numpy(want["rigid_body_state"][:, 1:])), H._bytes(torch.from_numpy(st["rigid_body_state"][:, 1:])))
        assert np.array_equal(H._bytes(torch.from_numpy(want["contact_forces"][:, 1:])), H._bytes(torch.from_numpy(st["contact_forces"][:, 1:])))
        assert np.array_equal(want["rigid_body_state"][:, 0, 7:], st["rigid_body_state"][:, 0, 7:])
        fell = want["fallen"] != 0
        assert (want["contact_forces"][fell, 0, 2] >= 200.0).all() and (want["contact_forces"][fell, 0, 2] >= st["contact_forces"][fell, 0, 2]).all()
        assert np.array_equal(want["contact_forces"][~fell, 0], st["contact_forces"][~fell, 0])
    assert all(v > 0 for v in seen.values()), seen


def test_non_finite_rows_stay_in_their_row():
    N, bad = 9, (1, 4, 8)
    st, env, buffers, before, step, want, trace = _run(N, True, 0, nan_rows=bad)
    clean, _ = BC.expected(BC.state(N, True, 0), True)
    good = [n for n in range(N) if n not in bad]
    for name in BO.WRITTEN:                                               # the oracle first: the finite envs do not notice
        assert np.array_equal(H._bytes(torch.from_numpy(want[name][good])), H._bytes(torch.from_numpy(clean[name][good]))), name
    assert not want["fallen"][list(bad)].any()
    step.balance(env)
    torch.cuda.synchronize()
    _compare(buffers, before, want, "NaN rows")


def test_the_entry_point_refuses_bad_constants_and_null_pointers():
    """A refusal is an error code ahead of any launch: nothing is written."""
    from dtc_amd import _ffi
    N = 5
    st, env, buffers, before, step, want, _ = _run(N, False)
    b = step.cfg.balance                                                  # past BalanceConfig.validate(), which SimStep ran
    for name, values in (("h_min", (0.0, -1.0, float("nan"), float("inf"))), ("fall_angle", (0.0, -1.0, float("nan"), float("inf"))),
                         ("fall_force", (0.0, 100.0, float("nan"), float("inf"))), ("gravity", (-1.0, float("nan"), float("inf"))),
                         ("lean_eps", (-1e-3, float("nan"), float("inf")))):
        kept = getattr(b, name)
        for v in values:
            setattr(b, name, v)
            with pytest.raises(_ffi.DtcError, match=name):
                step.balance(env)
        setattr(b, name, kept)
    kept, b.com_offset = b.com_offset, (float("nan"), 0.0)
    with pytest.raises(_ffi.DtcError, match="com_offset"):
        step.balance(env)
    b.com_offset = kept
    kept, step.cfg.feet = step.cfg.feet, (0, 8, 12, 16)
    with pytest.raises(_ffi.DtcError, match="foot body 0"):
        step.balance(env)
    step.cfg.feet = kept
    check = step._check
    step._check = lambda n, t, tail, dtype: None if t is None else check(n, t, tail, dtype)
    for name in ("lean", "fallen"):
        held = getattr(env, name)
        setattr(env, name, None)
        with pytest.raises(_ffi.DtcError, match="null lean / fallen"):
            step.balance(env)
        setattr(env, name, held)
    for name in st:
        if name == "lean":
            continue
        held = getattr(env, name)
        setattr(env, name, None)
        with pytest.raises(_ffi.DtcError, match="null tensor of the step"):
            step.balance(env)
        setattr(env, name, held)
    step._check = check
    lib, s, k = _ffi.lib(), _ffi.DtcSimStep(), step.cfg_struct()
    assert lib.dtc_sim_balance(None, k, step.balance_struct(), N, _ffi.stream()) != 0
    assert lib.dtc_sim_balance(s, None, step.balance_struct(), N, _ffi.stream()) != 0
    assert lib.dtc_sim_balance(s, k, None, N, _ffi.stream()) != 0
    assert lib.dtc_sim_balance(s, k, step.balance_struct(), 0, _ffi.stream()) != 0
    held, env.fallen = env.fallen, env.fallen.to(torch.int32)
    with pytest.raises(_ffi.DtcError, match="fallen"):                    # and the host side refuses a tensor of the wrong dtype
        step.balance(env)
    env.fallen = held
    torch.cuda.synchronize()
    for name, whole in buffers.items():                                   # nothing was launched
        assert np.array_equal(H._bytes(whole), before[name]), name
    step.balance(env)
    torch.cuda.synchronize()
    _compare(buffers, before, want, "after")
