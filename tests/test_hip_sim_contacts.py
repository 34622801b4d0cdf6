"""dtc_sim_contacts (csrc/sim_contacts.hip) through the C ABI against its numpy float32 restatement (tests/sim_contact_oracle.py):
equal bits on every output -- the thigh, shank and foot-xy rows of contact_forces, the knee positions in the shank rows of
rigid_body_state, leg_contact and stumbled -- on every byte of the rows and columns the kernel does not own (the base row with a
crash force, foot z, the hip rows, the other twelve columns of a shank row, every input) and on the guard bytes around each tensor,
in the harness of tests/test_hip_sim.py.  The states of tests/sim_contact_cases.py stand over a small table with a ledge, a wall and
holes; every case asserts from the oracle's own trace that it takes each branch.  tests/test_sim_contact_host.py shows on the CPU
what the model does.  GPU only."""
import types

import numpy as np
import pytest
import torch

import sim_contact_cases as CC
import sim_contact_oracle as CO
import test_hip_sim as H

pytestmark = pytest.mark.gpu
WRITTEN = ("contact_forces", "rigid_body_state") + CO.FLAGS


def _run(N, tilted, dense, nan_rows=(), **contact_kw):
    """The env's tensors inside guarded buffers, the step object, the bytes before the launch, the oracle's outputs and trace."""
    from dtc_amd import sim as SIM
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = CC.config(**contact_kw)
    st = CC.state(N, cfg, tilted, nan_rows)
    env, buffers = types.SimpleNamespace(), {}
    for name in ("base_pos", "base_quat", "rigid_body_state", "contact_forces"):
        view, buffers[name] = H._guarded(st[name], dev, 0)
        setattr(env, name, view)
    if dense:
        env.dof_pos, buffers["dof_pos"] = H._guarded(st["dof_pos"], dev, 0)
    else:                                                                 # the strided view of dof_state [N,D,2], as the env holds it
        vel = np.random.default_rng(5).standard_normal((N, 12)).astype(np.float32)
        dof_state, buffers["dof_state"] = H._guarded(np.stack([st["dof_pos"], vel], axis=2), dev, 0)
        env.dof_pos = dof_state[..., 0]
    for name, width in (("leg_contact", 8), ("stumbled", 4)):
        view, buffers[name] = H._guarded(np.full((N, width), 0xAB, dtype=np.uint8), dev, 0)
        setattr(env, name, view)
    before = {name: H._bytes(b).copy() for name, b in buffers.items()}
    step = SIM.SimStep(N, dev, cfg, torch.from_numpy(CC.terrain()))
    want, trace = CC.expected(st, cfg)
    return cfg, env, buffers, before, step, want, trace


def _compare(buffers, before, want, where):
    for name, whole in buffers.items():
        got = H._bytes(whole).reshape(-1)
        exp = before[name].reshape(-1).copy()
        if name in WRITTEN:
            a = np.ascontiguousarray(want[name])
            row = a[0].nbytes
            exp[H.GUARD * row:H.GUARD * row + a.nbytes] = a.view(np.uint8).reshape(-1)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, f"{where}: {name} differs in {bad.size} bytes, first at byte {bad[0]} of {got.size}"


@pytest.mark.parametrize("dense", [False, True], ids=["dof_state-view", "dense"])
@pytest.mark.parametrize("tilted", [False, True], ids=["level", "tilted"])
@pytest.mark.parametrize("N", [1, 3, 5, 257])
def test_sim_contacts_match_the_oracle_bit_for_bit(N, tilted, dense):
    """N = 1, 3: a partial workgroup; 5: a full one and a tail; 257: 64 full ones and a tail (4 envs per workgroup)."""
    cfg, env, buffers, before, step, want, trace = _run(N, tilted, dense)
    seen = CC.branches(trace, CO.contact_dict(cfg.contacts))
    assert all(v > 0 for v in seen.values()), seen
    step.contacts(env)
    torch.cuda.synchronize()
    _compare(buffers, before, want, f"N = {N}")
    # what the comparison above covers, said once more on the oracle's own arrays: the rows the kernel does not own kept their values
    st = CC.state(N, cfg, tilted)
    assert np.array_equal(want["contact_forces"][:, 0], st["contact_forces"][:, 0]) and (want["contact_forces"][:, 0, 2] == CC.CRASH).all()
    assert np.array_equal(want["contact_forces"][:, list(cfg.feet), 2], st["contact_forces"][:, list(cfg.feet), 2])
    hips = [t - 1 for t in cfg.thighs]
    assert np.array_equal(want["contact_forces"][:, hips], st["contact_forces"][:, hips])
    assert np.array_equal(want["rigid_body_state"][:, list(cfg.contacts.shanks), 3:], st["rigid_body_state"][:, list(cfg.contacts.shanks), 3:])


def test_non_finite_rows_flag_nothing_and_the_finite_envs_keep_their_bits():
    N, bad = 9, (1, 4, 8)
    cfg, env, buffers, before, step, want, trace = _run(N, True, False, nan_rows=bad)
    clean, _ = CC.expected(CC.state(N, cfg, True), cfg)
    good = [n for n in range(N) if n not in bad]
    for name in WRITTEN:                                                  # the oracle first: NaN rows give nothing, the others do not notice
        assert np.array_equal(H._bytes(torch.from_numpy(want[name][good])), H._bytes(torch.from_numpy(clean[name][good]))), name
    rows = list(cfg.thighs) + list(cfg.contacts.shanks)
    assert not want["leg_contact"][list(bad)].any() and not want["stumbled"][list(bad)].any()
    assert (want["contact_forces"][list(bad)][:, rows] == 0).all() and (want["contact_forces"][list(bad)][:, list(cfg.feet), :2] == 0).all()
    seen = CC.branches(trace, CO.contact_dict(cfg.contacts), rows=good)
    assert all(v > 0 for v in seen.values()), seen
    step.contacts(env)
    torch.cuda.synchronize()
    _compare(buffers, before, want, "NaN rows")


def test_the_entry_point_refuses_bad_constants_and_null_pointers():
    """A refusal is an error code ahead of any launch: nothing is written."""
    from dtc_amd import _ffi
    N = 5
    cfg, env, buffers, before, step, want, _ = _run(N, False, False)
    c = step.cfg.contacts                                                 # past ContactConfig.validate(), which SimStep ran
    for name in ("stiffness", "max_force", "probe", "wall_damping"):
        kept = getattr(c, name)
        for v in (0.0, -1.0, float("nan"), float("inf")):
            setattr(c, name, v)
            with pytest.raises(_ffi.DtcError, match=name):
                step.contacts(env)
        setattr(c, name, kept)
    for name in ("body_radius", "stumble_height", "min_speed"):
        kept = getattr(c, name)
        for v in (-1e-3, float("nan"), float("inf")):
            setattr(c, name, v)
            with pytest.raises(_ffi.DtcError, match=name):
                step.contacts(env)
        setattr(c, name, kept)
    kept = c.shanks
    for shanks in ((0, 7, 11, 15), (4, 7, 11, 15), (2, 7, 11, 15), (3, 3, 11, 15), (3, 7, 11, 17), (-1, 7, 11, 15)):
        c.shanks = shanks
        with pytest.raises(_ffi.DtcError, match="shank"):
            step.contacts(env)
    c.shanks = kept
    check = step._check
    step._check = lambda n, t, tail, dtype: None if t is None else check(n, t, tail, dtype)
    for name in CO.FLAGS:
        held = getattr(env, name)
        setattr(env, name, None)
        with pytest.raises(_ffi.DtcError, match="null leg_contact / stumbled"):
            step.contacts(env)
        setattr(env, name, held)
    for name in ("base_pos", "base_quat", "rigid_body_state", "contact_forces"):
        held = getattr(env, name)
        setattr(env, name, None)
        with pytest.raises(_ffi.DtcError, match="null tensor of the step"):
            step.contacts(env)
        setattr(env, name, held)
    step._check = check
    lib, s, k = _ffi.lib(), _ffi.DtcSimStep(), step.cfg_struct()
    assert lib.dtc_sim_contacts(None, k, step.contact_struct(), N, _ffi.stream()) != 0
    assert lib.dtc_sim_contacts(s, None, step.contact_struct(), N, _ffi.stream()) != 0
    assert lib.dtc_sim_contacts(s, k, None, N, _ffi.stream()) != 0
    assert lib.dtc_sim_contacts(s, k, step.contact_struct(), 0, _ffi.stream()) != 0
    held, env.stumbled = env.stumbled, env.stumbled.to(torch.int32)
    with pytest.raises(_ffi.DtcError, match="stumbled"):                  # and the host side refuses a tensor of the wrong dtype
        step.contacts(env)
    env.stumbled = held
    with pytest.raises(_ffi.DtcError):
        step.contacts(types.SimpleNamespace(**{**vars(env), "base_pos": env.base_pos.cpu()}))
    torch.cuda.synchronize()
    for name, whole in buffers.items():                                   # nothing was launched
        assert np.array_equal(H._bytes(whole), before[name]), name
    step.contacts(env)
    torch.cuda.synchronize()
    _compare(buffers, before, want, "after")
