"""dtc_sim_step (csrc/sim.hip) through the C ABI against its numpy float32 restatement (tests/sim_oracle.py): equal bits on every
output, over three consecutive steps, with every tensor allocated inside a NaN-filled buffer whose bytes outside the env rows are
compared too.  tests/test_sim_oracle.py shows on the CPU which branches the seeded inputs of tests/sim_cases.py reach.  GPU only."""
import numpy as np
import pytest
import torch

import sim_cases as CASES
import sim_oracle as O

pytestmark = pytest.mark.gpu
GUARD = 3                      # rows of NaN (0xFF bytes for the integer tensors) either side of every env tensor


def _guarded(a, dev, env_axis):
    """`a` on the device inside a buffer with GUARD extra rows either side of the env axis; returns (view, whole buffer)."""
    a = np.ascontiguousarray(a)
    shape = list(a.shape)
    shape[env_axis] += 2 * GUARD
    t = torch.from_numpy(a)
    buf = torch.empty(shape, dtype=t.dtype, device=dev)
    buf.view(torch.uint8).fill_(0xFF)
    view = buf.narrow(env_axis, GUARD, a.shape[env_axis])
    view.copy_(t)
    return view, buf


def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy()


class _Env:
    """The env's tensors on the device.  Ring buffers are time-major, so their env rows are not contiguous inside a guarded buffer:
    they are guarded along time instead, and the kernel sees them dense."""

    def __init__(self, st, dev):
        self.buffers = {}
        dof_state, whole = _guarded(np.stack([st["dof_pos"], st["dof_vel"]], axis=2), dev, 0)          # [N,D,2], as the reference
        self.buffers["dof_state"] = whole
        self.dof_state, self.dof_pos, self.dof_vel = dof_state, dof_state[..., 0], dof_state[..., 1]
        for name in O.STATE + O.INPUTS:
            if name in ("dof_pos", "dof_vel"):
                continue
            ring = name in ("lin_vel_buffer", "ang_vel_buffer", "cmd_buffer")
            view, whole = _guarded(st[name], dev, 0)
            if ring:                                                      # [T + 2 GUARD, N, W]: the middle T slices are contiguous
                assert view.is_contiguous()
            setattr(self, name, view)
            self.buffers[name] = whole

    def expect(self, new):
        """The whole buffers as they must be after a step that leaves `new` (the oracle's STATE) behind."""
        out = {}
        for name, whole in self.buffers.items():
            a = np.stack([new["dof_pos"], new["dof_vel"]], axis=2) if name == "dof_state" else new.get(name)
            e = np.frombuffer(bytes([0xFF]) * (whole.numel() * whole.element_size()), dtype=np.uint8).copy()
            if a is None:                                                 # an input: unchanged
                out[name] = None
                continue
            a = np.ascontiguousarray(a).astype(_NP[whole.dtype], copy=False)
            row = a[0].nbytes
            e[GUARD * row:GUARD * row + a.nbytes] = a.view(np.uint8).reshape(-1)
            out[name] = e
        return out


_NP = {torch.float32: np.float32, torch.int64: np.int64, torch.bool: np.bool_}


def _run(N, decimation, rough, seed=0):
    from dtc_amd import sim as SIM
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = CASES.config(decimation)
    st = CASES.state(N, cfg)
    env = _Env(st, dev)
    before = {name: _bytes(b) for name, b in env.buffers.items()}
    step = SIM.SimStep(N, dev, cfg, torch.from_numpy(CASES.terrain(rough)), seed=seed)
    return cfg, env, before, step


@pytest.mark.parametrize("rough", [False, True], ids=["flat", "rough"])
@pytest.mark.parametrize("decimation", [1, 4])
@pytest.mark.parametrize("N", [1, 3, 257])
def test_sim_step_matches_the_oracle_bit_for_bit(N, decimation, rough):
    cfg, env, before, step = _run(N, decimation, rough)
    ref = CASES.run(N, cfg, rough)
    dev = step.device
    for i, (a, u, new) in enumerate(ref):
        step.step(env, torch.from_numpy(a).to(dev), torch.from_numpy(u).to(dev))
        torch.cuda.synchronize()
        want = env.expect(new)
        for name, whole in env.buffers.items():
            got = _bytes(whole).reshape(-1)
            exp = before[name].reshape(-1) if want[name] is None else want[name]
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, f"step {i}: {name} differs in {bad.size} bytes, first at byte {bad[0]} of {got.size}"
    assert step.counter == 0                                              # given draws do not advance the call counter


def test_generated_command_draws():
    """u_cmd left out: the kernel's Philox draws -- the oracle's bits for the same key and counter, equal bits between two runs from
    the same seed, other bits under another seed or call counter, every resampled command inside its range."""
    N, decimation = 257, 4
    cfg = CASES.config(decimation)
    ref = CASES.run(N, cfg, False, u_given=False, seed=1234)
    runs = []
    for seed, first_counter in ((1234, 0), (1234, 0), (1235, 0), (1234, 7)):
        _, env, _, step = _run(N, decimation, False, seed=seed)
        step.counter = first_counter
        cmds = []
        for i, (a, _, new) in enumerate(ref):
            step.step(env, torch.from_numpy(a).to(step.device))
            cmds.append(env.commands.cpu().numpy().copy())
        assert step.counter == first_counter + len(ref)
        runs.append(np.stack(cmds))
    want = np.stack([new["commands"] for _, _, new in ref])
    assert np.array_equal(runs[0].view(np.int32), want.view(np.int32))
    assert np.array_equal(runs[0].view(np.int32), runs[1].view(np.int32))
    lens = np.stack([new["episode_length_buf"] for _, _, new in ref])
    due = lens % cfg.resampling_steps == 0
    assert due.sum() > 50
    for other in runs[2:]:
        assert (other[due] != runs[0][due]).any(axis=-1).mean() > 0.9
        assert np.array_equal(other[0][~due[0]], runs[0][0][~due[0]])
    c = runs[0][due]
    assert (np.abs(c[:, 0]) <= 0.75).all() and (np.abs(c[:, 1]) <= 0.75).all() and (np.abs(c[:, 2]) <= 0.5).all()
    small = np.hypot(c[:, 0], c[:, 1]) <= 0.1
    assert (c[small, :2] == 0).all()
    # the draws themselves: [0, 1), 24 bits, and spread over the range
    u = O.command_draws(O.config_dict(cfg, CASES.ROWS, CASES.COLS, seed=1234, counter=0), 4096)
    assert (u >= 0).all() and (u < 1).all() and np.array_equal(u * 2.0 ** 24, np.floor(u * 2.0 ** 24))
    assert abs(float(u.mean()) - 0.5) < 0.02 and u.min() < 0.01 and u.max() > 0.99


def test_cpu_tensors_are_refused():
    from dtc_amd import _ffi
    _, env, _, step = _run(3, 4, False)
    with pytest.raises(_ffi.DtcError):
        step.step(env, torch.zeros(3, 12))
