"""The recurrent trainers with their GRU recurrences on operand images (DTC_GRU_H2I=1 / dtc_set_gru_h2i(1): csrc/gru_h2i.hip behind
recurrent_heads.GruHead) next to the default path -- the recurrence of actor_critic_recurrent.py:92-116 over the padded trajectories of
utils/utils.py:33-70 -- on the same weights and inputs: one teacher-forced mini-batch step of RecurrentPPO and of the composite's
RecurrentDecoderPPO, two consecutive updates on two rollouts, and the switch itself."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dtc_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRU_WORKSPACE_24_1473_512 = 386187776       # dtc_gru_workspace(24, 1473, 512) of the build before the image recurrence existed


class _option:
    """dtc_set_gru_h2i(on) for the duration of a with-block, then back to the environment's choice."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from dtc_amd import _ffi
        _ffi.lib().dtc_set_gru_h2i(int(self.on))

    def __exit__(self, *exc):
        from dtc_amd import _ffi
        _ffi.lib().dtc_set_gru_h2i(-1)


def _spy_launches(monkeypatch):
    """Count the launches that tell the two paths apart."""
    from dtc_amd import h2i, ops
    count = dict(pack=0, fwd_h2i=0, bwd_h2i=0, fwd=0, bwd=0)

    def wrap(obj, name, key):
        orig = getattr(obj, name)

        def f(*a, **k):
            count[key] += 1
            return orig(*a, **k)
        monkeypatch.setattr(obj, name, f)
    wrap(h2i.HImage, "pack", "pack")
    wrap(ops, "gru_fwd_h2i", "fwd_h2i")
    wrap(ops, "gru_bwd_h2i", "bwd_h2i")
    wrap(ops, "gru_fwd", "fwd")
    wrap(ops, "gru_bwd", "bwd")
    return count


def _compare(res, arena):
    (m1, v1, r1, g1), (m0, v0, r0, g0) = res
    np.testing.assert_allclose(m1.cpu().numpy(), m0.cpu().numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(v1.cpu().numpy(), v0.cpu().numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(r1.numpy(), r0.numpy(), rtol=1e-5, atol=1e-6)
    worst = 0.0
    for name, (off, cnt, _shape) in arena.offsets.items():
        a, b = g1[off:off + cnt], g0[off:off + cnt]
        scale = float(b.abs().max()) + 1e-30
        err = float((a - b).abs().max()) / scale
        worst = max(worst, err)
        assert err <= 2e-5, (name, err)
    return worst


def _recurrent_ppo(n, seed=11):
    from dtc_amd.algorithms import RecurrentPPO
    from dtc_amd.modules import ActorCriticRecurrent
    torch.manual_seed(3)
    ac = ActorCriticRecurrent(53, 1389, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128],
                              activation='elu', rnn_type='gru', rnn_hidden_size=512, rnn_num_layers=1)
    alg = RecurrentPPO(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV)
    alg.init_storage(n, 24, [53], [1389], [12])
    return ac, alg


def _fill(alg, d, hid):
    for k, v in d.items():
        if k not in ("last_values", "observation_histories"):
            getattr(alg.storage, k).copy_(v)
    alg.storage.compute_returns(d["last_values"], 0.99, 0.95)
    alg.storage.step = 24
    alg.storage.saved_hidden_states_a, alg.storage.saved_hidden_states_c = [hid[0]], [hid[1]]


def test_recurrent_ppo_step_on_image_recurrences_next_to_the_default(monkeypatch):
    """RecurrentPPO at 256 envs x 24 (mini-batch = 1536 valid rows): one teacher-forced step with the option on and off, the bounds of
    test_recurrent_operand_image_path_next_to_the_converting_kernels; the option-on step launches no pack for hx / hp / the gate
    gradients (5 per head: 10 fewer than the default step)."""
    n = 256
    d = S.rollout(n, 24, seed=11, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(6)
    hid = [0.1 * torch.randn(24, 1, n, 512, generator=g, device=DEV) for _ in range(2)]
    count = _spy_launches(monkeypatch)
    res, packs = [], []
    for on in (True, False):
        ac, alg = _recurrent_ppo(n)
        alg.capture_grads = True
        _fill(alg, d, hid)
        batch = next(iter(alg.storage.reccurent_mini_batch_generator(4, 1)))
        assert alg._image_mode(24 * n // 4)
        before = dict(count)
        with _option(on):
            row = alg.step_minibatch(batch, 0, n // 4).cpu()
        used = {k: count[k] - before[k] for k in count}
        assert (used["fwd_h2i"], used["bwd_h2i"], used["fwd"], used["bwd"]) == ((2, 2, 0, 0) if on else (0, 0, 2, 2)), used
        packs.append(used["pack"])
        res.append((ac._actor_outs[-1].clone(), ac._critic_outs[-1].clone(), row, alg.captured["main"].clone()))
    assert packs[1] - packs[0] == 10, packs
    print("RecurrentPPO, option on vs off: largest gradient difference", _compare(res, ac.arena))


def test_composite_step_on_image_recurrences_next_to_the_default(monkeypatch):
    """RecurrentDecoderPPO (GRU + CE-net + foothold observations) at its smallest image-mode size (64 envs x 24: 384 rows per mini-batch):
    the teacher-forced policy step with the option on and off, same bounds; 9 packs fewer (5 for the critic's head, 4 for the actor's)."""
    from dtc_amd import ops
    from dtc_amd.algorithms import RecurrentDecoderPPO
    from dtc_amd.modules import ActorCriticDecoderRecurrent
    n, T = 64, 24
    d = S.rollout(n, T, seed=9, device=DEV)
    d["dones"][:, 0] = 0
    g = torch.Generator(device=DEV).manual_seed(78)
    hid = [0.1 * torch.randn(T, 1, n, 512, generator=g, device=DEV) for _ in range(2)]
    eps = torch.randn(2, T * (n // 4), 16, generator=g, device=DEV)
    count = _spy_launches(monkeypatch)
    seen = []
    orig_loss = ops.ppo_loss
    monkeypatch.setattr(ops, "ppo_loss", lambda mean, std, value, *a, **k: (seen.append((mean.clone(), value.clone())), orig_loss(mean, std, value, *a, **k))[1])
    res, packs = [], []
    for on in (True, False):
        torch.manual_seed(3)
        ac = ActorCriticDecoderRecurrent(53, 1389, 12)
        alg = RecurrentDecoderPPO(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV)
        alg.init_storage(n, T, [53], [1389], [265], [12])
        alg.capture_grads = True
        for k, v in d.items():
            if k != "last_values":
                getattr(alg.storage, k).copy_(v)
        alg.storage.compute_returns(d["last_values"], 0.99, 0.95)
        bt = next(iter(alg.recurrent_slices(hid[0], hid[1])))
        assert bt["idx"].numel() == 384 and alg._image_mode(ac._fwd_ws(384)) and alg._memory_images()
        before = dict(count)
        with _option(on):
            row = alg.step_minibatch(bt, eps[0], eps[1], which="ppo").cpu()
        used = {k: count[k] - before[k] for k in count}
        assert (used["fwd_h2i"], used["bwd_h2i"], used["fwd"], used["bwd"]) == ((2, 2, 0, 0) if on else (0, 0, 2, 2)), used
        packs.append(used["pack"])
        mean, value = seen[-1]
        res.append((mean, value, row, alg.captured["main"].clone()))
    assert packs[1] - packs[0] == 9, packs
    print("composite, option on vs off: largest gradient difference", _compare(res, ac.arena))


def test_two_consecutive_updates_with_the_option_on():
    """Two updates on two different rollouts with the option on: the slot maps (built once per update and mini-batch slot) and the images
    the kernels write must follow the new rollout.  Weights stay finite and the adaptive learning rate ends where the option-off run's
    does; after the second update every head's slot map is the inverse of that update's unpad_idx."""
    n = 64
    g = torch.Generator(device=DEV).manual_seed(5)
    hid = [0.1 * torch.randn(24, 1, n, 512, generator=g, device=DEV) for _ in range(2)]
    lrs, maps_ok = [], []
    for on in (True, False):
        ac, alg = _recurrent_ppo(n)
        with _option(on):
            for seed in (9, 10):
                d = S.rollout(n, 24, seed=seed, device=DEV)
                _fill(alg, d, hid)
                if on and seed == 10:
                    from dtc_amd.algorithms import recurrent_heads as RH
                    orig = RH.GruHead._slot_row

                    def spy(self, orig=orig):
                        s = orig(self)
                        want = torch.full_like(s, -1)
                        want[self.unpad_idx] = torch.arange(self.M, dtype=torch.int32, device=s.device)
                        maps_ok.append(bool(torch.equal(s, want)))
                        return s
                    RH.GruHead._slot_row = spy
                    try:
                        alg.update()
                    finally:
                        RH.GruHead._slot_row = orig
                else:
                    alg.update()
        assert all(bool(torch.isfinite(p).all()) for p in ac.parameters()), on
        lrs.append(alg.learning_rate)
    assert len(maps_ok) == 2 * alg.num_mini_batches * alg.num_learning_epochs and all(maps_ok), f"{maps_ok.count(False)} stale slot maps in the second update"
    assert lrs[0] == lrs[1], lrs


def test_switch_is_off_by_default_and_the_default_workspace_did_not_grow():
    from dtc_amd import _ffi, ops
    lib = _ffi.lib()
    if "DTC_GRU_H2I" not in os.environ:
        assert lib.dtc_get_gru_h2i() == 0 and not ops.gru_h2i_on()
    lib.dtc_set_gru_h2i(1)
    try:
        assert lib.dtc_get_gru_h2i() == 1
    finally:
        lib.dtc_set_gru_h2i(-1)
    assert lib.dtc_gru_workspace(24, 1473, 512) == GRU_WORKSPACE_24_1473_512
    assert lib.dtc_gru_h2i_workspace(24, 1473, 512) > 0


CHILD = r'''
import json, os, sys
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "deep-tracking-control_amd"))
import torch
from dtc_amd import _ffi, ops, synthetic as S
import test_gru_h2i_path as P
on = _ffi.lib().dtc_get_gru_h2i()
n = 64
g = torch.Generator(device=P.DEV).manual_seed(5)
hid = [0.1 * torch.randn(24, 1, n, 512, generator=g, device=P.DEV) for _ in range(2)]
ac, alg = P._recurrent_ppo(n)
P._fill(alg, S.rollout(n, 24, seed=9, device=P.DEV), hid)
calls = []
orig = ops.gru_fwd_h2i
ops.gru_fwd_h2i = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
alg.update()
ok = all(bool(torch.isfinite(p).all()) for p in ac.parameters())
print("RESULT " + json.dumps(dict(on=on, calls=len(calls), want=2 * alg.num_mini_batches * alg.num_learning_epochs, ok=ok)))
'''


def test_environment_switch_in_a_fresh_process():
    """DTC_GRU_H2I=1 is read by the library at its first use: a fresh process with it set trains on the image recurrences."""
    env = dict(os.environ, DTC_GRU_H2I="1")
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert res["on"] == 1 and res["ok"] and res["calls"] == res["want"] > 0, res
