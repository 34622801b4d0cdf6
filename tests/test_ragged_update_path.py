"""PPO(..., ragged_images=True): PPO.update on the operand-image schedule at mini-batch row counts that are no multiple of 128
(rsl_rl/rsl_rl/algorithms/ppo.py:189-338 at the reference's own sizes: legged_robot_config.py 100 envs x 24 steps / 4 mini-batches =
600 rows).  Sizes here: 20 / 44 / 100 envs x 24 steps in 4 mini-batches = 120 (below one tile), 264 (two tiles + 8), 600 rows.

The teacher-forced steps are tests/test_hip_ppo.py::_teacher_forced_step itself -- the scalars at 1e-5, the gradient and weight bounds
of test_update_teacher_forced_64 -- with one helper restated: the oracle's ReLU signs are packed into sign records of ceil(B / 32)
groups (that file's packer takes B % 32 == 0 only)."""
import numpy as np
import pytest
import torch

from dtc_amd import synthetic as S

DEV = "cuda:0"
SIZES = [20, 44, 100]                    # envs -> 120, 264, 600 rows per mini-batch


def _pack_sign_record_any(pos):
    """bool [B, W] -> the int16 sign-record words of ceil(B / 32) groups; the rows behind B of the last group are 0 bits"""
    B, W = pos.shape
    G = -(-B // 32)
    full = torch.zeros(G * 32, W, dtype=torch.bool)
    full[:B] = pos
    bits = full.view(G, 4, 2, 4, W).permute(0, 2, 1, 3, 4).reshape(G, 2, 16, W).to(torch.int32)
    words = (bits << torch.arange(16, dtype=torch.int32).view(1, 1, 16, 1)).sum(dim=2).reshape(-1, W)
    return torch.from_numpy(words.numpy().astype(np.uint16).view(np.int16))


def _pair(N, seed=4, oracle=True, **kw):
    """tests/test_hip_ppo.py::_pair with trainer-only keywords: (oracle RefPPO on the CPU or None, HIP PPO) with identical filled weights
    and rollout"""
    from dtc_amd.algorithms import PPO
    from dtc_amd.modules import ActorCriticDecoder
    from oracle import ppo_ref as OP
    torch.manual_seed(3)
    ref_ac = OP.fill_parameters_(OP.RefActorCriticDecoder(), 11)
    ref = None
    if oracle:
        ref = OP.RefPPO(ref_ac, learning_rate=1e-3, entropy_coef=0.003)
        ref.init_storage(N, 24)
    torch.manual_seed(3)
    ac = ActorCriticDecoder(53, 1389, 12)
    alg = PPO(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV, **kw)
    alg.init_storage(N, 24, [53], [1389], [265], [12])
    ac.load_state_dict(ref_ac.state_dict())
    d = S.rollout(N, 24, seed=seed)
    for k, v in d.items():
        if k == "last_values":
            continue
        if ref is not None:
            getattr(ref.storage, k).copy_(v)
        getattr(alg.storage, k).copy_(v.to(DEV))
    if ref is not None:
        ref.storage.compute_returns(d["last_values"], 0.99, 0.95)
    alg.storage.compute_returns(d["last_values"].to(DEV), 0.99, 0.95)
    return ref, alg


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n_envs", SIZES)
def test_update_teacher_forced_on_ragged_images(n_envs, monkeypatch):
    """two mini-batch steps (the second reuses the workspace's images and records) against the oracle: the bounds of
    test_update_teacher_forced_64, every ReLU record teacher-forced; and both steps ran on images"""
    import test_hip_ppo as T
    monkeypatch.setattr(T, "_pack_sign_record", _pack_sign_record_any)
    ref, alg = _pair(n_envs, ragged_images=True)
    perm, e1, e2 = S.update_noise(n_envs, 24, 4, 5, seed=123)
    mb = n_envs * 24 // 4
    assert mb % 128 != 0
    for k in range(2):
        T._teacher_forced_step(k, ref, alg, perm[k * mb:(k + 1) * mb], e1[k], e2[k])
        fw = alg.actor_critic._fwd_ws(mb)
        assert fw.ragged and alg._image_mode(fw)
        assert len(fw._masks) == 7 and all(m.numel() == -(-mb // 32) * 2 * w for m, w in ((fw._masks["c1"], 64), (fw._masks["t1"], 512)))


_WIDE_ENTRY_POINTS = ("linear_fwd", "linear_dgrad", "linear_wgrad", "wgrad_group", "linear_fwd_mse")


def _count_converting_launches(monkeypatch, alg, n_envs):
    """one update(); every call into the fp32 / converting (_h2, _s3) layer entry points of dtc_amd.ops while it runs"""
    from dtc_amd import ops
    calls = []
    for name in _WIDE_ENTRY_POINTS:
        inner = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda inner, name: lambda *a, **k: (calls.append(name), inner(*a, **k))[1])(inner, name))
    perm, e1, e2 = S.update_noise(n_envs, 24, 4, 5, seed=123)
    out = alg.update(perm=perm, eps1=e1.to(DEV), eps2=e2.to(DEV))
    monkeypatch.undo()
    assert all(np.isfinite(v) for v in out) and bool(torch.isfinite(alg.last_update_stats).all())
    return calls


@pytest.mark.gpu
def test_the_ragged_update_runs_on_images_only(monkeypatch):
    """20 envs (120 rows): with ragged_images the update launches no layer kernel outside the operand-image family; without it the same
    update goes through the converting kernels (so the counter does see them)"""
    _, alg = _pair(20, oracle=False, ragged_images=True)
    calls = _count_converting_launches(monkeypatch, alg, 20)
    fw = alg.actor_critic._fwd_ws(120)
    assert alg._image_mode(fw) and fw.ragged
    assert calls == [], sorted(set(calls))
    _, plain = _pair(20, oracle=False)
    calls = _count_converting_launches(monkeypatch, plain, 20)
    assert not plain._image_mode(plain.actor_critic._fwd_ws(120))
    assert {"linear_fwd", "linear_dgrad", "wgrad_group"} <= set(calls)


@pytest.mark.gpu
def test_default_is_untouched():
    """PPO() keeps today's rule: 20 envs (120 rows) off the image schedule, no sign record at that row count; 64 envs (384 rows) on it;
    the recurrent decoder trainer refuses the keyword"""
    from dtc_amd.algorithms import RecurrentDecoderPPO, RecurrentPPO
    from dtc_amd.modules import ActorCriticDecoder
    _, alg = _pair(20, oracle=False)
    perm, e1, e2 = S.update_noise(20, 24, 4, 5, seed=123)
    alg.step_minibatch(perm[:120], e1[0], e2[0])
    fw = alg.actor_critic._fwd_ws(120)
    assert not fw.ragged and not alg._image_mode(fw) and fw.relu_mask("t1", 512) is None and not fw.live_img
    _, alg = _pair(64, oracle=False)
    perm, e1, e2 = S.update_noise(64, 24, 4, 5, seed=123)
    alg.step_minibatch(perm[:384], e1[0], e2[0])
    fw = alg.actor_critic._fwd_ws(384)
    assert not fw.ragged and alg._image_mode(fw) and {"t1", "t2"} <= fw.live_img
    with pytest.raises(TypeError, match="ragged_images"):
        RecurrentDecoderPPO.__new__(RecurrentDecoderPPO).__init__(ActorCriticDecoder(53, 1389, 12), device="cpu", ragged_images=True)
    with pytest.raises(TypeError, match="ragged_images"):
        RecurrentPPO.__new__(RecurrentPPO).__init__(ActorCriticDecoder(53, 1389, 12), device="cpu", ragged_images=True)


@pytest.mark.gpu
def test_one_pass_at_a_ragged_row_count():
    """PPO(gemm_passes=1, ragged_images=True) at 20 envs: one mini-batch step from the same weights as the three-pass trainer, the
    data-dependent branches of the backward pass (ReLU sign records, CE-net outlier choice and median element) taken from the three-pass
    step as tests/test_onepass_path.py takes them from its oracle -- 1 - cosine of the whole gradient of either optimisation step within
    the figure profiles/h2i_onepass_accuracy.txt records for one pass (4.06e-07, its largest whole-gradient figure over three seeds; the
    three-pass side's own distance from float64 is six orders below) --, then a whole update() with finite statistics.  The library is
    back at three passes afterwards."""
    from dtc_amd import h2i
    ONE_PASS_COS = 4.06e-07          # profiles/h2i_onepass_accuracy.txt: cos_all, one pass
    perm, e1, e2 = S.update_noise(20, 24, 4, 5, seed=123)
    saved = {}

    def keep(fw, which):
        torch.cuda.synchronize()
        saved[which] = ({k: v.clone() for k, v in fw._masks.items()}, fw.mask.clone(), fw.info[:2].clone(), fw.mulv[:, 19:].clone())

    def force(fw, which):
        torch.cuda.synchronize()
        records, outliers, info, logvar = saved[which]
        for k, v in records.items():
            if not (which == "ppo" and k in ("c1", "c2", "d1", "d2")):
                fw._masks[k].copy_(v)
        differ = fw.mask != outliers
        fw.mulv[:, 19:][differ] = logvar[differ]
        fw.mask.copy_(outliers)
        fw.info[:2] = info
        torch.cuda.synchronize()

    for which, cap in (("vae", "vae"), ("ppo", "main")):       # each optimisation step from the SAME weights on both sides
        grads = []
        for kw, hook in ((dict(), keep), (dict(gemm_passes=1), force)):
            _, alg = _pair(20, oracle=False, ragged_images=True, **kw)
            alg.capture_grads, alg.after_forward_hook = True, hook
            row, _ = alg.step_minibatch(perm[:120], e1[0], e2[0], which=which)
            assert bool(torch.isfinite(row).all()) and alg._image_mode(alg.actor_critic._fwd_ws(120))
            grads.append(alg.captured[cap].double().reshape(-1))
        assert h2i.h2i_passes() == 3 and len(saved[which][0]) == (7 if which == "vae" else 3)
        a, b = grads
        dist = 1.0 - float(torch.dot(a, b) / (a.norm() * b.norm()))
        print(f"one pass at 120 rows, {which} step: 1 - cosine to three passes {dist:.2e} (bound {ONE_PASS_COS:.2e})")
        assert not torch.equal(a, b)
        assert dist <= ONE_PASS_COS, (which, dist)
    _, alg = _pair(20, oracle=False, gemm_passes=1, ragged_images=True)
    out = alg.update(perm=perm, eps1=e1.to(DEV), eps2=e2.to(DEV))
    assert all(np.isfinite(v) for v in out) and bool(torch.isfinite(alg.last_update_stats).all())
    assert bool(torch.isfinite(alg.actor_critic.arena.flat).all()) and h2i.h2i_passes() == 3


@pytest.mark.gpu
def test_a_diverged_env_stays_in_its_row_at_a_ragged_row_count():
    """tests/test_hip_ppo.py::test_a_diverged_env_stays_in_its_row_on_the_rollout_side on the update's forward pass at B = 120: the
    sample in row 119 -- the last row of the only tile, next to the 8 tail rows -- has inf / NaN observations and privileged
    observations.  Every other row of the policy step's forward outputs (terrain latent, actor / critic bodies, action mean, value) is
    bit-identical to the clean step; row 119 is not finite.  (The observation history stays clean: the CE-net's outlier statistics are
    batch-global in the reference itself.)"""
    perm, e1, e2 = S.update_noise(20, 24, 4, 5, seed=123)
    idx = perm[:120]
    outs = []
    for dirty in (False, True):
        _, alg = _pair(20, oracle=False, ragged_images=True)
        if dirty:
            row = int(idx[119])
            obs, priv = alg.storage.flat("observations"), alg.storage.flat("privileged_observations")
            obs[row, 3], obs[row, 40] = float("nan"), float("inf")
            priv[row] = float("nan")
        alg.step_minibatch(idx, e1[0], e2[0], which="ppo")
        fw = alg.actor_critic._fwd_ws(120)
        assert alg._image_mode(fw)
        outs.append([t.clone() for t in (fw.img("lt").to_tensor(), fw.img("a1").to_tensor(), fw.img("v1").to_tensor(), fw.a3, fw.v3, fw.mean, fw.val)])
    for name, c, d in zip(("l_t", "a1", "v1", "a3", "v3", "mean", "value"), *outs):
        assert torch.equal(c[:119].view(torch.int32), d[:119].view(torch.int32)), name
        assert bool(torch.isfinite(c).all()) and not bool(torch.isfinite(d[119]).all()), name


@pytest.mark.gpu
def test_two_trainers_on_one_model_each_get_their_own_schedule():
    """a default PPO and a PPO(ragged_images=True) on ONE model (one forward workspace per row count), 20 envs (120 rows), their
    step_minibatch calls alternating twice: after each call the workspace's `ragged` mark and live images are that trainer's (the
    assertions of test_default_is_untouched and test_the_ragged_update_runs_on_images_only), and the other trainer's _image_mode query
    in between changes nothing"""
    from dtc_amd.algorithms import PPO
    _, plain = _pair(20, oracle=False)
    ac = plain.actor_critic
    ragged = PPO(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV, ragged_images=True)
    ragged.init_storage(20, 24, [53], [1389], [265], [12])
    d = S.rollout(20, 24, seed=4)
    for k, v in d.items():
        if k != "last_values":
            getattr(ragged.storage, k).copy_(v.to(DEV))
    ragged.storage.compute_returns(d["last_values"].to(DEV), 0.99, 0.95)
    perm, e1, e2 = S.update_noise(20, 24, 4, 5, seed=123)
    fw = ac._fwd_ws(120)
    for k in range(2):
        row, _ = plain.step_minibatch(perm[:120], e1[k], e2[k])
        assert bool(torch.isfinite(row).all())
        assert not fw.ragged and not plain._image_mode(fw) and fw.relu_mask("t1", 512) is None and not fw.live_img
        asked = ragged._image_mode(fw)
        assert bool(asked) == (k == 1)                  # its own last schedule at 120 rows (none before its first step), not the mark
        assert not fw.ragged and fw.relu_mask("t1", 512) is None and not fw.live_img
        row, _ = ragged.step_minibatch(perm[:120], e1[k], e2[k])
        assert bool(torch.isfinite(row).all())
        assert fw.ragged and ragged._image_mode(fw) and {"t1", "t2"} <= fw.live_img
        live = set(fw.live_img)
        assert not plain._image_mode(fw)
        assert fw.ragged and fw.live_img == live and fw.relu_mask("t1", 512) is not None


# ------------------------------------------------------------------------------------------------ host side: no GPU
class _StandInWs:
    """what PPO._image_mode / PPO._resolve_schedule read of a forward workspace (test_images_ok_and_the_workspace_rule's stand-in,
    with the mark)"""

    def __init__(self, B, ragged=False):
        self.B, self.ragged = B, ragged


_SWITCHES = ("use_images", "narrow_images", "relu_masks", "group_wgrad", "fuse_height_loss")


def _rollouts():
    """a small rollout tensor, and test_images_ok_and_the_workspace_rule's 2 GiB one (no storage behind it)"""
    from dtc_amd import _ffi
    big = dict(privileged_observations=torch.empty_strided((400000, 1389), (1389, 1), device="meta"))
    assert 400000 * 1389 > _ffi.MAX_OPERAND_ELEMS
    return dict(observations=torch.empty(480, 53)), big


def test_image_mode_is_a_pure_query():
    """a default trainer asked about a workspace another trainer left marked ragged: the mark stays, nothing else appears on the
    workspace, and the answer is the default trainer's own (whole tiles only)"""
    from dtc_amd import ops
    from dtc_amd.algorithms import PPO
    from dtc_amd.modules import ActorCriticDecoder
    plain = PPO(ActorCriticDecoder(53, 1389, 12), device="cpu")
    for B in (120, 384, 600):
        ws = _StandInWs(B, ragged=True)
        got = plain._image_mode(ws)
        assert ws.ragged is True and vars(ws) == dict(B=B, ragged=True)
        assert got is (bool(ops.SPLIT) and B % 128 == 0)


def test_the_resolver_truth_table():
    """PPO._resolve_schedule over 120 / 384 / 600 rows x the trainer keywords x a small and a 2 GiB rollout x each switch of the image
    schedule off in turn: `whole` needs every switch, `images` every one but narrow_images, `ragged` a ragged row count + the flag or
    the 2 GiB tensor + `whole`; `passes` is gemm_passes; the resolver (and nothing else) marks the workspace.  ops.SPLIT as it stands."""
    from dtc_amd import ops
    from dtc_amd.algorithms import PPO, RecurrentDecoderPPO
    from dtc_amd.algorithms.ppo import Schedule
    from dtc_amd.modules import ActorCriticDecoder
    ac = ActorCriticDecoder(53, 1389, 12)
    small, big = _rollouts()
    split = bool(ops.SPLIT)
    seen = set()
    for kw in (dict(), dict(ragged_images=True), dict(gemm_passes=1), dict(gemm_passes=1, ragged_images=True)):
        alg = PPO(ac, device="cpu", **kw)
        for off in (None,) + _SWITCHES:
            for name in _SWITCHES:
                setattr(alg, name, name != off)
            for B in (120, 384, 600):
                for flat in (small, big):
                    ws = _StandInWs(B, ragged=B == 384)                      # a stale mark either way
                    got = alg._resolve_schedule(ws, flat)
                    ragged = split and off is None and B % 128 != 0 and (alg.ragged_images or flat is big)
                    images = split and off in (None, "narrow_images") and (B % 128 == 0 or ragged)
                    want = Schedule(images=images, whole=images and off is None, ragged=ragged, passes=kw.get("gemm_passes", 3))
                    assert got == want and all(type(v) is bool for v in got[:3]), (kw, off, B, flat is big, got, want)
                    assert ws.ragged is ragged and vars(ws) == dict(B=B, ragged=ragged)
                    assert alg._wants_ragged(B, flat) == (B % 128 != 0 and (alg.ragged_images or flat is big))
                    seen.add(got)
    if split:
        assert {(s.images, s.whole, s.ragged) for s in seen} == {(False, False, False), (True, False, False), (True, True, False), (True, True, True)}
    # the trajectory trainer: whole tiles only, never `whole`, never ragged -- not even for the 2 GiB tensor
    rec = RecurrentDecoderPPO(ac, device="cpu")
    assert rec.row_sets is False and PPO.row_sets is True
    for B in (120, 384, 600):
        ws = _StandInWs(B, ragged=True)
        assert rec._resolve_schedule(ws, big) == Schedule(images=split and B == 384, whole=False, ragged=False, passes=3)
        assert ws.ragged is False and rec._image_mode(ws) is (split and B == 384)


def test_both_opt_ins_are_refused_by_one_helper_with_one_text():
    """gemm_passes=1 and contain_nonfinite=True on a schedule that is not `whole` (120 rows, no ragged_images): DtcError out of
    PPO._needs_whole_step, the message names the opt-in, the row count, ops.SPLIT and every switch; containment adds its sentence about
    whole-tensor amax.  On a `whole` schedule the helper lets both through."""
    from dtc_amd import _ffi, ops
    from dtc_amd.algorithms import PPO
    from dtc_amd.algorithms.ppo import Schedule
    from dtc_amd.modules import ActorCriticDecoder
    ac = ActorCriticDecoder(53, 1389, 12)
    small, _ = _rollouts()

    class _Tw:
        B = 120
    msgs = {}
    for what, kw, call in (("gemm_passes=1", dict(gemm_passes=1), lambda alg, tw: alg._gemm_passes_scope(tw)),
                           ("contain_nonfinite=True", dict(contain_nonfinite=True), lambda alg, tw: alg._contained_perm(tw, torch.arange(480)))):
        alg, tw = PPO(ac, device="cpu", **kw), _Tw()
        tw.schedule = alg._resolve_schedule(_StandInWs(120), small)
        assert not tw.schedule.whole and tw.schedule.passes == kw.get("gemm_passes", 3)
        with pytest.raises(_ffi.DtcError) as e:
            call(alg, tw)
        assert e.traceback[-1].name == "_needs_whole_step"
        msg = msgs[what] = str(e.value)
        assert msg.startswith(f"{what} needs the operand-image schedule for the whole step") and "(this one: 120)" in msg
        assert f"ops.SPLIT = {ops.SPLIT}" in msg and "multiple of 128 rows" in msg
        assert all(name in msg for name in _SWITCHES + ("ragged_images=True",))
        tw.schedule = Schedule(True, True, True, tw.schedule.passes)
        PPO._needs_whole_step(tw, what)
    assert msgs["contain_nonfinite=True"].endswith("every other schedule reads whole rollout tensors (amax)")
    assert "amax" not in msgs["gemm_passes=1"]
    assert msgs["contain_nonfinite=True"].split(" needs ", 1)[1].startswith(msgs["gemm_passes=1"].split(" needs ", 1)[1])


def test_relu_mask_ok_no_longer_tests_the_row_count():
    from dtc_amd import ops
    for M in (1, 48, 120, 128, 600, 24576):
        assert ops.relu_mask_ok(M, 512) and ops.relu_mask_ok(M, 128) and ops.relu_mask_ok(M, 64)
        assert not ops.relu_mask_ok(M, 96) and not ops.relu_mask_ok(M, 53)
    assert not ops.relu_mask_ok(0, 512)


def test_record_size_counts_32_row_groups():
    from dtc_amd import _ffi
    lib = _ffi.lib()
    for M, groups in ((1, 1), (32, 1), (33, 2), (100, 4), (128, 4), (130, 5), (600, 19), (24576, 768)):
        assert lib.dtc_relu_mask_elems(M, 512) == groups * 2 * 512 and lib.dtc_relu_mask_elems(M, 64) == groups * 2 * 64


def test_unpack_helper_rounds_up_and_trims_on_a_numpy_record():
    """a record of 130 rows x 64 columns built with numpy: 5 groups of 32 rows; the helper decodes all 160 and trims to 130"""
    from dtc_amd import h2i
    rng = np.random.default_rng(5)
    M, N = 130, 64
    pos = np.zeros((160, N), dtype=bool)
    pos[:M] = rng.random((M, N)) < 0.5
    words = np.zeros((5, 2, N), dtype=np.uint16)
    for r in range(16):
        for half in range(2):
            words[:, half, :] |= (pos.reshape(5, 32, N)[:, (r & 3) + 8 * (r >> 2) + 4 * half, :].astype(np.uint16) << r)
    rec = torch.from_numpy(words.reshape(-1).view(np.int16).copy())
    got = h2i.unpack_sign_record(rec, M, N)
    assert got.shape == (M, N) and np.array_equal(got.numpy(), pos[:M])
    allrows = h2i.unpack_sign_groups(rec, M, N)
    assert allrows.shape == (160, N) and np.array_equal(allrows.numpy(), pos) and not allrows[M:].any()
    assert np.array_equal(h2i.unpack_sign_record(torch.from_numpy(_pack_sign_record_any(torch.from_numpy(pos[:M])).numpy().reshape(-1)), M, N).numpy(),
                          pos[:M])
    assert h2i.unpack_sign_record(rec[:4 * 2 * N], 128, N).shape == (128, N)          # whole groups: nothing to trim


def test_images_ok_and_the_workspace_rule():
    """ActorCriticDecoder.images_ok(ws, ragged) and the trainer's choice of the ragged schedule (PPO._wants_ragged), on stand-ins"""
    from dtc_amd import _ffi, ops
    from dtc_amd.algorithms import PPO
    from dtc_amd.modules import ActorCriticDecoder

    class _Ws:
        def __init__(self, B):
            self.B = B
    ac = ActorCriticDecoder(53, 1389, 12)
    for B in (120, 600):
        assert not ac.images_ok(_Ws(B)) and not ac.images_ok(_Ws(B), ragged=False) and bool(ac.images_ok(_Ws(B), ragged=True)) == bool(ops.SPLIT)
    assert bool(ac.images_ok(_Ws(384))) == bool(ops.SPLIT)
    small = dict(observations=torch.empty(480, 53))
    plain, ragged, onepass = PPO(ac, device="cpu"), PPO(ac, device="cpu", ragged_images=True), PPO(ac, device="cpu", gemm_passes=1)
    assert plain.ragged_images is False and ragged.ragged_images is True
    assert not plain._wants_ragged(120, small) and ragged._wants_ragged(120, small)
    assert not ragged._wants_ragged(384, small)                                  # whole tiles: nothing ragged about it
    assert not onepass._wants_ragged(120, small)                                 # one pass at a ragged row count needs the flag
    # a rollout tensor of 2 GiB and more has no form on the converting kernels: the image schedule without the flag
    big = dict(privileged_observations=torch.empty_strided((400000, 1389), (1389, 1), device="meta"))
    assert 400000 * 1389 > _ffi.MAX_OPERAND_ELEMS
    assert plain._wants_ragged(120, big) and not plain._wants_ragged(384, big)


def test_keyword_is_keyword_only_and_reaches_the_trainer_through_the_runner_config():
    import inspect
    from dtc_amd.algorithms import PPO, RecurrentPPO
    from dtc_amd.env import ReplayEnv
    from dtc_amd.runners import OnPolicyRunner
    sig = inspect.signature(PPO.__init__)
    assert sig.parameters["ragged_images"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["ragged_images"].default is False
    assert "ragged_images" not in inspect.signature(RecurrentPPO.__init__).parameters
    runner = dict(policy_class_name="ActorCriticDecoder", algorithm_class_name="PPO", num_steps_per_env=24, save_interval=10)
    for algo, want in ((dict(learning_rate=1e-3, ragged_images=True), True), (dict(learning_rate=1e-3), False)):
        r = OnPolicyRunner(ReplayEnv(8, "cpu"), dict(runner=runner, algorithm=algo, policy=dict()), log_dir=None, device="cpu")
        assert r.alg.ragged_images is want and r.alg.num_mini_batches == 4
    with pytest.raises(TypeError, match="ragged_images"):
        OnPolicyRunner(ReplayEnv(8, "cpu"), dict(runner=dict(runner, algorithm_class_name="RecurrentDecoderPPO",
                                                             policy_class_name="ActorCriticDecoderRecurrent"),
                                                 algorithm=dict(ragged_images=True), policy=dict()), log_dir=None, device="cpu")
