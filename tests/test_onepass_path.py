"""PPO(..., gemm_passes=1): the update's operand-image schedule on the hi planes alone (h2i.h2i_passes_as(1) around PPO.update /
step_minibatch; rsl_rl/rsl_rl/algorithms/ppo.py:189-338).  64 envs x 24 steps, 4 mini-batches of 384 rows, built as
tests/test_hip_ppo.py::test_update_teacher_forced_64 builds its case.

What one pass costs in accuracy is not derivable in closed form through five nonlinear layers, so it is MEASURED: one teacher-forced
mini-batch (VAE step + policy step, the oracle's ReLU signs and outlier choices forced as in tests/test_hip_ppo.py) against
oracle/ppo_ref.py run in float64 on the same inputs, over three (rollout, noise) seeds, `python tests/test_onepass_path.py`.  Its
output is profiles/h2i_onepass_accuracy.txt:

    one teacher-forced mini-batch (64 envs x 24 steps, 384 rows) against oracle/ppo_ref.py in float64; per figure: one pass | three passes
    seeds (rollout 4, noise 123)
      loss scalars and gradient norms, |got - oracle| / max(1, |oracle|):
        recons     7.41e-08 | 3.59e-08
        vel        1.89e-05 | 1.67e-09
        kld        1.70e-05 | 8.05e-08
        height     1.13e-06 | 1.49e-08
        vae_gnorm  1.51e-05 | 3.28e-08
        surrogate  4.49e-05 | 1.26e-08
        value      2.47e-05 | 2.43e-08
        entropy    2.68e-08 | 2.68e-08
        kl_mean    2.92e-05 | 1.21e-07
        gnorm      1.68e-04 | 1.06e-07
      vae step, whole gradient: relative L2 3.42e-04 | 1.56e-07; 1 - cosine 5.85e-08 | -2.84e-14
      ppo step, whole gradient: relative L2 9.02e-04 | 1.10e-06; 1 - cosine 3.93e-07 | 6.53e-13
    seeds (rollout 11, noise 321)
      loss scalars and gradient norms, |got - oracle| / max(1, |oracle|):
        recons     4.58e-06 | 4.17e-08
        vel        1.11e-05 | 2.56e-08
        kld        1.28e-05 | 2.68e-08
        height     2.26e-06 | 4.61e-08
        vae_gnorm  8.37e-07 | 1.64e-08
        surrogate  3.40e-05 | 3.31e-08
        value      2.23e-05 | 3.46e-08
        entropy    2.68e-08 | 2.68e-08
        kl_mean    4.10e-05 | 1.71e-07
        gnorm      1.34e-04 | 2.24e-07
      vae step, whole gradient: relative L2 3.49e-04 | 1.51e-07; 1 - cosine 6.08e-08 | -1.58e-14
      ppo step, whole gradient: relative L2 8.33e-04 | 1.01e-06; 1 - cosine 3.38e-07 | 5.66e-13
    seeds (rollout 7, noise 77)
      loss scalars and gradient norms, |got - oracle| / max(1, |oracle|):
        recons     5.74e-06 | 8.97e-09
        vel        3.06e-05 | 5.12e-08
        kld        1.88e-05 | 8.06e-08
        height     2.80e-06 | 2.60e-08
        vae_gnorm  1.22e-05 | 9.23e-09
        surrogate  7.88e-05 | 8.30e-09
        value      3.92e-05 | 2.30e-08
        entropy    2.68e-08 | 2.68e-08
        kl_mean    4.68e-05 | 1.19e-07
        gnorm      4.58e-04 | 2.47e-08
      vae step, whole gradient: relative L2 3.70e-04 | 1.90e-07; 1 - cosine 6.82e-08 | -2.64e-14
      ppo step, whole gradient: relative L2 1.01e-03 | 8.35e-07; 1 - cosine 4.06e-07 | 4.06e-13
    largest over the seeds (one pass | three passes):
      scalar     4.58e-04 | 2.24e-07
      l2_tensor  1.99e-03 | 1.60e-06
      cos_tensor 1.97e-06 | 9.28e-13
      l2_all     1.01e-03 | 1.10e-06
      cos_all    4.06e-07 | 6.53e-13
    (per parameter tensor: the file)

Each bound of BOUNDS is 4 x the largest one-pass figure of that table (the margin covers the seed-to-seed spread of a rounding-error
norm); the three-pass figures of the same run stand beside them and are asserted against the same bounds (they sit orders of magnitude
below)."""
import ctypes as C
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "deep-tracking-control_amd"), os.path.join(_root, "tests")]

from dtc_amd import synthetic as S

DEV = "cuda:0"
SEEDS = [(4, 123), (11, 321), (7, 77)]            # (rollout seed, noise seed)
SCALARS_VAE = ("recons", "vel", "kld", "height", "vae_gnorm")
SCALARS_PPO = ("surrogate", "value", "entropy", "kl_mean", "gnorm")
# 4 x the largest one-pass figure of profiles/h2i_onepass_accuracy.txt (module text)
BOUNDS = dict(scalar=4 * 4.58e-04, l2_tensor=4 * 1.99e-03, l2_all=4 * 1.01e-03, cos_tensor=4 * 1.97e-06, cos_all=4 * 4.06e-07)


def _pair64(rollout_seed, gemm_passes):
    """(oracle in float64 on the CPU, HIP trainer) with identical filled weights and rollout; the returns are computed in fp32 on both
    sides first (bit-identical: tests/test_hip_ppo.py), then the oracle's model and storage go to float64"""
    from dtc_amd.algorithms import PPO
    from dtc_amd.modules import ActorCriticDecoder
    from oracle import ppo_ref as OP
    torch.manual_seed(3)
    ref_ac = OP.fill_parameters_(OP.RefActorCriticDecoder(), 11)
    ref = OP.RefPPO(ref_ac, learning_rate=1e-3, entropy_coef=0.003)
    ref.init_storage(64, 24)
    torch.manual_seed(3)
    ac = ActorCriticDecoder(53, 1389, 12)
    kw = {} if gemm_passes is None else dict(gemm_passes=gemm_passes)
    alg = PPO(ac, learning_rate=1e-3, entropy_coef=0.003, device=DEV, **kw)
    alg.init_storage(64, 24, [53], [1389], [265], [12])
    ac.load_state_dict(ref_ac.state_dict())
    d = S.rollout(64, 24, seed=rollout_seed)
    for k, v in d.items():
        if k != "last_values":
            getattr(ref.storage, k).copy_(v)
            getattr(alg.storage, k).copy_(v.to(DEV))
    ref.storage.compute_returns(d["last_values"], 0.99, 0.95)
    alg.storage.compute_returns(d["last_values"].to(DEV), 0.99, 0.95)
    assert torch.equal(alg.storage.returns.cpu(), ref.storage.returns)
    ref_ac.double()
    for k in list(ref.storage.FIELDS) + ["advantages"]:
        setattr(ref.storage, k, getattr(ref.storage, k).double())
    return ref, alg


def _force_oracle_branches(ref, alg):
    """tests/test_hip_ppo.py::_force_oracle_signs for a float64 oracle: between the HIP forward and backward pass the ReLU sign records
    and the CE-net outlier classification / median element become the oracle's, so the gradients compared are those of one function"""
    from test_hip_ppo import _MASK_NAMES, _pack_sign_record

    def hook(fw, which):
        torch.cuda.synchronize()
        for ref_name, name in _MASK_NAMES.items():
            buf = fw._masks.get(name)
            if buf is None or ref_name not in ref.relu_masks or (which == "ppo" and name in ("c1", "c2", "d1", "d2")):
                continue
            buf.copy_(_pack_sign_record(ref.relu_masks[ref_name]).reshape(-1).to(buf.device))
        vae = ref.actor_critic.vae
        want = vae.last_outlier_mask.to(fw.mask.device)
        differ = fw.mask.bool() != want
        if bool(differ.any()):
            fw.mulv[:, 19:][differ] = vae.last_logvar.float().to(fw.mulv.device)[differ]
        fw.mask.copy_(want.to(torch.uint8))
        fw.info[:2] = torch.tensor([vae.last_outliers, vae.last_median_index], dtype=torch.int32, device=fw.info.device)
        torch.cuda.synchronize()

    alg.after_forward_hook = hook


def _grad_figures(grads_ref, alg, which):
    """per parameter tensor and overall: relative L2 error and 1 - cosine similarity of the HIP gradient against the oracle's"""
    arena = alg.actor_critic.arena
    rows, a_all, b_all = {}, [], []
    for name, g_ref in grads_ref.items():
        g = arena.view(alg.captured[which], name).double().cpu().reshape(-1)
        r = g_ref.double().reshape(-1)
        a_all.append(g)
        b_all.append(r)
        rows[name] = (float((g - r).norm() / r.norm()), 1.0 - float(torch.dot(g, r) / (g.norm() * r.norm())))
    g, r = torch.cat(a_all), torch.cat(b_all)
    return rows, (float((g - r).norm() / r.norm()), 1.0 - float(torch.dot(g, r) / (g.norm() * r.norm())))


def one_step(rollout_seed, noise_seed, gemm_passes):
    """One teacher-forced mini-batch (the first 384 rows of the permutation) against the float64 oracle -> dict of figures"""
    from dtc_amd.algorithms import ppo as P
    from oracle.ppo_ref import StepRecord
    from test_hip_ppo import _oracle_on_one_thread, _sync_from_oracle
    ref, alg = _pair64(rollout_seed, gemm_passes)
    perm, e1, e2 = S.update_noise(64, 24, 4, 5, seed=noise_seed)
    idx, e1, e2 = perm[:384], e1[0], e2[0]
    cols = dict(recons=P.S_RECONS, vel=P.S_VEL, kld=P.S_KLD, height=P.S_HEIGHT, vae_gnorm=P.S_VAE_GNORM, surrogate=P.S_SURR,
                value=P.S_VALUE, entropy=P.S_ENTROPY, kl_mean=P.S_KL, gnorm=P.S_GNORM)
    ref.capture_grads = alg.capture_grads = True
    _force_oracle_branches(ref, alg)
    rec, out = StepRecord(), dict(scalars={}, tensors={}, overall={})
    for which, keys, run_ref, gkey, cap in (("vae", SCALARS_VAE, lambda: ref.vae_step(idx, e1.double(), rec), "vae_grads", "vae"),
                                            ("ppo", SCALARS_PPO, lambda: ref.ppo_step(idx, e2.double(), rec), "grads", "main")):
        with torch.no_grad():                      # (the oracle's VAE step left float64 weights: both sides start from their fp32 values)
            for t in list(ref.actor_critic.parameters()):
                t.copy_(t.float().double())
        _sync_from_oracle(ref, alg)
        with _oracle_on_one_thread():
            run_ref()
        row, _ = alg.step_minibatch(idx, e1, e2, which=which)
        for key in keys:
            a, b = float(row[cols[key]]), float(getattr(rec, key))
            out["scalars"][key] = abs(a - b) / max(1.0, abs(b))
        out["tensors"][which], out["overall"][which] = _grad_figures(rec.extra[gkey], alg, cap)
    alg.after_forward_hook = None
    return out


def _worst(fig):
    """the five figures the bounds are set on, of one step's figures"""
    t = [v for which in fig["tensors"].values() for v in which.values()]
    return dict(scalar=max(fig["scalars"].values()), l2_tensor=max(a for a, _ in t), cos_tensor=max(b for _, b in t),
                l2_all=max(a for a, _ in fig["overall"].values()), cos_all=max(b for _, b in fig["overall"].values()))


def measure(seeds=SEEDS):
    print("one teacher-forced mini-batch (64 envs x 24 steps, 384 rows) against oracle/ppo_ref.py in float64; per figure: one pass | three passes")
    worst = {1: {}, 3: {}}
    for rs, ns in seeds:
        fig = {p: one_step(rs, ns, p) for p in (1, 3)}
        print(f"seeds (rollout {rs}, noise {ns})")
        print("  loss scalars and gradient norms, |got - oracle| / max(1, |oracle|):")
        for key in SCALARS_VAE + SCALARS_PPO:
            print(f"    {key:10s} {fig[1]['scalars'][key]:.2e} | {fig[3]['scalars'][key]:.2e}")
        for which in ("vae", "ppo"):
            o1, o3 = fig[1]["overall"][which], fig[3]["overall"][which]
            print(f"  {which} step, whole gradient: relative L2 {o1[0]:.2e} | {o3[0]:.2e}; 1 - cosine {o1[1]:.2e} | {o3[1]:.2e}")
            for name in fig[1]["tensors"][which]:
                t1, t3 = fig[1]["tensors"][which][name], fig[3]["tensors"][which][name]
                print(f"    {name:36s} relative L2 {t1[0]:.2e} | {t3[0]:.2e}; 1 - cosine {t1[1]:.2e} | {t3[1]:.2e}")
        for p in (1, 3):
            for k, v in _worst(fig[p]).items():
                worst[p][k] = max(worst[p].get(k, 0.0), v)
    print("largest over the seeds (one pass | three passes):")
    for k in worst[1]:
        print(f"  {k:10s} {worst[1][k]:.2e} | {worst[3][k]:.2e}")
    return worst


@pytest.mark.gpu
def test_default_is_unchanged():
    """PPO(..., gemm_passes=3) and PPO(...) give bit-identical weights, Adam state and learning rate after one update()"""
    outs = []
    for passes in (None, 3):
        _, alg = _pair64(4, passes)
        assert alg.gemm_passes == 3 and alg.arithmetic == "f32 (emulated: f16x2 split per operand, f32 accumulate)"
        perm, e1, e2 = S.update_noise(64, 24, 4, 5, seed=123)
        alg.update(perm=perm, eps1=e1.to(DEV), eps2=e2.to(DEV))
        arena = alg.actor_critic.arena
        outs.append([arena.flat.clone(), alg.optimizer.exp_avg.clone(), alg.optimizer.exp_avg_sq.clone(), alg.vae_optimizer.exp_avg.clone(),
                     alg.vae_optimizer.exp_avg_sq.clone(), alg.optimizer.lr_dev.clone(), torch.tensor([alg.learning_rate], dtype=torch.float64)])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int64),
                           b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int64))


@pytest.mark.gpu
def test_one_pass_arithmetic_string_and_keyword():
    from dtc_amd import h2i
    from dtc_amd.algorithms import PPO, RecurrentDecoderPPO
    from dtc_amd.modules import ActorCriticDecoder
    _, alg = _pair64(4, 1)
    assert alg.gemm_passes == 1 and alg.arithmetic == "f16 (block-scaled hi plane, f32 accumulate)"
    with pytest.raises(AttributeError):
        alg.arithmetic = "x"                                    # read-only
    with pytest.raises(ValueError):
        PPO(ActorCriticDecoder(53, 1389, 12), device=DEV, gemm_passes=2)
    with pytest.raises(TypeError):                               # keyword-only: the reference's positional signature is unchanged
        PPO(ActorCriticDecoder(53, 1389, 12), 5, 4, 0.2, 0.99, 0.95, 1.0, 0.01, 5e-4, 1.0, True, "adaptive", 0.01, DEV, 1)
    assert h2i.h2i_passes() == 3
    assert RecurrentDecoderPPO is not None


@pytest.mark.gpu
def test_one_pass_step_against_the_float64_oracle():
    """module text: every figure of one teacher-forced step (seeds 4 / 123) within 4 x the largest measured one-pass figure, one pass and
    three passes alike; and the one-pass gradient is NOT the three-pass one (its error sits well above three passes')"""
    from dtc_amd import h2i
    one, three = _worst(one_step(4, 123, 1)), _worst(one_step(4, 123, 3))
    assert h2i.h2i_passes() == 3
    for k, bound in BOUNDS.items():
        print(f"onepass path {k}: one pass {one[k]:.2e}, three passes {three[k]:.2e}, bound {bound:.2e}")
    for k, bound in BOUNDS.items():
        assert one[k] <= bound and three[k] <= bound, (k, one[k], three[k], bound)
    assert one["l2_all"] > 10 * three["l2_all"]


@pytest.mark.gpu
def test_rollout_side_does_not_follow_the_switch():
    """act / evaluate of a one-pass trainer and of a default one on a fixed observation: bit-identical before their first update, and
    the same bits with the library switched to one pass around the call; after the one-pass update the library is back at three"""
    from dtc_amd import h2i
    (ref, a1), (_, a3) = _pair64(4, 1), _pair64(4, 3)
    st = ref.storage
    d = lambda t: t.flatten(0, 1).float().to(DEV)
    g = torch.Generator().manual_seed(99)
    eps, noise = torch.randn(1536, 16, generator=g).to(DEV), torch.randn(1536, 12, generator=g).to(DEV)

    def rollout_side(alg):
        ac = alg.actor_critic
        actions = ac.act(d(st.observations), d(st.observation_histories), d(st.privileged_observations), None, eps=eps, noise=noise)
        values = ac.evaluate(d(st.observations), d(st.privileged_observations), d(st.base_vel))
        return [t.clone().view(torch.int32) for t in (actions, ac.action_mean, values, ac.get_actions_log_prob(actions))]

    r1, r3 = rollout_side(a1), rollout_side(a3)
    with h2i.h2i_passes_as(1):
        r1s = rollout_side(a1)
    for x, y, z in zip(r1, r3, r1s):
        assert torch.equal(x, y) and torch.equal(x, z)
    perm, e1, e2 = S.update_noise(64, 24, 4, 5, seed=123)
    w0 = a1.actor_critic.arena.flat.clone()
    a1.update(perm=perm, eps1=e1.to(DEV), eps2=e2.to(DEV))
    a3.update(perm=perm, eps1=e1.to(DEV), eps2=e2.to(DEV))
    assert h2i.h2i_passes() == 3
    w1, w3 = a1.actor_critic.arena.flat, a3.actor_critic.arena.flat
    assert bool(torch.isfinite(w1).all()) and not torch.equal(w1, w3) and not torch.equal(w1, w0)      # the update did follow it


@pytest.mark.gpu
def test_one_pass_refuses_to_leave_the_image_schedule():
    """a mini-batch of 300 rows (not a multiple of 128) and the split path switched off: update() / step_minibatch raise, nothing runs on
    other arithmetic, the library's setting is untouched"""
    from dtc_amd import _ffi, h2i, ops
    _, alg = _pair64(4, 1)
    perm, e1, e2 = S.update_noise(64, 24, 4, 5, seed=123)
    w0 = alg.actor_critic.arena.flat.clone()
    with pytest.raises(_ffi.DtcError, match="gemm_passes=1"):
        alg.step_minibatch(perm[:300], e1[0][:300], e2[0][:300])
    alg.num_mini_batches = 6                                     # 1536 / 6 = 256 rows would do; 5 -> 307 rows does not
    alg.num_mini_batches = 5
    with pytest.raises(_ffi.DtcError, match="gemm_passes=1"):
        alg.update()
    prev = ops.SPLIT, ops.H2
    try:
        ops.set_split(False)
        with pytest.raises(_ffi.DtcError, match="gemm_passes=1"):
            alg.step_minibatch(perm[:384], e1[0], e2[0])
    finally:
        ops.set_split(*prev)
    assert torch.equal(alg.actor_critic.arena.flat, w0) and h2i.h2i_passes() == 3


# ------------------------------------------------------------------------------------------------ host side: no GPU
def test_a_target_of_2_gib_is_refused_in_one_pass_mode():
    """the size check of dtc_linear_fwd_mse_h2i alone (tests/test_hip_wide_sources.py): a [400000, 1389] target (2.2 GB) with one pass set
    fails before any device work and says why; it does not run three passes.  Nothing large is allocated."""
    from dtc_amd import _ffi
    lib = _ffi.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    op = _ffi.DtcH2iOperand()
    op.nseg, op.width[0], op.img[0] = 1, 512, p.value
    call = lambda: lib.dtc_linear_fwd_mse_h2i(op, p, None, p, 1389, 400000, 696, p, 1.0, None, 0, p, p, 128, 693, None)
    assert lib.dtc_get_h2i_passes() == 3
    lib.dtc_set_h2i_passes(1)
    try:
        rc, err = call(), lib.dtc_last_error()
    finally:
        lib.dtc_set_h2i_passes(3)
    assert rc == -1 and b"one-pass" in err and b"2 GiB" in err, (rc, err)


if __name__ == "__main__":
    measure()
