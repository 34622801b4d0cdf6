"""The kernels of csrc/losses.hip against the float64 references of oracle/losses_ref.py, one operation at a time, at the shapes
where they change path: both action-count instantiations, every hidden width and activation of the fused heads, NULL biases and
index, strided rows, ragged batches, the capped strided passes of the VAE loss, the learning-rate floor and cap.

Bounds (against float64, tensors normalised by the reference's own largest magnitude): per-row gradients 2e-5 -- the figure the
whole-network gradients are held to in tests/test_hip_ppo.py; the same formulas in float32 on the CPU stay at 3e-6 -- ; the loss
scalars, the heads' mean / value and log-probabilities 2e-6 * max(1, |ref|); the bootstrap probability 2e-6; amax records, the
mirrored KL, an untouched learning rate and sampled actions exact.  Rows within rounding of a clip boundary
(losses_ref.near_boundary: float32 and float64 may pick different branches there) are left out of the per-row comparison
only; tests/test_losses_oracle.py caps their number for every case used here.  Every output is filled with NaN before the
launch, so a slot nobody wrote fails.  Each test prints its worst normalised errors (`ERR kernel output error bound`)."""
import math

import pytest
import torch

from dtc_amd import _ffi, ops
from oracle import losses_ref as LR
from test_losses_oracle import (ENTROPY_COEF, HEADS_CASES, HEADS_CLIP, LR_CASE, PPO_CASES, VALUE_COEF, flagged, heads_ref, ppo_ref,
                                row_cap)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G_TOL, S_TOL = 2e-5, 2e-6        # per-row gradients / scalars, mean, value, logp


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _report(kernel, name, err, bound):
    print(f"ERR {kernel} {name} {err:.3e} {bound:.0e}")


def _cfg(clip, clipped, adaptive=0, desired_kl=0.0, kl_mirror=None):
    c = _ffi.DtcPpoCfg()
    c.clip_param, c.value_loss_coef, c.entropy_coef, c.desired_kl = clip, VALUE_COEF, ENTROPY_COEF, desired_kl
    c.use_clipped_value_loss, c.adaptive_schedule = int(clipped), int(adaptive)
    c.kl_mirror = kl_mirror.data_ptr() if kl_mirror is not None else None
    return c


def _ws(factor=1):
    return ops.workspace(factor * int(_ffi.lib().dtc_loss_workspace(1)), DEV)


def _bits(x):
    return int(torch.tensor(float(x), dtype=torch.float32).view(torch.int32).item()) & 0xffffffff


def _record():
    return torch.zeros(int(_ffi.lib().dtc_amax_record_bytes()) // 4, dtype=torch.int32, device=DEV)


def _record_is_amax_of(rec, t, what):
    """The record holds exactly the bit pattern of the largest |value| of `t` (16 words on 16 cache lines: their maximum)."""
    got = max(int(v) & 0xffffffff for v in rec.view(-1).tolist())
    assert got == _bits(t.abs().max()), (what, hex(got), hex(_bits(t.abs().max())))


def _rows_close(kernel, name, got, ref, keep=None, tol=G_TOL):
    """max |got - ref| over the kept rows <= tol * max |ref| (over all rows); every row finite."""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{kernel} {name}: a value is not finite (an output slot nobody wrote?)"
    scale = float(ref.abs().max())
    d = (got - ref).abs()
    if keep is not None:
        d = d[keep]
    err = float(d.max()) if d.numel() else 0.0
    _report(kernel, name, err / scale if scale > 0 else err, tol)
    assert err <= tol * scale, (kernel, name, err, scale)


def _scalar_close(kernel, name, got, ref, tol=S_TOL):
    got, ref = float(got), float(ref)
    err = abs(got - ref) / max(1.0, abs(ref))
    _report(kernel, name, err, tol)
    assert err <= tol, (kernel, name, got, ref)


def _check_ppo_outputs(kernel, out, ref, clip, B):
    flag = flagged(ref, clip)
    assert int(flag.sum()) <= row_cap(B)
    keep = ~flag
    _rows_close(kernel, "dmean", out["dmean"], ref.dmean, keep)
    _rows_close(kernel, "dvalue", out["dvalue"], ref.dvalue, keep)
    # dstd: a branch flip on a flagged row adds or removes exactly that row's surrogate contribution
    got = out["dstd"].double().cpu()
    assert bool(torch.isfinite(got).all())
    scale = float(ref.dstd.abs().max())
    slack = ref.dstd_sur_rows[flag].abs().sum(0)
    err = (got - ref.dstd).abs()
    _report(kernel, "dstd", float((err - slack).clamp(min=0).max()) / scale, G_TOL)
    assert bool((err <= G_TOL * scale + slack).all()), (kernel, "dstd", err.tolist(), scale, slack.tolist())
    losses = out["losses"].cpu()
    for k, name in enumerate(("surrogate", "value_loss", "entropy", "kl")):
        _scalar_close(kernel, name, losses[k], ref.losses[k])


def _ppo_loss(inp, cfg, lr=None, ws=None):
    """dtc_ppo_loss on CPU inputs -> dict of device outputs (NaN-filled before the launch)."""
    B, A = inp["mean"].shape
    d = {k: _dev(v) for k, v in inp.items()}
    out = dict(dmean=_nan(B, A), dvalue=_nan(B), dstd=_nan(A), losses=_nan(4))
    ops.ppo_loss(d["mean"], d["std"], d["value"], d["actions"], d["old_logp"], d["old_mu"], d["old_sigma"], d["adv"], d["returns"],
                 d["old_values"], d["idx"], cfg, out["dmean"], out["dvalue"], out["dstd"], out["losses"], lr, ws if ws is not None else _ws())
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ dtc_ppo_loss
@pytest.mark.parametrize("case", PPO_CASES, ids=str)
def test_ppo_loss_against_float64(case):
    B, A, gather, clipped, clip, seed = case
    inp = LR.make_ppo_inputs(B, A, seed)
    ref = ppo_ref(inp, clip, clipped)
    out = _ppo_loss(inp if gather else LR.gathered(inp), _cfg(clip, clipped))
    _check_ppo_outputs(f"ppo_loss<{12 if A == 12 else 0}>", out, ref, clip, B)


def test_ppo_loss_on_policy_first_minibatch_step():
    """The state of every first mini-batch step: the policy IS the rollout policy (old_mu = mean, old_sigma = std, old_logp
    and actions from dtc_gaussian_act on the same rows).  Every ratio is 1 to rounding, so every row is in range, the
    surrogate is -mean(adv) and the KL is A * log(1 + 1e-5) (the 1e-5 inside ppo.py:298's logarithm)."""
    B, A, seed = LR_CASE
    inp = LR.gathered(LR.make_ppo_inputs(B, A, seed))
    mean, std = _dev(inp["mean"]), _dev(inp["std"])
    noise = torch.randn(B, A, generator=torch.Generator().manual_seed(seed)).to(DEV)
    actions, logp, mu, sigma = _nan(B, A), _nan(B), _nan(B, A), _nan(B, A)
    ops.gaussian_act(mean, std, noise, actions, logp, mu, sigma)
    inp.update(actions=actions.cpu(), old_logp=logp.cpu(), old_mu=mu.cpu(), old_sigma=sigma.cpu())
    assert torch.equal(inp["old_mu"], inp["mean"]) and torch.equal(inp["old_sigma"], inp["std"].expand(B, A))
    ref = ppo_ref(inp, 0.2, 1)
    assert float((ref.ratio - 1.0).abs().max()) <= 1e-4          # float32 log-probabilities of ~A terms against float64
    out = _ppo_loss(inp, _cfg(0.2, 1))
    _check_ppo_outputs("ppo_loss<12>", out, ref, 0.2, B)
    _scalar_close("ppo_loss<12>", "surrogate(on-policy)", out["losses"][0], -float(inp["adv"].double().mean()))
    _scalar_close("ppo_loss<12>", "kl(on-policy)", out["losses"][3], A * math.log(1.0 + 1e-5))


LR_RULE = [  # (desired_kl as a multiple of the batch's KL, lr before, lr after)
    (0.25, 1e-3, 1e-3 / 1.5), (4.0, 1e-3, 1e-3 * 1.5), (1.0, 1e-3, 1e-3),
    (0.25, 1.2e-5, 1e-5), (4.0, 9e-3, 1e-2),
]


@pytest.mark.parametrize("factor,lr0,want", LR_RULE)
def test_learning_rate_rule_on_the_device(factor, lr0, want):
    """ppo.py:301-307 with desired_kl set from the reference's own KL, a factor 2 inside each branch; the floor 1e-5 and the
    cap 1e-2.  The device divides / multiplies the float64 word once: equal to the host's result to the last bit or the one
    next to it; an untouched rate is bit-identical.  kl_mirror receives losses[3] bit for bit."""
    B, A, seed = LR_CASE
    inp = LR.make_ppo_inputs(B, A, seed)
    kl = float(ppo_ref(inp, 0.2, 1).losses[3])
    assert kl > 1e-3
    lr = torch.tensor([lr0], dtype=torch.float64, device=DEV)
    mirror = _nan(1)
    out = _ppo_loss(inp, _cfg(0.2, 1, adaptive=1, desired_kl=factor * kl, kl_mirror=mirror), lr=lr)
    got = float(lr.cpu())
    if want == lr0:
        assert got == lr0
    else:
        assert abs(got - want) <= 2.0 ** -52 * want, (got, want)
    assert torch.equal(mirror.view(torch.int32), out["losses"][3:4].view(torch.int32))
    _scalar_close("ppo_loss<12>", "kl", out["losses"][3], kl)


def test_learning_rate_untouched_without_the_adaptive_schedule():
    B, A, seed = LR_CASE
    inp = LR.make_ppo_inputs(B, A, seed)
    kl = float(ppo_ref(inp, 0.2, 1).losses[3])
    lr = torch.tensor([1.2345678912345e-3], dtype=torch.float64, device=DEV)
    before = lr.view(torch.int64).clone()
    mirror = _nan(1)
    out = _ppo_loss(inp, _cfg(0.2, 1, adaptive=0, desired_kl=0.25 * kl, kl_mirror=mirror), lr=lr)
    assert torch.equal(lr.view(torch.int64), before)
    assert torch.equal(mirror.view(torch.int32), out["losses"][3:4].view(torch.int32))


# ------------------------------------------------------------------------------------------------ dtc_ppo_heads_loss
def _heads_call(d, H, B, A, act, cfg, out, ld, recs, ws):
    """The C entry point itself (ops.ppo_heads_loss insists on contiguous rows).  ld = (ldha, ldhc, lddha, lddhc)."""
    p = lambda t: None if t is None else t.data_ptr()
    return _ffi.lib().dtc_ppo_heads_loss(
        p(d["Ha"]), ld[0], p(d["Hc"]), ld[1], H, p(d["Wa"]), p(d["ba"]), p(d["Wc"]), p(d["bc"]), _ffi.ACT[act], p(d["std"]),
        p(d["actions"]), p(d["old_logp"]), p(d["old_mu"]), p(d["old_sigma"]), p(d["adv"]), p(d["returns"]), p(d["old_values"]),
        p(d["idx"]), cfg, p(out["mean"]), p(out["value"]), p(out["dmean"]), p(out["dvalue"]), p(out["dHa"]), ld[2], p(out["dHc"]), ld[3],
        p(out["dstd"]), p(out["losses"]), None, p(ws), B, A, p(recs[0]), p(recs[1]), p(recs[2]), p(recs[3]), _ffi.stream())


def _heads_outputs(B, H, A, ldd=None):
    ldd = H if ldd is None else ldd
    return dict(mean=_nan(B, A), value=_nan(B), dmean=_nan(B, A), dvalue=_nan(B), dHa=_nan(B, ldd), dHc=_nan(B, ldd), dstd=_nan(A),
                losses=_nan(4))


@pytest.mark.parametrize("case", HEADS_CASES, ids=str)
def test_ppo_heads_loss_against_float64(case):
    """mean / value, the loss, and the two hidden-layer gradients of the fused kernel; the four amax records hold exactly the
    largest magnitude of the tensor the launch wrote.  Strided case: Ha / Hc are column blocks of [B, 3H] tensors, dHa / dHc go
    into column blocks of NaN-filled [B, 3H] tensors whose other columns must stay NaN."""
    B, H, A, act, bias, gather, strided, clipped, seed = case
    inp = LR.make_heads_inputs(B, H, A, act, bias, seed)
    ref = heads_ref(inp, act, HEADS_CLIP, clipped)
    d = {k: _dev(v) for k, v in (inp if gather else LR.gathered(inp)).items()}
    wide = 3 * H if strided else H
    if strided:
        g = torch.Generator().manual_seed(seed)
        wa, wc = torch.randn(B, wide, generator=g).to(DEV), torch.randn(B, wide, generator=g).to(DEV)
        wa[:, H:2 * H], wc[:, 2 * H:] = d["Ha"], d["Hc"]
        d["Ha"], d["Hc"] = wa[:, H:2 * H], wc[:, 2 * H:]
    out = _heads_outputs(B, H, A, wide)
    full = dict(dHa=out["dHa"], dHc=out["dHc"])
    if strided:
        out["dHa"], out["dHc"] = full["dHa"][:, :H], full["dHc"][:, H:2 * H]
    recs = [_record() for _ in range(4)]
    ws = _ws()
    rc = _heads_call(d, H, B, A, act, _cfg(HEADS_CLIP, clipped), out, (wide, wide, wide, wide), recs, ws)
    _ffi.check(rc, "dtc_ppo_heads_loss")
    torch.cuda.synchronize()
    kernel = f"ppo_heads_loss<{H},{12 if (H == 128 and A == 12) else 0}>"
    _check_ppo_outputs(kernel, out, ref, HEADS_CLIP, B)
    keep = ~flagged(ref, HEADS_CLIP)
    _rows_close(kernel, "dHa", out["dHa"], ref.dHa, keep)
    _rows_close(kernel, "dHc", out["dHc"], ref.dHc, keep)
    for name, r in (("mean", ref.mean), ("value", ref.value)):
        got = out[name].double().cpu().reshape(r.shape)
        err = float(((got - r).abs() / r.abs().clamp(min=1.0)).max())
        _report(kernel, name, err, S_TOL)
        assert err <= S_TOL, (name, err)
    if strided:
        assert bool(torch.isnan(full["dHa"][:, H:]).all()) and bool(torch.isnan(full["dHc"][:, :H]).all())
        assert bool(torch.isnan(full["dHc"][:, 2 * H:]).all())
    for rec, name in zip(recs, ("dHa", "dHc", "dmean", "dvalue")):
        _record_is_amax_of(rec, out[name], name)


# ------------------------------------------------------------------------------------------------ VAE losses
def _vae_inputs(B, seed, height):
    R = B + 37
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(R, generator=g)[:B].contiguous()
    next_obs, base_vel = torch.randn(R, 53, generator=g), torch.randn(R, 3, generator=g)
    recons = next_obs[idx] + 0.3 * torch.randn(B, 53, generator=g)
    zero_row = B // 2 if B > 1 else None
    if zero_row is not None:
        recons[zero_row] = next_obs[idx[zero_row]]                  # this row reproduces its target: its gradient row is exactly zero
    mulv = torch.cat([base_vel[idx] + 0.2 * torch.randn(B, 3, generator=g), torch.randn(B, 16, generator=g),
                      -3.0 + 5.0 * torch.rand(B, 16, generator=g)], 1).contiguous()      # log-variances in [-3, 2]
    d = dict(recons=recons, mulv=mulv, next_obs=next_obs, base_vel=base_vel, idx=idx, hrecon=None, priv=None)
    if height:
        d["priv"] = torch.randn(R, 1389, generator=g)
        d["hrecon"] = d["priv"][idx][:, 696:] + 0.3 * torch.randn(B, 693, generator=g)
    return d, zero_row


def _check_vae(kernel, out, ref, zero_row, rec):
    _rows_close(kernel, "d_recons", out["d_recons"], ref.d_recons)
    # the three column blocks of dmulv are three gradients of their own (velocity error, mu and log-variance of the KLD), the first
    # ~30 times smaller than the others: each is held to the bound on its own scale
    for name, c0, c1 in (("dmulv[vel]", 0, 3), ("dmulv[mu]", 3, 19), ("dmulv[lv]", 19, 35)):
        _rows_close(kernel, name, out["dmulv"][:, c0:c1], ref.dmulv[:, c0:c1])
    if ref.d_hrecon is not None:
        _rows_close(kernel, "d_hrecon", out["d_hrecon"], ref.d_hrecon)
    assert zero_row is None or bool((out["d_recons"][zero_row] == 0).all())
    _record_is_amax_of(rec, out["d_recons"], "d_recons")


@pytest.mark.parametrize("B", [1, 3, 4, 5, 13, 64, 65, 257, 1031, 24576 + 13])
def test_vae_loss_against_float64(B):
    """B = 24589: past the 2048-block cap of the height pass (and the 512-block cap of the recons pass stays inactive)."""
    inp, zero_row = _vae_inputs(B, 100 + B, height=True)
    ref = LR.vae_loss_ref(inp["recons"], inp["hrecon"], inp["mulv"], inp["next_obs"], inp["priv"], inp["base_vel"], inp["idx"])
    d = {k: _dev(v) for k, v in inp.items()}
    out = dict(d_recons=_nan(B, 53), d_hrecon=_nan(B, 693), dmulv=_nan(B, 35), losses=_nan(4))
    rec, ws = _record(), _ws()
    p = lambda t: t.data_ptr()
    _ffi.check(_ffi.lib().dtc_vae_loss(p(d["recons"]), p(d["hrecon"]), p(d["mulv"]), p(d["next_obs"]), p(d["priv"]), p(d["base_vel"]),
                                       p(d["idx"]), p(out["d_recons"]), p(out["d_hrecon"]), p(out["dmulv"]), p(out["losses"]), p(ws), B,
                                       p(rec), _ffi.stream()), "dtc_vae_loss")
    torch.cuda.synchronize()
    _check_vae("vae_loss", out, ref, zero_row, rec)
    for k, name in enumerate(("recons", "vel", "kld", "height")):
        _scalar_close("vae_loss", name, out["losses"][k], ref.losses[k])


@pytest.mark.parametrize("parts", [0, 37])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 13, 64, 65, 257, 1031, 32768 + 77])
def test_vae_loss_fused_against_float64(B, parts):
    """The form without the height pass (B = 32845: past the 512-block cap of the recons pass); the height loss is the sum of
    the float64 partials the terrain-decoder layer would have left, / (693 B) -- zero without partials."""
    inp, zero_row = _vae_inputs(B, 200 + B, height=False)
    ref = LR.vae_loss_ref(inp["recons"], None, inp["mulv"], inp["next_obs"], None, inp["base_vel"], inp["idx"])
    d = {k: _dev(v) for k, v in inp.items()}
    hpart = torch.rand(parts, generator=torch.Generator().manual_seed(B), dtype=torch.float64) * 693.0 * B / max(parts, 1) if parts else None
    out = dict(d_recons=_nan(B, 53), dmulv=_nan(B, 35), losses=_nan(4))
    rec, ws, hp = _record(), _ws(), _dev(hpart)
    p = lambda t: None if t is None else t.data_ptr()
    _ffi.check(_ffi.lib().dtc_vae_loss_fused(p(d["recons"]), p(d["mulv"]), p(d["next_obs"]), p(d["base_vel"]), p(d["idx"]),
                                             p(out["d_recons"]), p(out["dmulv"]), p(hp), parts,
                                             p(out["losses"]), p(ws), B, p(rec), _ffi.stream()), "dtc_vae_loss_fused")
    torch.cuda.synchronize()
    _check_vae("vae_loss_fused", out, ref, zero_row, rec)
    for k, name in enumerate(("recons", "vel", "kld")):
        _scalar_close("vae_loss_fused", name, out["losses"][k], ref.losses[k])
    _scalar_close("vae_loss_fused", "height", out["losses"][3], float(hpart.sum()) / (693.0 * B) if parts else 0.0)


# ------------------------------------------------------------------------------------------------ dtc_gaussian_act
@pytest.mark.parametrize("B,A,extra", [(1, 1, True), (255, 12, False), (256, 40, True), (257, 12, True), (4099, 1, False),
                                       (4099, 40, True), (1, 40, False)])
def test_gaussian_act_against_float64(B, A, extra):
    """actions: the compiler contracts noise * std + mean into ONE fused multiply-add (v_fma_f32 in the kernel's code), so they
    are bit-equal to the singly rounded value.  The float32 tensor expression rounds the product first, which moves the exact
    sum by at most half an ulp of the product before the final rounding: the two results differ by at most one ulp of the result
    plus half an ulp of the product (more than 1 ulp of the result only where product and mean cancel).  logp: the float64 log-probability of the actions the kernel emitted.  No 32-action limit here
    (A = 40)."""
    g = torch.Generator().manual_seed(300 + B + A)
    mean, noise = 0.5 * torch.randn(B, A, generator=g), torch.randn(B, A, generator=g)
    std = 0.3 + 0.7 * torch.rand(A, generator=g)
    actions, logp = _nan(B, A), _nan(B)
    mu, sigma = (_nan(B, A), _nan(B, A)) if extra else (None, None)
    ops.gaussian_act(_dev(mean), _dev(std), _dev(noise), actions, logp, mu, sigma)
    torch.cuda.synchronize()
    a = actions.cpu()
    assert torch.equal(a, LR.gaussian_act_fused(mean, std, noise))
    two_roundings, _ = LR.gaussian_act_ref(mean, std, noise)
    ulp = lambda t: t.abs().double().log2().floor().exp2() * 2.0 ** -23
    room = 0.5 * ulp(noise.double() * std.double()) + ulp(torch.maximum(a.abs(), two_roundings.abs()))
    assert bool(((a.double() - two_roundings.double()).abs() <= room).all())
    _, want = LR.gaussian_act_ref(mean, std, noise, actions=a)
    err = float(((logp.double().cpu() - want).abs() / want.abs().clamp(min=1.0)).max())
    _report("gaussian_act", "logp", err, S_TOL)
    assert err <= S_TOL
    if extra:
        assert torch.equal(mu.cpu(), mean) and torch.equal(sigma.cpu(), std.expand(B, A))


# ------------------------------------------------------------------------------------------------ dtc_bootstrap_probability
@pytest.mark.parametrize("regime", ["wide", "near_equal", "negative_mean"])
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 4096, 32768 + 5])
def test_bootstrap_probability_against_float64(n, regime):
    """1 - tanh(std / mean) on rewards spread as wide as their mean, on near-equal rewards (mean 1, spread 1e-4: the case the
    two-pass float64 sums exist for) and on a negative mean; n = 1 gives NaN (torch.std of one value)."""
    g = torch.Generator().manual_seed(400 + n)
    z = torch.randn(n, generator=g, dtype=torch.float64)
    r = {"wide": 1.0 + z, "near_equal": 1.0 + 1e-4 * z, "negative_mean": -2.0 + 0.5 * z}[regime].float()
    out, rd = torch.full((1,), 123.0, device=DEV), _dev(r)
    _ffi.check(_ffi.lib().dtc_bootstrap_probability(rd.data_ptr(), n, out.data_ptr(), _ffi.stream()), "dtc_bootstrap_probability")
    got, want = float(out.cpu()), LR.bootstrap_probability_ref(r)
    if n == 1:
        assert math.isnan(got) and math.isnan(want)
        return
    _report("bootstrap_probability", regime, abs(got - want), S_TOL)
    assert abs(got - want) <= 2e-6, (got, want)


# ------------------------------------------------------------------------------------------------ refusals
def _refused(rc, outputs):
    """An error code came back and nothing was launched: every output still holds its NaN fill."""
    torch.cuda.synchronize()
    assert rc != 0
    for t in outputs:
        assert bool(torch.isnan(t).all())


@pytest.mark.parametrize("B,A", [(4, 33), (4096 * 256 + 1, 1)])
def test_ppo_loss_refuses_too_many_actions_and_too_large_a_batch(B, A):
    """(Every tensor has its full size, so a launch that did happen would stay inside its buffers.)"""
    row, mat, one = (lambda: torch.zeros(B, device=DEV)), (lambda: torch.zeros(B, A, device=DEV)), (lambda *s: torch.ones(*s, device=DEV))
    ins = [mat(), one(A), row(), mat(), row(), mat(), one(B, A), row(), row(), row()]
    out, ws = [_nan(B, A), _nan(B), _nan(A), _nan(4)], _ws(2)
    rc = _ffi.lib().dtc_ppo_loss(*(t.data_ptr() for t in ins), None, _cfg(0.2, 1), *(t.data_ptr() for t in out), None, ws.data_ptr(), B, A,
                                 _ffi.stream())
    _refused(rc, out)


@pytest.mark.parametrize("B,H,pad", [(8, 96, 0), (4096 * 64 + 1, 64, 0), (8, 128, 2)], ids=["H=96", "B=4096*64+1", "stride%4"])
def test_ppo_heads_loss_refuses_bad_shapes(B, H, pad):
    """A hidden width outside {64, 128, 256}, a batch past the loss workspace, a row stride that is no multiple of 4.  (Every
    tensor has its full size, so a launch that did happen would stay inside its buffers.)"""
    A = 1
    z = lambda *s: torch.zeros(*s, device=DEV)
    d = dict(Ha=z(B, H + pad), Hc=z(B, H + pad), Wa=z(A, H), Wc=z(1, H), ba=None, bc=None, std=torch.ones(A, device=DEV), actions=z(B, A),
             old_logp=z(B), old_mu=z(B, A), old_sigma=torch.ones(B, A, device=DEV), adv=z(B), returns=z(B), old_values=z(B), idx=None)
    out = _heads_outputs(B, H, A)
    ws = _ws(2)
    rc = _heads_call(d, H, B, A, "elu", _cfg(0.2, 1), out, (H + pad, H + pad, H, H), [None] * 4, ws)
    _refused(rc, out.values())


def test_vae_loss_refuses_an_empty_batch():
    ins = [torch.zeros(1, w, device=DEV) for w in (53, 693, 35, 53, 1389, 3)] + [torch.zeros(1, dtype=torch.int64, device=DEV)]
    out, ws = [_nan(1, 53), _nan(1, 693), _nan(1, 35), _nan(4)], _ws()
    rc = _ffi.lib().dtc_vae_loss(*(t.data_ptr() for t in ins), *(t.data_ptr() for t in out), ws.data_ptr(), 0, None, _ffi.stream())
    _refused(rc, out)
