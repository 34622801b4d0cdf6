"""The float64 references of the loss kernels (oracle/losses_ref.py) checked on the CPU, and the conditions the GPU
comparison (tests/test_hip_losses.py) puts on its own inputs: few rows near a branch boundary, many rows in every branch.
The case tables of the GPU tests live here so that both modules see the same (B, A, seed)."""
import math

import pytest
import torch

from oracle import losses_ref as LR

VALUE_COEF, ENTROPY_COEF = 1.0, 0.003

# dtc_ppo_loss: (B, A, gather through idx, use_clipped_value_loss, clip, seed).  A = 12: the unrolled kernel, every other A
# the run-time-A kernel; B in {63, 65, 257} with both.
PPO_CASES = [
    (1, 12, True, 1, 0.2, 1), (1, 5, False, 0, 0.2, 2), (63, 12, True, 1, 0.2, 3), (63, 5, False, 1, 0.2, 4),
    (64, 13, True, 0, 0.2, 5), (65, 12, False, 1, 0.05, 6), (65, 32, True, 1, 0.2, 7), (255, 1, True, 1, 0.2, 8),
    (256, 12, True, 0, 0.2, 9), (257, 12, True, 1, 0.2, 10), (257, 13, False, 1, 0.05, 11), (1031, 5, True, 1, 0.2, 12),
    (1031, 12, False, 0, 0.05, 13), (4099, 12, True, 1, 0.2, 14), (4099, 32, True, 1, 0.2, 15), (4099, 1, False, 1, 0.05, 16),
]
# dtc_ppo_heads_loss: (B, H, A, act_prev, biases given, gather through idx, strided Ha / Hc / dHa / dHc, clipped, seed)
HEADS_CASES = [
    (1, 128, 12, "elu", True, True, False, 1, 21), (63, 128, 12, "elu", True, False, False, 1, 22),
    (64, 64, 5, "relu", True, True, False, 1, 23), (65, 256, 12, "tanh", False, True, False, 1, 24),
    (257, 128, 5, None, True, True, False, 1, 25), (257, 64, 12, "elu", False, False, False, 1, 26),
    (1031, 128, 12, "relu", True, True, False, 1, 27), (1031, 256, 32, "elu", True, True, False, 1, 28),
    (65, 128, 1, "tanh", True, False, False, 1, 29), (63, 64, 32, None, False, True, False, 1, 30),
    (257, 128, 12, "elu", True, True, True, 1, 31), (64, 256, 1, "relu", True, True, False, 0, 32),
]
HEADS_CLIP = 0.2
LR_CASE = (257, 12, 41)              # the learning-rate rule and the on-policy case: (B, A, seed)


def ppo_ref(inp, clip, clipped, dtype=torch.float64):
    return LR.ppo_loss_ref(inp["mean"], inp["std"], inp["value"], inp["actions"], inp["old_logp"], inp["old_mu"], inp["old_sigma"],
                           inp["adv"], inp["returns"], inp["old_values"], inp["idx"], clip, VALUE_COEF, ENTROPY_COEF, clipped, dtype)


def heads_ref(inp, act, clip, clipped, dtype=torch.float64):
    return LR.heads_ref(inp["Ha"], inp["Hc"], inp["Wa"], inp["ba"], inp["Wc"], inp["bc"], act, inp["std"], inp["actions"],
                        inp["old_logp"], inp["old_mu"], inp["old_sigma"], inp["adv"], inp["returns"], inp["old_values"], inp["idx"],
                        clip, VALUE_COEF, ENTROPY_COEF, clipped, dtype)


def flagged(ref, clip):
    return LR.near_boundary(ref.ratio, ref.dlt, ref.l1, ref.l2, clip)


def row_cap(B):
    return max(2, math.ceil(B / 500))


def test_log_prob_and_entropy_equal_torch_distributions():
    g = torch.Generator().manual_seed(0)
    x, mu = torch.randn(301, 13, generator=g, dtype=torch.float64), torch.randn(301, 13, generator=g, dtype=torch.float64)
    sigma = 0.05 + 2.0 * torch.rand(13, generator=g, dtype=torch.float64)
    d = torch.distributions.Normal(mu, sigma.expand_as(mu))
    torch.testing.assert_close(LR.normal_log_prob(x, mu, sigma), d.log_prob(x).sum(-1), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(LR.normal_entropy(sigma), d.entropy()[0].sum(-1), rtol=1e-13, atol=1e-13)
    # ... and through the public reference: the entropy scalar, and old_logp of the recipe (ratio = 1 on the old policy)
    inp = LR.make_ppo_inputs(65, 5, 3)
    r = ppo_ref(inp, 0.2, 1)
    assert abs(float(r.losses[2]) - float(torch.distributions.Normal(0.0, inp["std"].double()).entropy().sum())) <= 1e-12
    lp = torch.distributions.Normal(inp["old_mu"].double(), inp["old_sigma"].double()).log_prob(inp["actions"].double()).sum(-1)
    assert float((lp.float() - inp["old_logp"]).abs().max()) == 0.0


@pytest.mark.parametrize("case", PPO_CASES, ids=str)
def test_ppo_cases_have_few_rows_near_a_branch_boundary(case):
    B, A, gather, clipped, clip, seed = case
    inp = LR.make_ppo_inputs(B, A, seed)
    n = int(flagged(ppo_ref(inp, clip, clipped), clip).sum())
    print(f"near-boundary rows: {n} of {B} (cap {row_cap(B)})")
    assert n <= row_cap(B)
    r0, r1 = ppo_ref(inp, clip, clipped), ppo_ref(LR.gathered(inp), clip, clipped)         # idx = None reads the same rows
    assert torch.equal(r0.dmean, r1.dmean) and torch.equal(r0.losses, r1.losses)


@pytest.mark.parametrize("case", HEADS_CASES + [LR_CASE], ids=str)
def test_heads_cases_have_few_rows_near_a_branch_boundary(case):
    if len(case) == 3:
        B, A, seed = case
        n = int(flagged(ppo_ref(LR.make_ppo_inputs(B, A, seed), 0.2, 1), 0.2).sum())
    else:
        B, H, A, act, bias, gather, strided, clipped, seed = case
        n = int(flagged(heads_ref(LR.make_heads_inputs(B, H, A, act, bias, seed), act, HEADS_CLIP, clipped), HEADS_CLIP).sum())
    print(f"near-boundary rows: {n} of {B} (cap {row_cap(B)})")
    assert n <= row_cap(B)


def branch_shares(ref, adv, clip):
    """Share of the rows in each branch of the two clips (clip = 0.2, the value clip on)."""
    clip = LR._f32(clip)
    lo, hi = ref.ratio < 1.0 - clip, ref.ratio > 1.0 + clip
    mid = ~lo & ~hi
    fail = ref.dlt.abs() > clip
    s = {}
    for name, m in (("low", lo), ("in", mid), ("high", hi)):
        s[name + "/adv>0"], s[name + "/adv<0"] = m & (adv > 0), m & (adv < 0)
    s["vclip pass"], s["vclip fail"] = ~fail, fail
    s["l1>l2"], s["l1<l2"] = fail & (ref.l1 > ref.l2), fail & (ref.l1 < ref.l2)
    return {k: float(v.double().mean()) for k, v in s.items()}


# the (B, A) the recipe was drawn up on, and every clip = 0.2 case of the GPU tests with B >= 257 and A >= 5 (the recipe is built
# for clip = 0.2: at 0.05 the in-range band holds fewer rows by construction)
SHARE_CASES = [(257, 12, 0), (1031, 5, 0), (4099, 12, 0), (4099, 32, 0), (24589, 12, 0)] + \
              [(B, A, seed) for B, A, _, clipped, clip, seed in PPO_CASES if B >= 257 and A >= 5 and clip == 0.2 and clipped] + [LR_CASE]


@pytest.mark.parametrize("B,A,seed", SHARE_CASES)
def test_every_branch_holds_a_twentieth_of_the_rows(B, A, seed):
    inp = LR.make_ppo_inputs(B, A, seed)
    ref = ppo_ref(inp, 0.2, 1)
    shares = branch_shares(ref, inp["adv"][inp["idx"]].double(), 0.2)
    print({k: round(v, 3) for k, v in shares.items()})
    for k, v in shares.items():
        assert v >= 0.05, (k, v)


@pytest.mark.parametrize("case", [c for c in HEADS_CASES if c[0] >= 257 and c[2] >= 5 and c[7]], ids=str)
def test_every_branch_holds_a_twentieth_of_the_rows_heads(case):
    B, H, A, act, bias, gather, strided, clipped, seed = case
    inp = LR.make_heads_inputs(B, H, A, act, bias, seed)
    shares = branch_shares(heads_ref(inp, act, HEADS_CLIP, 1), inp["adv"][inp["idx"]].double(), HEADS_CLIP)
    print({k: round(v, 3) for k, v in shares.items()})
    for k, v in shares.items():
        assert v >= 0.05, (k, v)


def test_float32_evaluation_of_the_reference_stays_inside_the_bounds():
    """The bounds of the GPU comparison leave room: the same formulas in float32 on the CPU against float64."""
    for B, A, seed in ((257, 12, 0), (4099, 32, 0)):
        inp = LR.make_ppo_inputs(B, A, seed)
        r64, r32 = ppo_ref(inp, 0.2, 1), ppo_ref(inp, 0.2, 1, torch.float32)
        keep = ~flagged(r64, 0.2)
        for name in ("dmean", "dvalue"):
            a, b = getattr(r32, name).double()[keep], getattr(r64, name)[keep]
            assert float((a - b).abs().max()) <= 2e-5 * float(getattr(r64, name).abs().max()), name
        assert float((r32.losses.double() - r64.losses).abs().max()) <= 2e-6


def test_heads_reference_gradients_through_the_saved_output():
    """dHa of heads_ref (autograd through act(act^-1(H))) equals (dmean Wa) * act'(H) written out, per activation."""
    for act, dact in (("relu", lambda y: (y > 0).double()), ("elu", lambda y: torch.where(y > 0, torch.ones_like(y), y + 1.0)),
                      ("tanh", lambda y: 1.0 - y * y), (None, lambda y: torch.ones_like(y))):
        inp = LR.make_heads_inputs(65, 64, 5, act, True, 3)
        r = heads_ref(inp, act, 0.2, 1)
        want_a = (r.dmean @ inp["Wa"].double()) * dact(inp["Ha"].double())
        want_c = (r.dvalue[:, None] @ inp["Wc"].double()) * dact(inp["Hc"].double())
        assert float((r.dHa - want_a).abs().max()) <= 1e-12 * float(want_a.abs().max()), act
        assert float((r.dHc - want_c).abs().max()) <= 1e-12 * float(want_c.abs().max()), act


def test_vae_reference_on_a_hand_computed_batch():
    B = 3
    g = torch.Generator().manual_seed(5)
    recons, hrecon, mulv = torch.randn(B, 53, generator=g), torch.randn(B, 693, generator=g), torch.randn(B, 35, generator=g)
    next_obs, priv, vel = torch.randn(B + 2, 53, generator=g), torch.randn(B + 2, 1389, generator=g), torch.randn(B + 2, 3, generator=g)
    idx = torch.tensor([4, 0, 2])
    r = LR.vae_loss_ref(recons, hrecon, mulv, next_obs, priv, vel, idx)
    d = recons.double() - next_obs.double()[idx]
    assert abs(float(r.losses[0]) - float((d * d).sum() / (53 * B))) <= 1e-13
    torch.testing.assert_close(r.d_recons, 2.0 * d / (53 * B), rtol=1e-12, atol=0)
    mu, lv = mulv.double()[:, 3:19], mulv.double()[:, 19:]
    torch.testing.assert_close(r.dmulv[:, 3:19], 4.0 * mu / B, rtol=1e-12, atol=0)
    torch.testing.assert_close(r.dmulv[:, 19:], -2.0 * (1.0 - lv.exp()) / B, rtol=1e-12, atol=1e-15)
    dh = hrecon.double() - priv.double()[idx][:, 696:]
    assert abs(float(r.losses[3]) - float((dh * dh).mean())) <= 1e-13
    assert float(LR.vae_loss_ref(recons, None, mulv, next_obs, priv, vel, idx).losses[3]) == 0.0


def test_bootstrap_reference():
    r = torch.tensor([1.0, 2.0, 4.0])
    assert abs(LR.bootstrap_probability_ref(r) - (1.0 - math.tanh(float(r.std()) / float(r.mean())))) <= 1e-7
    assert math.isnan(LR.bootstrap_probability_ref(torch.ones(1)))
