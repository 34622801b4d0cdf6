"""Plain-torch CPU references of the loss, action and bootstrap kernels of csrc/losses.hip (TEST INFRASTRUCTURE ONLY).

Every function restates ONE operation from its formula (rsl_rl/rsl_rl/algorithms/ppo.py:205-247 and :288-327,
actor_critic_decoder.py:404-407, the header comments of csrc/losses.hip and include/dtc_hip.h) on float32 inputs that are
converted to `dtype` (float64 by default) first.  Gradients come from torch.autograd on that graph -- none of them is
written out by hand, so a slip in the kernels' hand-written backward cannot repeat itself here.  The scalar parameters
the kernels receive as floats (clip, the two loss coefficients) are rounded to float32 before use: that is the value
the device sees.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

OBS, HGT, PRIV, LAT = 53, 693, 1389, 16
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def _rows(t, idx, dtype):
    t = t.detach()
    return (t if idx is None else t[idx]).to(dtype)


def normal_log_prob(x, mu, sigma):
    """sum_j log N(x_j; mu_j, sigma_j)"""
    return (-((x - mu) ** 2) / (2.0 * sigma ** 2) - torch.log(sigma) - HALF_LOG_2PI).sum(-1)


def normal_entropy(sigma):
    """sum_j (1/2 + 1/2 ln(2 pi) + ln sigma_j)"""
    return (0.5 + HALF_LOG_2PI + torch.log(sigma)).sum(-1)


def ppo_loss_ref(mean, std, value, actions, old_logp, old_mu, old_sigma, adv, returns, old_values, idx, clip, value_coef,
                 entropy_coef, clipped, dtype=torch.float64):
    """ppo.py:288-327 on one mini-batch.  mean [B, A], std [A], value [B]; the rollout tensors have R >= B rows and are read
    through `idx` (None: row b itself).  Returns a namespace:
      losses        the four scalars in the kernel's order: surrogate, value, entropy, KL
      dmean, dvalue, dstd   gradients of  surrogate + value_coef * value - entropy_coef * entropy
      ratio, dlt    per row: the probability ratio and value - old_value
      l1, l2        per row: the unclipped and the clipped squared value error (None without the value clip)
      dstd_sur_rows [B, A]: what row b's surrogate term contributes to dstd[j]"""
    clip, value_coef, entropy_coef = _f32(clip), _f32(value_coef), _f32(entropy_coef)
    mean = mean.detach().to(dtype).requires_grad_(True)
    std = std.detach().to(dtype).reshape(-1).requires_grad_(True)
    value = value.detach().to(dtype).reshape(-1).requires_grad_(True)
    B, A = mean.shape
    a, mo, so = (_rows(t.reshape(-1, A), idx, dtype) for t in (actions, old_mu, old_sigma))
    lp0, ad, ret, v0 = (_rows(t.reshape(-1), idx, dtype) for t in (old_logp, adv, returns, old_values))
    std_rows = std.unsqueeze(0).expand(B, A)          # a node of its own: its gradient is the per-row share of dstd
    logp = normal_log_prob(a, mean, std_rows)
    entropy = normal_entropy(std)
    with torch.no_grad():
        kl = (torch.log(std / so + 1.0e-5) + (so ** 2 + (mo - mean) ** 2) / (2.0 * std ** 2) - 0.5).sum(-1).mean()
    ratio = torch.exp(logp - lp0)
    s1 = -ad * ratio
    s2 = -ad * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    surrogate = torch.max(s1, s2).mean()
    dlt = value - v0
    if clipped:
        vc = v0 + dlt.clamp(-clip, clip)
        l1, l2 = (value - ret) ** 2, (vc - ret) ** 2
        value_loss = torch.max(l1, l2).mean()
    else:
        l1 = l2 = None
        value_loss = ((ret - value) ** 2).mean()
    loss = surrogate + value_coef * value_loss - entropy_coef * entropy
    dstd_sur_rows, = torch.autograd.grad(surrogate, std_rows, retain_graph=True)
    dmean, dvalue, dstd = torch.autograd.grad(loss, (mean, value, std))
    det = lambda t: None if t is None else t.detach()
    return SimpleNamespace(losses=torch.stack([surrogate, value_loss, entropy, kl]).detach(), dmean=dmean, dvalue=dvalue, dstd=dstd,
                           ratio=ratio.detach(), dlt=dlt.detach(), l1=det(l1), l2=det(l2), dstd_sur_rows=dstd_sur_rows)


def _act_inverse(y, act):
    """The pre-activation z with act(z) = y (where several exist -- relu at 0 -- the one whose derivative is the
    kernel's: 0)."""
    if act in (None, "none", "relu"):
        return y.clone()
    if act == "elu":
        return torch.where(y > 0, y, torch.log1p(y.clamp(max=0.0)))
    if act == "tanh":
        return torch.atanh(y)
    raise ValueError(act)


def _act(z, act):
    if act in (None, "none"):
        return z
    return {"relu": torch.relu, "elu": torch.nn.functional.elu, "tanh": torch.tanh}[act](z)


def heads_ref(Ha, Hc, Wa, ba, Wc, bc, act_prev, std, actions, old_logp, old_mu, old_sigma, adv, returns, old_values, idx, clip,
              value_coef, entropy_coef, clipped, dtype=torch.float64):
    """dtc_ppo_heads_loss: mean = Ha Wa^T + ba, value = Hc Wc^T + bc, then ppo_loss_ref.  Ha / Hc are POST-activation values
    of `act_prev`; dHa / dHc are the gradients with respect to the PRE-activations, found by autograd through act(z) with
    z = act^-1(H) -- the same quantity the kernel forms from the saved output as (d_out W) * act'(H)."""
    za = _act_inverse(Ha.detach().to(dtype), act_prev).requires_grad_(True)
    zc = _act_inverse(Hc.detach().to(dtype), act_prev).requires_grad_(True)
    ya, yc = _act(za, act_prev), _act(zc, act_prev)
    Wa64, Wc64 = Wa.detach().to(dtype), Wc.detach().to(dtype).reshape(1, -1)
    mean = ya @ Wa64.t() + (ba.detach().to(dtype) if ba is not None else 0.0)
    value = (yc @ Wc64.t()).reshape(-1) + (bc.detach().to(dtype).reshape(()) if bc is not None else 0.0)
    r = ppo_loss_ref(mean, std, value, actions, old_logp, old_mu, old_sigma, adv, returns, old_values, idx, clip, value_coef,
                     entropy_coef, clipped, dtype)
    r.dHa, r.dHc = torch.autograd.grad((mean, value), (za, zc), (r.dmean, r.dvalue))
    r.mean, r.value = mean.detach(), value.detach()
    return r


def vae_loss_ref(recons, hrecon, mulv, next_obs, priv, base_vel, idx, dtype=torch.float64):
    """ppo.py:205-247.  recons [B, 53], hrecon [B, 693] or None (the fused form: no height term), mulv [B, 35] =
    [velocity 3 | mu 16 | log-variance 16]; next_obs / priv / base_vel are read through idx.  Returns the four losses in
    the kernel's order (recons, vel, kld, height) and the gradients of  recons + vel + 4 kld + height."""
    recons = recons.detach().to(dtype).requires_grad_(True)
    mulv = mulv.detach().to(dtype).requires_grad_(True)
    B = recons.shape[0]
    rl = ((recons - _rows(next_obs, idx, dtype)) ** 2).mean(-1).mean()
    vel = ((mulv[:, :3] - _rows(base_vel, idx, dtype)) ** 2).mean()
    mu, lv = mulv[:, 3:3 + LAT], mulv[:, 3 + LAT:3 + 2 * LAT]
    kld = (-0.5 * (1.0 + lv - mu ** 2 - lv.exp()).sum(1)).mean()
    leaves = [recons, mulv]
    if hrecon is not None:
        hrecon = hrecon.detach().to(dtype).requires_grad_(True)
        height = ((hrecon - _rows(priv, idx, dtype)[:, HGT + 3:]) ** 2).mean()
        leaves.append(hrecon)
    else:
        height = torch.zeros((), dtype=dtype)
    g = torch.autograd.grad(rl + vel + 4.0 * kld + height, leaves)
    return SimpleNamespace(losses=torch.stack([rl, vel, kld, height]).detach(), d_recons=g[0], dmulv=g[1],
                           d_hrecon=g[2] if hrecon is not None else None, B=B)


def gaussian_act_ref(mean, std, noise, actions=None, dtype=torch.float64):
    """ppo.py:141-148: actions = mean + std * noise as float32 tensors compute it (the product rounded, then the sum
    rounded), and the log-probability of the float32 actions under N(mean, std) in `dtype`.  `actions`: evaluate the
    log-probability at these float32 actions instead (the ones a kernel emitted)."""
    if actions is None:
        actions = noise.float() * std.float() + mean.float()
    logp = normal_log_prob(actions.to(dtype), mean.to(dtype), std.to(dtype).reshape(-1))
    return actions, logp


def gaussian_act_fused(mean, std, noise):
    """noise * std + mean with ONE rounding (a fused multiply-add): the float64 product of two float32 values is exact."""
    return (noise.double() * std.double() + mean.double()).float()


def bootstrap_probability_ref(rewards):
    """actor_critic_decoder.py:404-407: 1 - tanh(std / mean), unbiased std.  Mean and std in float64, both rounded to
    float32 before the division (the reference's tensors are float32 from there on); n = 1 gives NaN as torch.std does."""
    r = rewards.detach().reshape(-1).double()
    n = r.numel()
    mean = r.sum() / n
    var = ((r - mean) ** 2).sum() / torch.tensor(float(n - 1), dtype=torch.float64)
    cv = var.sqrt().float() / mean.float()
    return float(1.0 - torch.tanh(cv.double()))


def near_boundary(ratio, dlt, l1, l2, clip):
    """Rows on which float32 and float64 may legitimately take different branches of max / clamp: the ratio within 1e-4
    (relative) of 1 +- clip, |value - old_value| within 1e-5 of clip, or a value-clipped row whose two squared errors agree
    to 1e-5 relative.  l1 / l2 None (no value clip): the ratio criterion alone."""
    clip = _f32(clip)
    m = ((ratio - (1.0 - clip)).abs() <= 1e-4 * (1.0 - clip)) | ((ratio - (1.0 + clip)).abs() <= 1e-4 * (1.0 + clip))
    if l1 is not None:
        m = m | ((dlt.abs() - clip).abs() <= 1e-5)
        m = m | ((dlt.abs() > clip) & ((l1 - l2).abs() <= 1e-5 * torch.maximum(l1, l2)))
    return m


def make_ppo_inputs(B, A, seed, R=None, mean=None, value=None):
    """The input recipe of the loss tests: float32 CPU tensors with a large share of rows in every branch of the
    surrogate and value clips at clip = 0.2.  The rollout tensors have R = B + 37 rows, `idx` is a random B-subset of
    them and mean / value belong to the rows idx selects.  `mean` [B, A] / `value` [B] (the fused-heads tests: the outputs
    of the two heads) replace the drawn ones; the rollout rows are then drawn around them by the same rules (returns =
    value - 0.3 N instead of value = returns + 0.3 N)."""
    R = B + 37 if R is None else R
    g = torch.Generator().manual_seed(seed)
    N = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    std = 0.3 + 0.7 * torch.rand(A, generator=g, dtype=torch.float64)
    mean_R = 0.5 * N(R, A)
    idx = torch.randperm(R, generator=g)[:B].contiguous()
    if mean is not None:
        mean_R[idx] = mean.double().reshape(B, A)
    old_mu = (mean_R + 0.05 * N(R, A)).float()
    old_sigma = (std * (1.0 + 0.05 * N(R, A))).clamp(min=0.05).float()
    actions = (old_mu.double() + old_sigma.double() * N(R, A)).float()
    old_logp = normal_log_prob(actions.double(), old_mu.double(), old_sigma.double()).float()
    adv, returns, dv = N(R).float(), N(R), 0.3 * N(R)
    value_R = returns + dv
    if value is not None:
        value_R[idx] = value.double().reshape(B)
        returns = value_R - dv
    value_R, returns = value_R.float(), returns.float()
    old_values = (value_R.double() + 0.3 * N(R)).float()
    return dict(mean=mean_R.float()[idx].contiguous(), std=std.float(), value=value_R[idx].contiguous(), actions=actions,
                old_logp=old_logp, old_mu=old_mu, old_sigma=old_sigma, adv=adv, returns=returns, old_values=old_values, idx=idx)


def make_heads_inputs(B, H, A, act, bias, seed):
    """Inputs of the fused heads: post-activation hidden values Ha / Hc [B, H] of `act`, head weights scaled so that the
    means spread like the recipe's (0.5) and the values like its returns (1), optional biases, and the rollout rows
    make_ppo_inputs draws around the heads' float64 outputs."""
    g = torch.Generator().manual_seed(seed + 7919)
    Ha, Hc = (_act(torch.randn(B, H, generator=g, dtype=torch.float64), act).float() for _ in range(2))
    rms = lambda t: float(t.double().pow(2).mean().sqrt())
    Wa = (torch.randn(A, H, generator=g, dtype=torch.float64) * (0.5 / (math.sqrt(H) * rms(Ha)))).float()
    Wc = (torch.randn(1, H, generator=g, dtype=torch.float64) * (1.0 / (math.sqrt(H) * rms(Hc)))).float()
    ba = (0.1 * torch.randn(A, generator=g)).float() if bias else None
    bc = (0.1 * torch.randn(1, generator=g)).float() if bias else None
    mean = Ha.double() @ Wa.double().t() + (ba.double() if bias else 0.0)
    value = (Hc.double() @ Wc.double().t()).reshape(-1) + (bc.double() if bias else 0.0)
    inp = make_ppo_inputs(B, A, seed, mean=mean, value=value)
    inp.update(Ha=Ha, Hc=Hc, Wa=Wa, Wc=Wc, ba=ba, bc=bc)
    return inp


ROLLOUT_KEYS = ("actions", "old_logp", "old_mu", "old_sigma", "adv", "returns", "old_values")


def gathered(inp):
    """The same mini-batch with the rollout tensors already gathered (for calls with idx = None)."""
    out = dict(inp)
    for k in ROLLOUT_KEYS:
        out[k] = inp[k][inp["idx"]].contiguous()
    out["idx"] = None
    return out
