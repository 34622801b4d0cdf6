"""float64 references of the two batch-global blocks (TEST INFRASTRUCTURE: only tests/ import this; numpy only).

  * the CE-net latent block, csrc/latent.hip (rsl_rl/rsl_rl/modules/actor_critic_decoder.py:274-302):
        mean = lv.mean(); std = lv.std(); out = (lv < mean - 2 std) | (lv > mean + 2 std)
        lv[out] = lv[~out].median()                 (lower median, over the whole batch)
        z = eps * exp(0.5 lv) + mu[:, 3:]
    on the [B, 35] output of the fused head (columns 0..18 mu, 19..34 log-variance), and its backward pass;
  * the advantage normalisation, csrc/gae.hip (rsl_rl/rsl_rl/storage/rollout_storage.py:151-152), with the sample count and the
    sum handed in from outside as the data-parallel ranks do.

Every bound below is a count of float32 roundings, in units of U = 2^-24 (half an ulp relative to the rounded value), written
next to the figure it bounds; none is a measured number."""
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
LAT, MU, LD = 16, 19, 35
MAX_WG, WG_ELEMS, WG_THREADS = 256, 1024, 256          # launch of the latent kernels: at most 256 workgroups of 256 threads, 1024 elements each


def float_key(x):
    """uint32 keys whose unsigned order is the order of the float32 values, -0.0 below +0.0 (the order the radix select ranks in)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_bits(k):
    """the float32 bit pattern of a key"""
    k = np.uint32(k)
    return np.uint32(k & np.uint32(0x7FFFFFFF)) if k & np.uint32(0x80000000) else np.uint32(~k)


def lowest_index_with_bits(lv, out, bits):
    """lowest flat index (row * 16 + col) among the kept elements whose bit pattern is `bits` (-1: none)"""
    hit = np.flatnonzero((np.ascontiguousarray(lv, dtype=np.float32).view(np.uint32).ravel() == np.uint32(bits)) & ~out.ravel())
    return int(hit[0]) if hit.size else -1


def latent_fwd(mulv, eps):
    """mulv float32 [B, 35], eps float32 [B, 16] ->
        mean, std      float64, two-pass, std unbiased
        lo, hi         mean -+ 2 std
        out            bool [B, 16]
        undecided      bool [B, 16]: |lv - lo| or |lv - hi| <= 8 U (|mean| + 2 std).  The kernel rounds the mean, the doubled std and
                       their sum / difference to float32: under four half-ulps of the largest of them; the band leaves a factor two
        kept           number of non-outliers
        median_bits    uint32 bit pattern of the lower median (rank (kept - 1) // 2) of the kept float32 values
        median         the same as float32
        em             lowest flat index among the kept elements whose bits equal the median's
        lv             float32 [B, 16] with the outliers replaced (exact)
        z64            eps exp(0.5 lv) + mu[:, 3:] in float64
        z_bound        4 U (|eps| exp(0.5 lv) + |mu|): two units for expf's one ulp, one for the product, one for the sum"""
    mulv, eps = np.asarray(mulv, dtype=np.float32), np.asarray(eps, dtype=np.float32)
    assert mulv.ndim == 2 and mulv.shape[1] == LD and eps.shape == (mulv.shape[0], LAT)
    lv32 = np.ascontiguousarray(mulv[:, MU:])
    lv = lv32.astype(np.float64)
    n = lv.size
    mean = math.fsum(lv.ravel()) / n
    std = math.sqrt(math.fsum(((lv - mean) ** 2).ravel()) / (n - 1))
    lo, hi = mean - 2.0 * std, mean + 2.0 * std
    out = (lv < lo) | (lv > hi)
    band = 8.0 * U * (abs(mean) + 2.0 * std)
    undecided = (np.abs(lv - lo) <= band) | (np.abs(lv - hi) <= band)
    keys = np.sort(float_key(lv32)[~out])
    kept = int(keys.size)
    assert kept > 0
    bits = key_bits(keys[(kept - 1) // 2])
    median = np.array([bits], dtype=np.uint32).view(np.float32)[0]
    em = lowest_index_with_bits(lv32, out, bits)
    rep = np.where(out, median, lv32).astype(np.float32)
    e64, mu64 = eps.astype(np.float64), mulv[:, 3:MU].astype(np.float64)
    sd = np.exp(0.5 * rep.astype(np.float64))
    return SimpleNamespace(mean=mean, std=std, lo=lo, hi=hi, out=out, undecided=undecided, kept=kept, median_bits=int(bits),
                           median=median, em=em, lv=rep, z64=e64 * sd + mu64, z_bound=4.0 * U * (np.abs(e64) * sd + np.abs(mu64)))


def bwd_path_length(B):
    """L: the additions on the longest path of lat_bwd_kernel's sum of the replaced entries' gradients.  The launch has
    g = min(256, ceil(16 B / 1024)) workgroups of 256 threads; a thread adds its ceil(16 B / (256 g)) elements one after the other,
    six shuffle levels add the 64 lanes of a wave, two more the four waves ((a + b) + (c + d)), the last workgroup adds the g partials
    one after the other and one addition puts the total onto the median element:
        L = ceil(16 B / (256 g)) + 6 + 2 + g + 1          (24576 rows: 6 + 6 + 2 + 256 + 1 = 271)"""
    n = LAT * int(B)
    g = min(MAX_WG, max(1, -(-n // WG_ELEMS)))
    return -(-n // (WG_THREADS * g)) + 6 + 2 + g + 1


def latent_bwd(dmulv_in, dz, eps, lv_replaced, out, em):
    """The gradient dtc_cenet_latent_bwd leaves in dmulv [B, 35] (float64), given the incoming one, dL/dz, and what the forward pass
    left (the replaced log-variances, the outlier mask, the median element's flat index) ->
        grad           float64 [B, 35]:
                         columns 0..2   unchanged
                         columns 3..18  the float32 sum dmulv_in + dz (one rounding: compared exactly, see `exact`)
                         kept log-variance entries  dmulv_in + dz eps 0.5 exp(0.5 lv)
                         replaced entries           0.0 exactly
                         the median element         its own value + the float64 sum of the replaced entries' gradients
        bound          float64 [B, 35]: 0 where the value is exact; kept entries 6 U (|dmulv_in| + |term|) (expf two units, the three
                       products and the sum one each); the median element its own kept-entry bound + U L sum |replaced gradients|
                       with L = bwd_path_length(B)
        exact          bool [B, 35]: bound == 0 and the float32 value is fully specified
        pre_update     the median element's own value, before the replaced entries' sum is added (the kernel records it too)
        pre_bound      its bound
        amax           the value the dmulv amax record must hold: max(|grad|.max(), |pre_update|)
        replaced_sum, replaced_abs_sum, L"""
    d = np.asarray(dmulv_in, dtype=np.float32)
    dz, eps, lv = (np.asarray(a, dtype=np.float32) for a in (dz, eps, lv_replaced))
    out = np.asarray(out, dtype=bool)
    B = d.shape[0]
    assert d.shape == (B, LD) and dz.shape == eps.shape == lv.shape == out.shape == (B, LAT) and 0 <= em < B * LAT
    assert not out.ravel()[em]
    grad, bound = d.astype(np.float64), np.zeros((B, LD))
    grad[:, 3:MU] = (d[:, 3:MU] + dz).astype(np.float64)                          # float32 addition: the one rounding of the kernel
    term = dz.astype(np.float64) * eps.astype(np.float64) * 0.5 * np.exp(0.5 * lv.astype(np.float64))
    g = d[:, MU:].astype(np.float64) + term
    gb = 6.0 * U * (np.abs(d[:, MU:].astype(np.float64)) + np.abs(term))
    L = bwd_path_length(B)
    rsum, rabs = math.fsum(g[out]), math.fsum(np.abs(g[out]))
    r, c = divmod(int(em), LAT)
    pre, pre_bound = float(g[r, c]), float(gb[r, c])
    g, gb = np.where(out, 0.0, g), np.where(out, 0.0, gb)
    g[r, c] = pre + rsum
    gb[r, c] = pre_bound + U * L * rabs
    grad[:, MU:], bound[:, MU:] = g, gb
    return SimpleNamespace(grad=grad, bound=bound, exact=bound == 0.0, pre_update=pre, pre_bound=pre_bound,
                           amax=max(float(np.abs(grad).max()), abs(pre)), replaced_sum=rsum, replaced_abs_sum=rabs, L=L)


def adv_stats(a, count, mean_sum=None):
    """a float32 (any shape), count the number of samples of the WHOLE batch, mean_sum their sum (default: those of `a`) ->
        sum            sum a                                    (float64, exactly rounded)
        sqdev          sum (a - mean)^2, mean = mean_sum / count
        mean, std      std = sqrt(sqdev / (count - 1))
        norm           (a - mean) / (std + 1e-8)
        bound          U (|mean| / std + 5 |norm|) per element: one unit for rounding the mean to float32, one for the difference,
                       two for std + 1e-8 and one for the division"""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    s = math.fsum(a.ravel())
    mean = (s if mean_sum is None else float(mean_sum)) / float(count)
    sq = math.fsum(((a - mean) ** 2).ravel())
    std = math.sqrt(sq / (float(count) - 1.0))
    norm = (a - mean) / (std + 1e-8)
    return SimpleNamespace(sum=s, sqdev=sq, mean=mean, std=std, norm=norm, bound=U * (abs(mean) / std + 5.0 * np.abs(norm)))
