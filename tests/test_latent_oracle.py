"""The float64 references of the CE-net latent block and of the advantage normalisation (oracle/latent_ref.py) checked on the
CPU, and the conditions the GPU comparison (tests/test_hip_latent.py) puts on its own inputs.  The case tables of the GPU tests
live here so that both modules see the same inputs.

LATENT_CASES = value pattern x B.  B: 1 (16 elements), 3, 64 (1024 elements: exactly one workgroup), 65 (16 elements in a second
workgroup), 16384 (256 workgroups, exactly one pass), 16385 (16 elements in a second pass), 24576 (the project's mini-batch).
Patterns of the log-variance columns:
    gauss    0.3 N(0, 1) - 0.2
    heavy    gauss, 3 % of the entries pushed 1 .. 20 away on either side
    ties     gauss rounded to multiples of 1/8: thousands of elements share the median's bits
    narrow   1.125 + 0.03 N(0, 1) clipped into [1.0, 1.25): one bin of the select's first level
    signs    1e-3 N(0, 1) with ~30 % +0.0, ~30 % -0.0 and ~2 % denormals
    uniform  U(-1, 1): the 2 std rule flags nothing (from B = 64 on)
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import gae as OG
from oracle import latent_ref as LREF

PATTERNS = ("gauss", "heavy", "ties", "narrow", "signs", "uniform")
BATCHES = (1, 3, 64, 65, 16384, 16385, 24576)
LATENT_CASES = [(p, B) for p in PATTERNS for B in BATCHES]

ADV_SIZES = (2, 255, 256, 257, 262144, 262145, 524288, 524289, 786432)
ADV_PATTERNS = ("unit", "offset50", "tiny")            # N(0, 1), 50 + N(0, 1), 1e-4 N(0, 1)
ADV_CASES = [(p, n) for p in ADV_PATTERNS for n in ADV_SIZES]
ADV_SHARDS = ((786432, 300001), (257, 100))            # (n, rows of the first shard): two unequal shards


def latent_inputs(pattern, B):
    """-> (mulv float32 [B, 35], eps float32 [B, 16]), from numpy.random.default_rng(1000 + B)"""
    rng = np.random.default_rng(1000 + B)
    gauss = 0.3 * rng.standard_normal((B, 16)) - 0.2
    mu, eps = rng.standard_normal((B, 19)), rng.standard_normal((B, 16))
    if pattern == "gauss":
        lv = gauss
    elif pattern == "heavy":
        far = rng.random((B, 16)) < 0.03
        lv = gauss + far * np.where(rng.random((B, 16)) < 0.5, -1.0, 1.0) * rng.uniform(1.0, 20.0, (B, 16))
    elif pattern == "ties":
        lv = np.round(gauss * 8.0) / 8.0
    elif pattern == "narrow":
        lv = np.clip(1.125 + 0.03 * rng.standard_normal((B, 16)), 1.0, np.nextafter(np.float32(1.25), np.float32(0.0)))
    elif pattern == "signs":
        lv, kind = 1e-3 * rng.standard_normal((B, 16)), rng.random((B, 16))
        lv = np.where(kind < 0.3, 0.0, np.where(kind < 0.6, -0.0, lv))
        lv = np.where((kind >= 0.6) & (kind < 0.62), np.where(lv < 0, -1.0, 1.0) * rng.uniform(1e-45, 1e-38, (B, 16)), lv)
    elif pattern == "uniform":
        lv = rng.uniform(-1.0, 1.0, (B, 16))
    else:
        raise KeyError(pattern)
    mulv = np.concatenate([mu, _off_the_thresholds(lv.astype(np.float32)), ], axis=1).astype(np.float32)
    return np.ascontiguousarray(mulv), np.ascontiguousarray(eps.astype(np.float32))


def _off_the_thresholds(lv):
    """Elements within two widths of the undecided band (oracle/latent_ref.py) of mean -+ 2 std move eight widths towards the mean: a
    handful of the 4e5 elements of the dense patterns (narrow: float32 values 1.2e-7 apart against a band of 5.6e-7), which shifts
    the thresholds themselves by 1e-11.  test_latent_cases_meet_their_conditions asserts the result with the reference alone."""
    x = lv.astype(np.float64)
    mean, std = x.mean(), x.std(ddof=1)
    band = 8.0 * LREF.U * (abs(mean) + 2.0 * std)
    for t in (mean - 2.0 * std, mean + 2.0 * std):
        near = np.abs(x - t) <= 2.0 * band
        x = np.where(near, t + np.sign(mean - t) * 8.0 * band, x)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=2)
def latent_case(pattern, B):
    """(mulv, eps, float64 reference of the forward pass); shared, read-only"""
    mulv, eps = latent_inputs(pattern, B)
    ref = LREF.latent_fwd(mulv, eps)
    for a in (mulv, eps, ref.out, ref.lv, ref.z64, ref.z_bound):
        a.setflags(write=False)
    return mulv, eps, ref


def latent_grads(B):
    """incoming dmulv [B, 35] (all 35 columns) and dL/dz [B, 16] of the backward tests"""
    rng = np.random.default_rng(5000 + B)
    return rng.standard_normal((B, 35)).astype(np.float32), rng.standard_normal((B, 16)).astype(np.float32)


def adv_inputs(pattern, n):
    a = np.random.default_rng(2000 + n).standard_normal(n)
    return {"unit": a, "offset50": 50.0 + a, "tiny": 1e-4 * a}[pattern].astype(np.float32)


# ------------------------------------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("case", LATENT_CASES, ids=str)
def test_latent_cases_meet_their_conditions(case):
    """No element within rounding of a threshold (the GPU test asserts an exact mask), and what each pattern is there for."""
    pattern, B = case
    mulv, eps, ref = latent_case(pattern, B)
    lv = mulv[:, 19:]
    nout = int(ref.out.sum())
    ties = int((lv.view(np.uint32)[~ref.out] == np.uint32(ref.median_bits)).sum())
    print(f"{pattern} B={B}: outliers {nout}, kept {ref.kept}, elements with the median's bits {ties}, em {ref.em}")
    assert int(ref.undecided.sum()) == 0
    assert bool(np.isfinite(lv).all()) and ref.kept + nout == 16 * B and ties >= 1
    # a float32 transcription of the kernel's threshold arithmetic classifies every element as float64 does
    meanf, thr = np.float32(ref.mean), np.float32(2.0) * np.float32(ref.std)
    assert np.array_equal((lv < meanf - thr) | (lv > meanf + thr), ref.out)
    if pattern == "uniform" and B >= 64:                  # (2 std of U(-1, 1) is 1.155 > 1; the std of 16 or 48 samples can fall short of it)
        assert nout == 0
    if pattern == "heavy" and B >= 64:
        assert nout > 0.01 * 16 * B
    if pattern == "narrow":
        assert len(set((LREF.float_key(lv) >> np.uint32(21)).ravel().tolist())) == 1
        assert B < 64 or nout > 0
    if pattern == "ties" and B >= 16384:
        assert ties >= 1000
    if pattern == "signs" and B >= 64:
        u = lv.view(np.uint32)
        assert int((u == 0).sum()) > 0.25 * 16 * B and int((u == 0x80000000).sum()) > 0.25 * 16 * B
        assert int(((u & 0x7F800000) == 0).sum() - ((u & 0x7FFFFFFF) == 0).sum()) > 0.01 * 16 * B          # denormals
        assert (ref.median_bits & 0x7FFFFFFF) == 0


def test_latent_cases_cover_both_parities_of_the_kept_count():
    par = {latent_case(p, B)[2].kept % 2 for p, B in LATENT_CASES if B >= 16384}
    assert par == {0, 1}
    for p in PATTERNS:                                            # ... and so does every pattern that flags anything
        if p != "uniform":
            assert {latent_case(p, B)[2].kept % 2 for B in BATCHES if B >= 64} == {0, 1}, p


# ------------------------------------------------------------------------------------------------ the reference itself
def test_keys_order_like_the_values():
    x = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-45, 1e-40, 2.0, np.inf], dtype=np.float32)
    k = LREF.float_key(x)
    assert bool((np.diff(k.astype(np.int64)) > 0).all())
    assert [int(LREF.key_bits(v)) for v in k] == x.view(np.uint32).tolist()


@pytest.mark.parametrize("B", BATCHES)
def test_latent_fwd_equals_the_model_code_in_float32(B):
    """actor_critic_decoder.py:274-302 in plain float32 torch on the gauss cases: mask, median and replaced values equal, z inside
    z_bound."""
    mulv, eps, ref = latent_case("gauss", B)
    lvf = torch.from_numpy(mulv[:, 19:].copy())
    mean, std = lvf.mean(), lvf.std()
    out = (lvf < mean - 2 * std) | (lvf > mean + 2 * std)
    med = lvf[~out].median()
    lvf[out] = med
    z = torch.from_numpy(eps.copy()) * torch.exp(0.5 * lvf) + torch.from_numpy(mulv[:, 3:19].copy())
    assert np.array_equal(out.numpy(), ref.out)
    assert int(med.view(torch.int32)) & 0xffffffff == ref.median_bits
    assert np.array_equal(lvf.numpy().view(np.uint32), ref.lv.view(np.uint32))
    ratio = float((np.abs(z.double().numpy() - ref.z64) / ref.z_bound).max())
    print(f"B={B}: float32 torch z error / z_bound {ratio:.3f}")
    assert ratio <= 1.0
    assert ref.lv.ravel()[ref.em].view(np.uint32) == ref.median_bits and not ref.out.ravel()[ref.em]
    assert abs(ref.mean - float(mulv[:, 19:].astype(np.float64).mean())) <= 1e-15
    assert abs(ref.std - float(mulv[:, 19:].astype(np.float64).std(ddof=1))) <= 1e-14 * ref.std


def test_lower_median_and_lowest_index_on_a_hand_made_case():
    """kept values 1 1 2 2 3 3 4 4 (even count 8: rank 3 -> 2.0, first at flat index 2), one outlier at 100"""
    lv = np.full((2, 16), 2.0, dtype=np.float32)
    lv[0, :2], lv[1, :6] = 1.0, 3.0
    lv[1, 6:] = 2.0
    lv[0, 7] = 100.0
    mulv = np.zeros((2, 35), dtype=np.float32)
    mulv[:, 19:] = lv
    ref = LREF.latent_fwd(mulv, np.ones((2, 16), dtype=np.float32))
    assert int(ref.out.sum()) == 1 and ref.out[0, 7] and ref.kept == 31
    assert float(ref.median) == 2.0 and ref.em == 2 and float(ref.lv[0, 7]) == 2.0
    lv[:] = np.arange(32, dtype=np.float32).reshape(2, 16)              # nothing flagged, even count: the LOWER of the middle two
    mulv[:, 19:] = lv
    ref = LREF.latent_fwd(mulv, np.ones((2, 16), dtype=np.float32))
    assert int(ref.out.sum()) == 0 and float(ref.median) == 15.0 and ref.em == 15
    assert np.allclose(ref.z64, np.exp(0.5 * lv.astype(np.float64)), rtol=1e-15)


def test_latent_bwd_equals_autograd_in_float64():
    """through torch.where and the median, on a small case of distinct values with several outliers"""
    B = 7
    rng = np.random.default_rng(77)
    mulv = rng.standard_normal((B, 35)).astype(np.float32)
    mulv[:, 19:] = (0.3 * rng.standard_normal((B, 16)) - 0.2).astype(np.float32)
    mulv[1, 20], mulv[4, 30], mulv[6, 34] = 3.0, -4.0, 2.5
    eps = rng.standard_normal((B, 16)).astype(np.float32)
    assert np.unique(mulv[:, 19:]).size == 16 * B
    ref = LREF.latent_fwd(mulv, eps)
    assert int(ref.out.sum()) >= 3 and int(ref.undecided.sum()) == 0
    d_in, dz = (a.copy() for a in latent_grads(B))
    lv = torch.from_numpy(mulv[:, 19:].astype(np.float64)).requires_grad_(True)
    mu = torch.from_numpy(mulv[:, :19].astype(np.float64)).requires_grad_(True)
    mean, std = lv.mean(), lv.std()
    out = (lv < mean - 2 * std) | (lv > mean + 2 * std)
    assert np.array_equal(out.numpy(), ref.out)
    lvf = torch.where(out, lv[~out].median(), lv)
    assert np.array_equal(lvf.detach().numpy(), ref.lv.astype(np.float64))
    z = torch.from_numpy(eps.astype(np.float64)) * torch.exp(0.5 * lvf) + mu[:, 3:]
    assert np.allclose(z.detach().numpy(), ref.z64, rtol=1e-14, atol=1e-15)
    d64 = torch.from_numpy(d_in.astype(np.float64))
    ((z * torch.from_numpy(dz.astype(np.float64))).sum() + (lvf * d64[:, 19:]).sum() + (mu * d64[:, :19]).sum()).backward()
    want = torch.cat([mu.grad, lv.grad], dim=1).numpy()
    got = LREF.latent_bwd(d_in, dz, eps, ref.lv, ref.out, ref.em)
    assert np.array_equal(got.grad[:, :3], d_in[:, :3].astype(np.float64))
    assert np.abs(got.grad[:, 3:19] - want[:, 3:19]).max() <= 2.0 ** -24 * np.abs(want[:, 3:19]).max()      # one float32 rounding
    assert np.abs(got.grad[:, 19:] - want[:, 19:]).max() <= 1e-13
    assert bool((got.grad[:, 19:][ref.out] == 0).all()) and bool((got.bound[:, 19:][ref.out] == 0).all())
    r, c = divmod(ref.em, 16)
    assert abs(got.grad[r, 19 + c] - got.pre_update - got.replaced_sum) <= 1e-15
    assert got.bound[r, 19 + c] == got.pre_bound + LREF.U * got.L * got.replaced_abs_sum and got.replaced_abs_sum > 0
    assert got.amax == max(np.abs(got.grad).max(), abs(got.pre_update))
    assert bool((got.bound[:, 19:][~ref.out] > 0).all()) and bool(got.exact[:, :19].all())


def test_backward_path_length_follows_the_launch():
    """ceil(16 B / (256 g)) + 6 + 2 + g + 1 with g = min(256, ceil(16 B / 1024))"""
    assert LREF.bwd_path_length(1) == 1 + 6 + 2 + 1 + 1
    assert LREF.bwd_path_length(64) == 4 + 6 + 2 + 1 + 1
    assert LREF.bwd_path_length(65) == 3 + 6 + 2 + 2 + 1
    assert LREF.bwd_path_length(16384) == 4 + 6 + 2 + 256 + 1
    assert LREF.bwd_path_length(16385) == 5 + 6 + 2 + 256 + 1
    assert LREF.bwd_path_length(24576) == 271


@pytest.mark.parametrize("case", [c for c in ADV_CASES if c[1] in (2, 257, 262145)], ids=str)
def test_adv_stats_equals_numpy_in_float64(case):
    pattern, n = case
    a = adv_inputs(pattern, n)
    r = LREF.adv_stats(a, n)
    a64 = a.astype(np.float64)
    assert abs(r.sum - a64.sum()) <= 1e-13 * np.abs(a64).sum()
    assert abs(r.mean - a64.mean()) <= 1e-13 * np.abs(a64).mean()
    assert abs(r.std - a64.std(ddof=1)) <= 1e-12 * r.std
    assert abs(r.sqdev - ((a64 - a64.mean()) ** 2).sum()) <= 1e-12 * r.sqdev
    assert np.allclose(r.norm, (a64 - a64.mean()) / (a64.std(ddof=1) + 1e-8), rtol=1e-11, atol=1e-12)
    # the shards of a data-parallel run: global count and sum, local squared deviations
    k = max(1, n // 3)
    parts = [LREF.adv_stats(s, n, mean_sum=r.sum) for s in (a[:k], a[k:])]
    assert abs(parts[0].sqdev + parts[1].sqdev - r.sqdev) <= 1e-14 * r.sqdev
    assert parts[0].mean == r.mean


def test_adv_stats_equals_the_gae_oracle():
    """oracle/gae.py normalises in float32 from float64 moments: inside the bound adv_stats states for exactly that arithmetic"""
    rng = np.random.default_rng(9)
    for off in (0.0, 50.0):
        ret, val = (off + rng.standard_normal((24, 300))).astype(np.float32), rng.standard_normal((24, 300)).astype(np.float32)
        norm, mean, std = OG.normalize_advantages(ret, val)
        r = LREF.adv_stats((ret - val).astype(np.float32), ret.size)
        assert abs(mean - r.mean) <= 1e-13 * max(1.0, abs(r.mean)) and abs(std - r.std) <= 1e-13 * r.std
        ratio = float((np.abs(norm.astype(np.float64) - r.norm) / r.bound).max())
        print(f"offset {off}: oracle/gae.py error / bound {ratio:.3f}")
        assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ the comparisons of the GPU tests
# tests/test_hip_latent.py hands the kernels' outputs (numpy) to the functions below.  They live here so that the CPU suite can run them
# too: on a float32 transcription of the kernels (every case must pass) and against deliberately wrong references (the assertion
# meant to catch each must fail).
class Checks:
    """The assertions of one comparison: every one is evaluated; done() fails with the names of all that did not hold."""

    def __init__(self, what):
        self.what, self.failed = what, []

    def ok(self, name, cond, detail=""):
        if not bool(cond):
            self.failed.append(f"{name} {detail}".strip())
        return bool(cond)

    def names(self):
        return {f.split(":")[0].split(" ")[0] for f in self.failed}

    def done(self):
        assert not self.failed, (self.what, self.failed)


def report(kernel, name, err, bound):
    print(f"ERR {kernel} {name} {err:.3e} {bound:.0e}")


def f32_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _worst(err, bound):
    """largest err / bound (a zero bound asks for a zero error); inf where a value is not finite"""
    err, bound = np.asarray(err, dtype=np.float64).ravel(), np.asarray(bound, dtype=np.float64).ravel()
    if err.size == 0:
        return 0.0
    if not np.isfinite(err).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def check_forward(what, pattern, mulv_in, ref, got):
    """got: mulv [B, 35], z [B, 16], mask uint8 [B, 16], info (4 ints), z_amax (the record's value as an integer) as the launch left
    them.  -> (Checks, what the backward comparison needs: em, the replaced log-variances, the median's bits).  `signs`: the median is
    a zero; either zero is accepted, and the index and the replaced values are then asked for that zero."""
    c = Checks(what)
    lv_in = np.ascontiguousarray(mulv_in[:, 19:])
    c.ok("mask", np.array_equal(got.mask, ref.out.astype(np.uint8)), f"{int((got.mask != ref.out).sum())} differ")
    c.ok("info[0]", int(got.info[0]) == int(ref.out.sum()), f"{int(got.info[0])} != {int(ref.out.sum())}")
    bits, i1 = int(got.info[2]) & 0xffffffff, int(got.info[1])
    want, em, lv = ref.median_bits, ref.em, ref.lv
    if pattern == "signs" and bits != want and (bits & 0x7fffffff) == 0 and (want & 0x7fffffff) == 0:
        want, em = bits, LREF.lowest_index_with_bits(lv_in, ref.out, bits)
        lv = np.where(ref.out, np.array([bits], dtype=np.uint32).view(np.float32)[0], lv_in).astype(np.float32)
    c.ok("info[2]", bits == want, f"{bits:#x} != {want:#x}")
    c.ok("info[1]", i1 == em, f"{i1} != {em}")
    c.ok("element_at_info[1]", 0 <= i1 < lv_in.size and int(_u32(lv_in).ravel()[i1]) == bits and not ref.out.ravel()[i1])
    c.ok("replaced", np.array_equal(_u32(got.mulv[:, 19:]), _u32(lv)))
    c.ok("mu_untouched", np.array_equal(_u32(got.mulv[:, :19]), _u32(mulv_in[:, :19])))
    ratio = _worst(np.abs(got.z.astype(np.float64) - ref.z64), ref.z_bound)
    report("cenet_latent_fwd", "z", ratio, 1.0)
    c.ok("z", ratio <= 1.0, f"error / bound {ratio:.3f}")
    c.ok("z_amax", got.z_amax is None or int(got.z_amax) == f32_bits(np.abs(got.z).max()))
    return c, SimpleNamespace(em=em, lv=lv, bits=want)


def check_backward(what, d_in, bref, out, em, got):
    """got: dmulv [B, 35] as the launch left it, amax (the record's value as an integer, None: no record given)"""
    c = Checks(what)
    g = got.dmulv
    c.ok("cols0..2", np.array_equal(_u32(g[:, :3]), _u32(d_in[:, :3])))
    c.ok("cols3..18", np.array_equal(_u32(g[:, 3:19]), _u32(bref.grad[:, 3:19].astype(np.float32))) and
         np.array_equal(bref.grad[:, 3:19].astype(np.float32).astype(np.float64), bref.grad[:, 3:19]))
    glv, r, col = g[:, 19:].astype(np.float64), em // 16, em % 16
    kept = ~out
    kept[r, col] = False
    err = np.abs(glv - bref.grad[:, 19:])
    ratio = _worst(err[kept], bref.bound[:, 19:][kept])
    report("cenet_latent_bwd", "kept", ratio, 1.0)
    c.ok("kept", ratio <= 1.0, f"error / bound {ratio:.3f}")
    c.ok("replaced", bool((g[:, 19:][out] == 0.0).all()), f"{int((g[:, 19:][out] != 0.0).sum())} not zero")
    ratio = _worst(err[r, col], bref.bound[r, 19 + col])
    report("cenet_latent_bwd", "median_element", ratio, 1.0)
    c.ok("median_element", ratio <= 1.0, f"error / bound {ratio:.3f} of {bref.bound[r, 19 + col]:.3e}")
    if got.amax is not None:
        # the record holds the final gradient's largest magnitude, or the median element's own value where that was larger before the
        # replaced entries' sum arrived (the kernel records both): exactly the former wherever the latter cannot exceed it
        final = f32_bits(np.abs(g).max())
        pre_hi = f32_bits(np.nextafter(np.float32(abs(bref.pre_update) + bref.pre_bound), np.float32(np.inf)))
        rec = int(got.amax)
        val = float(np.array([rec], dtype=np.uint32).view(np.float32)[0])
        tol = max(float(bref.bound.max()), bref.pre_bound) + LREF.U * bref.amax
        c.ok("amax", final <= rec <= max(final, pre_hi) and abs(val - bref.amax) <= tol, f"{rec:#x}: final {final:#x}, pre-update {pre_hi:#x}")
    return c


def check_adv(what, a, count, r, sqdev=None, norm=None):
    """sqdev: stats[1] after dtc_adv_sqdev on `a`; norm: `a` after dtc_adv_normalize; r: adv_stats(a, count, the sum handed in)"""
    c = Checks(what)
    if sqdev is not None:
        tol = 1e-12 * r.sqdev * max(1, int(np.ceil(np.log2(a.size))))
        err = abs(float(sqdev) - r.sqdev)
        report("adv_sqdev", "stats[1]", err / tol if np.isfinite(err) else np.inf, 1.0)
        c.ok("stats[1]", err <= tol, f"{float(sqdev)!r} against {r.sqdev!r}")
    if norm is not None:
        ratio = _worst(np.abs(norm.astype(np.float64) - r.norm), r.bound)
        report("adv_normalize", "advantages", ratio, 1.0)
        c.ok("norm", ratio <= 1.0, f"error / bound {ratio:.3f}")
    return c


# ---- float32 transcriptions of the kernels (numpy): the stand-in for the device on a CPU-only machine
def _exp32(x):
    """a correctly rounded float32 exponential (numpy's own float32 exp is good to 2.5 ulp only, the device's expf to 1)"""
    return np.exp(x.astype(np.float64)).astype(np.float32)


def transcribe_forward(mulv, eps):
    lv = np.ascontiguousarray(mulv[:, 19:])
    x = lv.astype(np.float64)
    n, s, q = x.size, x.sum(), (x * x).sum()
    var = max((q - s * s / n) / (n - 1), 0.0)
    meanf, thr = np.float32(s / n), np.float32(2.0) * np.float32(np.sqrt(var))
    out = (lv < meanf - thr) | (lv > meanf + thr)
    keys = np.sort(LREF.float_key(lv)[~out])
    bits = int(LREF.key_bits(keys[(keys.size - 1) // 2]))
    med = np.array([bits], dtype=np.uint32).view(np.float32)[0]
    res = mulv.copy()
    res[:, 19:] = np.where(out, med, lv)
    z = (eps * _exp32(np.float32(0.5) * res[:, 19:]) + mulv[:, 3:19]).astype(np.float32)
    return SimpleNamespace(mulv=res, z=z, mask=out.astype(np.uint8), info=[int(out.sum()), LREF.lowest_index_with_bits(lv, out, bits), bits, 0],
                           z_amax=f32_bits(np.abs(z).max()))


def transcribe_backward(d_in, dz, eps, lv, out, em):
    g = d_in.copy()
    g[:, 3:19] = d_in[:, 3:19] + dz
    glv = (d_in[:, 19:] + dz * eps * (np.float32(0.5) * _exp32(np.float32(0.5) * lv))).astype(np.float32)
    acc = glv[out].sum(dtype=np.float32)
    glv[out] = 0.0
    pre = glv[em // 16, em % 16]
    glv[em // 16, em % 16] = pre + acc
    g[:, 19:] = glv
    return SimpleNamespace(dmulv=g, amax=f32_bits(max(np.abs(g).max(), abs(pre))))


def transcribe_adv(a, count, mean_sum, sqdev=None):
    mean = mean_sum / count
    sq = float(((a.astype(np.float64) - mean) ** 2).sum())
    std = np.float32(np.sqrt((sq if sqdev is None else sqdev) / (count - 1.0)))
    return sq, ((a - np.float32(mean)) / (std + np.float32(1e-8))).astype(np.float32)


@pytest.mark.parametrize("case", LATENT_CASES, ids=str)
def test_comparisons_accept_a_float32_transcription_of_the_latent_kernels(case):
    pattern, B = case
    mulv, eps, ref = latent_case(pattern, B)
    got = transcribe_forward(mulv, eps)
    c, fwd = check_forward(str(case), pattern, mulv, ref, got)
    c.done()
    d_in, dz = latent_grads(B)
    bref = LREF.latent_bwd(d_in, dz, eps, fwd.lv, ref.out, fwd.em)
    check_backward(str(case), d_in, bref, ref.out, fwd.em, transcribe_backward(d_in, dz, eps, fwd.lv, ref.out, fwd.em)).done()
    if pattern == "uniform" and B >= 64:
        assert bref.replaced_abs_sum == 0.0 and bref.grad[fwd.em // 16, 19 + fwd.em % 16] == bref.pre_update


@pytest.mark.parametrize("case", ADV_CASES, ids=str)
def test_comparisons_accept_a_float32_transcription_of_the_advantage_kernels(case):
    pattern, n = case
    a = adv_inputs(pattern, n)
    r = LREF.adv_stats(a, n)
    sq, norm = transcribe_adv(a, float(n), r.sum)
    check_adv(str(case), a, n, r, sq, norm).done()


def _copy(ns, **kw):
    d = dict(vars(ns))
    d.update(kw)
    return SimpleNamespace(**d)


def _with_median(ref, mulv, eps, bits, em=None):
    """the forward reference had it picked `bits` as the median (and `em` as its element)"""
    lv_in = mulv[:, 19:]
    med = np.array([bits], dtype=np.uint32).view(np.float32)[0]
    lv = np.where(ref.out, med, lv_in).astype(np.float32)
    sd = np.exp(0.5 * lv.astype(np.float64))
    return _copy(ref, median_bits=int(bits), median=med, lv=lv, em=LREF.lowest_index_with_bits(lv_in, ref.out, bits) if em is None else em,
                 z64=eps.astype(np.float64) * sd + mulv[:, 3:19].astype(np.float64))


def test_every_assertion_of_the_forward_comparison_can_fail():
    """Each reference below is wrong in one deliberate way; the transcription of the kernel stands in for the device.  The assertion
    named next to it must fail (others may fail with it)."""
    def failed(pattern, B, wrong, mulv_in=None):
        mulv, eps, ref = latent_case(pattern, B)
        c, _ = check_forward("wrong reference", pattern, mulv if mulv_in is None else mulv_in(mulv), wrong(mulv, eps, ref), transcribe_forward(mulv, eps))
        return c.names()

    # population instead of unbiased std: moves the thresholds of a 16-element batch by 3 %
    def population(mulv, eps, ref):
        x = mulv[:, 19:].astype(np.float64)
        return _copy(ref, out=(x < x.mean() - 2 * x.std(ddof=0)) | (x > x.mean() + 2 * x.std(ddof=0)))
    hit = [failed(p, B, population) for p, B in LATENT_CASES if B <= 3]
    assert any({"mask", "info[0]"} <= h for h in hit), hit

    # rank kept // 2 instead of (kept - 1) // 2, on an even kept count of distinct values
    def upper_median(mulv, eps, ref):
        assert ref.kept % 2 == 0
        keys = np.sort(LREF.float_key(mulv[:, 19:])[~ref.out])
        return _with_median(ref, mulv, eps, int(LREF.key_bits(keys[ref.kept // 2])))
    assert {"info[2]", "info[1]", "replaced"} <= failed("gauss", 64, upper_median)

    # the median's element taken as the HIGHEST index among the ties
    def highest(mulv, eps, ref):
        hit = np.flatnonzero((_u32(mulv[:, 19:]).ravel() == ref.median_bits) & ~ref.out.ravel())
        return _copy(ref, em=int(hit[-1]))
    assert failed("ties", 65, highest) == {"info[1]"}

    # keys of negative values not inverted (the negative values rank in reverse order)
    def negatives_reversed(mulv, eps, ref):
        keys = np.sort(_u32(mulv[:, 19:])[~ref.out] ^ np.uint32(0x80000000))
        return _with_median(ref, mulv, eps, int(keys[(ref.kept - 1) // 2] ^ np.uint32(0x80000000)))
    assert {"info[2]", "replaced"} <= failed("gauss", 16385, negatives_reversed)

    # the element the reference calls the median's is an outlier to it
    def em_flagged(mulv, eps, ref):
        out = ref.out.copy()
        out.ravel()[ref.em] = True
        return _copy(ref, out=out)
    assert {"mask", "element_at_info[1]"} <= failed("heavy", 65, em_flagged)

    # the reference's input differs in one mean
    def other_mu(mulv):
        m = mulv.copy()
        m[0, 0] = -m[0, 0]
        return m
    assert failed("gauss", 3, lambda mulv, eps, ref: ref, other_mu) == {"mu_untouched"}

    # z from mu[:, 2:18] (one column off), and with exp(lv / 2) rounded to float16-like 11 bits (a fast-math exponential)
    assert failed("gauss", 65, lambda mulv, eps, ref: _copy(ref, z64=ref.z64 - mulv[:, 3:19] + mulv[:, 2:18])) == {"z"}
    def coarse_exp(mulv, eps, ref):
        sd = np.exp(0.5 * ref.lv.astype(np.float64)) * (1.0 + 2.0 ** -21)
        return _copy(ref, z64=eps.astype(np.float64) * sd + mulv[:, 3:19].astype(np.float64))
    assert failed("gauss", 16385, coarse_exp) == {"z"}

    # z amax: the largest z instead of the largest |z| (on a case whose largest magnitude is negative)
    for p, B in LATENT_CASES:
        mulv, eps, ref = latent_case(p, B)
        got = transcribe_forward(mulv, eps)
        if -got.z.min() > got.z.max():
            got.z_amax = f32_bits(got.z.max())
            assert check_forward("signed maximum", p, mulv, ref, got)[0].names() == {"z_amax"}
            break
    else:
        raise AssertionError("no case with a negative largest magnitude")


def test_every_assertion_of_the_backward_comparison_can_fail():
    pattern, B = "heavy", 65
    mulv, eps, ref = latent_case(pattern, B)
    d_in, dz = latent_grads(B)
    got = transcribe_backward(d_in, dz, eps, ref.lv, ref.out, ref.em)
    good = LREF.latent_bwd(d_in, dz, eps, ref.lv, ref.out, ref.em)
    assert good.replaced_abs_sum > 0

    def failed(bref, d=d_in, out=ref.out, em=ref.em, g=got):
        return check_backward("wrong reference", d, bref, out, em, g).names()
    assert failed(good) == set()
    # the incoming gradient of the first three columns taken as zero (what the earlier test fed)
    zeroed = d_in.copy()
    zeroed[:, :3] = 0.0
    assert failed(good, d=zeroed) == {"cols0..2"}
    # dmulv_in + dz left in float64 (no float32 rounding)
    wide = good.grad.copy()
    wide[:, 3:19] = d_in[:, 3:19].astype(np.float64) + dz.astype(np.float64)
    assert failed(_copy(good, grad=wide)) == {"cols3..18"}
    # d exp(lv / 2) / d lv without its factor 1/2
    twice = good.grad.copy()
    twice[:, 19:] = np.where(ref.out, 0.0, 2.0 * good.grad[:, 19:] - d_in[:, 19:])
    assert "kept" in failed(_copy(good, grad=twice))
    # one more element flagged than the kernel replaced
    out = ref.out.copy()
    extra = int(np.flatnonzero(~out.ravel())[5])
    assert extra != ref.em
    out.ravel()[extra] = True
    assert "replaced" in failed(LREF.latent_bwd(d_in, dz, eps, ref.lv, out, ref.em), out=out)
    # the replaced entries' sum lands on the highest-index element holding the median value's bits / misses one entry / is left out
    r, col = ref.em // 16, 19 + ref.em % 16
    short = good.grad.copy()
    short[r, col] -= float(np.abs(good.grad[:, 19:]).max()) * 1e-3 + 10 * good.bound[r, col]
    assert failed(_copy(good, grad=short)) == {"median_element"}
    nosum = good.grad.copy()
    nosum[r, col] = good.pre_update
    assert "median_element" in failed(_copy(good, grad=nosum))
    mulv_t, eps_t, ref_t = latent_case("ties", 65)
    hi = int(np.flatnonzero((_u32(mulv_t[:, 19:]).ravel() == ref_t.median_bits) & ~ref_t.out.ravel())[-1])
    got_t = transcribe_backward(d_in, dz, eps_t, ref_t.lv, ref_t.out, ref_t.em)
    assert {"kept", "median_element"} <= failed(LREF.latent_bwd(d_in, dz, eps_t, ref_t.lv, ref_t.out, hi), out=ref_t.out, em=hi, g=got_t)
    # amax of the log-variance columns only / of a gradient without the record of the pre-update value where that one is the largest
    small = _copy(got, amax=f32_bits(np.abs(got.dmulv[:, 19:]).max()))
    assert np.abs(got.dmulv[:, :19]).max() > np.abs(got.dmulv[:, 19:]).max()
    assert failed(good, g=small) == {"amax"}
    big = _copy(got, amax=f32_bits(2.0 * np.abs(got.dmulv).max()))
    assert failed(good, g=big) == {"amax"}


def test_every_assertion_of_the_advantage_comparison_can_fail():
    n, k = ADV_SHARDS[0]
    a = adv_inputs("offset50", n)
    whole = LREF.adv_stats(a, n)
    sq, norm = transcribe_adv(a, float(n), whole.sum)
    assert check_adv("right", a, n, whole, sq, norm).names() == set()
    # population instead of unbiased std (1 / (2 n) = 6e-7 relative, against 5 * 2^-24 = 3e-7)
    unit = adv_inputs("unit", n)
    ru = LREF.adv_stats(unit, n)
    squ, normu = transcribe_adv(unit, float(n), ru.sum)
    wrong = _copy(ru, norm=(unit.astype(np.float64) - ru.mean) / (np.sqrt(ru.sqdev / n) + 1e-8))
    assert check_adv("population std", unit, n, wrong, squ, normu).names() == {"norm"}
    # a shard whose reference takes count = n_local: its mean is the shard's share of the global sum
    shard = a[:k]
    sq_k, _ = transcribe_adv(shard, float(n), whole.sum)
    right, wrong = LREF.adv_stats(shard, n, mean_sum=whole.sum), LREF.adv_stats(shard, k, mean_sum=whole.sum)
    assert check_adv("shard", shard, n, right, sq_k, None).names() == set()
    assert check_adv("count = n_local", shard, k, wrong, sq_k, None).names() == {"stats[1]"}
