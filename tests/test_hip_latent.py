"""The two batch-global blocks against the float64 references of oracle/latent_ref.py, at and past their launch caps:
dtc_cenet_latent_fwd[_img] / dtc_cenet_latent_bwd (csrc/latent.hip: 256 workgroups x 1024 elements, then a grid-stride loop) on
every (value pattern, B) of tests/test_latent_oracle.py, and dtc_adv_sqdev / dtc_adv_normalize (csrc/gae.hip: 1024 / 2048 workgroups
x 256) on plain arrays with the sum written from the host, on two shards with the global count, and behind dtc_gae.

What is exact is compared exactly (the mask, the outlier count, the median's bits and element, the replaced values, the untouched
columns, the single-rounding columns of the gradient, the zeroed entries, the amax records, everything the workspace discipline and
the operand image promise); everything else against the roundings counted in oracle/latent_ref.py (`ERR kernel output ratio 1`:
error / bound, which must stay below 1).  The comparisons themselves are tests/test_latent_oracle.py's check_forward /
check_backward / check_adv, which the CPU suite runs against deliberately wrong references.  Every output is filled with NaN (info
and the mask with a sentinel) before the launch.

Worst error / bound measured on an MI355X (all cases): z 0.52; kept log-variance gradients 0.44; the median element 0.11; normalised
advantages 0.81; stats[1] 2.8e-5 of its bound (the two shards against the whole array 2.0e-5); stats[0] behind dtc_gae exact; the
decoded operand image 1.2e-7 of the row's largest element against 2^-21 = 4.8e-7, and byte for byte the encoding.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dtc_amd import _ffi, h2i, ops
from oracle import gae as OG
from oracle import h2image as OH
from oracle import latent_ref as LREF
from test_latent_oracle import (ADV_CASES, ADV_PATTERNS, ADV_SHARDS, LATENT_CASES, adv_inputs, check_adv, check_backward, check_forward,
                                latent_case, latent_grads, report)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                   # (a copy: the shared cases are read-only)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _workspace(fill=0xFF):
    """the latent block's scratch, every byte `fill`: the launches must not rely on what it held"""
    return torch.full((int(_ffi.lib().dtc_cenet_workspace(1)) + 8,), fill, dtype=torch.uint8, device=DEV)


def _record():
    return torch.zeros(int(_ffi.lib().dtc_amax_record_bytes()) // 4, dtype=torch.int32, device=DEV)


def _record_value(rec):
    return None if rec is None else max(int(v) & 0xffffffff for v in rec.cpu().tolist())


def _p(t):
    return None if t is None else t.data_ptr()


def _forward(mulv, eps, ws, image=False, record=True):
    """dtc_cenet_latent_fwd[_img] on copies of the CPU inputs -> device tensors (mulv rewritten in place)"""
    B = mulv.shape[0]
    d = SimpleNamespace(mulv=_dev(mulv), eps=_dev(eps), z=_nan(B, 16), mask=torch.full((B, 16), 0xAA, dtype=torch.uint8, device=DEV),
                        info=torch.full((4,), SENTINEL, dtype=torch.int32, device=DEV), rec=_record() if record else None,
                        img=h2i.HImage(B, 19, DEV) if image else None, ws=ws, B=B)
    lib = _ffi.lib()
    if image:
        rc = lib.dtc_cenet_latent_fwd_img(_p(d.mulv), _p(d.eps), _p(d.z), _p(d.mask), _p(d.info), _p(ws), B, _p(d.rec), d.img.ptr(), _ffi.stream())
    else:
        rc = lib.dtc_cenet_latent_fwd(_p(d.mulv), _p(d.eps), _p(d.z), _p(d.mask), _p(d.info), _p(ws), B, _p(d.rec), _ffi.stream())
    _ffi.check(rc, "dtc_cenet_latent_fwd")
    torch.cuda.synchronize()
    return d


def _forward_host(d):
    return SimpleNamespace(mulv=d.mulv.cpu().numpy(), z=d.z.cpu().numpy(), mask=d.mask.cpu().numpy(), info=d.info.cpu().tolist(),
                           z_amax=_record_value(d.rec))


def _backward(d, d_in, dz, record=True):
    """dtc_cenet_latent_bwd on what the forward call `d` left (its workspace included) -> (dmulv on the host, the record's value)"""
    dm, rec = _dev(d_in), _record() if record else None
    _ffi.check(_ffi.lib().dtc_cenet_latent_bwd(_p(dm), _p(_dev(dz)), _p(d.eps), _p(d.mulv), _p(d.mask), _p(d.info), _p(d.ws), d.B, _p(rec),
                                               _ffi.stream()), "dtc_cenet_latent_bwd")
    torch.cuda.synchronize()
    return SimpleNamespace(dmulv=dm.cpu().numpy(), amax=_record_value(rec))


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ the latent block
@pytest.mark.parametrize("case", LATENT_CASES, ids=str)
def test_latent_forward_against_float64(case):
    pattern, B = case
    mulv, eps, ref = latent_case(pattern, B)
    got = _forward_host(_forward(mulv, eps, _workspace()))
    assert got.info[3] == 0
    check_forward(f"cenet_latent_fwd {case}", pattern, mulv, ref, got)[0].done()


@pytest.mark.parametrize("B", [65, 16385])
def test_latent_forward_on_constant_input(B):
    """All log-variances 0.37: n x is exact in float64, the variance is zero to rounding and the thresholds round to x or the floats
    next to it: no outlier, the median is x and its element the first."""
    rng = np.random.default_rng(3000 + B)
    mulv = rng.standard_normal((B, 35)).astype(np.float32)
    mulv[:, 19:] = np.float32(0.37)
    eps = rng.standard_normal((B, 16)).astype(np.float32)
    ref = LREF.latent_fwd(mulv, eps)
    assert ref.std == 0.0 and ref.mean == float(np.float32(0.37)) and not ref.out.any() and ref.em == 0
    assert ref.median_bits == int(np.array([0.37], dtype=np.float32).view(np.uint32)[0])
    got = _forward_host(_forward(mulv, eps, _workspace()))
    assert got.info == [0, 0, ref.median_bits, 0]
    check_forward(f"cenet_latent_fwd constant B={B}", "constant", mulv, ref, got)[0].done()


@pytest.mark.parametrize("case", LATENT_CASES, ids=str)
def test_latent_backward_against_float64(case):
    """Random incoming gradient in all 35 columns, random dL/dz; no element is excused."""
    pattern, B = case
    mulv, eps, ref = latent_case(pattern, B)
    d = _forward(mulv, eps, _workspace())
    c, fwd = check_forward(f"cenet_latent_fwd {case}", pattern, mulv, ref, _forward_host(d))
    c.done()
    d_in, dz = latent_grads(B)
    bref = LREF.latent_bwd(d_in, dz, eps, fwd.lv, ref.out, fwd.em)
    got = _backward(d, d_in, dz)
    check_backward(f"cenet_latent_bwd {case}", d_in, bref, ref.out, fwd.em, got).done()
    if pattern == "uniform" and B >= 64:                          # nothing replaced: the median element keeps its own value
        assert bref.replaced_abs_sum == 0.0


def test_latent_workspace_is_reusable_and_needs_no_initialisation():
    """Forward and backward on case A, on case B (another grid size), on A again, all on ONE workspace that started as 0xFF bytes:
    the third results equal the first bit for bit, and those of a run on a fresh, zeroed workspace (the histogram header is zeroed
    again by every forward call, the arrival ticket reset by every backward call).  With and without the amax record the gradient
    is the same."""
    def run(case, ws, record=True):
        mulv, eps, _ = latent_case(*case)
        d = _forward(mulv, eps, ws)
        f = _forward_host(d)
        b = _backward(d, *latent_grads(case[1]), record=record)
        return f, b

    def same(x, y):
        fx, bx = x
        fy, by = y
        return (_same_bits(fx.mulv, fy.mulv) and _same_bits(fx.z, fy.z) and _same_bits(fx.mask, fy.mask) and fx.info == fy.info and
                fx.z_amax == fy.z_amax and _same_bits(bx.dmulv, by.dmulv))

    A, Bc = ("heavy", 16385), ("ties", 65)
    ws = _workspace(0xFF)
    first, other, third = run(A, ws), run(Bc, ws), run(A, ws)
    assert same(first, third) and first[1].amax == third[1].amax
    assert same(first, run(A, _workspace(0x00)))
    assert same(other, run(Bc, _workspace(0x00)))
    assert same(other, run(Bc, ws))                               # ... and the small grid after the large one
    without = run(A, ws, record=False)
    assert without[1].amax is None and same(first, without)


@pytest.mark.parametrize("case", [("heavy", 16385), ("gauss", 24576)], ids=str)
def test_latent_forward_writes_the_operand_image(case):
    """dtc_cenet_latent_fwd_img: the image decodes (oracle/h2image.py) to [z | mu[:, :3]] within 2^-21 of each row's largest element
    -- the format's bound, tests/test_hip_h2i.py -- with zero padding columns, and is byte for byte the encoding of those values; z,
    the mask, info and the replaced values are those of the call without an image."""
    pattern, B = case
    mulv, eps, ref = latent_case(pattern, B)
    plain = _forward_host(_forward(mulv, eps, _workspace()))
    d = _forward(mulv, eps, _workspace(), image=True)
    got = _forward_host(d)
    assert _same_bits(got.z, plain.z) and _same_bits(got.mask, plain.mask) and got.info == plain.info and _same_bits(got.mulv, plain.mulv)
    assert got.z_amax == plain.z_amax
    rt, st = -(-B // 128), 2
    raw = d.img.buf.view(torch.uint8).cpu().numpy()
    chunks = raw[:rt * st * 8192].view(np.uint16).reshape(rt, st, 2, 256, 8)
    exps = raw[rt * st * 8192:rt * st * 8192 + rt * 512].view(np.int32).reshape(rt, 1, 128)
    want = np.concatenate([got.z, mulv[:, :3]], axis=1)
    dec = OH.decode(chunks, exps, rt * 128, 32)
    assert not dec[:, 19:].any() and not dec[B:].any()
    err = np.abs(dec[:B, :19].astype(np.float64) - want).max(axis=1) / np.abs(want).max(axis=1)
    report("cenet_latent_fwd_img", "image", float(err.max()), 2.0 ** -21)
    assert float(err.max()) <= 2.0 ** -21
    want_c, want_e = OH.encode(want)
    assert np.array_equal(exps, want_e) and np.array_equal(chunks, want_c)


# ------------------------------------------------------------------------------------------------ advantage statistics
def _stats(total):
    return torch.tensor([total, float("nan")], dtype=torch.float64, device=DEV)


def _sqdev(a_dev, total, count):
    st = _stats(total)
    ops.adv_sqdev(a_dev, st, count)
    torch.cuda.synchronize()
    got = st.cpu().tolist()
    assert got[0] == total                                        # an input: left alone
    return got[1]


def _normalize(a_dev, total, sqdev, count):
    out = a_dev.clone()
    ops.adv_normalize(out, torch.tensor([total, sqdev], dtype=torch.float64, device=DEV), count)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", ADV_CASES, ids=str)
def test_advantage_statistics_against_float64(case):
    """stats[0] written from the host as the float64 sum; stats[1] and the normalised advantages at 1, 1024 / 2048 workgroups and
    one element past them."""
    pattern, n = case
    a = adv_inputs(pattern, n)
    r = LREF.adv_stats(a, n)
    a_dev = _dev(a)
    sq = _sqdev(a_dev, r.sum, n)
    check_adv(f"adv {case}", a, n, r, sq, _normalize(a_dev, r.sum, sq, n)).done()
    assert _same_bits(a_dev.cpu().numpy(), a)


@pytest.mark.parametrize("pattern", ADV_PATTERNS)
@pytest.mark.parametrize("n,k", ADV_SHARDS)
def test_advantage_statistics_of_two_shards(n, k, pattern):
    """The data-parallel contract of rollout_storage.compute_returns: every rank calls dtc_adv_sqdev on its own shard with the GLOBAL
    count and the GLOBAL sum, the partial results are added, and every rank normalises its shard with the two global numbers."""
    a = adv_inputs(pattern, n)
    whole = LREF.adv_stats(a, n)
    a_dev = _dev(a)
    shards = (a_dev[:k], a_dev[k:])
    sq_whole = _sqdev(a_dev, whole.sum, n)
    check_adv(f"adv whole {pattern} {n}", a, n, whole, sq_whole, None).done()
    parts = [_sqdev(s, whole.sum, n) for s in shards]
    for s, got, lo in zip(shards, parts, (0, k)):
        part = a[lo:lo + s.numel()]
        check_adv(f"adv shard {pattern} {n} @{lo}", part, n, LREF.adv_stats(part, n, mean_sum=whole.sum), got, None).done()
    tol = 1e-12 * whole.sqdev * math.ceil(math.log2(n))
    total = parts[0] + parts[1]
    report("adv_sqdev", "shards", abs(total - sq_whole) / tol, 1.0)
    assert abs(total - sq_whole) <= tol and abs(total - whole.sqdev) <= tol
    norm_whole = _normalize(a_dev, whole.sum, sq_whole, n)
    check_adv(f"adv normalised {pattern} {n}", a, n, whole, None, norm_whole).done()
    for s, lo in zip(shards, (0, k)):                             # the summed value written back
        assert _same_bits(_normalize(s, whole.sum, total, n), norm_whole[lo:lo + s.numel()])


def test_gae_to_normalised_advantages_past_the_workgroup_cap():
    """dtc_gae -> dtc_adv_sqdev -> dtc_adv_normalize at T = 24, N = 11000 (264000 samples: past 1024 workgroups x 256): returns and
    raw advantages equal oracle/gae.py bit for bit, stats[0] is the float64 sum of the raw advantages (at most 24 + 6 + 4 additions
    in the scan kernel and 1 + 6 + 4 in the finishing one: 2^-53 x 64 x sum |a|), stats[1] and the output follow adv_stats of the
    kernel's own raw advantages and its own stats[0]."""
    T, N = 24, 11000
    rng = np.random.default_rng(11000)
    rewards, values = rng.standard_normal((T, N)).astype(np.float32), rng.standard_normal((T, N)).astype(np.float32)
    dones, last = (rng.random((T, N)) < 0.05).astype(np.uint8), rng.standard_normal(N).astype(np.float32)
    ret, adv = _nan(T, N, 1), _nan(T, N, 1)
    stats = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    ops.gae(_dev(rewards).view(T, N, 1), _dev(values).view(T, N, 1), _dev(dones).view(T, N, 1), _dev(last).view(N, 1), 0.99, 0.95, ret, adv, stats)
    raw_dev = adv.clone()
    ops.adv_sqdev(adv, stats, T * N)
    ops.adv_normalize(adv, stats, T * N)
    torch.cuda.synchronize()
    want_ret = OG.gae_scan(rewards, values, dones, last, 0.99, 0.95)
    assert _same_bits(ret.cpu().numpy().reshape(T, N), want_ret)
    raw = raw_dev.cpu().numpy().reshape(T, N)
    assert _same_bits(raw, (want_ret - values).astype(np.float32))
    s0, s1 = stats.cpu().tolist()
    exact = LREF.adv_stats(raw, T * N)
    tol0 = 2.0 ** -53 * 64 * float(np.abs(raw.astype(np.float64)).sum())
    report("gae", "stats[0]", abs(s0 - exact.sum) / tol0, 1.0)
    assert abs(s0 - exact.sum) <= tol0
    check_adv("gae -> sqdev -> normalize", raw, T * N, LREF.adv_stats(raw, T * N, mean_sum=s0), s1, adv.cpu().numpy().reshape(T, N)).done()
