"""One-pass mode of the operand-image GEMM family (dtc_set_h2i_passes(1), h2i.h2i_passes_as(1): hi hi' alone; csrc/gemm_h2i.hip
h2i_tile<.., PASSES = 1>, csrc/wgrad_h2i.hip wgrad_h2i_group_body<1>) -- the products of the nn.Linear stacks of
rsl_rl/rsl_rl/modules/actor_critic_decoder.py:98-188, 323-349 on 11-bit operands.

Error model.  hi = fp16(x 2^e), e from the row block's largest element: hi = x (1 + d), |d| <= 2^-11 for every element no more than
2^28 below its block's largest (smaller ones: at most 2^-39 of the block's largest).  For C = A B^T
    |C - C_exact| <= (2^-10 + 2^-22) (|A| |B|^T) + K 2^-38 max|A_m| max|B_n| + fp32 accumulation (ROW_TOL = 2e-6 per row, as in
                     three-pass mode: the accumulators are the same)
Two assertions follow, neither tuned to what the kernels deliver:
    1. exactly the hi hi' product: the hi planes of both operands formed on the CPU (oracle/h2image.py exponents / weight operands,
       oracle/wgrad_image_ref.planes), multiplied in float64; the kernel's fp32 result agrees per row to ROW_TOL of the row's largest
       element (data gradient: also < 1e-5).  A dropped stage, a wrong wait count or a stale plane fails here.
    2. against the float64 product of the ORIGINAL fp32 operands: within 1.05 x 2^-10 x (|A| |B|^T) element by element plus 2e-6 of
       the row's largest element.
Sanity: on Gaussian operands the per-row error against the true product is above 1e-5 (three passes: ~3e-7) -- the mode is on.
Everything runs inside h2i_passes_as(1); the GEMM tests run on 64-row (default) and 128-row-only tiles."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import h2image as HI
from oracle import wgrad_image_ref as WREF
from test_hip_h2i import ROW_TOL, _act, _row_err, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUE_TOL = 1.05 * 2.0 ** -10


@pytest.fixture(params=["rows64_default", "rows128_only"])
def tile_rows(request):
    """64-row tiles where the library picks them (launches of at most one 128 x 128 tile per CU) | 128-row tiles only: the SELF path."""
    from dtc_amd import _ffi
    _ffi.lib().dtc_h2i_rows64_max(-1 if request.param == "rows64_default" else 0)
    yield request.param
    _ffi.lib().dtc_h2i_rows64_max(-1)


@pytest.fixture(autouse=True)
def one_pass():
    from dtc_amd import h2i
    with h2i.h2i_passes_as(1):
        yield
    assert h2i.h2i_passes() == 3


# ---------------------------------------------------------------- hi planes on the CPU
def _hi(A, ex):
    """float64 values of the hi plane of A [M, K] under the exponents ex [row tiles, k blocks, 128]: fp16(x 2^e) 2^-e"""
    A = np.asarray(A, dtype=np.float32)
    hi, _ = WREF.planes(A, ex)
    rt, kb = ex.shape[:2]
    e = np.where(ex == HI.EZERO, 0, ex).transpose(0, 2, 1).reshape(rt * 128, kb)
    v = np.ldexp(hi.astype(np.float64).reshape(rt * 128, kb, 128), -e[:, :, None]).reshape(rt * 128, kb * 128)
    return torch.from_numpy(v[:A.shape[0], :A.shape[1]].copy())


def hi_rows(X):
    X = X.float().cpu().numpy()
    return _hi(X, HI.exponents(X))


def hi_weights(W, trans, rows, ranges):
    """hi planes of the weight image's operand, one [rows, cw] float64 block per (row range, column range): out[row range][column range]"""
    out = [[] for _ in rows]
    for P in HI.weight_operand(W.float().cpu().numpy(), trans, rows, ranges):
        v, r0 = _hi(P, HI.weight_exponents(P)), 0
        for i, (_, nr) in enumerate(rows):
            out[i].append(v[r0:r0 + nr])
            r0 += -(-nr // 128) * 128
    return out


def _assert_rows(y, ref_hi, ref_true, absprod, what, dgrad=False):
    """assertions 1 and 2 of the module text on the fp32 result y"""
    e1 = _row_err(y, ref_hi)
    y, ref_true = y.double().cpu(), ref_true.double().cpu()
    err = (y - ref_true).abs()
    bound = TRUE_TOL * absprod + 2e-6 * ref_true.abs().amax(dim=1, keepdim=True)
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"onepass {what}: vs hi hi' per row {e1:.2e} (tolerance {ROW_TOL:.0e}); vs true product {worst:.3f} of its bound; "
          f"per-row error vs true {_row_err(y, ref_true):.2e}")
    assert e1 < ROW_TOL and (not dgrad or e1 < 1e-5), (what, e1)
    assert bool((err <= bound).all()), (what, worst)


def _block_max(Y, N):
    M = Y.shape[0]
    blk = torch.zeros(M, -(-N // 128) * 128, device=Y.device)
    blk[:, :N] = Y.abs()
    return blk.view(M, -1, 128).amax(dim=2, keepdim=True).expand(-1, -1, 128).reshape(M, -1)[:, :N]


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("M,N,K,act", [(130, 128, 265, "relu"), (384, 512, 693, "relu"), (300, 693, 512, None), (1024, 512, 512, "relu"),
                                       (512, 35, 64, None)])
def test_forward_is_the_hi_product(tile_rows, M, N, K, act):
    from dtc_amd import h2i, ops
    assert h2i.h2i_passes() == 1
    g = torch.Generator().manual_seed(M + N + 3 * K)
    X = _rows(M, K, g, span=12, zero_frac=0.05)                  # rows over 12 decades: the 128-column borders rescale
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) * 1e-13                      # (a bias would swamp the small rows' products)
    hw = hi_weights(W, 0, [(0, N)], [(0, K)])[0][0]
    ref_hi = _act(hi_rows(X) @ hw.T + b.double(), act)
    ref = _act(X.double() @ W.double().T + b.double(), act)
    Xd, Wd, bd = X.to(DEV), W.to(DEV), b.to(DEV)
    Y = torch.full((M, N), float("nan"), device=DEV)
    Yimg = h2i.HImage(M, N, DEV)
    mask = ops.relu_mask(M, N, DEV) if (act == "relu" and ops.relu_mask_ok(M, N)) else None
    h2i.linear_fwd(h2i.HImage.from_tensor(Xd), Wd, bd, Y, Yimg, act, mask=mask)
    _assert_rows(Y, ref_hi, ref, X.double().abs() @ W.double().abs().T, f"fwd {M}x{N}x{K}")
    # sign record and image: the producers are unchanged
    if mask is not None:
        assert torch.equal(h2i.unpack_sign_record(mask, M, N), Y > 0)
    assert bool(((Yimg.to_tensor() - Y).abs() <= _block_max(Y, N) * 2.0 ** -21).all())
    if (M, N, K) == (1024, 512, 512):                            # image only (no fp32 result) gives the same image
        Yimg2 = h2i.HImage(M, N, DEV)
        h2i.linear_fwd(h2i.HImage.from_tensor(Xd), Wd, bd, None, Yimg2, act)
        assert torch.equal(Yimg2.buf, Yimg.buf)


def test_forward_two_operand_images_and_column_map(tile_rows):
    """the actor's first layer: [l_t image | packed narrow block image] against W's columns [72:584 | 0:72]"""
    from dtc_amd import h2i
    g = torch.Generator().manual_seed(11)
    M = 640
    lt, nb = _rows(M, 512, g, span=12, zero_frac=0.05), torch.randn(M, 72, generator=g) * 3
    W, b = torch.randn(512, 584, generator=g) / 24, torch.randn(512, generator=g) * 1e-13
    cat = torch.cat([nb, lt], 1).double()
    ref = torch.nn.functional.elu(cat @ W.double().T + b.double())
    hw = hi_weights(W, 0, [(0, 512)], [(72, 512), (0, 72)])[0]
    ref_hi = torch.nn.functional.elu(hi_rows(lt) @ hw[0].T + hi_rows(nb) @ hw[1].T + b.double())
    Y = torch.empty(M, 512, device=DEV)
    h2i.linear_fwd([h2i.HImage.from_tensor(lt.to(DEV)), h2i.HImage.from_tensor(nb.to(DEV))], W.to(DEV), b.to(DEV), Y, None, "elu", cols=[72, 0])
    _assert_rows(Y, ref_hi, ref, cat.abs() @ W.double().abs().T, "fwd two images 640x512x(512 + 72)")


def test_gaussian_operands_show_one_pass(tile_rows):
    """the mode really is one pass: on Gaussian operands the per-row error against the true product is above 1e-5 (three passes: ~3e-7),
    and the same call outside the block is back below ROW_TOL"""
    from dtc_amd import h2i
    g = torch.Generator().manual_seed(77)
    M, N, K = 1024, 512, 512
    X, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    ref = X.double() @ W.double().T
    Xi, Wd = h2i.HImage.from_tensor(X.to(DEV)), W.to(DEV)
    Y1, Y3 = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    h2i.linear_fwd(Xi, Wd, None, Y1, None, None)
    with h2i.h2i_passes_as(3):
        h2i.linear_fwd(Xi, Wd, None, Y3, None, None)
    e1, e3 = _row_err(Y1, ref), _row_err(Y3, ref)
    print(f"onepass sanity {M}x{N}x{K}: per-row error vs true, one pass {e1:.2e}, three passes {e3:.2e}")
    assert e1 > 1e-5 and e3 < ROW_TOL


# ---------------------------------------------------------------- fused MSE layer
def test_fused_mse_layer(tile_rows):
    from dtc_amd import h2i
    M, N, K = 300, 693, 512
    g = torch.Generator().manual_seed(M)
    X, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    T = torch.randn(2 * M, 1389, generator=g)
    idx = torch.randint(0, 2 * M, (M,), generator=g)
    tgt = T[idx][:, 696:696 + N].double()
    e = (X.double() @ W.double().T + b.double()) - tgt
    e_hi = (hi_rows(X) @ hi_weights(W, 0, [(0, N)], [(0, K)])[0][0].T + b.double()) - tgt
    absprod = X.double().abs() @ W.double().abs().T
    dY = torch.empty(M, N, device=DEV)
    dYimg = h2i.HImage(M, N, DEV)
    part = torch.zeros(h2i.mse_parts(M, N), dtype=torch.float64, device=DEV)
    n = h2i.linear_fwd_mse(h2i.HImage.from_tensor(X.to(DEV)), W.to(DEV), b.to(DEV), T.to(DEV), 696, idx.to(DEV), dY, dYimg, part)
    s = 2.0 / (M * N)
    _assert_rows(dY, e_hi * s, e * s, absprod * s, f"fused mse {M}x{N}x{K}")
    # the loss: every e is within d = TRUE_TOL x absprod + 2e-6 x its row's largest |e| of the true one (assertion 2), so
    # |sum e_k^2 - sum e^2| <= sum d (2 |e| + d); against the hi hi' residuals: the fp32 rounding of e alone
    d = TRUE_TOL * absprod + 2e-6 * e.abs().amax(dim=1, keepdim=True)
    got, want = float(part[:n].sum()), float((e * e).sum())
    print(f"onepass fused mse loss: {got:.9e} vs true {want:.9e} (bound {float((d * (2 * e.abs() + d)).sum()):.2e}), vs hi hi' {float((e_hi * e_hi).sum()):.9e}")
    assert abs(got - want) <= float((d * (2 * e.abs() + d)).sum())
    assert abs(got - float((e_hi * e_hi).sum())) <= 1e-6 * float((e_hi * e_hi).sum())
    assert float((dYimg.to_tensor() - dY).abs().max()) <= 2.0 ** -21 * float(dY.abs().max())


# ---------------------------------------------------------------- data gradient
@pytest.mark.parametrize("M,N,K,mode", [(1024, 512, 512, "mask"), (640, 256, 512, "elu"), (512, 53, 128, "mask"), (256, 64, 531, "none")])
def test_dgrad_heavy_tailed_rows(tile_rows, M, N, K, mode):
    """dX = (dZ W) act'(.), dZ rows log-uniform over 1e-8 .. 1 of the largest, 30 % of them exactly zero"""
    from dtc_amd import h2i, ops
    g = torch.Generator().manual_seed(M + N + K)
    dZ = _rows(M, N, g, span=8, zero_frac=0.3)
    W = torch.randn(N, K, generator=g) / N ** 0.5
    Xs = torch.randn(M, K, generator=g)
    ref = dZ.double() @ W.double()
    ref_hi = hi_rows(dZ) @ hi_weights(W, 1, [(0, K)], [(0, N)])[0][0].T
    kw = dict()
    if mode == "mask":
        mask = ops.relu_mask(M, K, DEV)
        Yf = torch.empty(M, K, device=DEV)
        # the sign record as the forward kernel writes it: a ReLU layer whose pre-activation is Xs (fp16 rounding keeps the signs)
        h2i.linear_fwd(h2i.HImage.from_tensor(Xs.to(DEV)), torch.eye(K, device=DEV), None, Yf, None, "relu", mask=mask)
        assert torch.equal(Yf.cpu() > 0, Xs > 0)
        keep = (Xs > 0).double()
        ref, ref_hi = ref * keep, ref_hi * keep
        kw = dict(mask=mask)
    elif mode == "elu":
        Ys = torch.nn.functional.elu(Xs)
        bw = lambda r: torch.where(Ys.double() > 0, r, r * (Ys.double() + 1.0))       # (a factor in (0, 1]: the bound of the product holds)
        ref, ref_hi = bw(ref), bw(ref_hi)
        kw = dict(Xsaved=Ys.to(DEV), act="elu")
    dX = torch.full((M, K), float("nan"), device=DEV)
    dXimg = h2i.HImage(M, K, DEV)
    h2i.linear_dgrad(h2i.HImage.from_tensor(dZ.to(DEV)), W.to(DEV), dX, dXimg, **kw)
    _assert_rows(dX, ref_hi, ref, dZ.double().abs() @ W.double().abs(), f"dgrad {M}x{N}x{K} {mode}", dgrad=True)
    assert bool(((dXimg.to_tensor() - dX).abs() <= _block_max(dX, K) * 2.0 ** -21).all())


def test_dgrad_window_add_and_segmented_destination(tile_rows):
    """the actor's first layer backward (tests/test_hip_h2i.py, same call): window [72, 584) -> d l_t as an image with a second fp32
    contribution added first; window [53, 72) -> dz (16) | d mu (3, accumulating); both windows in one launch"""
    from dtc_amd import h2i
    from dtc_amd._ffi import seg, segmat
    g = torch.Generator().manual_seed(3)
    M = 512
    dZ, W = torch.randn(M, 512, generator=g), torch.randn(512, 584, generator=g) / 22
    other = torch.randn(M, 512, generator=g)
    full, absfull = dZ.double() @ W.double(), dZ.double().abs() @ W.double().abs()
    hz = hi_rows(dZ)
    hw = hi_weights(W, 1, [(72, 512), (53, 19)], [(0, 512)])
    lt_hi, nar_hi = hz @ hw[0][0].T, hz @ hw[1][0].T
    # (one window alone: its weight image is the same rows of W^T with their own exponents -- a row's exponent block is its own 128 rows)
    assert torch.equal(hi_weights(W, 1, [(72, 512)], [(0, 512)])[0][0], hw[0][0])
    dZi, Wd = h2i.HImage.from_tensor(dZ.to(DEV)), W.to(DEV)
    dlt = h2i.HImage(M, 512, DEV)
    h2i.linear_dgrad(dZi, Wd, None, dlt, window=(72, 512), add=other.to(DEV))
    want = full[:, 72:] + other.double()
    got = dlt.to_tensor()
    # (the image adds 2^-22 of the row block's largest element: inside ROW_TOL and the 2e-6 of assertion 2)
    _assert_rows(got, lt_hi + other.double(), want, absfull[:, 72:], "dgrad window [72, 584) + add -> image", dgrad=True)
    dz, dmu = torch.full((M, 16), float("nan"), device=DEV), torch.ones(M, 35, device=DEV)
    nar1 = hi_weights(W, 1, [(53, 19)], [(0, 512)])[0][0]
    h2i.linear_dgrad(dZi, Wd, segmat([seg(dz, 0, 16), seg(dmu, 0, 3, accumulate=True)]), None, window=(53, 19))
    n1 = hz @ nar1.T
    _assert_rows(dz, n1[:, :16], full[:, 53:69], absfull[:, 53:69], "dgrad window [53, 69) -> dz", dgrad=True)
    _assert_rows(dmu[:, :3], n1[:, 16:] + 1.0, full[:, 69:72] + 1.0, absfull[:, 69:72], "dgrad window [69, 72) -> d mu (accumulating)", dgrad=True)
    assert float((dmu[:, 3:] - 1).abs().max()) == 0.0
    # both windows in ONE launch: four image tiles + one fp32 tile
    dlt2 = h2i.HImage(M, 512, DEV)
    dz2, dmu2 = torch.full((M, 16), float("nan"), device=DEV), torch.zeros(M, 35, device=DEV)
    h2i.linear_dgrad(dZi, Wd, segmat([seg(None, 0, 512), seg(dz2, 0, 16), seg(dmu2, 0, 3)]), dlt2, window=[(72, 512), (53, 19)])
    _assert_rows(dlt2.to_tensor(), lt_hi, full[:, 72:], absfull[:, 72:], "dgrad two windows -> image", dgrad=True)
    _assert_rows(dz2, nar_hi[:, :16], full[:, 53:69], absfull[:, 53:69], "dgrad two windows -> dz", dgrad=True)
    _assert_rows(dmu2[:, :3], nar_hi[:, 16:], full[:, 69:72], absfull[:, 69:72], "dgrad two windows -> d mu", dgrad=True)
    assert float(dmu2[:, 3:].abs().max()) == 0.0


# ---------------------------------------------------------------- chains
def test_encoder_chains_equal_the_per_layer_one_pass_launches_bit_for_bit(tile_rows):
    """the CE-net encoder 265 -> 128 (ReLU, sign record) -> 64 -> 35 as one forward launch, and d mulv -> head^T -> ce1^T (sign record)
    as one data-gradient launch, M = 384: every result equals the per-layer one-pass calls bit for bit -- and differs from three passes"""
    from dtc_amd import h2i, ops
    M = 384
    g = torch.Generator().manual_seed(41)
    w = lambda n, k: (torch.randn(n, k, generator=g) / k ** 0.5).to(DEV)
    bias = lambda n: torch.randn(n, generator=g).to(DEV)
    hist = h2i.HImage.from_tensor(_rows(M, 265, g, span=3).to(DEV))
    We, be = [w(128, 265), w(64, 128), w(35, 64)], [bias(128), bias(64), bias(35)]
    dm = h2i.HImage.from_tensor(_rows(M, 35, g, span=5, zero_frac=0.2).to(DEV))

    def run(chain):
        e1, e = h2i.HImage(M, 128, DEV), h2i.HImage(M, 64, DEV)
        m1 = ops.relu_mask(M, 128, DEV).zero_()
        mulv = torch.zeros(M, 35, device=DEV)
        enc = [dict(X=hist, W=We[0], b=be[0], Yimg=e1, act="relu", mask=m1), dict(X=e1, W=We[1], b=be[1], Yimg=e),
               dict(X=e, W=We[2], b=be[2], Y=mulv)]
        g_head, g_ce1 = h2i.HImage(M, 64, DEV), h2i.HImage(M, 128, DEV)
        benc = [dict(dZimg=dm, W=We[2], dXimg=g_head), dict(dZimg=g_head, W=We[1], dXimg=g_ce1, mask=m1)]
        if chain:
            h2i.linear_fwd_chain(enc)
            h2i.linear_dgrad_chain(benc)
        else:
            for L in enc:
                h2i.linear_fwd(L["X"], L["W"], L.get("b"), L.get("Y"), L.get("Yimg"), L.get("act"), L.get("mask"))
            for L in benc:
                h2i.linear_dgrad(L["dZimg"], L["W"], None, L["dXimg"], mask=L.get("mask"))
        torch.cuda.synchronize()
        return [t.clone() for t in (e1.buf, e.buf, m1, mulv, g_head.buf, g_ce1.buf)]

    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t
    a, b = run(True), run(False)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(bits(x), bits(y)), i
    assert float(a[3].abs().max()) > 0
    with h2i.h2i_passes_as(3):
        c = run(True)
    assert not torch.equal(bits(a[0]), bits(c[0])) and not torch.equal(bits(a[5]), bits(c[5]))


# ---------------------------------------------------------------- weight gradients
def _wgrad_rows(M, C, g, block_steps):
    """rows of a 128-row block within 2^4 of each other (dZ and X together: 2^8, the factors f stay normal fp16); the blocks step
    through `block_steps` octaves so that the accumulators change scale at the block borders"""
    s = torch.exp2(-4.0 * torch.rand(M, 1, generator=g))
    blk = torch.tensor([block_steps[(m // 128) % len(block_steps)] for m in range(M)], dtype=torch.float32)[:, None]
    return torch.randn(M, C, generator=g) * s * torch.exp2(-blk)


@pytest.mark.parametrize("M", [384, 4101])
def test_wgrad_group_is_the_hi_product(M):
    """two jobs, (N, K) = (128, 265) and (53, 128); M = 384 (one 128-row block per batch slice) and 4101 (two blocks per slice -- the
    smallest such M of tests/test_hip_wgrad_image.py -- and a ragged last block): dW and db by assertions 1 and 2"""
    from dtc_amd import h2i, ops
    g = torch.Generator().manual_seed(M)
    shapes = [(128, 265), (53, 128)]
    assert WREF.slices(M, sum(-(-N // 128) * -(-K // 128) for N, K in shapes))[1] // 128 == (1 if M == 384 else 2)
    jobs, data = [], []
    for N, K in shapes:
        dZ, X = _wgrad_rows(M, N, g, (0, 5, 2, 9)), _wgrad_rows(M, K, g, (0,))
        dW, db = torch.full((N, K + 8), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
        jobs.append((h2i.HImage.from_tensor(dZ.to(DEV)), h2i.HImage.from_tensor(X.to(DEV)), dW, 8, db))
        data.append((dZ, X))
    h2i.wgrad_group(jobs, M, ops.workspace(h2i.wgrad_group_workspace_bytes(jobs, M), DEV))
    for (dZi, Xi, dW, c0, db), (dZ, X) in zip(jobs, data):
        hz, hx = hi_rows(dZ), hi_rows(X)
        what = f"wgrad {M}x{dZi.K}x{Xi.K}"
        _assert_rows(dW[:, c0:], hz.T @ hx, dZ.double().T @ X.double(), dZ.double().abs().T @ X.double().abs(), what)
        assert bool(torch.isnan(dW[:, :c0]).all())                      # columns outside the job's window are untouched
        # bias: db = dZ^T 1 -- the same two assertions with B = a row of ones, per feature against its own sum of magnitudes
        got, rb_hi, rb, sb = db.double().cpu(), hz.sum(0), dZ.double().sum(0), dZ.double().abs().sum(0)
        e1 = float(((got - rb_hi).abs() / hz.abs().sum(0).clamp_min(1e-300)).max())
        print(f"onepass {what}: bias vs hi plane {e1:.2e} of the feature's sum of magnitudes; vs true {float(((got - rb).abs() / sb).max()):.2e}")
        assert e1 < ROW_TOL
        assert bool(((got - rb).abs() <= TRUE_TOL * sb + 2e-6 * rb.abs().max()).all())


# ---------------------------------------------------------------- containment
def test_non_finite_elements_stay_in_their_rows(tile_rows):
    from dtc_amd import h2i
    g = torch.Generator().manual_seed(9)
    M, N, K = 384, 512, 693
    X, W = torch.randn(M, K, generator=g), (torch.randn(N, K, generator=g) / 26).to(DEV)
    Xb = X.clone()
    Xb[7, 100] = float("nan")
    Xb[300, 5] = float("inf")
    bad = torch.zeros(M, dtype=torch.bool, device=DEV)
    bad[[7, 300]] = True
    Y0, Y1 = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    I0, I1 = h2i.HImage(M, N, DEV), h2i.HImage(M, N, DEV)
    h2i.linear_fwd(h2i.HImage.from_tensor(X.to(DEV)), W, None, Y0, I0, "elu")
    h2i.linear_fwd(h2i.HImage.from_tensor(Xb.to(DEV)), W, None, Y1, I1, "elu")
    assert torch.equal(Y0[~bad].view(torch.int32), Y1[~bad].view(torch.int32))                    # every other row: bit-identical
    assert bool(torch.isfinite(Y0).all())
    nonfinite_rows = ~torch.isfinite(Y1).all(dim=1)
    assert torch.equal(nonfinite_rows, bad)                                                       # exactly the rows that hold them
    assert torch.equal(I0.to_tensor()[~bad], I1.to_tensor()[~bad])


# ---------------------------------------------------------------- switch hygiene
_NEVER_SWITCHED = r"""
import sys
sys.path[:0] = [ROOT, ROOT + "/deep-tracking-control_amd", ROOT + "/tests"]
import torch
from dtc_amd import _ffi
assert _ffi.lib().dtc_get_h2i_passes() == 3                      # at load
import test_hip_h2i_onepass as T
fw, dW, db = T._hygiene_results()
torch.save(dict(fw=fw.cpu(), dW=dW.cpu(), db=db.cpu()), sys.argv[1])
assert _ffi.lib().dtc_get_h2i_passes() == 3
"""


def _hygiene_results():
    """forward 1024 x 512 x 512 and the weight gradient of a 384-row batch at whatever the library's setting is"""
    from dtc_amd import h2i, ops
    g = torch.Generator().manual_seed(2024)
    M, N, K = 1024, 512, 512
    X, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    Y = torch.empty(M, N, device=DEV)
    h2i.linear_fwd(h2i.HImage.from_tensor(X.to(DEV)), W.to(DEV), b.to(DEV), Y, None, "relu")
    dZ, Xw = torch.randn(384, 128, generator=g), torch.randn(384, 265, generator=g)
    dW, db = torch.empty(128, 265, device=DEV), torch.empty(128, device=DEV)
    jobs = [(h2i.HImage.from_tensor(dZ.to(DEV)), h2i.HImage.from_tensor(Xw.to(DEV)), dW, 0, db)]
    h2i.wgrad_group(jobs, 384, ops.workspace(h2i.wgrad_group_workspace_bytes(jobs, 384), DEV))
    torch.cuda.synchronize()
    return Y, dW, db


def test_switch_hygiene(tmp_path):
    """after h2i_passes_as(1) exits the results are those of a process that never switched, bit for bit; a value other than 1 or 3 is
    refused and changes nothing; the library loads with 3"""
    from dtc_amd import _ffi, h2i
    lib = _ffi.lib()
    assert lib.dtc_get_h2i_passes() == 1                          # (the autouse block of this file)
    one = _hygiene_results()
    lib.dtc_set_h2i_passes(2)
    assert lib.dtc_get_h2i_passes() == 1 and b"dtc_set_h2i_passes(2)" in lib.dtc_last_error()
    with pytest.raises(ValueError):
        h2i.set_h2i_passes(2)
    with h2i.h2i_passes_as(3):
        lib.dtc_set_h2i_passes(0)
        assert lib.dtc_get_h2i_passes() == 3
        with pytest.raises(RuntimeError), h2i.h2i_passes_as(1):   # an exception inside the block: the setting is restored
            assert h2i.h2i_passes() == 1
            raise RuntimeError("inside")
        assert h2i.h2i_passes() == 3
        back = _hygiene_results()
    out = tmp_path / "never_switched.pt"
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + _NEVER_SWITCHED, str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    ref = torch.load(out)
    for name, got, o in zip(("fw", "dW", "db"), back, one):
        assert torch.equal(got.cpu().view(torch.int32), ref[name].view(torch.int32)), name
        assert not torch.equal(o.cpu().view(torch.int32), ref[name].view(torch.int32)), name      # (and one pass is something else)
