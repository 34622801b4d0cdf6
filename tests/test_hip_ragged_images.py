"""Operand-image kernels at row counts that are no multiple of the 128-row tile (csrc/h2i_core.hpp "Tail rows"; the nn.Linear stacks
of rsl_rl/rsl_rl/modules/actor_critic_decoder.py:98-188 at the reference's own mini-batch sizes: 600, 192 and 48 rows):

  * ReLU sign records at any M, forward and data gradient, both row-tile instantiations (every test runs on 64-row and on 128-row tiles);
  * the chains against the per-layer launches, with records;
  * no result for a row < M, and no weight gradient, depends on the planes of the rows >= M of an image's last row tile;
  * the weight gradient over M = 300 rows against M = 384 with 84 all-zero dZ rows.

M in {1, 100, 130, 300}: a lone partial tile (64 or 128 rows), a 32-row group that straddles M (100 = 3 x 32 + 4, 130 = 4 x 32 + 2,
300 = 9 x 32 + 12), a full tile plus a tail.  Widths 512 x 512 and the 64-column form (64 x 531 forward, 128 -> 64 backward)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROW_TOL = 2e-6          # the per-row bound of tests/test_hip_h2i.py
MS = [1, 100, 130, 300]
SENTINEL = 0x1234


@pytest.fixture(autouse=True, params=["rows64_default", "rows128_only"])
def tile_rows(request):
    """Every test runs on 64-row tiles where the library picks them (64 < M, few tiles) and on 128-row tiles only."""
    from dtc_amd import _ffi
    _ffi.lib().dtc_h2i_rows64_max(-1 if request.param == "rows64_default" else 0)
    yield request.param
    _ffi.lib().dtc_h2i_rows64_max(-1)


def _rows(M, K, g, span=6, zero_frac=0.0):
    X = torch.randn(M, K, generator=g) * 10.0 ** (-span * torch.rand(M, 1, generator=g))
    if zero_frac:
        X[torch.rand(M, generator=g) < zero_frac] = 0.0
    return X


def _row_err(y, ref):
    y, ref = y.double().cpu(), ref.double().cpu()
    num, den = (y - ref).abs().amax(dim=1), ref.abs().amax(dim=1)
    zero = den == 0
    assert float(num[zero].max() if zero.any() else 0.0) == 0.0
    return float((num[~zero] / den[~zero]).max()) if (~zero).any() else 0.0


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _planes(img):
    """the plane bytes of an image as int16 [row tile, stage, plane, row in tile, 16]: a row's two 16-byte slots are adjacent (rslot)"""
    rt, st = -(-img.M // 128), -(-img.K // 16)
    return img.buf.view(torch.int16)[: rt * st * 4096].view(rt, st, 2, 128, 16)


def _nan_tails(img):
    """fp16 NaN (0x7e00) into the planes of the rows >= M of the last row tile; the exponent entries stay as they are"""
    if img.M % 128:
        _planes(img)[-1, :, :, img.M % 128:, :] = 0x7e00
    return img


def _stale_result_tail(img):
    """a result image as a reused workspace buffer may hold it: fp16 NaN planes and a live exponent in the rows M .. 64 ceil(M / 64) - 1
    -- the tail rows every launch visits.  (On 64-row tiles a 64-row half of the last row tile that lies wholly behind M belongs to no
    workgroup: it stays as allocated -- zeros, HI_EZERO --, which the callers below assert as well.)"""
    lo, hi = img.M % 128, -(-img.M // 64) * 64 - (img.M // 128) * 128
    _planes(img)[-1, :, :, lo:hi, :] = 0x7e00
    img.exps()[-1, :, lo:hi] = 5
    return img


def _copy(img):
    from dtc_amd import h2i
    out = h2i.HImage(img.M, img.K, DEV)
    out.buf.copy_(img.buf)
    return out


def _decode_tile_rows(img):
    """all 128 ceil(M / 128) rows of the image as fp32 (dtc_h2i_unpack on the tile-rounded row count: same tiles, same exponent table)"""
    from dtc_amd import _ffi
    rows = -(-img.M // 128) * 128
    out = torch.full((rows, img.K), float("nan"), device=DEV)
    _ffi.check(_ffi.lib().dtc_h2i_unpack(img.ptr(), rows, img.K, _ffi.ptr(out), out.stride(0), _ffi.stream()), "dtc_h2i_unpack")
    return out


def _tail_exps(img):
    return img.exps()[-1, :, img.M % 128:] if img.M % 128 else img.exps()[:0]


def _guarded_record(M, N):
    """a sign record of exactly dtc_relu_mask_elems(M, N) words inside a larger buffer of sentinel words, every word preset to all ones"""
    from dtc_amd import _ffi
    n = int(_ffi.lib().dtc_relu_mask_elems(M, N))
    assert n == -(-M // 32) * 2 * N
    big = torch.full((n + 8 * N,), SENTINEL, dtype=torch.int16, device=DEV)
    big[:n] = -1
    return big[:n], big[n:]


@pytest.mark.parametrize("N,K", [(512, 512), (64, 531)])
@pytest.mark.parametrize("M", MS)
def test_forward_writes_a_sign_record_at_any_row_count(M, N, K):
    """rows < M within 2e-6 of float64 per row; the record = (y > 0) of the kernel's own fp32 output exactly for rows < M, 0 bits for
    the rows >= M of the last 32-row group, no word behind ceil(M / 32) groups; the result image holds zeros / HI_EZERO behind M"""
    from dtc_amd import h2i
    g = torch.Generator().manual_seed(7 * M + N)
    X, W, b = _rows(M, K, g, zero_frac=0.05), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g) * 1e-9
    ref = torch.relu(X.double() @ W.double().T + b.double())
    Y = torch.full((M, N), float("nan"), device=DEV)
    Yimg = h2i.HImage(M, N, DEV)
    _stale_result_tail(Yimg)
    mask, guard = _guarded_record(M, N)
    h2i.linear_fwd(h2i.HImage.from_tensor(X.to(DEV)), W.to(DEV), b.to(DEV), Y, Yimg, "relu", mask=mask)
    err = _row_err(Y, ref)
    print(f"ragged fwd {M}x{N}x{K}: per-row err {err:.2e}")
    assert err < ROW_TOL
    rec = h2i.unpack_sign_groups(mask, M, N)
    assert rec.shape[0] == -(-M // 32) * 32
    assert torch.equal(rec[:M], Y > 0) and torch.equal(h2i.unpack_sign_record(mask, M, N), Y > 0)
    assert not bool(rec[M:].any())
    assert bool((guard == SENTINEL).all())
    dec = _decode_tile_rows(Yimg)
    assert float(dec[M:].abs().max()) == 0.0 and bool((_tail_exps(Yimg) == 0x7fff).all())
    assert float((dec[:M] - Y).abs().max()) <= 2.0 ** -21 * float(Y.abs().max())


@pytest.mark.parametrize("N,K", [(512, 512), (128, 64)])
@pytest.mark.parametrize("M", MS)
def test_dgrad_reads_the_sign_record_at_any_row_count(M, N, K):
    """dX = (dZ W) masked by the record of a [M, K] ReLU output: bit for bit the unmasked launch with the masked entries set to 0; the
    rows >= M of the dX image decode to zeros with HI_EZERO exponents, whatever the image held before"""
    from dtc_amd import h2i
    g = torch.Generator().manual_seed(11 * M + K)
    dZ, W = _rows(M, N, g, span=8, zero_frac=0.3), torch.randn(N, K, generator=g) / N ** 0.5
    pre = torch.randn(M, K, generator=g)
    mask, guard = _guarded_record(M, K)
    Yf = torch.empty(M, K, device=DEV)
    h2i.linear_fwd(h2i.HImage.from_tensor(pre.to(DEV)), torch.eye(K, device=DEV), None, Yf, None, "relu", mask=mask)
    dZi, Wd = h2i.HImage.from_tensor(dZ.to(DEV)), W.to(DEV)
    plain, masked = torch.full((M, K), float("nan"), device=DEV), torch.full((M, K), float("nan"), device=DEV)
    img_plain, img_masked = h2i.HImage(M, K, DEV), h2i.HImage(M, K, DEV)
    _stale_result_tail(img_masked)
    h2i.linear_dgrad(dZi, Wd, plain, img_plain)
    h2i.linear_dgrad(dZi, Wd, masked, img_masked, mask=mask)
    want = torch.where(Yf > 0, plain, torch.zeros_like(plain))
    assert torch.equal(_bits(masked), _bits(want))
    assert 0 < int((Yf > 0).sum()) < Yf.numel() or M == 1
    assert _row_err(masked, (dZ.double() @ W.double()) * (Yf.double().cpu() > 0)) < ROW_TOL
    dec = _decode_tile_rows(img_masked)
    assert float(dec[M:].abs().max()) == 0.0 and bool((_tail_exps(img_masked) == 0x7fff).all())
    assert float((dec[:M] - masked).abs().max()) <= 2.0 ** -21 * float(masked.abs().max())
    assert bool((guard == SENTINEL).all())


def test_chains_with_sign_records_equal_the_per_layer_launches_at_200_rows():
    """M = 200 (a full tile + 72 rows; 64-row tiles: three full + 8 rows): the CE-net's narrow stacks (64-column record form included) and
    a wide 512 -> 256 -> 128 ReLU stack, forward and data gradient, as ONE launch per direction -- images, exponents, fp32 outputs and
    sign records equal the per-layer launches bit for bit"""
    from dtc_amd import h2i, ops
    M = 200
    g = torch.Generator().manual_seed(41)
    w = lambda n, k: (torch.randn(n, k, generator=g) / k ** 0.5).to(DEV)
    bias = lambda n: torch.randn(n, generator=g).to(DEV)
    hist = h2i.HImage.from_tensor(_rows(M, 265, g, span=3).to(DEV))
    zmu, lt = h2i.HImage.from_tensor(torch.randn(M, 19, generator=g).to(DEV)), h2i.HImage.from_tensor(_rows(M, 512, g, span=2).to(DEV))
    We, be = [w(128, 265), w(64, 128), w(35, 64)], [bias(128), bias(64), bias(35)]
    Wd, bd = [w(64, 531), w(128, 64), w(53, 128)], [bias(64), bias(128), bias(53)]
    Ww, bw = [w(256, 512), w(128, 256)], [bias(256), bias(128)]
    dm = h2i.HImage.from_tensor(_rows(M, 35, g, span=5, zero_frac=0.2).to(DEV))
    dr = h2i.HImage.from_tensor(_rows(M, 53, g, span=5).to(DEV))
    G3 = h2i.HImage.from_tensor(_rows(M, 128, g, span=5, zero_frac=0.1).to(DEV))

    def run(chain):
        fwd = h2i.linear_fwd_chain if chain else (lambda Ls: [h2i.linear_fwd(L["X"], L["W"], L.get("b"), L.get("Y"), L.get("Yimg"), L.get("act"),
                                                                            L.get("mask")) for L in Ls])
        bwd = h2i.linear_dgrad_chain if chain else (lambda Ls: [h2i.linear_dgrad(L["dZimg"], L["W"], None, L["dXimg"], mask=L.get("mask")) for L in Ls])
        rec = lambda n: ops.relu_mask(M, n, DEV).zero_()
        e1, e, c1, c2, a2, a3 = (h2i.HImage(M, n, DEV) for n in (128, 64, 64, 128, 256, 128))
        m1, mc1, mc2, ma2, ma3 = rec(128), rec(64), rec(128), rec(256), rec(128)
        mulv, recon, o3 = torch.zeros(M, 35, device=DEV), torch.zeros(M, 53, device=DEV), torch.zeros(M, 128, device=DEV)
        fwd([dict(X=hist, W=We[0], b=be[0], Yimg=e1, act="relu", mask=m1), dict(X=e1, W=We[1], b=be[1], Yimg=e), dict(X=e, W=We[2], b=be[2], Y=mulv)])
        fwd([dict(X=[zmu, lt], W=Wd[0], b=bd[0], Yimg=c1, act="relu", mask=mc1), dict(X=c1, W=Wd[1], b=bd[1], Yimg=c2, act="relu", mask=mc2),
             dict(X=c2, W=Wd[2], b=bd[2], Y=recon)])
        fwd([dict(X=lt, W=Ww[0], b=bw[0], Yimg=a2, act="relu", mask=ma2), dict(X=a2, W=Ww[1], b=bw[1], Y=o3, Yimg=a3, act="relu", mask=ma3)])
        g_head, g_ce1, g_cd2, g_cd1, g_a2, g_lt = (h2i.HImage(M, n, DEV) for n in (64, 128, 128, 64, 256, 512))
        bwd([dict(dZimg=dm, W=We[2], dXimg=g_head), dict(dZimg=g_head, W=We[1], dXimg=g_ce1, mask=m1)])
        bwd([dict(dZimg=dr, W=Wd[2], dXimg=g_cd2, mask=mc2), dict(dZimg=g_cd2, W=Wd[1], dXimg=g_cd1, mask=mc1)])
        bwd([dict(dZimg=G3, W=Ww[1], dXimg=g_a2, mask=ma2), dict(dZimg=g_a2, W=Ww[0], dXimg=g_lt)])
        torch.cuda.synchronize()
        return [t.clone() for t in (e1.buf, e.buf, c1.buf, c2.buf, a2.buf, a3.buf, m1, mc1, mc2, ma2, ma3, mulv, recon, o3, g_head.buf, g_ce1.buf,
                                    g_cd2.buf, g_cd1.buf, g_a2.buf, g_lt.buf)]

    a, b = run(True), run(False)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(_bits(x), _bits(y)), i
    assert all(float(a[i].abs().max()) > 0 for i in (11, 12, 13)) and all(bool(a[i].ne(0).any()) for i in (6, 7, 8, 9, 10))
    assert bool(_bits(a[19])[: 2 * 32 * 1024].ne(0).any())                 # the last gradient image's planes, not just its exponents


@pytest.mark.parametrize("M", MS)
def test_results_do_not_depend_on_the_tail_rows_of_their_inputs(M):
    """forward, data gradient (with a record) and the grouped weight gradient on images whose rows >= M hold fp16 NaN in both planes:
    fp32 rows, result images, sign records, dW and db are bit for bit those of the run on clean (zero) tails"""
    from dtc_amd import h2i, ops
    g = torch.Generator().manual_seed(3 * M)
    N, K = 512, 512
    X, W, b = _rows(M, K, g, span=3), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    dZ = _rows(M, N, g, span=8, zero_frac=0.3 if M > 1 else 0.0)
    Wd, bd = W.to(DEV), b.to(DEV)
    Xc, dZc = h2i.HImage.from_tensor(X.to(DEV)), h2i.HImage.from_tensor(dZ.to(DEV))

    def run(Xi, dZi):
        Y, dX = torch.full((M, N), float("nan"), device=DEV), torch.full((M, K), float("nan"), device=DEV)
        Yimg, dXimg = h2i.HImage(M, N, DEV), h2i.HImage(M, K, DEV)
        mask = ops.relu_mask(M, N, DEV).zero_()
        h2i.linear_fwd(Xi, Wd, bd, Y, Yimg, "relu", mask=mask)
        h2i.linear_dgrad(dZi, Wd, dX, dXimg, mask=mask)          # (N == K: the record of the forward's output masks the [M, K] gradient)
        dW, db = torch.full((N, K), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
        jobs = [(dZi, Xi, dW, 0, db)]
        h2i.wgrad_group(jobs, M, ops.workspace(h2i.wgrad_group_workspace_bytes(jobs, M), DEV))
        torch.cuda.synchronize()
        return [t.clone() for t in (Y, Yimg.buf, mask, dX, dXimg.buf, dW, db)]

    clean = run(Xc, dZc)
    dirty = run(_nan_tails(_copy(Xc)), _nan_tails(_copy(dZc)))
    for name, x, y in zip(("Y", "Y image", "record", "dX", "dX image", "dW", "db"), clean, dirty):
        assert torch.equal(_bits(x), _bits(y)), name
    assert bool(torch.isfinite(clean[5]).all()) and bool(torch.isfinite(clean[6]).all()) and float(clean[5].abs().max()) > 0
    assert _row_err(clean[5], dZ.double().T @ X.double()) < ROW_TOL


def test_weight_gradient_of_300_rows_equals_384_rows_with_zero_gradient_rows():
    """(X, dZ) over M = 300 against M = 384 whose 84 extra dZ rows are all zero (the extra X rows are not): both are three 128-row blocks
    in eight slices of one block each (dtc_wgrad_group_h2i: splits = 8, rows_per_split = 128 at 16 + 8 tiles), the same row-slice
    schedule, so dW and db are compared BIT FOR BIT (the float64 form of the comparison is not needed)."""
    from dtc_amd import h2i, ops
    g = torch.Generator().manual_seed(300)
    outs = []
    shapes = [(512, 512), (128, 265)]
    data = [(_rows(384, N, g, span=8, zero_frac=0.3), _rows(384, K, g, span=3)) for N, K in shapes]
    for M in (300, 384):
        jobs = []
        for (N, K), (dZ, X) in zip(shapes, data):
            dZ = dZ.clone()
            dZ[300:] = 0.0
            dW, db = torch.full((N, K), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
            jobs.append((h2i.HImage.from_tensor(dZ[:M].to(DEV)), h2i.HImage.from_tensor(X[:M].to(DEV)), dW, 0, db))
        h2i.wgrad_group(jobs, M, ops.workspace(h2i.wgrad_group_workspace_bytes(jobs, M), DEV))
        torch.cuda.synchronize()
        outs.append([(j[2].clone(), j[4].clone()) for j in jobs])
    for (N, K), (dZ, X), (w3, b3), (w4, b4) in zip(shapes, data, outs[0], outs[1]):
        assert torch.equal(_bits(w3), _bits(w4)) and torch.equal(_bits(b3), _bits(b4)), (N, K)
        assert _row_err(w3, dZ[:300].double().T @ X[:300].double()) < ROW_TOL
