"""The skeleton of the image-operand GEMM tile (csrc/gemm_h2i.hip, h2i_tile): the number of 16-column stages of the reduction (all residues
mod 3, fewer than 3, up to MAX_TB = 16 exponent blocks), the exponent prologue (blocks without content inherit, across the borders of a
row operand's images too) and the operands the epilogue requests ahead (bias, sign record, target rows).  Two kinds of checks: every row /
feature against float64 under the bounds of tests/test_hip_h2i.py, and bit identities -- appending all-zero columns to both operands of a
product changes the number of stages and blocks the kernel walks and must change no bit of any result."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROW_TOL = 2e-6          # per-row / per-feature relative error bound of tests/test_hip_h2i.py


@pytest.fixture(autouse=True, params=["rows64_default", "rows128_only"])
def tile_rows(request):
    """every test on 64-row tiles (the default for small launches) and on 128-row tiles, as tests/test_hip_h2i.py"""
    from dtc_amd import _ffi
    _ffi.lib().dtc_h2i_rows64_max(-1 if request.param == "rows64_default" else 0)
    yield request.param
    _ffi.lib().dtc_h2i_rows64_max(-1)


def _act(v, act):
    return torch.relu(v) if act == "relu" else torch.nn.functional.elu(v) if act == "elu" else v


def _row_err(y, ref):
    """max over rows of (largest element error of the row / largest |element| of the row); all-zero reference rows must be exact"""
    y, ref = y.double().cpu(), ref.double().cpu()
    num = (y - ref).abs().amax(dim=1)
    den = ref.abs().amax(dim=1)
    zero = den == 0
    assert float(num[zero].max() if zero.any() else 0.0) == 0.0
    return float((num[~zero] / den[~zero]).max()) if (~zero).any() else 0.0


def _col_err(y, ref):
    return _row_err(y.T, ref.T)


def _rows(M, K, g, span=12, zero_frac=0.0):
    """rows log-uniform over 10^-span .. 1 of the largest, a fraction of them exactly zero"""
    X = torch.randn(M, K, generator=g) * 10.0 ** (-span * torch.rand(M, 1, generator=g))
    if zero_frac:
        X[torch.rand(M, generator=g) < zero_frac] = 0.0
    return X


def _feature_weights(F, R, g, span=40.0):
    """[F, R] weights whose F image rows are log-uniform over 2^-span .. 1 inside every 128-row block (a quarter full-size); where R spans
    several 128-column blocks some rows are 2^-30 smaller in one block and some exactly zero in one block (the first zero one in block 0)"""
    s = torch.exp2(-span * torch.rand(F, generator=g, dtype=torch.float64))
    for t0 in range(0, F, 128):
        n = min(128, F - t0)
        s[t0 + torch.randperm(n, generator=g)[:max(1, n // 4)]] = 1.0
    W = (torch.randn(F, R, generator=g, dtype=torch.float64) / R ** 0.5 * s[:, None]).float()
    nkb = -(-R // 128)
    if nkb > 1:
        for i, f in enumerate(torch.randperm(F, generator=g)[:max(2, F // 8)].tolist()):
            b = 0 if i == 1 else int(torch.randint(nkb, (1,), generator=g))
            if i % 2:
                W[f, 128 * b:128 * b + 128] = 0.0
            else:
                W[f, 128 * b:128 * b + 128] *= 2.0 ** -30
    return W


def _image_within_22_bits(img, Y):
    """every element of the image within 2^-21 of its row block's largest element"""
    M, N = Y.shape
    blk = torch.zeros(M, -(-N // 128) * 128, device=DEV)
    blk[:, :N] = Y.abs()
    blk = blk.view(M, -1, 128).amax(dim=2, keepdim=True).expand(-1, -1, 128).reshape(M, -1)[:, :N]
    return bool(((img.to_tensor() - Y).abs() <= blk * 2.0 ** -21).all())


def _pad(t, p, dim):
    """t with p zero columns (dim 1) / rows (dim 0) appended"""
    if p == 0:
        return t
    shape = list(t.shape)
    shape[dim] = p
    return torch.cat([t, torch.zeros(shape, dtype=t.dtype, device=t.device)], dim=dim)


def _same_bits(a, b):
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t   # noqa: E731
    return torch.equal(bits(a), bits(b))


def _fwd_outputs(X, W, b, act, masked):
    """(fp32 result, result image bytes, sign record) of act(X W^T + b); X: tensor or list of tensors (one image each)"""
    from dtc_amd import h2i, ops
    Xs = X if isinstance(X, list) else [X]
    M, N = Xs[0].shape[0], W.shape[0]
    imgs = [h2i.HImage.from_tensor(x.contiguous()) for x in Xs]
    Y, Yimg = torch.full((M, N), float("nan"), device=DEV), h2i.HImage(M, N, DEV)
    mask = ops.relu_mask(M, N, DEV).zero_() if masked else None
    h2i.linear_fwd(imgs if len(imgs) > 1 else imgs[0], W, b, Y, Yimg, act, mask=mask)
    torch.cuda.synchronize()
    return [Y, Yimg.buf.clone()] + ([mask] if masked else [])


def _dgrad_outputs(dZ, W, mode, Xs, mask):
    """(fp32 result, result image bytes) of (dZ W) act'"""
    from dtc_amd import h2i
    M, K = dZ.shape[0], W.shape[1]
    dX, dXimg = torch.full((M, K), float("nan"), device=DEV), h2i.HImage(M, K, DEV)
    kw = dict(mask=mask) if mode == "mask" else dict(Xsaved=Xs, act="elu") if mode == "elu" else dict()
    h2i.linear_dgrad(h2i.HImage.from_tensor(dZ.contiguous()), W.contiguous(), dX, dXimg, **kw)
    torch.cuda.synchronize()
    return [dX, dXimg.buf.clone()]


def _sign_record(M, K, g):
    """(record, fp32 signs) of a ReLU layer with K outputs, as the forward kernel writes it"""
    from dtc_amd import h2i, ops
    pre = torch.randn(M, K, generator=g).to(DEV)
    mask, Yf = ops.relu_mask(M, K, DEV).zero_(), torch.empty(M, K, device=DEV)
    h2i.linear_fwd(h2i.HImage.from_tensor(pre), torch.eye(K, device=DEV), None, Yf, None, "relu", mask=mask)
    return mask, Yf > 0


# ---- the number of stages: S = 1, 1, 2, 3, 4, 5, 8, 9, 10, 17, 65, 128 (every residue mod 3, S < 3, more than 8 blocks, MAX_TB blocks)
@pytest.mark.parametrize("R", [5, 16, 32, 48, 64, 80, 128, 144, 160, 272, 1040, 2048])
def test_stage_count_sweep_forward_and_data_gradient(R):
    from dtc_amd import h2i
    for M in (64, 200):
        for N in (128, 140):
            g = torch.Generator().manual_seed(R + 7 * M + N)
            X = _rows(M, R, g, span=12, zero_frac=0.05)
            W = torch.randn(N, R, generator=g) / R ** 0.5
            b = torch.randn(N, generator=g) * 1e-13                       # (a larger bias would swamp the small rows' products)
            ref = torch.relu(X.double() @ W.double().T + b.double())
            Y, Yimg = torch.full((M, N), float("nan"), device=DEV), h2i.HImage(M, N, DEV)
            h2i.linear_fwd(h2i.HImage.from_tensor(X.to(DEV)), W.to(DEV), b.to(DEV), Y, Yimg, "relu")
            err = _row_err(Y, ref)
            print(f"fwd {M}x{N}x{R}: per-row err {err:.2e}")
            assert err < ROW_TOL
            assert _image_within_22_bits(Yimg, Y)
            # data gradient with the same reduction: dZ [M, R], W [R, N]
            dZ = _rows(M, R, g, span=8, zero_frac=0.3)
            Wt = torch.randn(R, N, generator=g) / R ** 0.5
            dX, dXimg = torch.full((M, N), float("nan"), device=DEV), h2i.HImage(M, N, DEV)
            h2i.linear_dgrad(h2i.HImage.from_tensor(dZ.to(DEV)), Wt.to(DEV), dX, dXimg)
            err = _row_err(dX, dZ.double() @ Wt.double())
            print(f"dgrad {M}x{R}x{N}: per-row err {err:.2e}")
            assert err < ROW_TOL
            assert _image_within_22_bits(dXimg, dX)


# ---- zero padding changes no bit.  R = 64: the padded reductions stay inside block 0 (S = 4 .. 7); R = 96: 16 columns stay inside, 32 fill
# the block, 48 cross into a new, all-zero block (S = 6 .. 9, the new block's exponents are HI_EZERO); one of S .. S + 3 is a multiple of 3
PADS = (0, 16, 32, 48)


@pytest.mark.parametrize("R", [64, 96])
@pytest.mark.parametrize("act", ["relu", "elu", None])
def test_zero_padding_changes_no_bit_forward(R, act):
    g = torch.Generator().manual_seed(R)
    M, N = 200, 128
    X, W, b = _rows(M, R, g, span=6, zero_frac=0.05).to(DEV), (torch.randn(N, R, generator=g) / R ** 0.5).to(DEV), torch.randn(N, generator=g).to(DEV)
    outs = [_fwd_outputs(_pad(X, p, 1), _pad(W, p, 1), b, act, act == "relu") for p in PADS]
    assert float(outs[0][0].abs().max()) > 0
    for o in outs[1:]:
        assert all(_same_bits(a, c) for a, c in zip(outs[0], o))


@pytest.mark.parametrize("R", [64, 96])
@pytest.mark.parametrize("mode", ["mask", "elu", "none"])
def test_zero_padding_changes_no_bit_data_gradient(R, mode):
    g = torch.Generator().manual_seed(R + 1)
    M, K = 200, 128
    dZ, W = _rows(M, R, g, span=6, zero_frac=0.2).to(DEV), (torch.randn(R, K, generator=g) / R ** 0.5).to(DEV)
    Xs = torch.nn.functional.elu(torch.randn(M, K, generator=g)).to(DEV)
    mask = _sign_record(M, K, g)[0] if mode == "mask" else None
    outs = [_dgrad_outputs(_pad(dZ, p, 1), _pad(W, p, 0), mode, Xs, mask) for p in PADS]
    assert float(outs[0][0].abs().max()) > 0
    for o in outs[1:]:
        assert all(_same_bits(a, c) for a, c in zip(outs[0], o))


@pytest.mark.parametrize("R", [64, 96])
def test_zero_padding_changes_no_bit_fused_mse(R):
    from dtc_amd import h2i
    g = torch.Generator().manual_seed(R + 2)
    M, N = 200, 140
    X, W, b = torch.randn(M, R, generator=g).to(DEV), (torch.randn(N, R, generator=g) / R ** 0.5).to(DEV), torch.randn(N, generator=g).to(DEV)
    T, idx = torch.randn(2 * M, 300, generator=g).to(DEV), torch.randint(0, 2 * M, (M,), generator=g).to(DEV)
    outs = []
    for p in PADS:
        dY, dYimg = torch.full((M, N), float("nan"), device=DEV), h2i.HImage(M, N, DEV)
        part = torch.zeros(h2i.mse_parts(M, N), dtype=torch.float64, device=DEV)
        n = h2i.linear_fwd_mse(h2i.HImage.from_tensor(_pad(X, p, 1)), _pad(W, p, 1), b, T, 100, idx, dY, dYimg, part)
        torch.cuda.synchronize()
        outs.append([dY, dYimg.buf.clone(), part[:n].clone()])
    e = (X.double() @ W.double().T + b.double()) - T[idx][:, 100:100 + N].double()
    assert _row_err(outs[0][0], e * (2.0 / (M * N))) < ROW_TOL
    assert abs(float(outs[0][2].sum()) - float((e * e).sum())) <= 1e-6 * float((e * e).sum())
    for o in outs[1:]:
        assert all(_same_bits(a, c) for a, c in zip(outs[0], o))


@pytest.mark.parametrize("R", [32, 64, 256])            # S = 2, 4, 16
def test_zero_padding_changes_no_bit_one_pass(R):
    from dtc_amd import h2i
    g = torch.Generator().manual_seed(R + 3)
    M, N = 200, 128
    X, W, b = _rows(M, R, g, span=6).to(DEV), (torch.randn(N, R, generator=g) / R ** 0.5).to(DEV), torch.randn(N, generator=g).to(DEV)
    dZ, Wt = _rows(M, R, g, span=6, zero_frac=0.2).to(DEV), (torch.randn(R, N, generator=g) / R ** 0.5).to(DEV)
    mask = _sign_record(M, N, g)[0]
    with h2i.h2i_passes_as(1):
        outs = [_fwd_outputs(_pad(X, p, 1), _pad(W, p, 1), b, "relu", True) + _dgrad_outputs(_pad(dZ, p, 1), _pad(Wt, p, 0), "mask", None, mask)
                for p in PADS]
    assert h2i.h2i_passes() == 3
    ref = torch.relu(X.double() @ W.double().T + b.double())
    assert _row_err(outs[0][0], ref) < 2.0 ** -8          # 11-bit operands: the one-pass kernels ran, on the right operands
    for o in outs[1:]:
        assert all(_same_bits(a, c) for a, c in zip(outs[0], o))


# ---- several operand images.  (19 | 512): S = 2 + 32; (512 | 53 | 19): S = 32 + 4 + 2; (19 | 512 | 19): S = 36, the last image ends on the
# last stage of a trip.  Rows whose MIDDLE image is all zero inherit the first image's exponent across two segment borders.
@pytest.mark.parametrize("widths,cols", [((19, 512), (512, 0)), ((512, 53, 19), (72, 19, 0)), ((19, 512, 19), (0, 38, 19))])
def test_several_operand_images_accuracy_and_padding_identity(widths, cols):
    from dtc_amd import h2i
    g = torch.Generator().manual_seed(sum(widths))
    M, N = 200, 140
    parts = [_rows(M, w, g, span=4) for w in widths]
    mid = len(widths) // 2
    parts[mid][::3] = 0.0                                   # every third row: nothing in the middle (of two: the second) image
    parts[0][5] = 0.0                                       # a row that starts with an empty image
    parts[-1][7] = 0.0
    Kt = sum(widths)
    W = _feature_weights(N, Kt, g)
    b = torch.randn(N, generator=g) * 1e-6
    full = torch.zeros(M, Kt)
    for c0, p in zip(cols, parts):
        full[:, c0:c0 + p.shape[1]] = p
    ref = torch.nn.functional.elu(full.double() @ W.double().T + b.double())
    Y = torch.full((M, N), float("nan"), device=DEV)
    h2i.linear_fwd([h2i.HImage.from_tensor(p.to(DEV)) for p in parts], W.to(DEV), b.to(DEV), Y, None, "elu", cols=list(cols))
    er, ec = _row_err(Y, ref), _col_err(Y, ref)
    print(f"fwd {widths}: per-row err {er:.2e}, per-feature err {ec:.2e}")
    assert er < ROW_TOL and ec < ROW_TOL
    # padding identity, images side by side: zero columns behind the LAST image and behind W's columns
    Ws = torch.cat([W[:, c0:c0 + w] for c0, w in zip(cols, widths)], dim=1).to(DEV)
    xs = [p.to(DEV) for p in parts]
    outs = [_fwd_outputs(xs[:-1] + [_pad(xs[-1], p, 1)], _pad(Ws, p, 1), b.to(DEV), "elu", False) for p in PADS]
    assert _row_err(outs[0][0], ref) < ROW_TOL
    for o in outs[1:]:
        assert all(_same_bits(a, c) for a, c in zip(outs[0], o))


# ---- the exponent walk: 2, 6, 9 and 16 blocks; rows whose first, a middle or the last block is exactly zero; weights with zero blocks
@pytest.mark.parametrize("nb", [2, 6, 9, 16])
def test_exponent_walk_zero_blocks(nb):
    from dtc_amd import h2i
    g = torch.Generator().manual_seed(nb)
    M, N, R = 200, 140, 128 * nb                           # the last row tile is partly empty
    def operand(span):                                     # noqa: E306
        X = _rows(M, R, g, span=span)
        X[0::7, :128] = 0.0                                # first block
        X[1::7, 128 * (nb // 2):128 * (nb // 2) + 128] = 0.0
        X[2::7, R - 128:] = 0.0                            # last block
        X[3::7, :R - 128] = 0.0                            # everything but the last block
        X[4::7] = 0.0                                      # nothing at all
        X[6::7, 128 * (nb // 2):] *= 2.0 ** -20            # the scale drops at a border
        return X
    X, W = operand(12), _feature_weights(N, R, g)
    ref = X.double() @ W.double().T
    Y = torch.full((M, N), float("nan"), device=DEV)
    h2i.linear_fwd(h2i.HImage.from_tensor(X.to(DEV)), W.to(DEV), None, Y, None, None)
    er, ec = _row_err(Y, ref), _col_err(Y, ref)
    print(f"fwd walk {nb} blocks: per-row err {er:.2e}, per-feature err {ec:.2e}")
    assert er < ROW_TOL and ec < ROW_TOL
    assert float(Y[4::7].abs().max()) == 0.0
    dZ, Wt = operand(8), _feature_weights(N, R, g).T.contiguous()      # [R, N]: the rows of the W^T image are the input features
    ref = dZ.double() @ Wt.double()
    dX = torch.full((M, N), float("nan"), device=DEV)
    h2i.linear_dgrad(h2i.HImage.from_tensor(dZ.to(DEV)), Wt.to(DEV), dX, None)
    er, ec = _row_err(dX, ref), _col_err(dX, ref)
    print(f"dgrad walk {nb} blocks: per-row err {er:.2e}, per-feature err {ec:.2e}")
    assert er < ROW_TOL and ec < ROW_TOL
    assert float(dX[4::7].abs().max()) == 0.0


# ---- the bit identities of tests/test_hip_h2i.py at reductions of 64, 256 and 19 + 512 (S = 4, 16, 34)
def _first_operand(M, R, g):
    return [_rows(M, w, g, span=4, zero_frac=0.1).to(DEV) for w in ((19, 512) if R == 531 else (R,))]


@pytest.mark.parametrize("R", [64, 256, 531])
def test_64_row_tiles_equal_128_row_tiles_bit_for_bit(R, tile_rows):
    from dtc_amd import _ffi
    g = torch.Generator().manual_seed(R + 4)
    M, N = 640, 128
    xs = _first_operand(M, R, g)
    W, b = (torch.randn(N, R, generator=g) / R ** 0.5).to(DEV), torch.randn(N, generator=g).to(DEV)
    dZ, Wt = _rows(M, R if R != 531 else 256, g, span=6, zero_frac=0.2).to(DEV), None
    Wt = (torch.randn(dZ.shape[1], N, generator=g) / 16).to(DEV)
    mask = _sign_record(M, N, g)[0]
    out = []
    for mx in (-1, 0):
        _ffi.lib().dtc_h2i_rows64_max(mx)
        out.append(_fwd_outputs(xs, W, b, "relu", True) + _dgrad_outputs(dZ, Wt, "mask", None, mask))
    assert float(out[0][0].abs().max()) > 0 and float(out[0][3].abs().max()) > 0
    assert all(_same_bits(a, c) for a, c in zip(*out))


@pytest.mark.parametrize("R", [64, 256, 531])
def test_chains_equal_the_per_layer_launches_bit_for_bit(R):
    """forward R -> 64 (ReLU, sign record) -> 128 and the data-gradient chain back through 128 -> 64 -> R' (R' = R, or 256 for the two-image input)"""
    from dtc_amd import h2i, ops
    g = torch.Generator().manual_seed(R + 5)
    M = 640
    xs = [h2i.HImage.from_tensor(x) for x in _first_operand(M, R, g)]
    w = lambda n, k: (torch.randn(n, k, generator=g) / k ** 0.5).to(DEV)      # noqa: E731
    Rb = 256 if R == 531 else R
    W1, b1, W2, b2, Wb = w(64, R), torch.randn(64, generator=g).to(DEV), w(128, 64), torch.randn(128, generator=g).to(DEV), w(64, Rb)
    dY = h2i.HImage.from_tensor(_rows(M, 128, g, span=5, zero_frac=0.1).to(DEV))

    def run(chain):
        h1, h2 = h2i.HImage(M, 64, DEV), h2i.HImage(M, 128, DEV)
        m1 = ops.relu_mask(M, 64, DEV).zero_()
        y2 = torch.zeros(M, 128, device=DEV)
        h2i.fwd_layers([dict(X=xs if len(xs) > 1 else xs[0], W=W1, b=b1, Yimg=h1, act="relu", mask=m1), dict(X=h1, W=W2, b=b2, Y=y2, Yimg=h2)], chain)
        g1, g0 = h2i.HImage(M, 64, DEV), h2i.HImage(M, Rb, DEV)
        h2i.dgrad_layers([dict(dZimg=dY, W=W2, dXimg=g1, mask=m1), dict(dZimg=g1, W=Wb, dXimg=g0)], chain)
        torch.cuda.synchronize()
        return [t.clone() for t in (h1.buf, h2.buf, m1, y2, g1.buf, g0.buf)]

    a, c = run(True), run(False)
    assert float(a[3].abs().max()) > 0
    for i, (x, y) in enumerate(zip(a, c)):
        assert _same_bits(x, y), i
