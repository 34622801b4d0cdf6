"""Sources of 2 GiB and more on the operand-image path: a 32768-env x 24-step rollout holds 786 432 rows of 1389 privileged
observations, 4 369 416 192 bytes -- past 2^31 and past 2^32.  The image pack (h2i.HImage.pack) and the target load of the fused MSE
layer (h2i.linear_fwd_mse) take such a tensor through their 64-bit instantiations; everything else keeps refusing it.

A gathered operand is a function of the selected rows only, so nothing here needs a reference computed at this size: every GPU
comparison is bit for bit against the SAME call on a compact copy of the selected rows (below 2 GiB: the instantiation
tests/test_hip_h2i.py pins to fp64 references), with the index list remapped to arange.  The big tensor is torch.empty, allocated once;
only the rows a test reads are filled."""
import ctypes as C

import pytest
import torch

DEV = "cuda:0"
ROWS, COLS = 786432, 1389
# row 386 516 starts 752 bytes before 2^31, row 773 032 starts 1504 bytes before 2^32: both straddle; 0 and 786 431 are the ends
SPECIAL = [0, 386515, 386516, 386517, 773031, 773032, 773033, 786431]
M_FULL, M_TAIL = 1536, 1500          # 12 whole 128-row tiles | a partial last row tile


def index_list():
    """1536 rows: the special ones, equal shares of seeded random rows below 2^31, between 2^31 and 2^32 and beyond 2^32 bytes, shuffled
    (the first 1500 of them -- the specials included -- are the list of the partial-tile cases), then 36 more rows as padding."""
    g = torch.Generator().manual_seed(2031)
    share = -(-(M_TAIL - len(SPECIAL)) // 3)
    parts = [torch.tensor(SPECIAL)]
    for lo, hi in ((0, 386516), (386516, 773032), (773032, ROWS)):
        parts.append(lo + torch.randperm(hi - lo, generator=g)[:share])
    head = torch.cat(parts)[:M_TAIL]
    assert set(SPECIAL) <= set(head.tolist())
    head = head[torch.randperm(M_TAIL, generator=g)]
    pad = torch.randint(0, ROWS, (M_FULL - M_TAIL,), generator=g)
    return torch.cat([head, pad]).contiguous()


@pytest.fixture(scope="module")
def big():
    """dict: the [786432, 1389] privileged tensor, [786432, 53] observations and [786432, 3] base velocities (torch.empty; the 1536
    listed rows filled with seeded randn), the index list on the device, and the compact copies of the listed rows."""
    g = torch.Generator().manual_seed(2032)
    idx = index_list().to(DEV)
    out = dict(idx=idx, arange=torch.arange(M_FULL, device=DEV))
    for name, w in (("priv", COLS), ("obs", 53), ("base_vel", 3)):
        t = torch.empty(ROWS, w, device=DEV)
        c = torch.randn(M_FULL, w, generator=g).to(DEV)
        t[idx] = c
        out[name] = t
        out[name + "_c"] = t[idx].contiguous()          # (rows listed twice hold the value written last in both)
    assert out["priv"].numel() * 4 > 1 << 32
    yield out
    out.clear()


def _operand(form, src, idx, z, mulv):
    from dtc_amd._ffi import seg, segmat
    sfx = "" if src == "big" else "_c"
    p, o, v = (form[1][k + sfx] for k in ("priv", "obs", "base_vel"))
    w = src == "big"
    if form[0] == "heights":
        return segmat([seg(p, 0, 693, gather=True, wide=w)], idx)
    if form[0] == "critic":
        return segmat([seg(o, 0, 53, gather=True, wide=w), seg(v, 0, 3, gather=True, wide=w), seg(p, 693, 696, gather=True, wide=w)], idx)
    return segmat([seg(o, 0, 53, gather=True, wide=w), seg(z, 0, 16), seg(mulv, 0, 3)], idx)      # obs gathered and below 2 GiB


@pytest.mark.gpu
@pytest.mark.parametrize("form,K", [("heights", 693), ("critic", 752), ("actor_narrow", 72)])
def test_pack_of_gathered_rows_beyond_2_gib_equals_the_pack_of_a_compact_copy(big, form, K):
    """M = 1500 (a partial last row tile), the operands as the trainers build them.  Both image buffers are zero-filled (HImage does),
    then the whole buffers -- data and exponent blocks -- must be equal."""
    from dtc_amd import h2i
    M = M_TAIL
    g = torch.Generator().manual_seed(7)
    z, mulv = torch.randn(M, 16, generator=g).to(DEV), torch.randn(M, 35, generator=g).to(DEV)
    wide = h2i.HImage(M, K, DEV).pack(_operand((form, big), "big", big["idx"][:M], z, mulv))
    want = h2i.HImage(M, K, DEV).pack(_operand((form, big), "compact", big["arange"][:M], z, mulv))
    assert torch.equal(wide.buf.view(torch.int64), want.buf.view(torch.int64))
    if form == "heights":                                   # (and the image is the rows' image at all)
        assert float((wide.to_tensor() - big["priv_c"][:M, :693]).abs().max()) <= 2.0 ** -21 * float(big["priv_c"][:M, :693].abs().max())


@pytest.mark.gpu
def test_nan_in_a_row_beyond_4_gib_stays_in_its_image_row(big):
    from dtc_amd import h2i
    from dtc_amd._ffi import seg, segmat
    M, idx, priv = M_TAIL, big["idx"][:M_TAIL], big["priv"]
    src = 786431                                            # its bytes start at 4 369 410 636
    where = (idx == src).nonzero().flatten()
    assert where.numel() == 1
    clean = h2i.HImage(M, 693, DEV).pack(segmat([seg(priv, 0, 693, gather=True, wide=True)], idx)).to_tensor()
    keep = float(priv[src, 100])
    try:
        priv[src, 100] = float("nan")
        img = h2i.HImage(M, 693, DEV).pack(segmat([seg(priv, 0, 693, gather=True, wide=True)], idx))
        comp = big["priv_c"].clone()
        comp[where, 100] = float("nan")
        want = h2i.HImage(M, 693, DEV).pack(segmat([seg(comp, 0, 693, gather=True)], big["arange"][:M]))
    finally:
        priv[src, 100] = keep
    assert torch.equal(img.buf.view(torch.int64), want.buf.view(torch.int64))
    got = img.to_tensor()
    other = torch.ones(M, dtype=torch.bool, device=DEV)
    other[where] = False
    assert torch.equal(got[other], clean[other])            # every other row: bit-identical
    assert not bool(torch.isfinite(got[where, 100]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("M", [M_FULL, M_TAIL])
def test_fused_mse_layer_against_a_target_beyond_2_gib(big, M):
    """The terrain decoder's output layer with its loss: K = 512, N = 693, target columns 696 ..: fp32 dY, the dY image and every partial
    of the squared-error sum are those of the compact target."""
    from dtc_amd import h2i
    g = torch.Generator().manual_seed(M)
    K, N = 512, 693
    X = h2i.HImage.from_tensor(torch.randn(M, K, generator=g).to(DEV))
    W, b = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV), torch.randn(N, generator=g).to(DEV)
    outs = []
    for target, tidx in ((big["priv"], big["idx"][:M]), (big["priv_c"], big["arange"][:M])):
        dY = torch.full((M, N), float("nan"), device=DEV)
        dYimg = h2i.HImage(M, N, DEV)
        part = torch.full((h2i.mse_parts(M, N),), -1.0, dtype=torch.float64, device=DEV)
        n = h2i.linear_fwd_mse(X, W, b, target, 696, tidx.contiguous(), dY, dYimg, part)
        outs.append((n, dY, dYimg.buf.view(torch.int64), part))
    (n0, dY0, img0, part0), (n1, dY1, img1, part1) = outs
    assert n0 == n1 == part0.numel()
    assert torch.equal(dY0, dY1) and bool(torch.isfinite(dY0).all())
    assert torch.equal(img0, img1)
    assert torch.equal(part0, part1) and float(part0.sum()) > 0.0
    # (and the loss is the loss: against fp64 on the compact rows, as tests/test_hip_h2i.py::test_fused_mse_layer)
    e = (X.to_tensor().double() @ W.double().T + b.double()) - big["priv_c"][:M, 696:696 + N].double()
    assert abs(float(part0.sum()) - float((e * e).sum())) <= 1e-6 * float((e * e).sum())


# ------------------------------------------------------------------------------------------------ host side: no GPU
class _Fake:
    """Tensor-like with the metadata of a [400000, 1389] device tensor (2.2 GB) and no memory behind it."""
    shape = (400000, 1389)
    dtype = torch.float32
    is_cuda = True

    def dim(self):
        return 2

    def stride(self, i):
        return (1389, 1)[i]

    def data_ptr(self):
        return 4096


def test_seg_refuses_a_wide_source_unless_asked():
    from dtc_amd import _ffi
    with pytest.raises(_ffi.DtcError, match="2 GiB"):
        _ffi.seg(_Fake(), 0, 693, gather=True)
    s = _ffi.seg(_Fake(), 0, 693, gather=True, wide=True)
    assert (s.width, s.rows, s.ld, s.gather) == (693, 400000, 1389, 1)


def test_entry_points_outside_the_image_path_refuse_a_wide_segment_before_any_device_work():
    from dtc_amd import _ffi
    lib = _ffi.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    m = _ffi.DtcSegMat()
    m.nseg, m.cols, m.idx = 1, 693, p.value
    m.seg[0] = _ffi.seg(_Fake(), 0, 693, gather=True, wide=True)
    for call, who in ((lambda: lib.dtc_linear_fwd(m, p, p, p, 8, 4, 8, 693, 0, None), b"dtc_linear_fwd"),
                      (lambda: lib.dtc_pack_cols(m, p, 693, 4, None, None), b"dtc_pack_cols"),
                      (lambda: lib.dtc_amax(m, 4, p, None), b"dtc_amax")):
        rc, err = call(), lib.dtc_last_error()
        assert rc == -1, (who, rc)
        assert who in err and b"operand-image path" in err and b"2 GiB" in err, err
    m.seg[0].gather = 0                                     # not gathered: 4 rows of it would fit, the matrix as declared does not
    assert lib.dtc_linear_fwd(m, p, p, p, 8, 4, 8, 693, 0, None) == -1 and b"operand-image path" in lib.dtc_last_error()


def test_an_operand_image_of_2_gib_names_the_mini_batch_count():
    from dtc_amd import _ffi, h2i
    with pytest.raises(_ffi.DtcError, match="num_mini_batches") as e:
        h2i.HImage(400000, 1389, "cpu")                     # 400000 x 1392 x 4 bytes of planes alone
    assert "400000" in str(e.value)
