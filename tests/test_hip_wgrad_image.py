"""The image weight gradient (csrc/wgrad_h2i.hip: wgrad_h2i_group_kernel + wgrad_h2i_reduce_kernel) against the numpy restatement of
its scaling scheme (oracle/wgrad_image_ref.py), element by element, on the input families of tests/test_wgrad_image_oracle.py.

What is compared with what.  The operands are the images actually passed, decoded (HImage.to_tensor / exps).
    kernel vs emulation   |got - emu| / S per element, S[n, k] = sum over the rows the scheme keeps of |dZ[m, n]| |X[m, k]|: a sparse
                          feature is judged on its own scale, never against its row's or the tensor's largest element.  Where S = 0
                          (all-zero features, features that live only in dropped rows) the kernel must return exactly 0.
    tolerance             the larger of 8 x the single-pass fp32 kernel's error against float64 on the same decoded operands (same
                          normalisation; the margin of test_hip_h2i._assert_like_fp32) and WREF.chain_tolerance: (stages per slice x
                          3 MFMAs + slices) x 2^-24, the kernel's fp32 addition chain.
    scheme vs truth       asserted against the oracle's own bound only (it holds by derivation, dropped rows included).
The emulation runs under rescale = "bounded": the rule the kernel has had since the range test below showed its accumulators
overflowing at a block border (profiles/wgrad_image_errors.txt).

dtc_h2i_rows64_max does not reach this kernel (it picks the row tile of the forward / data-gradient launches in gemm_h2i.hip only), so
the weight-gradient tests run once; the forward / data-gradient test at the end of the file runs at both settings.
Every test prints its figures as lines starting with "WGI"; profiles/wgrad_image_errors.txt is one run's output."""
import numpy as np
import pytest
import torch

from oracle import wgrad_image_ref as WREF
from test_wgrad_image_oracle import (BLOCK_MS, BLOCKS_PER_SLICE, CAP_KINDS, CAP_ROW_K, RANGE_KINDS, TIER_CASES, TIERS, block_inputs,
                                     cap_feature_group, cap_inputs, column_group, feature_group, range_inputs, tier_inputs)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tiles(N, K):
    return -(-N // 128) * -(-K // 128)


def _launch(pairs, wcol0=0, pad=0, bias=None):
    """pairs: [(dZ, X) float32 numpy].  One grouped launch -> per job (dZimg, Ximg, dW view, db | None, the whole gradient buffer)"""
    from dtc_amd import h2i, ops
    M = pairs[0][0].shape[0]
    jobs, full = [], []
    for j, (dZ, X) in enumerate(pairs):
        N, K = dZ.shape[1], X.shape[1]
        buf = torch.full((N, wcol0 + K + pad), float("nan"), device=DEV)
        db = torch.full((N,), float("nan"), device=DEV) if (bias is None or bias[j]) else None
        jobs.append((h2i.HImage.from_tensor(torch.from_numpy(dZ).to(DEV)), h2i.HImage.from_tensor(torch.from_numpy(X).to(DEV)),
                     buf[:, :wcol0 + K], wcol0, db))
        full.append(buf)
    nbytes = h2i.wgrad_group_workspace_bytes(jobs, M)
    ws = ops.workspace(nbytes, DEV)
    h2i.wgrad_group(jobs, M, ws)
    torch.cuda.synchronize()
    return jobs, full, ws, nbytes


def _fp32_kernel(dZf, Xf):
    """the single-pass fp32 MFMA kernel on the decoded operands (what h2i.wgrad_group's capture compares with)"""
    from dtc_amd import ops
    M, N, K = dZf.shape[0], dZf.shape[1], Xf.shape[1]
    natW, natb = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    nj = [(dZf, Xf, natW, natb)]
    ops.wgrad_group(nj, M, ops.workspace(ops.wgrad_group_workspace_bytes(nj, M, False), DEV), split=False)
    return natW.double().cpu().numpy(), natb.double().cpu().numpy()


def _compare(job, tiles_total, what, rescale="bounded"):
    """-> namespace of the job's figures (printed); _assert_job asserts kernel vs emulation within tolerance, scheme vs truth within its bound"""
    dZimg, Ximg, dWv, wcol0, db = job
    M, N, K = dZimg.M, dZimg.K, dWv.shape[1] - wcol0
    dZf, Xf = dZimg.to_tensor(), Ximg.to_tensor()[:, :K].contiguous()
    dZd, Xd = dZf.double().cpu().numpy(), Xf.double().cpu().numpy()
    assert np.isfinite(dZd).all() and np.isfinite(Xd).all()
    eZ, eX = dZimg.exps().cpu().numpy(), Ximg.exps().cpu().numpy()[:, :-(-K // 128)]
    emu = WREF.emulate(dZd, Xd, eZ, eX, M, rescale=rescale, tiles_total=tiles_total)
    tW, tb = WREF.truth(dZd, Xd)
    natW, natb = _fp32_kernel(dZf, Xf)
    got = dWv[:, wcol0:].double().cpu().numpy()
    r = emu
    r.got, r.tW, r.tb, r.natW, r.natb = got, tW, tb, natW, natb
    r.chain = WREF.chain_tolerance(M, tiles_total)
    r.err = WREF.rel(np.abs(got - emu.dW), emu.S)
    r.fp32 = WREF.rel(np.abs(natW - tW), emu.S_all)
    r.scheme = WREF.rel(np.abs(emu.dW - tW), emu.S_all)
    r.tol = max(8 * r.fp32, r.chain)
    line = f"WGI {what}: kernel vs emulation {r.err:.2e} of S (tolerance {r.tol:.2e}: fp32 kernel vs float64 {r.fp32:.2e}, chain {r.chain:.2e}); " \
           f"emulation vs float64 {r.scheme:.2e} of S_all, rows dropped {int(emu.dropped.sum())} of {M}"
    if db is not None:
        r.gotb = db.double().cpu().numpy()
        r.errb = WREF.rel(np.abs(r.gotb - emu.db), emu.Sb)
        r.fp32b = WREF.rel(np.abs(natb - tb), emu.Sb_all)
        r.tolb = max(8 * r.fp32b, r.chain)
        line += f"; bias {r.errb:.2e} (tolerance {r.tolb:.2e}, fp32 kernel {r.fp32b:.2e})"
    print(line)
    r.what, r.has_bias = what, db is not None
    return r


def _assert_job(r):
    assert np.isfinite(r.got).all(), r.what
    assert (np.abs(r.dW - r.tW) <= r.bound).all() and (np.abs(r.db - r.tb) <= r.bound_b).all(), r.what
    assert r.err <= r.tol, (r.what, r.err, r.tol)
    if r.has_bias:
        assert np.isfinite(r.gotb).all() and r.errb <= r.tolb, (r.what, r.errb, r.tolb)


# ---------------------------------------------------------------- a. tiers x sparse features
@pytest.mark.parametrize("shape,mode", TIER_CASES)
def test_tiers_and_sparse_features(shape, mode):
    """features that live in one tier of rows only, per tier: kernel vs restatement within tolerance, exactly 0 from k = 25, bias per
    feature against Sb.  Before the bias factors carried 2^15 the "dz" cases failed here: the bias gradient of a feature living in
    the k = 24 rows was 1.25e-5 / 1.29e-5 of its Sb off the restatement (k = 20: 9e-7; tolerance 1.9e-6), the matrix pipe keeping no
    product bits below about 2^-24 (profiles/wgrad_image_errors.txt)."""
    M, N, K = shape
    dZ, X, tier = tier_inputs(shape, mode)
    jobs, _, _, _ = _launch([(dZ, X)])
    r = _compare(jobs[0], _tiles(N, K), f"tiers {M}x{N}x{K} {mode}")
    gz, gx = feature_group(N), column_group(K)
    dense = gx == -1
    for g, k in [(-1, "dense")] + list(enumerate(TIERS)):
        sel = gz == g
        print(f"WGI   bias, features of tier {k} ({mode}): kernel vs emulation {WREF.rel(np.abs(r.gotb - r.db)[sel], r.Sb[sel]):.2e} of Sb, "
              f"emulation vs float64 {WREF.rel(np.abs(r.db - r.tb)[sel], r.Sb_all[sel]):.2e}, fp32 kernel vs float64 "
              f"{WREF.rel(np.abs(r.natb - r.tb)[sel], r.Sb_all[sel]):.2e}")
    # per tier: the features that live in that tier's rows only, over the dense input features
    for g, k in enumerate(TIERS):
        sel = np.ix_(gz == g, dense)
        ek = WREF.rel(np.abs(r.got - r.dW)[sel], r.S[sel])
        es = WREF.rel(np.abs(r.dW - r.tW)[sel], r.S_all[sel])
        e32 = WREF.rel(np.abs(r.natW - r.tW)[sel], r.S_all[sel])
        print(f"WGI   tier k = {k:2d} ({mode}): kernel vs emulation {ek:.2e}, emulation vs float64 {es:.2e}, fp32 kernel vs float64 {e32:.2e}")
        if k >= WREF.DROP_K:
            assert (r.got[gz == g] == 0).all() and (r.dW[gz == g] == 0).all() and (np.abs(r.tW[sel]) > 0).all()
        else:
            assert ek <= r.tol and (r.got[sel] != 0).all()
            # what the derivation promises a feature of this tier: 2^-22 for the product left out plus 2^-(38 - k) for fp16
            assert es <= 2.0 ** -22 * 1.01 + 2.0 ** -(38 - k)
    _assert_job(r)
    assert (r.got[gz == 10] == 0).all() and (r.got[:, gx == 10] == 0).all()
    lost_cols = np.isin(gx, [i for i, k in enumerate(TIERS) if k >= WREF.DROP_K])
    assert (r.got[:, lost_cols] == 0).all()
    # bias: per feature against Sb; a tier whose distance sits on dZ alone is dropped from k = 25, any other is kept
    lost = np.isin(gz, [i for i, k in enumerate(TIERS) if k >= WREF.DROP_K])
    assert (r.gotb[gz == 10] == 0).all()
    if mode == "dz":
        assert (r.gotb[lost] == 0).all() and (r.db[lost] == 0).all() and (r.tb[lost] != 0).all()
    else:
        assert (r.Sb == r.Sb_all).all() and WREF.rel(np.abs(r.gotb - r.tb), r.Sb_all) <= r.tolb


# ---------------------------------------------------------------- b. blocks per slice and ragged ends
def _two_launches_same_bits(pairs, jobs):
    again, _, _, _ = _launch(pairs)
    for a, b in zip(jobs, again):
        assert torch.equal(a[2], b[2]) and torch.equal(a[4], b[4])


@pytest.mark.parametrize("M", BLOCK_MS)
def test_blocks_per_slice_and_ragged_ends(M):
    dZ, X, state = block_inputs(M, 128, 128)
    jobs, _, _, nbytes = _launch([(dZ, X)])
    splits, rps = WREF.slices(M, 1)
    assert nbytes == splits * (128 * 128 + 128) * 4 == WREF.workspace_bytes(M, [(128, 128)])          # the slices the library planned
    assert rps // 128 == BLOCKS_PER_SLICE[M]
    r = _compare(jobs[0], 1, f"blocks M = {M} ({rps // 128} per slice, states {np.bincount(state, minlength=4).tolist()})")
    steps = [b[3] - a[3] for a, b in zip(r.T, r.T[1:]) if a[2] // (rps // 128) == b[2] // (rps // 128)]
    if steps:
        print(f"WGI   T steps at the borders inside a slice: {min(steps)} .. {max(steps)}")
    _assert_job(r)
    zero_rows = ~np.abs(dZ).any(axis=0)
    assert (r.got[zero_rows] == 0).all()
    _two_launches_same_bits([(dZ, X)], jobs)


def test_blocks_with_many_tiles():
    """N = K = 1024 at M = 4096: 64 tiles, 8 slices of 4 blocks"""
    M, N, K = 4096, 1024, 1024
    dZ, X, state = block_inputs(M, N, K)
    jobs, _, _, nbytes = _launch([(dZ, X)])
    assert WREF.slices(M, 64) == (8, 512) and nbytes == 8 * (64 * 128 * 128 + 8 * 8 * 128) * 4
    _assert_job(_compare(jobs[0], 64, f"blocks M = {M} x {N} x {K} (4 per slice, 64 tiles)"))
    _two_launches_same_bits([(dZ, X)], jobs)


# ---------------------------------------------------------------- c. range across the blocks of a slice
@pytest.mark.parametrize("kind", RANGE_KINDS)
def test_range_across_the_blocks_of_a_slice(kind):
    """an O(1) block followed, in the same slice, by one at 1e-20 x 1e-12 ("up"), the reverse ("down"), a dZ block at 1e30 followed by one
    at 1e-26 ("bias"): finite operands give finite gradients, the ones of the bounded rescale.  On the commit before the bound "up"
    returned inf / nan in all 16384 elements of dW, "bias" in all of dW and db (profiles/wgrad_image_errors.txt)."""
    dZ, X = range_inputs(kind)
    jobs, _, _, nbytes = _launch([(dZ, X)])
    assert nbytes == 24 * (128 * 128 + 128) * 4 and WREF.slices(4096, 1) == (24, 256)
    got, gotb = jobs[0][2], jobs[0][4]
    print(f"WGI range {kind}: {int((~torch.isfinite(got)).sum())} non-finite of {got.numel()} in dW, {int((~torch.isfinite(gotb)).sum())} of "
          f"{gotb.numel()} in db")
    r = _compare(jobs[0], 1, f"range {kind}")
    _assert_job(r)
    # and the float64 answer itself, to fp32 accuracy: the rows the bound drops are 1e-32 of every element's sum
    assert WREF.rel(np.abs(r.got - r.tW), r.S_all) <= r.tol and WREF.rel(np.abs(r.gotb - r.tb), r.Sb_all) <= r.tolb


@pytest.mark.parametrize("kind", list(CAP_KINDS))
def test_a_block_beyond_the_cap_is_attenuated_against_the_slices_smallest_scale(kind):
    """the bound where it attenuates instead of dropping (inputs: "cap" in tests/test_wgrad_image_oracle.py): the last block of every
    slice lies 90 octaves above the slice's smallest scale -- in one step ("partial"), or over two steps of 45 after a falling one, the
    smallest scale being the second block's, or the first block being all zero ("stairs") -- so its factors carry 18 octaves: features
    living in its rows at 18 / 21 / 24 equal the restatement per element, those at 25 / 28 are exactly 0 (the uncapped rule, a cap
    against the scale in force, or one against the first block's scale would return their gradient), bias alike"""
    M, levels = CAP_KINDS[kind]
    dZ, X, pos, tier, down = cap_inputs(kind)
    jobs, _, _, nbytes = _launch([(dZ, X)])
    assert WREF.slices(M, 1)[1] == 128 * len(levels) and nbytes == WREF.workspace_bytes(M, [(128, 128)])
    r = _compare(jobs[0], 1, f"cap {kind} (levels {levels})")
    gz = cap_feature_group(128)
    dense_cols = np.arange(128) % 16 != 5
    assert r.dropped.sum() > 100
    for g, kr in enumerate(CAP_ROW_K):
        sel, k = np.ix_(gz == g, dense_cols), 18 + kr
        ek = WREF.rel(np.abs(r.got - r.dW)[sel], r.S[sel])
        es = WREF.rel(np.abs(r.dW - r.tW)[sel], r.S_all[sel])
        eb = WREF.rel(np.abs(r.gotb - r.db)[gz == g], r.Sb[gz == g])
        print(f"WGI   cap {kind}, features in the capped block's rows at k = {k}: kernel vs emulation {ek:.2e}, emulation vs float64 {es:.2e}, "
              f"bias kernel vs emulation {eb:.2e}")
        if k >= WREF.DROP_K:
            assert (r.got[gz == g] == 0).all() and (r.gotb[gz == g] == 0).all() and (np.abs(r.tW[sel]) > 0).all() and (r.tb[gz == g] != 0).all()
        else:
            assert ek <= r.tol and eb <= r.tolb and (r.got[sel] != 0).all() and (r.gotb[gz == g] != 0).all()
    for g in (5, 6):           # all rows of the capped block / of the block before it
        sel = np.ix_(gz == g, dense_cols)
        assert WREF.rel(np.abs(r.got - r.dW)[sel], r.S[sel]) <= r.tol and (r.got[sel] != 0).all()
    _assert_job(r)
    assert (r.got[gz == 7] == 0).all() and (r.gotb[gz == 7] == 0).all()


# ---------------------------------------------------------------- d. group mechanics
GROUP_SHAPES = [(1, 128), (128, 1), (140, 5), (5, 140), (12, 128), (128, 256), (256, 140), (130, 130), (64, 64), (1, 1), (300, 17), (17, 300)]


def test_twelve_jobs_unaligned_windows_and_a_job_without_bias():
    """MAX_JOBS_H jobs of mixed shapes in one launch; the gradient window starts at column 3 of a wider, NaN-filled buffer (the reduce
    kernel's element-wise stores: the window's rows are not 16-byte aligned); jobs 2 and 7 have no bias gradient"""
    M = 700
    rng = np.random.default_rng(12)
    pairs = []
    for N, K in GROUP_SHAPES:
        dZ = (rng.standard_normal((M, N)) * np.exp2(-rng.integers(0, 28, (M, 1))) * (rng.random((M, N)) > 0.3)).astype(np.float32)
        X = (rng.standard_normal((M, K)) * np.exp2(-rng.integers(0, 10, (M, 1)))).astype(np.float32)
        pairs.append((dZ, X))
    assert len(pairs) == WREF.MAX_JOBS
    bias = [j not in (2, 7) for j in range(12)]
    jobs, full, _, nbytes = _launch(pairs, wcol0=3, pad=6, bias=bias)
    assert nbytes == WREF.workspace_bytes(M, GROUP_SHAPES)
    tiles_total = sum(_tiles(N, K) for N, K in GROUP_SHAPES)
    for j, (job, buf, (N, K)) in enumerate(zip(jobs, full, GROUP_SHAPES)):
        assert (job[4] is None) == (not bias[j])
        _assert_job(_compare(job, tiles_total, f"group job {j} {M}x{N}x{K} at column 3 of {buf.shape[1]}"))
        assert bool(torch.isnan(buf[:, :3]).all()) and bool(torch.isnan(buf[:, 3 + K:]).all())          # outside the window: untouched


def test_thirteen_jobs_and_a_misaligned_workspace_are_rejected():
    from dtc_amd import _ffi, h2i, ops
    M = 256
    g = torch.Generator().manual_seed(1)
    mk = lambda: (h2i.HImage.from_tensor(torch.randn(M, 16, generator=g).to(DEV)), h2i.HImage.from_tensor(torch.randn(M, 16, generator=g).to(DEV)),
                  torch.zeros(16, 16, device=DEV), 0, None)
    jobs = [mk() for _ in range(13)]
    ws = ops.workspace(h2i.wgrad_group_workspace_bytes(jobs[:12], M) * 2 + 64, DEV)
    with pytest.raises(_ffi.DtcError):
        h2i.wgrad_group_workspace_bytes(jobs, M)
    with pytest.raises(_ffi.DtcError):
        h2i.wgrad_group(jobs, M, ws)
    assert "13" in _ffi.lib().dtc_last_error().decode()
    assert ws.data_ptr() % 16 == 0
    with pytest.raises(_ffi.DtcError):
        h2i.wgrad_group(jobs[:12], M, ws[1:])                     # 8 bytes behind a 16-byte boundary
    assert "aligned" in _ffi.lib().dtc_last_error().decode()
    torch.cuda.synchronize()
    assert all(float(j[2].abs().max()) == 0.0 for j in jobs)      # nothing was launched
    h2i.wgrad_group(jobs[:12], M, ws)                             # the same jobs, accepted
    torch.cuda.synchronize()
    assert all(float(j[2].abs().max()) > 0.0 for j in jobs[:12])


# ---------------------------------------------------------------- e. forward / data gradient: activation rows whose own blocks differ
@pytest.fixture(params=["rows64_default", "rows128_only"])
def tile_rows(request):
    from dtc_amd import _ffi
    _ffi.lib().dtc_h2i_rows64_max(-1 if request.param == "rows64_default" else 0)
    yield request.param
    _ffi.lib().dtc_h2i_rows64_max(-1)


def _row_blocks(M, g):
    """[M, 512]: the four 128-column blocks of every row at O(1), 2^-40, all zero (inherits its predecessor's scale) and 2^+20"""
    A = torch.randn(M, 512, generator=g)
    A[:, 128:256] *= 2.0 ** -40
    A[:, 256:384] = 0.0
    A[:, 384:] *= 2.0 ** 20
    return A


def _feature_blocks(Wt):
    """Wt [features, 512]: feature f sees all four blocks (f % 4 == 0), the first two only (1: the 2^-40 block is 2^-40 of its sum),
    the 2^-40 block alone (2), all but the first (3) -- without this the 2^20 block would hide every other border from every feature"""
    f = torch.arange(Wt.shape[0])
    Wt[f % 4 == 1, 256:] = 0.0
    Wt[f % 4 == 2, :128] = 0.0
    Wt[f % 4 == 2, 256:] = 0.0
    Wt[f % 4 == 3, :128] = 0.0
    return Wt


def test_forward_and_data_gradient_with_row_blocks_of_different_scale(tile_rows):
    from dtc_amd import h2i, ops
    from test_hip_h2i import _assert_like_fp32
    g = torch.Generator().manual_seed(77)
    M = 130
    # forward: X (130, 512) against a (128, 512) weight
    X, W = _row_blocks(M, g).to(DEV), _feature_blocks(torch.randn(128, 512, generator=g) / 512 ** 0.5).to(DEV)
    Ximg = h2i.HImage.from_tensor(X)
    Y = torch.full((M, 128), float("nan"), device=DEV)
    h2i.linear_fwd(Ximg, W, None, Y, None, None)
    Xf = Ximg.to_tensor()
    nat = torch.empty(M, 128, device=DEV)
    ops.linear_fwd(Xf, W, None, nat, None, split=False)
    ref = Xf.double() @ W.double().T
    _assert_like_fp32(Y, ref, nat, f"WGI fwd 130x128x512, row blocks 1 / 2^-40 / 0 / 2^20 ({tile_rows})")
    for grp in range(4):           # each group of features on its own: its rows are not measured against the 2^20 features
        _assert_like_fp32(Y[:, grp::4], ref[:, grp::4], nat[:, grp::4], f"WGI fwd, features seeing blocks {('all', '0 1', '1', '1 3')[grp]} ({tile_rows})")
    # data gradient: dZ (130, 512) against a (512, 128) weight
    dZ, W2 = _row_blocks(M, g).to(DEV), _feature_blocks(torch.randn(128, 512, generator=g) / 512 ** 0.5).T.contiguous().to(DEV)
    dZimg = h2i.HImage.from_tensor(dZ)
    dX = torch.full((M, 128), float("nan"), device=DEV)
    h2i.linear_dgrad(dZimg, W2, dX)
    dZf = dZimg.to_tensor()
    nat2 = torch.empty(M, 128, device=DEV)
    ops.linear_dgrad(dZf, W2, nat2, None, None, split=False)
    ref2 = dZf.double() @ W2.double()
    _assert_like_fp32(dX, ref2, nat2, f"WGI dgrad 130x512x128, row blocks 1 / 2^-40 / 0 / 2^20 ({tile_rows})")
    for grp in range(4):
        _assert_like_fp32(dX[:, grp::4], ref2[:, grp::4], nat2[:, grp::4], f"WGI dgrad, features seeing blocks {('all', '0 1', '1', '1 3')[grp]} ({tile_rows})")
