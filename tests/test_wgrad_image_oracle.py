"""The numpy restatement of the image weight gradient's scaling scheme (oracle/wgrad_image_ref.py) checked on the CPU against
float64 truth and against its own bound, and the input families of the GPU comparison (tests/test_hip_wgrad_image.py): the builders
live here so that both modules see the same inputs.

Families (all values sign x U[1, 2) x a power of two, so a row's exponent -- and with it its distance k below the block's top row
-- is exactly what the builder says):
    tiers   (M, N, K) x mode: inside every 128-row block the rows sit at k in TIERS below the top; mode puts k on dZ alone ("dz"),
            on X alone ("x") or half on each ("split": the bias factor sees eZ only).  dZ features by n % 12: 0 dense, 1..10 non-zero
            only in the rows of tier n % 12 - 1, 11 all zero; X is dense except columns c % 16 == 5 (non-zero only in the rows of tier
            (c // 16) % 10) and column 11 (all zero).
    blocks  M (N = K = 128, and one 1024 x 1024 job): every 128-row block has its own scale on each operand, stepping by up to 20
            octaves per operand (40 in T) in either direction; blocks that are all zero (the first block of slice 0, the last of
            slice 1 among them), blocks with dZ live and X zero (first of slice 2) and the reverse (first of slice 3), rows spread
            over 12 octaves inside a block, 30 % of dZ's entries zero.
    range   M = 4096, one tile, two blocks per slice: "up" = an O(1) block followed by one at 1e-20 x 1e-12, "down" = the reverse
            order, "bias" = a dZ block at 1e30 followed by one at 1e-26.
    cap     the bound on the rescale where it attenuates instead of dropping: the blocks of a slice sit at CAP_LEVELS octaves below
            the slice's loudest block, all of it on dZ (so T and Tz step alike), rows inside a block at CAP_ROW_K below its top.
            "partial" (M = 4096, two blocks per slice): levels (0, 90) -- one step beyond the cap, the second block's factors carry
            the remaining 18 octaves: rows at 18, 21, 24 are attenuated, rows at 25, 28 dropped.  "stairs" (M = 9300, four per slice):
            levels (30, 0, 45, 90) -- no step exceeds 72, the last block is 90 above the slice's smallest scale, which is not the
            first block's; in every third slice the first block is all zero (it must not count as the smallest).  dZ features by
            n % 16: 4..8 live only in the last block of a slice, in its rows of tier n % 16 - 4; 9 in all rows of the last block; 10 in
            all rows of the block before it; 11 all zero; the rest dense.  X columns c % 16 == 5 live only in the last block.
"""
import functools

import numpy as np
import pytest

from oracle import h2image as H
from oracle import wgrad_image_ref as WREF

TIERS = (0, 3, 8, 14, 17, 20, 24, 25, 31, 40)
TIER_SHAPES = ((256, 128, 128), (256, 140, 265))
TIER_MODES = ("dz", "x", "split")
TIER_CASES = [(s, m) for s in TIER_SHAPES for m in TIER_MODES]
BLOCK_MS = (1, 100, 1001, 4101, 6200, 9300)
BLOCKS_PER_SLICE = {1: 1, 100: 1, 1001: 1, 4101: 2, 6200: 3, 9300: 4}
BLOCK_CASES = [(M, 128, 128) for M in BLOCK_MS] + [(4096, 1024, 1024)]
RANGE_KINDS = ("up", "down", "bias")
CAP_KINDS = {"partial": (4096, (0, 90)), "stairs": (9300, (30, 0, 45, 90))}
CAP_ROW_K = (0, 3, 6, 7, 10)


def _unit(rng, shape):
    return (rng.uniform(1.0, 2.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def tier_of_rows(M, seed):
    """index into TIERS of every row: each 128-row block holds every tier (its first row the top one), shuffled"""
    rng = np.random.default_rng(seed)
    t = np.concatenate([np.concatenate([[0], rng.permutation(np.arange(1, 128) % 10)]) for _ in range(-(-M // 128))])
    return t[:M]


def feature_group(N):
    """-1 dense, 0..9 the tier the feature lives in, 10 all zero"""
    return np.arange(N) % 12 - 1


def column_group(K):
    c = np.arange(K)
    g = np.where(c % 16 == 5, (c // 16) % 10, -1)
    g[11 if K > 11 else 0] = 10
    return g


@functools.lru_cache(maxsize=None)
def tier_inputs(shape, mode):
    """-> (dZ float32 [M, N], X float32 [M, K], tier index per row)"""
    M, N, K = shape
    rng = np.random.default_rng(100 * N + K + TIER_MODES.index(mode))
    tier = tier_of_rows(M, N + K)
    k = np.array(TIERS)[tier]
    kz = {"dz": k, "x": 0 * k, "split": k // 2}[mode]
    kx = k - kz
    gz, gx = feature_group(N), column_group(K)
    dZ = np.ldexp(_unit(rng, (M, N)), -kz[:, None]) * ((gz[None, :] == -1) | (gz[None, :] == tier[:, None]))
    X = np.ldexp(_unit(rng, (M, K)), -kx[:, None]) * ((gx[None, :] == -1) | (gx[None, :] == tier[:, None]))
    return dZ.astype(np.float32), X.astype(np.float32), tier


@functools.lru_cache(maxsize=None)
def block_inputs(M, N, K):
    """-> (dZ, X, state per block: 0 both live, 1 all zero, 2 dZ live / X zero, 3 X live / dZ zero)"""
    rng = np.random.default_rng(7000 + M + N)
    nb = -(-M // 128)
    _, rps = WREF.slices(M, -(-N // 128) * -(-K // 128))
    bps = rps // 128
    state = rng.choice([0, 0, 0, 0, 0, 1, 2, 3], nb)
    forced = {0: 1, 2 * bps - 1: 1, 2 * bps: 2, 3 * bps: 3, 1: 0, nb - 1: 0}     # block -> state; later entries win
    if nb == 1:
        forced = {0: 0}
    for b, s in forced.items():
        if b < nb:
            state[b] = s
    sz = np.clip(np.cumsum(rng.integers(-20, 21, nb)), -50, 50)
    sx = np.clip(np.cumsum(rng.integers(-20, 21, nb)), -50, 50)
    rows_z = rng.integers(0, 13, nb * 128)
    rows_x = rng.integers(0, 13, nb * 128)
    rows_z[::128] = rows_x[::128] = 0
    ez = (np.repeat(sz, 128) - rows_z)[:M]
    ex = (np.repeat(sx, 128) - rows_x)[:M]
    st = np.repeat(state, 128)[:M]
    dZ = np.ldexp(_unit(rng, (M, N)), ez[:, None]) * (rng.random((M, N)) > 0.3) * np.isin(st, (0, 2))[:, None]
    X = np.ldexp(_unit(rng, (M, K)), ex[:, None]) * np.isin(st, (0, 3))[:, None]
    return dZ.astype(np.float32), X.astype(np.float32), state


@functools.lru_cache(maxsize=None)
def range_inputs(kind):
    """-> (dZ, X): M = 4096, N = K = 128; the blocks of a slice (two each) alternate between the two scales"""
    M, N, K = 4096, 128, 128
    rng = np.random.default_rng(30 + RANGE_KINDS.index(kind))
    odd = (np.arange(M) // 128) % 2 == 1
    small = odd if kind != "down" else ~odd
    if kind == "bias":
        sz, sx = np.where(small, 1e-26, 1e30), np.ones(M)
    else:
        sz, sx = np.where(small, 1e-20, 1.0), np.where(small, 1e-12, 1.0)
    dZ = _unit(rng, (M, N)).astype(np.float64) * sz[:, None]
    X = _unit(rng, (M, K)).astype(np.float64) * sx[:, None]
    return dZ.astype(np.float32), X.astype(np.float32)


def cap_feature_group(N):
    """-1 dense, 0..4 the tier of the slice's last block the feature lives in, 5 all of the last block, 6 all of the block before it,
    7 all zero"""
    g = np.arange(N) % 16 - 4
    return np.where((g >= 0) & (g <= 7), g, -1)


@functools.lru_cache(maxsize=None)
def cap_inputs(kind):
    """-> (dZ, X, per row: position of its block in its slice, per row: index into CAP_ROW_K, per row: octaves below the slice's
    loudest block); N = K = 128"""
    M, levels = CAP_KINDS[kind]
    N = K = 128
    rng = np.random.default_rng(50 + len(levels))
    nb, bps = -(-M // 128), len(levels)
    assert WREF.slices(M, 1)[1] == bps * 128
    pos = np.repeat(np.arange(nb) % bps, 128)[:M]
    sl = np.repeat(np.arange(nb) // bps, 128)[:M]
    tier = np.concatenate([np.concatenate([[0], rng.permutation(np.arange(1, 128) % len(CAP_ROW_K))]) for _ in range(nb)])[:M]
    down = np.array(levels)[pos] + np.array(CAP_ROW_K)[tier]
    gz = cap_feature_group(N)
    last = pos == bps - 1
    on = (gz[None, :] == -1) | ((gz[None, :] == tier[:, None]) & last[:, None]) | ((gz[None, :] == 5) & last[:, None]) | \
         ((gz[None, :] == 6) & (pos == bps - 2)[:, None])
    dZ = np.ldexp(_unit(rng, (M, N)), (40 - down)[:, None]) * on
    X = _unit(rng, (M, K)) * ((np.arange(K) % 16 != 5)[None, :] | last[:, None])
    if kind == "stairs":
        dead = (pos == 0) & (sl % 3 == 1)
        dZ[dead] = 0.0
        X[dead] = 0.0
    return dZ.astype(np.float32), X.astype(np.float32), pos, tier, down


def cpu_images(dZ, X):
    """the decoded operands and exponent tables of the images a pack of (dZ, X) writes"""
    eZ, eX = H.exponents(dZ), H.exponents(X)
    return WREF.decoded(dZ, eZ), WREF.decoded(X, eX), eZ, eX


def _families():
    """(builder, rescale rule): every family under both rules; the 64-tile job under the kernel's rule alone (its blocks step as those
    of the single-tile cases do)"""
    for rescale in ("as_built", "bounded"):
        for shape, mode in TIER_CASES:
            yield pytest.param(lambda s=shape, m=mode: tier_inputs(s, m)[:2], rescale, id=f"tiers-{shape[1]}x{shape[2]}-{mode}-{rescale}")
        for M, N, K in BLOCK_CASES:
            if N == 128 or rescale == "bounded":
                yield pytest.param(lambda a=(M, N, K): block_inputs(*a)[:2], rescale, id=f"blocks-{M}x{N}-{rescale}")
        for kind in RANGE_KINDS:
            yield pytest.param(lambda k=kind: range_inputs(k), rescale, id=f"range-{kind}-{rescale}")
        for kind in CAP_KINDS:
            yield pytest.param(lambda k=kind: cap_inputs(k)[:2], rescale, id=f"cap-{kind}-{rescale}")


@pytest.mark.parametrize("build,rescale", list(_families()))
def test_scheme_stays_within_its_own_bound(build, rescale):
    """emulation against float64 truth of the decoded operands: inside the bound element by element, before any kernel is involved"""
    dZ, X = build()
    M = dZ.shape[0]
    dZd, Xd, eZ, eX = cpu_images(dZ, X)
    assert np.isfinite(dZd).all() and np.isfinite(Xd).all()
    emu = WREF.emulate(dZd, Xd, eZ, eX, M, rescale=rescale)
    tW, tb = WREF.truth(dZd, Xd)
    eW, eb = np.abs(emu.dW - tW), np.abs(emu.db - tb)
    assert (eW <= emu.bound).all(), float((eW - emu.bound).max())
    assert (eb <= emu.bound_b).all(), float((eb - emu.bound_b).max())
    # the bound is no blanket: where no row was dropped it is the 2^-22 of the product left out plus the subnormal roundings of rows
    # that are at least 2^-11 below the top (lo reaches fp16's subnormals 11 octaves before hi does)
    clean = emu.S == emu.S_all
    assert WREF.rel(emu.bound[clean], emu.S[clean]) <= 2.0 ** -15 * 1.01
    print(f"scheme vs truth: {WREF.rel(eW, emu.S_all):.2e} of S_all (bound {WREF.rel(emu.bound, emu.S_all):.2e}), "
          f"bias {WREF.rel(eb, emu.Sb_all):.2e}, rows dropped {int(emu.dropped.sum())} of {M}")


@pytest.mark.parametrize("shape,mode", TIER_CASES)
def test_tier_inputs_sit_where_they_claim(shape, mode):
    """the exponent tables of the tier inputs put every row exactly k below its block's top, on the operand the mode names"""
    dZ, X, tier = tier_inputs(shape, mode)
    M, N, K = shape
    eZ, eX = H.exponents(dZ), H.exponents(X)
    k = np.array(TIERS)[tier]
    for tr in range(eZ.shape[1]):
        for tc in range(eX.shape[1]):
            esum = (eZ[:, tr] + eX[:, tc]).reshape(-1)[:M]
            assert np.array_equal(esum - 28, k)
    kz = (eZ[:, 0].reshape(-1)[:M] - 14)
    assert np.array_equal(kz, {"dz": k, "x": 0 * k, "split": k // 2}[mode])
    # dense features are dense, tier features live in their tier only, the zero feature is zero
    gz = feature_group(N)
    for g in range(10):
        assert (dZ[tier != g][:, gz == g] == 0).all() and (dZ[tier == g][:, gz == g] != 0).all()
    assert (dZ[:, gz == -1] != 0).all() and (dZ[:, gz == 10] == 0).all()


def test_fp16_keeps_min_22_38_minus_k_bits_and_nothing_from_k_25():
    """a row of an image times fp16(2^-k): error relative to the row's largest element, k = 0 .. 24, and the factor itself from 25 on"""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((128, 128)) * np.exp2(rng.uniform(-12, 0, (128, 128)))).astype(np.float32)
    ex = H.exponents(x)
    hi, lo = WREF.planes(x, ex)
    top = np.abs(hi.astype(np.float64)).max(axis=1)
    assert (top >= 2.0 ** 14).all() and (top < 2.0 ** 15).all()
    exact = hi.astype(np.float64) + lo.astype(np.float64)
    for k in range(0, 25):
        f = np.float16(2.0 ** -k)
        assert float(f) == 2.0 ** -k
        got = ((hi * f).astype(np.float64) + (lo * f).astype(np.float64)) * 2.0 ** k
        err = float((np.abs(got - exact).max(axis=1) / top).max())
        bits = WREF.bits_kept(k)
        print(f"k = {k:2d}: error 2^{np.log2(err) if err else -np.inf:.1f} of the row's largest element, {bits} bits kept by the derivation")
        # the multiplication adds at most 2^-(38 - k) (two subnormal roundings of 2^-25 against a top of 2^(14 - k)) ...
        assert err <= 2.0 ** -(38 - k)
        # ... and from the k at which lo's low bits cross 2^-24 it really does lose them: the figure is the kernel's, not a loose bound
        if k >= 8:
            assert err >= 2.0 ** -(39 - k) / 4
        if k == 0:
            assert err == 0.0
        if bits < 22:
            assert err <= 2.0 ** -bits
    assert WREF.bits_kept(24) == 14 and WREF.bits_kept(16) == 22 and WREF.bits_kept(17) == 21
    for k in range(25, 45):
        f = np.ldexp(np.float32(1.0), max(-k, WREF.F_CLAMP)).astype(np.float16)
        assert float(f) == 0.0 and WREF.bits_kept(k) == 0
        assert not (hi * f).any() and not (lo * f).any()


@pytest.mark.parametrize("kind", RANGE_KINDS)
def test_unbounded_rescale_overflows_where_the_bounded_one_gives_the_answer(kind):
    dZ, X = range_inputs(kind)
    M = dZ.shape[0]
    dZd, Xd, eZ, eX = cpu_images(dZ, X)
    tW, tb = WREF.truth(dZd, Xd)
    assert np.isfinite(dZd).all() and np.isfinite(Xd).all() and np.isfinite(tW.astype(np.float32)).all()
    built = WREF.emulate(dZd, Xd, eZ, eX, M, rescale="as_built", want_bound=False)
    bounded = WREF.emulate(dZd, Xd, eZ, eX, M, rescale="bounded")
    assert built.rows_per_split == 256 and built.splits == 24
    steps = [b[3] - a[3] for a, b in zip(built.T, built.T[1:]) if b[2] % 2 == 1]
    print(f"{kind}: T steps at the borders inside a slice {min(steps)} .. {max(steps)}; as built: {int((~np.isfinite(built.dW32)).sum())} inf / nan in dW, "
          f"{int((~np.isfinite(built.db32)).sum())} in db")
    if kind == "down":
        assert np.isfinite(built.dW32).all() and np.isfinite(built.db32).all()          # a falling scale cannot overflow
    else:
        # every slice's accumulators reach +-inf; the reduce kernel's sum of the slices is then inf or (inf - inf) nan
        assert max(steps) > 100 and not np.isfinite(built.dW32).any()
        assert (not np.isfinite(built.db32).any()) == (kind == "bias") and np.isfinite(built.db32).all() == (kind == "up")
    # bounded: finite, and the float64 answer to fp32 accuracy (32 roundings of partial sums <= S: 2 blocks per slice, 16 slices)
    assert np.isfinite(bounded.dW32).all() and np.isfinite(bounded.db32).all()
    assert WREF.rel(np.abs(bounded.dW32 - tW), bounded.S_all) < 40 * 2.0 ** -24
    assert WREF.rel(np.abs(bounded.db32 - tb), bounded.Sb_all) < 40 * 2.0 ** -24
    assert (np.abs(bounded.dW - tW) <= bounded.bound).all()


def test_a_feature_that_lives_only_in_dropped_rows_gets_exactly_zero():
    shape = TIER_SHAPES[1]
    for mode in TIER_MODES:
        dZ, X, tier = tier_inputs(shape, mode)
        dZd, Xd, eZ, eX = cpu_images(dZ, X)
        emu = WREF.emulate(dZd, Xd, eZ, eX, shape[0])
        tW, tb = WREF.truth(dZd, Xd)
        gz, gx = feature_group(shape[1]), column_group(shape[2])
        lost = np.isin(gz, [i for i, k in enumerate(TIERS) if k >= WREF.DROP_K])
        assert lost.sum() >= 3 * (shape[1] // 12)
        dense_cols = gx == -1
        assert (emu.dW[lost] == 0).all() and (np.abs(tW[lost][:, dense_cols]) > 0).all()
        assert (emu.S[lost] == 0).all() and (emu.S_all[lost][:, dense_cols] > 0).all()
        assert np.array_equal(emu.dropped, np.array(TIERS)[tier] >= WREF.DROP_K)
        # the bias factor sees eZ alone: the feature's bias gradient is lost only where the whole distance sits on dZ
        assert (emu.db[lost] == 0).all() == (mode == "dz") and (tb[lost] != 0).all()
        # kept tiers are there, the all-zero feature and column are zero
        kept = (gz >= 0) & (gz < 10) & ~lost
        assert (emu.dW[kept][:, dense_cols] != 0).all()
        assert (emu.dW[gz == 10] == 0).all() and (emu.dW[:, gx == 10] == 0).all()


def test_slices_and_workspace_restate_the_plan():
    for M, bps in BLOCKS_PER_SLICE.items():
        s, rps = WREF.slices(M, 1)
        assert rps // 128 == bps and s * rps >= M, (M, s, rps)
    assert WREF.slices(4096, 64) == (8, 512) and WREF.slices(4096, 1) == (24, 256) and WREF.slices(256, 6) == (8, 128)
    assert WREF.workspace_bytes(4096, [(128, 128)]) == 24 * (128 * 128 + 128) * 4
    assert WREF.workspace_bytes(256, [(140, 265)]) == 8 * (6 * 128 * 128 + 3 * 2 * 128) * 4


def test_the_bound_on_the_scale_changes_nothing_on_ordinary_data():
    """no border of the tier and block inputs' neighbours-in-scale, nor of rows spread over 1e-8 .. 1, steps further than the cap:
    the same T, the same factors, the same sums"""
    rng = np.random.default_rng(11)
    M = 1024
    dZ = (rng.standard_normal((M, 128)) * 10.0 ** (-8 * rng.random((M, 1))) * (rng.random((M, 1)) > 0.3)).astype(np.float32)
    X = (rng.standard_normal((M, 128)) * 10.0 ** (-3 * rng.random((M, 1)))).astype(np.float32)
    for a, b in ((dZ, X), tier_inputs(TIER_SHAPES[0], "split")[:2]):
        dZd, Xd, eZ, eX = cpu_images(a, b)
        one = WREF.emulate(dZd, Xd, eZ, eX, a.shape[0], rescale="as_built", tiles_total=64, want_bound=False)
        two = WREF.emulate(dZd, Xd, eZ, eX, a.shape[0], rescale="bounded", tiles_total=64, want_bound=False)
        assert one.T == two.T and np.array_equal(one.dW32, two.dW32) and np.array_equal(one.db32, two.db32)


@pytest.mark.parametrize("kind", list(CAP_KINDS))
def test_the_bound_attenuates_a_block_beyond_the_cap_against_the_slices_smallest_scale(kind):
    """where the remainder of a capped step is below 25 octaves the block is attenuated, not dropped: its rows keep what rows that far
    below a block's top keep, features that live in its rows at 25 and more get exactly 0 where the uncapped rule returns their
    gradient, and the cap counts from the smallest scale of the slice so far, wherever in the slice that was"""
    dZ, X, pos, tier, down = cap_inputs(kind)
    M, levels = CAP_KINDS[kind]
    bps = len(levels)
    dZd, Xd, eZ, eX = cpu_images(dZ, X)
    # the inputs sit where they claim: eZ = 14 - 40 + octaves below the loudest block, eX = 14
    live = np.abs(dZ).any(axis=1)
    assert np.array_equal(eZ[:, 0].reshape(-1)[:M][live], (down - 26)[live]) and (eX[:, 0].reshape(-1)[:M][live] == 14).all()
    steps = np.diff(levels)
    assert steps.max() <= WREF.RESCALE_CAP or kind == "partial"
    assert max(levels) - min(levels) - WREF.RESCALE_CAP == 18 and (kind == "partial" or levels.index(min(levels)) > 0)
    built = WREF.emulate(dZd, Xd, eZ, eX, M, rescale="as_built")
    bounded = WREF.emulate(dZd, Xd, eZ, eX, M, rescale="bounded")
    tW, tb = WREF.truth(dZd, Xd)
    # T and Tz: the two rules differ in the last block of every full slice, by the 18 octaves that go into the factors, and nowhere else
    nfull = 0
    for (_, _, b, T1, Tz1), (_, _, _, T2, Tz2) in zip(built.T, bounded.T):
        if b % bps == bps - 1:
            assert (T1 - T2, Tz1 - Tz2) == (18, 18), (b, T1, T2, Tz1, Tz2)
            nfull += 1
        else:
            assert (T1, Tz1) == (T2, Tz2)
    assert nfull == (-(-M // 128)) // bps
    # rows: attenuated (kept, f < 1) and dropped ones, as the tiers say
    k_total = 18 + np.array(CAP_ROW_K)[tier]
    lastb = (pos == bps - 1) & live
    assert np.array_equal(bounded.dropped, lastb & (k_total >= WREF.DROP_K)) and not built.dropped.any()
    assert (lastb & (k_total < WREF.DROP_K)).sum() > 100
    # the sums: features that live in the last block's rows at 25 / 28 are exactly 0 under the bound, their gradient otherwise
    gz = cap_feature_group(128)
    dense_cols = np.arange(128) % 16 != 5
    for g, kr in enumerate(CAP_ROW_K):
        sel = np.ix_(gz == g, dense_cols)
        k = 18 + kr
        if k >= WREF.DROP_K:
            assert (bounded.dW[gz == g] == 0).all() and (bounded.db[gz == g] == 0).all() and (bounded.S[gz == g] == 0).all()
            assert (built.dW[sel] != 0).all() and (built.db[gz == g] != 0).all()
        else:
            es = WREF.rel(np.abs(bounded.dW - tW)[sel], bounded.S_all[sel])
            print(f"{kind}: feature in the capped block's rows at k = {k}: scheme vs truth {es:.2e}")
            assert (bounded.dW[sel] != 0).all() and es <= 2.0 ** -22 * 1.01 + 2.0 ** -(38 - k)
            eb = WREF.rel(np.abs(built.dW - tW)[sel], built.S_all[sel])
            assert eb <= 2.0 ** -22 * 1.01                                     # the uncapped rule keeps 22 bits here ...
            if k == 24:
                assert es > 8 * eb                                             # ... the capped one what a row 24 below the top keeps
            assert np.array_equal(bounded.db[gz == g], tb[gz == g])            # a power-of-two factor: exact
    # the block before the last is not capped (45 above the smallest, or the loudest itself): its features keep all their bits
    sel = np.ix_(gz == 6, dense_cols)
    assert WREF.rel(np.abs(bounded.dW - tW)[sel], bounded.S_all[sel]) <= 2.0 ** -22 * 1.01
    assert (np.abs(bounded.dW - tW) <= bounded.bound).all() and (np.abs(bounded.db - tb) <= bounded.bound_b).all()
    assert np.isfinite(bounded.dW32).all() and np.isfinite(bounded.db32).all()
    assert WREF.rel(np.abs(bounded.dW32 - bounded.dW), bounded.S) < WREF.chain_tolerance(M, 1)


def test_planes_and_decoded_equal_the_format_restatement():
    """planes() / decoded() against oracle/h2image.py's byte-exact encode / decode: the same hi / lo planes, the same decoded values"""
    rng = np.random.default_rng(3)
    for M, K in ((130, 265), (256, 128), (1, 5)):
        A = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-30, 30, (M, 1)))).astype(np.float32)
        A[rng.random((M, K)) < 0.2] = 0.0
        if M > 1:
            A[3] = 0.0
        chunks, ex = H.encode(A)
        hi, lo = WREF.planes(A, ex)
        r = np.arange(128)
        for t in range(chunks.shape[0]):
            for st in range(chunks.shape[1]):
                for h in range(2):
                    slot = 2 * r + (h ^ ((r >> 3) & 1))
                    cols = slice(st * 16 + 8 * h, st * 16 + 8 * h + 8)
                    assert np.array_equal(chunks[t, st, 0, slot], hi[t * 128:(t + 1) * 128, cols].view(np.uint16))
                    assert np.array_equal(chunks[t, st, 1, slot], lo[t * 128:(t + 1) * 128, cols].view(np.uint16))
        assert np.array_equal(WREF.decoded(A, ex), H.decode(chunks, ex, M, K).astype(np.float64))
