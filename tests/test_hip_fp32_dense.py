"""The single-pass fp32 MFMA dense layers (csrc/gemm.hip: linear_fwd_kernel, linear_dgrad_kernel; csrc/wgrad.hip: linear_wgrad_kernel,
wgrad_reduce_kernel) against float64, every template instance at its own shapes.  The case tables and two checks of them run on the CPU,
everything else needs the GPU.

The kernels are reached on purpose: the tests call the C entry points (dtc_linear_fwd, _mask, _amax, _list, _mse; dtc_linear_dgrad, _mask,
_split; dtc_linear_wgrad with the split switch off) through _ffi, not through ops' routing, and the library's launch profile must show
exactly the expected linear_fwd / linear_dgrad / linear_wgrad + wgrad_reduce launch of the case's work (2 M N K) and nothing else (no
weight image, pack or amax launch).  Which template instance a shape gets is host arithmetic, restated below (`fwd_variant`,
`dgrad_variant`, `split_variant`, `wgrad_variant`); test_case_tables_reach_every_variant holds the tables to it.

Every forward and data-gradient shape runs with DTC_GEMM_DEEP_BLOCKS = 0 and = 100000: the single-stage and the two-stages-ahead kernel
must agree bit for bit, and the result is measured against float64.  That is the only way linear_fwd_kernel<64, deep> and
linear_dgrad_kernel<64, deep> run at all: a 64-wide launch has at least 320 workgroups (pick_bn_rows) and the default threshold is 300.

Measures (tests/recurrence_ref.py): forward and data gradient row_rel = the largest error of a row over that row's largest reference
element; for the `heavy` inputs also S = max |got - ref| / (|X| |W|^T + |b|) per element; weight gradient s_rel (dW) and s_rel_bias (db).
Each is held to bound(e32) = 8 x the same measure of torch's fp32 product of the same operands on the CPU (at least 2^-20, at most 2e-5).
No reference row is all zero (checked on the CPU too).  No case needed a kernel fix.

One-column outputs -- forward (129, 1, 128), data gradient (129, 128, 1) -- are held to the S measure, on plain inputs too, and their
row measure is printed, not asserted (`row 1col` below).  With one element per row, row_rel is that element's relative error, which has
no bound where its 128 terms cancel: of 129 rows some always cancel to 1e-2 of their terms and less, and torch's own fp32 product then
misses float64 by 1.5e-5 / 3.0e-5 on the CPU next to the GPU and by 6.8e-5 / 1.35e-4 on another (the kernels: 6.0e-5 / 1.13e-4), at and
past the 2e-5 ceiling that bounds it.  No summation order in fp32 meets that, so it says nothing about the kernel; against its own terms
the same outputs are within 1.0e-7 (bound 9.5e-7).

One run on an MI355X, one line per case; every entry is error / e32 / bound in units of 1e-7; e32 is the figure of the CPU that ran next to
it (another CPU's fp32 matrix product sums in another order and moves e32 by a small factor).  `a = b`: the kernels of the two thresholds.

Forward (dtc_linear_fwd, _mask, _amax, _list; dtc_linear_fwd_mse with the sum of squares as `sumsq`):

case, kind, kernels                                                               row           row 1col                  S              sumsq
fwd (14885, 693, 72) plain fwd<128> = fwd<128>                           4.7/4.5/36.1                  -                  -                  -
fwd (14885, 693, 72) heavy fwd<128> = fwd<128>                           6.9/7.0/56.0                  -       3.1/3.3/26.3                  -
fwd (14976, 768, 64) plain fwd<128> = fwd<128>                           4.7/4.8/38.4                  -                  -                  -
fwd (5000, 500, 140) plain fwd<64> = fwd<64,deep>                        6.8/5.6/44.5                  -                  -                  -
fwd (5000, 500, 140) heavy fwd<64> = fwd<64,deep>                        8.9/9.7/77.5                  -       3.0/3.3/26.8                  -
fwd (5120, 512, 40) plain fwd<64> = fwd<64,deep>                         4.0/3.1/25.1                  -                  -                  -
fwd (2200, 500, 100) plain fwd<32> = fwd<32,deep>                        4.3/4.1/32.8                  -                  -                  -
fwd (2200, 500, 100) heavy fwd<32> = fwd<32,deep>                        7.2/6.3/50.3                  -       2.8/3.2/25.4                  -
fwd (300, 70, 100) plain fwd<32> = fwd<32,deep>                          4.2/5.2/41.3                  -                  -                  -
fwd (300, 70, 100) heavy fwd<32> = fwd<32,deep>                          9.3/5.7/45.5                  -       1.8/1.7/13.9                  -
fwd (256, 64, 48) plain fwd<32> = fwd<32,deep>                           2.8/3.1/24.9                  -                  -                  -
fwd (129, 1, 128) plain fwd<32> = fwd<32,deep>                                      -  599.0/145.3/200.0        1.0/0.4/9.5                  -
fwd (257, 12, 128) plain fwd<32> = fwd<32,deep>                          5.7/5.7/46.0                  -                  -                  -
fwd (64, 35, 19) plain fwd<32> = fwd<32,deep>                            1.4/1.6/13.1                  -                  -                  -
mse (300, 693, 64) plain fwd<64,MSE>                                     3.0/2.9/23.3                  -                  -        0.0/0.0/9.5
mse (300, 693, 64) heavy fwd<64,MSE>                                     6.1/4.9/39.2                  -       2.7/2.6/20.7        0.2/0.1/9.5
mse (1000, 70, 128) plain fwd<64,MSE>                                    4.8/5.1/40.5                  -                  -        0.0/0.0/9.5
mse (130, 70, 1) plain fwd<64,MSE>                                       1.3/1.3/10.6                  -                  -        0.0/0.0/9.5
mse (257, 35, 15) plain fwd<64,MSE>                                      1.7/2.1/16.9                  -                  -        0.0/0.0/9.5
fwd (256, 64, 48) plain layout ld                                        2.8/3.1/24.9                  -                  -                  -
fwd (256, 64, 48) plain layout off4                                      2.8/3.1/24.9                  -                  -                  -
fwd (256, 64, 48) plain layout odd                                       2.8/3.1/24.9                  -                  -                  -
fwd gathered (256, 70, 100) plain                                        5.4/4.8/38.4                  -                  -                  -
fwd (300, 70, 100) plain layout ld                                       4.2/5.2/41.3                  -                  -                  -
fwd (300, 70, 100) plain layout off4                                     4.2/5.2/41.3                  -                  -                  -
fwd (300, 70, 100) plain layout odd                                      4.2/5.2/41.3                  -                  -                  -
fwd gathered (300, 70, 100) plain                                        4.9/4.1/32.4                  -                  -                  -

Data gradient (dtc_linear_dgrad, _mask, _split; a / n / p: accumulating, NULL and plain destination segments):

case, kind, kernels                                                               row           row 1col                  S
dgrad (5000, 70, 500) plain dgrad<64> = dgrad<64,deep>                   6.1/6.1/49.0                  -                  -
dgrad (5000, 70, 500) heavy dgrad<64> = dgrad<64,deep>                   7.5/6.8/54.6                  -       5.8/6.2/49.5
dgrad (2200, 70, 500) plain dgrad<32> = dgrad<32,deep>                   6.2/7.5/59.9                  -                  -
dgrad (2200, 70, 500) heavy dgrad<32> = dgrad<32,deep>                   8.5/9.2/73.7                  -       5.5/5.3/42.5
dgrad (300, 100, 70) a plain dgrad<32> = dgrad<32,deep>                  4.4/4.4/35.0                  -                  -
dgrad (300, 100, 70) a heavy dgrad<32> = dgrad<32,deep>                  6.7/5.6/45.0                  -       3.4/2.9/22.9
dgrad (129, 128, 1) plain dgrad<32> = dgrad<32,deep>                                - 1134.0/295.8/200.0        0.9/0.3/9.5
dgrad (257, 128, 12) plain dgrad<32> = dgrad<32,deep>                    8.4/8.6/68.9                  -                  -
dgrad (300, 40, 117) np plain dgrad<32> = dgrad<32,deep>                 3.3/4.6/36.5                  -                  -
dgrad (2200, 70, 500) pap plain dgrad<32> = dgrad<32,deep>               4.8/4.8/38.3                  -                  -
dgrad (257, 24, 83) pap plain dgrad<32> = dgrad<32,deep>                 2.6/2.6/20.6                  -                  -
dgrad (14976, 24, 768) mask plain dgrad<64> = dgrad<64,deep>             4.4/4.4/34.8                  -                  -
dgrad (5120, 40, 512) mask plain dgrad<64> = dgrad<64,deep>              4.7/4.4/34.9                  -                  -
dgrad (256, 48, 64) mask plain dgrad<32> = dgrad<32,deep>                4.3/3.6/29.1                  -                  -
dgrad (256, 48, 64) plain layout ld                                      4.3/3.6/29.1                  -                  -
dgrad (256, 48, 64) plain layout off4                                    4.3/3.6/29.1                  -                  -
dgrad (256, 48, 64) plain layout odd                                     4.3/3.6/29.1                  -                  -
dgrad (300, 100, 70) plain layout ld                                     5.9/6.2/49.3                  -                  -
dgrad (300, 100, 70) plain layout off4                                   5.9/6.2/49.3                  -                  -
dgrad (300, 100, 70) plain layout odd                                    5.9/6.2/49.3                  -                  -
split (130, 96, 64) / 1 plain split<32>                                  4.8/4.8/38.6                  -                  -
split (130, 96, 64) / 3 plain split<32>                                  3.0/3.0/24.0                  -                  -
split (130, 96, 64) / 3 heavy split<32>                                  6.7/7.2/57.6                  -       3.7/3.6/28.5
split (5000, 384, 500) / 1 plain split<64>                              15.2/7.9/63.2                  -                  -
split (5000, 384, 500) / 3 plain split<64>                               7.8/7.6/60.9                  -                  -
split (5000, 384, 500) / 3 heavy split<64>                              11.1/9.7/77.9                  -       7.3/7.3/58.1

Weight gradient (dtc_linear_wgrad, split switch off):

case, kind, kernels                                                                dW                 db
wgrad (1100, 128, 130) plain wgrad<64> reduce<4> 16 splits                0.4/1.0/9.5        0.1/0.2/9.5
wgrad (1100, 128, 130) heavy wgrad<64> reduce<4> 16 splits               1.2/2.8/22.6        0.4/0.3/9.5
wgrad (3000, 12, 128) plain wgrad<64> reduce<16> 24 splits                0.3/0.3/9.5        0.1/0.1/9.5
wgrad (3000, 12, 128) heavy wgrad<64> reduce<16> 24 splits                0.9/0.9/9.5        0.1/0.2/9.5
wgrad (777, 70, 32) plain wgrad<32> reduce<4> 8 splits                    0.4/0.6/9.5        0.1/0.1/9.5
wgrad (777, 70, 32) heavy wgrad<32> reduce<4> 8 splits                   2.1/2.3/18.6        0.6/0.8/9.5
wgrad (1100, 1, 128) plain wgrad<64> reduce<4> 16 splits                  0.3/1.1/9.5        0.0/0.0/9.5
wgrad (1536, 512, 752) gathered plain wgrad<64> reduce<4> 16 splits        0.4/0.7/9.5        0.1/0.2/9.5
wgrad (129, 35, 64) plain wgrad<64> reduce<4> 8 splits                   0.6/1.9/14.8        0.2/0.3/9.5
wgrad (129, 35, 64) plain layout ld                                      0.6/1.9/14.8        0.2/0.3/9.5
wgrad (129, 35, 64) plain layout off4                                    0.6/1.9/14.8        0.2/0.3/9.5
wgrad (129, 35, 64) plain layout odd                                     0.6/1.9/14.8        0.2/0.3/9.5
wgrad (129, 35, 64) plain layout gather                                  0.9/1.8/14.2        0.3/0.3/9.5
wgrad (777, 70, 32) plain layout ld                                       0.4/0.6/9.5        0.1/0.1/9.5
wgrad (777, 70, 32) plain layout off4                                     0.4/0.6/9.5        0.1/0.1/9.5
wgrad (777, 70, 32) plain layout odd                                      0.4/0.6/9.5        0.1/0.1/9.5
wgrad (777, 70, 32) plain layout gather                                   0.4/0.6/9.5        0.1/0.2/9.5
"""
import contextlib
import ctypes
import functools

import pytest
import torch

import recurrence_ref as rr

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = -7777.0
ENV = "DTC_GEMM_DEEP_BLOCKS"
THRESHOLDS = ("0", "100000")
F = torch.nn.functional


# ---------------------------------------------------------------- the launches' host arithmetic, restated
BM, BK = 128, 16                                        # gemm_core.hpp:13-17


def cdiv(a, b):
    return -(-a // b)


def wide_tiles(rows, cols):                             # gemm.hip:807-810
    return cols >= 128 and cdiv(rows, BM) * cdiv(cols, 128) >= 700


def pick_bn_rows(rows, cols):                           # gemm.hip:812-816
    return 32 if cols <= 32 or cdiv(rows, BM) * cdiv(cols, 64) < 320 else 64


def grid_for(row_tiles, col_tiles):                     # gemm_core.hpp:124
    return 8 * cdiv(row_tiles, 8) * col_tiles


def _deep(grid, thr):                                   # gemm.hip:824-827 (deep_variant; 300 without the variable)
    return grid <= thr


def fwd_variant(M, N, thr=300):                         # gemm.hip:875-893
    if wide_tiles(M, N):
        return "fwd<128>"
    bn = pick_bn_rows(M, N)
    return f"fwd<{bn},deep>" if _deep(grid_for(cdiv(M, BM), cdiv(N, bn)), thr) else f"fwd<{bn}>"


def dgrad_variant(M, cols, thr=300):                    # gemm.hip:993-1010; cols = K minus the leading NULL segments
    bn = pick_bn_rows(M, cols)
    return f"dgrad<{bn},deep>" if _deep(grid_for(cdiv(M, BM), cdiv(cols, bn)), thr) else f"dgrad<{bn}>"


def split_variant(M, K, nsplit):                        # gemm.hip:1040-1047 (never deep)
    return "split<32>" if K <= 32 or cdiv(M, BM) * cdiv(K, 64) * nsplit < 320 else "split<64>"


def part_ld(K):                                         # gemm_core.hpp:23
    return (K + 4) & ~3


def wgrad_variant(M, N, widths):                        # wgrad.hip (pick_bn, dtc_linear_wgrad), wgrad_plan.hpp (wgrad_slices, SLICES_LAYER)
    """-> (partial kernel, reduce kernel, splits, rows per split); widths: the segments of X"""
    K = sum(widths)
    bn = 32 if K <= 32 else 64
    tiles = cdiv(N, BM) * sum(cdiv(w, bn) for w in widths)
    splits = min(max(1024 // tiles // 8 * 8, 8), cdiv(cdiv(M, BK * 8), 8) * 8)
    red = 4 if N * part_ld(K) >= 1 << 17 or splits <= 16 else 16
    return f"wgrad<{bn}>", f"reduce<{red}>", splits, cdiv(cdiv(M, splits), BK) * BK


# ---------------------------------------------------------------- case tables
# forward (M, N, K, activation, entry point, also `heavy`)
FWD_CASES = [
    (14885, 693, 72, "elu", "fwd", True),               # <128>: 117 x 6 = 702 tiles, row tail 37, column tail 53, K % 16 = 8
    (14976, 768, 64, "relu", "amax+mask", False),       # <128>: full tiles, sign record, wide epilogue, amax record
    (5000, 500, 140, "relu", "fwd", True),              # <64> / <64,deep>: 40 x 8 = 320 blocks, grid 320
    (5120, 512, 40, "relu", "mask", False),             # <64> / <64,deep>: full tiles, sign record
    (2200, 500, 100, None, "list", True),               # <32>: grid 384 (non-deep at the default threshold)
    (300, 70, 100, "elu", "amax", True),                # <32,deep> at the default threshold
    (256, 64, 48, "relu", "mask", False),               # <32>: full tiles, sign record
    (129, 1, 128, "elu", "fwd", False),                 # one output feature, a one-row tail
    (257, 12, 128, None, "fwd", False),
    (64, 35, 19, "relu", "fwd", False),                 # half a row tile, K = 16 + 3
]
# output layer + MSE (M, N, K, also `heavy`): always linear_fwd_kernel<64, MSE>
MSE_CASES = [(300, 693, 64, True), (1000, 70, 128, False), (130, 70, 1, False), (257, 35, 15, False)]
# data gradient (M, N, K, activation, destination segments or None, entry point, also `heavy`); the tile follows the output width K
DGRAD_CASES = [
    (5000, 70, 500, "relu", None, "dgrad", True),                                           # <64> / <64,deep>
    (2200, 70, 500, None, None, "dgrad", True),                                             # <32>, grid 384
    (300, 100, 70, "elu", (("acc", 70),), "dgrad", True),                                   # <32,deep>; accumulating, with act'
    (129, 128, 1, "elu", None, "dgrad", False),
    (257, 128, 12, None, None, "dgrad", False),
    (300, 40, 117, None, (("null", 53), ("plain", 64)), "dgrad", False),                    # two segments, the leading one NULL
    (2200, 70, 500, None, (("plain", 100), ("acc", 144), ("plain", 256)), "dgrad", False),  # three, wide stores inside a segment
    (257, 24, 83, None, (("plain", 16), ("acc", 3), ("plain", 64)), "dgrad", False),        # three, unaligned
    (14976, 24, 768, "relu", None, "mask", False),                                          # sign record of a <128> forward
    (5120, 40, 512, "relu", None, "mask", False),                                           # sign record, <64> at exactly 320 blocks
    (256, 48, 64, "relu", None, "mask", False),                                             # sign record, <32>
]
# dtc_linear_dgrad_split (M, N, K, nsplit, also `heavy`)
SPLIT_CASES = [(130, 96, 64, 1, False), (130, 96, 64, 3, True), (5000, 384, 500, 1, False), (5000, 384, 500, 3, True)]
# weight gradient with the split switch off (M, N, K, segments of X or None, also `heavy`); a segment: (width, col0, source width, gather)
CRITIC_X = ((53, 0, 53, True), (3, 0, 3, True), (696, 693, 1389, True))
WGRAD_CASES = [
    (1100, 128, 130, None, True),                       # a wide layer (N K >= 128^2, M >= 1024): <64>, 16 splits, reduce<4>
    (3000, 12, 128, None, True),                        # 24 splits, reduce<16>
    (777, 70, 32, None, True),                          # <32>
    (1100, 1, 128, None, False),                        # one output feature
    (1536, 512, 752, CRITIC_X, False),                  # segmented and gathered X, repeated indices
    (129, 35, 64, None, False),                         # 8 splits of 32 rows: the fifth holds one row, three are empty
]
LAYOUTS = ("ld", "off4", "odd")
FWD_LAYOUT_SHAPES = [(256, 64, 48, "relu"), (300, 70, 100, "elu")]          # full tiles (the wide epilogue while it may) / tails
DGRAD_LAYOUT_SHAPES = [(256, 48, 64, "relu"), (300, 100, 70, "elu")]
WGRAD_LAYOUT_SHAPES = [(129, 35, 64), (777, 70, 32)]
GATHER_X = ((53, 0, 53, True), (16, 0, 16, False), (3, 0, 35, False), (28, 5, 40, True))          # K = 100
# row independence: one shape per variant (the threshold that selects it)
FWD_ROW_SHAPES = [(14885, 693, 72, "elu", "0"), (5000, 500, 140, "relu", "0"), (5000, 500, 140, "relu", "100000"),
                  (2200, 500, 100, None, "0"), (300, 70, 100, "elu", "100000")]
DGRAD_ROW_SHAPES = [(5000, 70, 500, "relu", "0"), (5000, 70, 500, "relu", "100000"), (2200, 70, 500, None, "0"),
                    (300, 100, 70, "elu", "100000")]

REQUIRED_VARIANTS = {"fwd<128>", "fwd<64>", "fwd<64,deep>", "fwd<32>", "fwd<32,deep>", "fwd<64,MSE>", "dgrad<64>", "dgrad<64,deep>",
                     "dgrad<32>", "dgrad<32,deep>", "split<32>", "split<64>", "wgrad<64>", "wgrad<32>", "reduce<4>", "reduce<16>"}


def _kinds(heavy):
    return ("plain", "heavy") if heavy else ("plain",)


def _skip(segs):
    """leading NULL columns of a destination"""
    n = 0
    for kind, w in segs or ():
        if kind != "null":
            break
        n += w
    return n


def _widths(K, spec):
    return [s[0] for s in spec] if spec else [K]


# ---------------------------------------------------------------- inputs and float64 references (CPU)
def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * p for k, p in zip(key, (1, 7, 31, 1009, 5003))) + 12345)


def _act(z, act):
    return torch.relu(z) if act == "relu" else F.elu(z) if act == "elu" else z


def _act_bwd(g, y, act):
    """the derivative through the saved post-activation output, as the data-gradient epilogue takes it"""
    if act == "relu":
        return g * (y > 0)
    if act == "elu":
        return torch.where(y > 0, g, g * (y + 1.0))
    return g


def _rows_heavy(t, g):
    return t * 10.0 ** (12.0 * torch.rand(t.shape[0], 1, generator=g) - 6.0)


def _feat(n, g):
    return 2.0 ** (-12.0 * torch.rand(n, generator=g))


def _sources(g, M, spec):
    """segments (width, col0, source width, gather) -> (sources, idx with repeated and out-of-order entries, the logical [M, K] matrix)"""
    R = M + 311
    idx = torch.randint(0, R, (M,), generator=g)
    idx[1] = idx[0]
    idx[M - 1] = idx[M // 2]
    srcs = [torch.randn(R if gather else M, ld, generator=g) for (_w, _c, ld, gather) in spec]
    X = torch.cat([(s[idx] if gather else s)[:, c0:c0 + w] for s, (w, c0, _ld, gather) in zip(srcs, spec)], dim=1)
    return srcs, idx, X


def _yardstick(f, S):
    """f(dtype) -> the float64 reference, e32 of the fp32 run of the same expression in row_rel (and in S), all-zero reference rows"""
    ref, y32 = f(torch.float64), f(torch.float32)
    e32, zero = rr.row_rel(y32, ref)
    return dict(ref=ref, e32=e32, zero=zero, S=S, e32s=None if S is None else rr.s_rel_terms(y32, ref, S))


@functools.lru_cache(maxsize=6)
def fwd_case(M, N, K, act, kind, spec=None, mse=False):
    g = _gen(M, N, K, kind == "heavy", mse)
    c = dict(shape=(M, N, K), act=act, kind=kind, spec=spec)
    if spec:
        c["srcs"], c["idx"], X = _sources(g, M, spec)
    else:
        X = torch.randn(M, K, generator=g)
    W, b = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    if kind == "heavy":
        f = _feat(N, g)
        X, W, b = _rows_heavy(X, g), W * f[:, None], b * f
    c.update(X=X, W=W, b=b)
    S = X.double().abs() @ W.double().abs().T + b.double().abs()
    if mse:
        # dY = ((X W^T + b) - target[tidx, tcol0 : tcol0 + N]) * scale; scale as the fp32 number the kernel is handed
        c.update(T=torch.randn(M + 50, N + 5, generator=g), tidx=torch.randint(0, M + 50, (M,), generator=g), tcol0=3,
                 scale=float(torch.tensor(2.0 / (M * N), dtype=torch.float32)))
        err = lambda dt: (X.to(dt) @ W.to(dt).T + b.to(dt)) - c["T"].to(dt)[c["tidx"], 3:3 + N]
        c.update(_yardstick(lambda dt: err(dt) * c["scale"], (S + c["T"].double()[c["tidx"], 3:3 + N].abs()) * c["scale"]))
        c["sq"] = float((err(torch.float64) ** 2).sum())
        c["e32sq"] = abs(float((err(torch.float32).double() ** 2).sum()) - c["sq"]) / c["sq"]
    else:
        c.update(_yardstick(lambda dt: _act(X.to(dt) @ W.to(dt).T + b.to(dt), act), S))
    if kind != "heavy" and N > 1:
        c["S"] = c["e32s"] = None
    return c


@functools.lru_cache(maxsize=6)
def dgrad_case(M, N, K, act, segs, kind, nsplit=0):
    g = _gen(M, N, K, kind == "heavy", 2 + nsplit)
    dZ, W = torch.randn(M, N, generator=g), torch.randn(N, K, generator=g) / N ** 0.5
    Xs = None
    if act == "relu":
        Xs = (torch.rand(M, K, generator=g) < 0.5).float()          # 0 / 1: dtc_linear_dgrad_mask reads the same signs from a record
    elif act == "elu":
        Xs = F.elu(torch.randn(M, K, generator=g))
    base = torch.randn(M, K, generator=g)
    acc = torch.zeros(K)
    col = 0
    for kind_s, w in segs or ():
        acc[col:col + w] = float(kind_s == "acc")
        col += w
    if kind == "heavy":
        dZ, W = _rows_heavy(dZ, g), W * _feat(N, g)[:, None] * _feat(K, g)[None, :]
        base = base * dZ.abs().amax(1, keepdim=True) * 2.0 ** -6
    base = base * acc
    c = dict(shape=(M, N, K), act=act, kind=kind, segs=segs, dZ=dZ, W=W, Xs=Xs, base=base)
    if nsplit:
        ch = N // nsplit

        def prod(dt, magnitudes=False):
            z, w = (dZ.to(dt).abs(), W.to(dt).abs()) if magnitudes else (dZ.to(dt), W.to(dt))
            return torch.stack([z[:, i * ch:(i + 1) * ch] @ w[i * ch:(i + 1) * ch] for i in range(nsplit)])
        c.update(_yardstick(prod, prod(torch.float64, True)))
    else:
        lo = _skip(segs)                                # measured on the columns that have a destination
        f = lambda dt: (_act_bwd(dZ.to(dt) @ W.to(dt), None if Xs is None else Xs.to(dt), act) + base.to(dt))[:, lo:]
        c.update(_yardstick(f, (dZ.double().abs() @ W.double().abs() + base.double().abs())[:, lo:]))
    if kind != "heavy" and c["ref"].shape[-1] > 1:
        c["S"] = c["e32s"] = None
    return c


@functools.lru_cache(maxsize=6)
def wgrad_case(M, N, K, spec, kind):
    g = _gen(M, N, K, kind == "heavy", 9)
    c = dict(shape=(M, N, K), kind=kind, spec=spec)
    if spec:
        c["srcs"], c["idx"], X = _sources(g, M, spec)
    else:
        X = torch.randn(M, K, generator=g)
    dZ = torch.randn(M, N, generator=g) / M ** 0.5
    if kind == "heavy":
        dZ = _rows_heavy(dZ, g) * _feat(N, g)[None, :]
    c.update(X=X, dZ=dZ, dW=dZ.double().T @ X.double(), db=dZ.double().sum(0))
    c["e32"] = dict(dW=rr.s_rel(dZ.T @ X, c["dW"], dZ, X), db=rr.s_rel_bias(dZ.sum(0), c["db"], dZ))
    return c


def _all_cases():
    """(what, builder) of every case the GPU tests measure, in the tables' order"""
    for M, N, K, act, _entry, heavy in FWD_CASES:
        for kind in _kinds(heavy):
            yield f"fwd ({M}, {N}, {K}) {kind}", functools.partial(fwd_case, M, N, K, act, kind)
    for M, N, K, heavy in MSE_CASES:
        for kind in _kinds(heavy):
            yield f"mse ({M}, {N}, {K}) {kind}", functools.partial(fwd_case, M, N, K, None, kind, None, True)
    for M, N, K, act, segs, _entry, heavy in DGRAD_CASES:
        for kind in _kinds(heavy):
            yield f"dgrad ({M}, {N}, {K}) {kind}", functools.partial(dgrad_case, M, N, K, act, segs, kind)
    for M, N, K, nsplit, heavy in SPLIT_CASES:
        for kind in _kinds(heavy):
            yield f"split ({M}, {N}, {K}) / {nsplit} {kind}", functools.partial(dgrad_case, M, N, K, None, None, kind, nsplit)
    for M, N, K, act in FWD_LAYOUT_SHAPES:
        yield f"fwd gathered ({M}, 70, 100)", functools.partial(fwd_case, M, 70, 100, act, "plain", GATHER_X)


# ---------------------------------------------------------------- CPU checks of the tables
def test_case_tables_reach_every_variant():
    """Every template instance the issue names is launched by some case, at the forced thresholds and -- for the non-deep <64> and <32>
    and the deep <32> -- at the default one; the notes of the tables hold."""
    seen, default = set(), set()
    for M, N, K, _act, entry, _h in FWD_CASES:
        seen |= {fwd_variant(M, N, int(t)) for t in THRESHOLDS}
        default.add(fwd_variant(M, N))
        if "mask" in entry:                                         # gemm.hip:880-884: every tile of the launch is a full one
            bn = 128 if wide_tiles(M, N) else pick_bn_rows(M, N)
            assert M % BM == 0 and N % bn == 0, (M, N, bn)
    seen |= {"fwd<64,MSE>"} if MSE_CASES else set()
    for M, _N, K, _act, segs, entry, _h in DGRAD_CASES:
        seen |= {dgrad_variant(M, K - _skip(segs), int(t)) for t in THRESHOLDS}
        default.add(dgrad_variant(M, K - _skip(segs)))
        if entry == "mask":                                         # gemm.hip:1001
            assert M % BM == 0 and K % pick_bn_rows(M, K) == 0 and not segs
    for M, N, K, nsplit, _h in SPLIT_CASES:
        assert N % nsplit == 0
        seen.add(split_variant(M, K, nsplit))
    for M, N, K, spec, _h in WGRAD_CASES:
        seen |= set(wgrad_variant(M, N, _widths(K, spec))[:2])
    assert seen == REQUIRED_VARIANTS, (REQUIRED_VARIANTS - seen, seen - REQUIRED_VARIANTS)
    assert {"fwd<128>", "fwd<64>", "fwd<32>", "fwd<32,deep>", "dgrad<64>", "dgrad<32>", "dgrad<32,deep>"} <= default, default
    assert not any(v.endswith("64,deep>") for v in default), "a 64-wide launch has >= 320 workgroups: deep only by the variable"
    # the notes of the tables
    assert cdiv(14885, BM) * cdiv(693, 128) == 702 and 14885 % BM == 37 and 693 % 128 == 53 and 72 % BK
    assert grid_for(cdiv(5000, BM), cdiv(500, 64)) == 320 and grid_for(cdiv(2200, BM), cdiv(500, 32)) == 384
    assert grid_for(cdiv(5120, BM), cdiv(512, 64)) == 320
    assert wgrad_variant(1100, 128, [130]) == ("wgrad<64>", "reduce<4>", 16, 80) and 128 * 130 >= 128 * 128
    assert wgrad_variant(3000, 12, [128])[:3] == ("wgrad<64>", "reduce<16>", 24)
    assert wgrad_variant(777, 70, [32])[0] == "wgrad<32>"
    assert wgrad_variant(1536, 512, _widths(752, CRITIC_X))[:3] == ("wgrad<64>", "reduce<4>", 16)
    assert wgrad_variant(129, 35, [64])[2:] == (8, 32)              # splits 0-3 hold 32 rows, split 4 one, splits 5-7 none
    for shapes, family in ((FWD_ROW_SHAPES, fwd_variant), (DGRAD_ROW_SHAPES, dgrad_variant)):
        rows = {family(M, K if family is dgrad_variant else N, int(thr)) for M, N, K, _a, thr in shapes}
        assert rows == {v for v in REQUIRED_VARIANTS if v.startswith(family.__name__[:-8] + "<") and "MSE" not in v}, rows
    assert sum(w for w, *_ in GATHER_X) == 100


def test_no_reference_row_is_all_zero():
    """row_rel leaves out rows whose reference is all zero: no case has one (seeds and activations chosen for it), every yardstick is
    finite, and the weight-gradient references have no output without a term."""
    for what, build in _all_cases():
        c = build()
        assert c["zero"] == 0, what
        assert c["e32"] == c["e32"] and (c["e32s"] is None or c["e32s"] == c["e32s"]), what
    for M, N, K, spec, heavy in WGRAD_CASES:
        for kind in _kinds(heavy):
            c = wgrad_case(M, N, K, spec, kind)
            assert bool((c["dZ"].abs().T @ c["X"].abs() > 0).all()) and all(v == v for v in c["e32"].values()), (M, N, K, kind)


# ---------------------------------------------------------------- device side
def _lib():
    from dtc_amd import _ffi
    return _ffi, _ffi.lib()


@contextlib.contextmanager
def _split_off():
    """the library's split-precision switch off (dtc_linear_wgrad then keeps every layer on csrc/wgrad.hip); restored"""
    _ffi, lib = _lib()
    prev = lib.dtc_get_gemm_split()
    lib.dtc_set_gemm_split(0)
    try:
        yield lib
    finally:
        lib.dtc_set_gemm_split(prev)


def _profile():
    from test_hip_recurrence_bptt import _profile as profile
    return profile()


def _expect(rep, **want):
    """the launch profile holds exactly these classes: name -> (launches, work)"""
    assert rep == {k: (n, float(w)) for k, (n, w) in want.items()}, (rep, want)


def _geom(R, Cw, layout):
    """-> (row stride, offset of the first element in floats, rows of the buffer)"""
    return {"plain": (Cw, 0, R), "ld": (cdiv(Cw + 5, 4) * 4, 0, R + 3), "off4": (cdiv(Cw, 4) * 4, 1, R),
            "odd": (Cw + 1 + Cw % 2, 0, R + 1)}[layout]


def _inp(t, layout="plain"):
    """CPU [R, C] -> a device view of it with the layout's row stride and base; everything around it is NaN"""
    R, Cw = t.shape
    ld, off, rows = _geom(R, Cw, layout)
    buf = torch.full((off + rows * ld,), NAN, device=DEV)
    v = buf[off:].view(rows, ld)[:R, :Cw]
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 if layout == "off4" else 0) and (layout != "odd" or ld % 2 == 1)
    return v


def _flat(t, layout="plain"):
    """a contiguous operand (W), 4 bytes off a 16-byte boundary in the `off4` layout"""
    buf = torch.full((t.numel() + 1,), NAN, device=DEV)
    v = buf[1 if layout == "off4" else 0:][:t.numel()].view(t.shape)
    v.copy_(t)
    return v


class _Out:
    """A destination [M, w] at columns c0.. of a [M, cols] tensor in `layout`.  What the call owns is NaN (or `base` for an accumulating
    one), everything else of the buffer -- the other columns, the row padding, the rows from M on -- a sentinel that must survive."""

    def __init__(self, M, w, layout="plain", c0=0, cols=None, base=None):
        cols = c0 + w if cols is None else cols
        ld, off, rows = _geom(M, cols, layout)
        self.buf = torch.full((off + rows * ld,), SENTINEL, device=DEV)
        self.full = self.buf[off:].view(rows, ld)[:M, :cols]
        self.t = self.full[:, c0:c0 + w]
        if base is None:
            self.t.fill_(NAN)
        else:
            self.t.copy_(base)
        self.ld, self.before = ld, self.buf.clone()
        self.owned = torch.zeros_like(self.buf, dtype=torch.bool)
        self.owned[off:].view(rows, ld)[:M, c0:c0 + w] = True

    def check(self, what):
        assert torch.equal(self.buf[~self.owned], self.before[~self.owned]), (what, "a store outside the destination")
        assert bool(torch.isfinite(self.t).all()), (what, "an element nobody wrote, or a non-finite result")
        return self.t


class _NoCheck(_Out):
    """a destination whose content may be non-finite (the NaN-row runs)"""

    def check(self, what):
        assert torch.equal(self.buf[~self.owned], self.before[~self.owned]), what
        return self.t


def _x_operand(c, layout="plain"):
    """the case's X as a DtcSegMat: one plain segment, or its gathered sources"""
    _ffi, _ = _lib()
    if "srcs" in c:
        return _ffi.segmat([_ffi.seg(_inp(s, layout), c0, w, gather=gather) for s, (w, c0, _ld, gather) in zip(c["srcs"], c["spec"])],
                           c["idx"].to(DEV))
    return _ffi.segmat([_ffi.seg(_inp(c["X"], layout), 0, c["X"].shape[1])])


def _hold(what, got, c):
    ref = c["ref"]
    assert bool(torch.isfinite(got).all()), (what, "non-finite")
    err, zero = rr.row_rel(got, ref)
    assert zero == 0, (what, "all-zero reference rows")
    one = ref.shape[-1] == 1                            # one column: a row's measure is one element's relative error -> S (docstring)
    assert not one or c["S"] is not None
    rows = [("row 1col" if one else "row", err, c["e32"])] + ([("S", rr.s_rel_terms(got, ref, c["S"]), c["e32s"])] if c["S"] is not None else [])
    bad = []
    for k, e, e32 in rows:
        bd = rr.bound(e32)
        print(f"FP32D {what} | {k} | err {e:.3e} | e32 {e32:.3e} | bound {bd:.3e}")
        if not e <= bd and k != "row 1col":
            bad.append((k, e, e32, bd))
    assert not bad, (what, bad)


def _sign_record(P):
    """[M, K] bool -> the record dtc_linear_fwd_mask writes for these signs (as int32 words): bit r of word [(row // 32) * 2 + half][col]
    <-> row 32 * blk + 4 * half + (r & 3) + 8 * (r >> 2)"""
    M, K = P.shape
    bits = P.cpu().view(M // 32, 4, 2, 4, K).permute(0, 2, 1, 3, 4).reshape(M // 32, 2, 16, K).to(torch.int32)
    return (bits << torch.arange(16, dtype=torch.int32).view(1, 1, 16, 1)).sum(dim=2).reshape(-1, K)


def _as_int16(words):
    return ((words + 32768) % 65536 - 32768).to(torch.int16)


# ---------------------------------------------------------------- forward
def _fwd_launch(c, entry, Xs, W, b, out, take, thr):
    """one forward launch through `entry` -> (Y, sign record or None); the profile shows one linear_fwd of 2 M N K and nothing else"""
    _ffi, lib = _lib()
    M, N, K = c["shape"]
    p, st, a = _ffi.ptr, _ffi.stream(), _ffi.ACT[c["act"]]
    mask = torch.full((int(lib.dtc_relu_mask_elems(M, N)),), 0x5555, dtype=torch.int16, device=DEV) if "mask" in entry else None
    rec = torch.zeros(int(lib.dtc_amax_record_bytes()) // 4, dtype=torch.int32, device=DEV) if "amax" in entry else None
    what = f"{entry} {c['shape']} {ENV}={thr}"
    if take:
        take()
    if entry == "fwd":
        _ffi.check(lib.dtc_linear_fwd(Xs, p(W), p(b), p(out.t), out.ld, M, N, K, a, st), what)
    elif entry == "mask":
        _ffi.check(lib.dtc_linear_fwd_mask(Xs, p(W), p(b), p(out.t), out.ld, p(mask), M, N, K, st), what)
    elif entry in ("amax", "amax+mask"):
        _ffi.check(lib.dtc_linear_fwd_amax(Xs, p(W), p(b), p(out.t), out.ld, p(mask), p(rec), M, N, K, a, st), what)
    else:
        layers = (_ffi.DtcFwdLayer * 1)()
        L = layers[0]
        L.X, L.W, L.b, L.Y, L.ldy, L.N, L.K, L.act = Xs, p(W), p(b), p(out.t), out.ld, N, K, a
        _ffi.check(lib.dtc_linear_fwd_list(layers, 1, M, st), what)
    if take:
        _expect(take(), linear_fwd=(1, 2.0 * M * N * K))
    Y = out.check(what)
    if rec is not None:                                 # the record's value: the largest |Y| the launch wrote, as bits
        assert int(rec.max()) == int(Y.abs().max().view(torch.int32)), what
    return Y, mask


def _fwd_both(c, entry, monkeypatch, take, layout="plain"):
    """the case under both thresholds: bit-identical -> (Y, sign record)"""
    M, N, _K = c["shape"]
    Xs, W, b = _x_operand(c, layout), _flat(c["W"], layout), c["b"].to(DEV)
    outs = []
    for thr in THRESHOLDS:
        monkeypatch.setenv(ENV, thr)
        outs.append(_fwd_launch(c, entry, Xs, W, b, _Out(M, N, layout), take, thr))
    assert torch.equal(outs[0][0], outs[1][0]), "single-stage and two-stages-ahead kernels differ"
    assert outs[0][1] is None or torch.equal(outs[0][1], outs[1][1])
    return outs[1]


@gpu
@pytest.mark.parametrize("M,N,K,act,entry,kind", [s[:5] + (k,) for s in FWD_CASES for k in _kinds(s[5])])
def test_forward_vs_fp64(M, N, K, act, entry, kind, monkeypatch):
    c = fwd_case(M, N, K, act, kind)
    with _profile() as take:
        Y, mask = _fwd_both(c, entry, monkeypatch, take)
    _hold(f"fwd ({M}, {N}, {K}) {kind} {fwd_variant(M, N, 0)} = {fwd_variant(M, N, 100000)}", Y, c)
    if mask is not None:
        assert torch.equal(mask.cpu().view(-1, N).to(torch.int32) & 0xFFFF, _sign_record(Y > 0))


def _mse_launch(c, take, dY, X=None):
    _ffi, lib = _lib()
    M, N, K = c["shape"]
    p = _ffi.ptr
    Xs = _x_operand(c) if X is None else _ffi.segmat([_ffi.seg(X, 0, K)])
    W, b, T, tidx = c["W"].to(DEV), c["b"].to(DEV), c["T"].to(DEV), c["tidx"].to(DEV)
    n_part = int(lib.dtc_linear_fwd_mse_parts(M, N))
    assert n_part == grid_for(cdiv(M, BM), cdiv(N, 64))
    parts = torch.full((n_part + 4,), NAN, dtype=torch.float64, device=DEV)
    parts[n_part:] = SENTINEL
    if take:
        take()
    _ffi.check(lib.dtc_linear_fwd_mse(Xs, p(W), p(b), p(T), T.stride(0), T.shape[0], c["tcol0"], p(tidx),
                                      ctypes.c_float(c["scale"]), p(dY.t), dY.ld, p(parts), M, N, K, _ffi.stream()), f"mse {c['shape']}")
    if take:
        _expect(take(), linear_fwd=(1, 2.0 * M * N * K))
    assert bool((parts[n_part:] == SENTINEL).all())
    return dY.check(f"mse {c['shape']}"), parts[:n_part]


@gpu
@pytest.mark.parametrize("M,N,K,kind", [s[:3] + (k,) for s in MSE_CASES for k in _kinds(s[3])])
def test_forward_mse_vs_fp64(M, N, K, kind, monkeypatch):
    """dtc_linear_fwd_mse: dL/dY per row, and the sum of the workgroups' partial sums of squares (a padding workgroup writes 0) within
    bound(e32) of the float64 sum, e32 the relative error of the fp32 run's sum.  The threshold variable changes nothing here."""
    c = fwd_case(M, N, K, None, kind, None, True)
    outs = []
    with _profile() as take:
        for thr in THRESHOLDS:
            monkeypatch.setenv(ENV, thr)
            outs.append(_mse_launch(c, take, _Out(M, N)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    dY, parts = outs[1]
    _hold(f"mse ({M}, {N}, {K}) {kind} fwd<64,MSE>", dY, c)
    assert bool(torch.isfinite(parts).all())
    err, bd = abs(float(parts.sum()) - c["sq"]) / c["sq"], rr.bound(c["e32sq"])
    print(f"FP32D mse ({M}, {N}, {K}) {kind} fwd<64,MSE> | sumsq | err {err:.3e} | e32 {c['e32sq']:.3e} | bound {bd:.3e}")
    assert err <= bd


@gpu
@pytest.mark.parametrize("layout", LAYOUTS + ("gather",))
@pytest.mark.parametrize("M,N,K,act", FWD_LAYOUT_SHAPES)
def test_forward_layouts(M, N, K, act, layout, monkeypatch):
    """ldy beyond the width and a taller buffer (`ld`), Y, X and W 4 bytes off a 16-byte boundary (`off4`), odd row strides (`odd`: the
    scalar stores): nothing outside the destination changes, every element of it is written, and the values are those of the plain
    layout bit for bit.  `gather`: X = four segments, two gathered through an index with repeated and out-of-order entries, the third a
    column window of a wider source; the k order changes at the segment borders, so it is held to float64 only."""
    with _profile() as take:
        if layout == "gather":
            c = fwd_case(M, 70, 100, act, "plain", GATHER_X)
            Y, _ = _fwd_both(c, "fwd", monkeypatch, take)
            _hold(f"fwd gathered ({M}, 70, 100) plain", Y, c)
            return
        c = fwd_case(M, N, K, act, "plain")
        plain, _ = _fwd_both(c, "fwd", monkeypatch, take)
        Y, _ = _fwd_both(c, "fwd", monkeypatch, take, layout)
    assert torch.equal(Y, plain)
    _hold(f"fwd ({M}, {N}, {K}) plain layout {layout}", Y, c)


def _row_checks(run, rows, r0):
    """run(reverse, nan_row) -> per-row output [.., rows, width] (rows on axis -2): two runs, the row-reversed problem, a NaN in row r0"""
    clean, again = run(False, None), run(False, None)
    assert torch.equal(clean, again), "two runs differ"
    assert torch.equal(clean, run(True, None).flip(-2)), "the row-reversed problem is not the row-reversed output"
    dirty = run(False, r0)
    keep = torch.ones(rows, dtype=torch.bool, device=DEV)
    keep[r0] = False
    assert bool(torch.isfinite(clean).all())
    assert torch.equal(clean[..., keep, :], dirty[..., keep, :]), "a NaN in one row reached another"
    assert not bool(torch.isfinite(dirty[..., r0, :]).all(-1).any()), "the row with the NaN"


def _with_nan(t, r0, whole=False):
    t = t.clone()
    t[r0, slice(None) if whole else min(7, t.shape[1] - 1)] = NAN
    return t


@gpu
@pytest.mark.parametrize("M,N,K,act,thr", FWD_ROW_SHAPES)
def test_forward_rows_are_independent(M, N, K, act, thr, monkeypatch):
    _ffi, lib = _lib()
    c = fwd_case(M, N, K, act, "plain")
    monkeypatch.setenv(ENV, thr)
    W, b = c["W"].to(DEV), c["b"].to(DEV)

    def run(reverse, nan_row):
        X = c["X"] if nan_row is None else _with_nan(c["X"], nan_row)
        X = (X.flip(0) if reverse else X).contiguous().to(DEV)
        Y = torch.full((M, N), NAN, device=DEV)
        _ffi.check(lib.dtc_linear_fwd(_ffi.segmat([_ffi.seg(X, 0, K)]), _ffi.ptr(W), _ffi.ptr(b), _ffi.ptr(Y), N, M, N, K, _ffi.ACT[act],
                                      _ffi.stream()), "dtc_linear_fwd")
        return Y
    _row_checks(run, M, M // 2 + 5)


@gpu
def test_forward_mse_rows_are_independent():
    M, N, K = MSE_CASES[0][:3]
    c = fwd_case(M, N, K, None, "plain", None, True)
    tidx = c["tidx"]

    def run(reverse, nan_row):
        X = c["X"] if nan_row is None else _with_nan(c["X"], nan_row)
        c2 = dict(c, tidx=tidx.flip(0) if reverse else tidx)
        return _mse_launch(c2, None, _NoCheck(M, N), (X.flip(0) if reverse else X).contiguous().to(DEV))[0]
    _row_checks(run, M, M // 2 + 5)


# ---------------------------------------------------------------- data gradient
def _destination(c, layout="plain", cls=_Out):
    """-> (DtcSegMat, [(first column, width, _Out)] of the non-NULL segments).  Every segment is its own tensor; an accumulating one sits
    at column 4 of a tensor 8 columns wider than itself and starts from the case's `base`."""
    _ffi, _ = _lib()
    M, _N, K = c["shape"]
    segs, outs, col = [], [], 0
    for kind, w in c["segs"] or (("plain", K),):
        if kind == "null":
            segs.append(_ffi.seg(None, 0, w))
        elif kind == "acc":
            o = cls(M, w, layout, c0=4, cols=w + 8, base=c["base"][:, col:col + w])
            segs.append(_ffi.seg(o.full, 4, w, accumulate=True))
            outs.append((col, w, o))
        else:
            o = cls(M, w, layout)
            segs.append(_ffi.seg(o.full, 0, w))
            outs.append((col, w, o))
        col += w
    return _ffi.segmat(segs), outs


def _dgrad_launch(c, entry, dZ, W, Xs, take, thr, layout="plain", cls=_Out):
    """one data-gradient launch -> dX [M, K - leading NULL columns] put together from the destination segments"""
    _ffi, lib = _lib()
    M, N, K = c["shape"]
    p, st = _ffi.ptr, _ffi.stream()
    dXs, outs = _destination(c, layout, cls)
    what = f"{entry} {c['shape']} {ENV}={thr}"
    if take:
        take()
    if entry == "mask":
        _ffi.check(lib.dtc_linear_dgrad_mask(p(dZ), dZ.stride(0), p(W), dXs, p(Xs), M, N, K, st), what)
    else:
        _ffi.check(lib.dtc_linear_dgrad(p(dZ), dZ.stride(0), p(W), dXs, p(Xs), Xs.stride(0) if Xs is not None else 0, M, N, K,
                                        _ffi.ACT[c["act"]], st), what)
    skip = _skip(c["segs"])
    if take:
        _expect(take(), linear_dgrad=(1, 2.0 * M * N * (K - skip)))
    dX = torch.full((M, K - skip), NAN, device=DEV)
    for col, w, o in outs:
        dX[:, col - skip:col - skip + w] = o.check(what)
    return dX


def _dgrad_both(c, entry, monkeypatch, take, layout="plain"):
    dZ, W = _inp(c["dZ"], layout), _flat(c["W"], layout)
    Xs = None if c["Xs"] is None else _inp(c["Xs"], layout)
    outs = []
    for thr in THRESHOLDS:
        monkeypatch.setenv(ENV, thr)
        outs.append(_dgrad_launch(c, "dgrad", dZ, W, Xs, take, thr, layout))
        if entry == "mask":                             # the record of the same signs gives the same bits
            rec = _as_int16(_sign_record(c["Xs"] > 0)).to(DEV)
            assert torch.equal(outs[-1], _dgrad_launch(c, "mask", dZ, W, rec, take, thr, layout)), "sign record != saved activation"
    assert torch.equal(outs[0], outs[1]), "single-stage and two-stages-ahead kernels differ"
    return outs[1]


@gpu
@pytest.mark.parametrize("M,N,K,act,segs,entry,kind", [s[:6] + (k,) for s in DGRAD_CASES for k in _kinds(s[6])])
def test_data_gradient_vs_fp64(M, N, K, act, segs, entry, kind, monkeypatch):
    c = dgrad_case(M, N, K, act, segs, kind)
    with _profile() as take:
        dX = _dgrad_both(c, entry, monkeypatch, take)
    cols = K - _skip(segs)
    tag = "".join(k[0] for k, _ in segs or ())
    _hold(f"dgrad ({M}, {N}, {K}){' ' + tag if tag else ''}{' mask' if entry == 'mask' else ''} {kind} {dgrad_variant(M, cols, 0)} = "
          f"{dgrad_variant(M, cols, 100000)}", dX, c)


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,N,K,act", DGRAD_LAYOUT_SHAPES)
def test_data_gradient_layouts(M, N, K, act, layout, monkeypatch):
    """lddx, lddz and ldxs beyond the widths with NaN around the operands, bases 4 bytes off a 16-byte boundary, odd row strides; for
    the full-tile shape the sign-record form as well.  Same bits as the plain layout, nothing outside the destination touched."""
    c = dgrad_case(M, N, K, act, None, "plain")
    entry = "mask" if act == "relu" else "dgrad"
    with _profile() as take:
        plain = _dgrad_both(c, entry, monkeypatch, take)
        dX = _dgrad_both(c, entry, monkeypatch, take, layout)
    assert torch.equal(dX, plain)
    _hold(f"dgrad ({M}, {N}, {K}) plain layout {layout}", dX, c)


@gpu
@pytest.mark.parametrize("M,N,K,act,thr", DGRAD_ROW_SHAPES)
def test_data_gradient_rows_are_independent(M, N, K, act, thr, monkeypatch):
    c = dgrad_case(M, N, K, act, None, "plain")
    monkeypatch.setenv(ENV, thr)
    W = c["W"].to(DEV)

    def run(reverse, nan_row):
        dZ = c["dZ"] if nan_row is None else _with_nan(c["dZ"], nan_row)
        f = (lambda t: t.flip(0).contiguous().to(DEV)) if reverse else (lambda t: t.to(DEV))
        return _dgrad_launch(c, "dgrad", f(dZ), W, None if c["Xs"] is None else f(c["Xs"]), None, thr, cls=_NoCheck)
    _row_checks(run, M, M // 2 + 5)


def _split_launch(c, nsplit, dZ, take, cls=_Out):
    """dtc_linear_dgrad_split -> [nsplit, M, K]: chunk g of the reduction into its own matrix, split_stride apart"""
    _ffi, lib = _lib()
    M, N, K = c["shape"]
    out = cls(nsplit * M, K)
    W = c["W"].to(DEV)
    if take:
        take()
    _ffi.check(lib.dtc_linear_dgrad_split(_ffi.ptr(dZ), dZ.stride(0), _ffi.ptr(W), _ffi.ptr(out.t), out.ld, M * out.ld, M, N, K, nsplit,
                                          _ffi.stream()), f"split {c['shape']} / {nsplit}")
    if take:
        _expect(take(), linear_dgrad=(1, 2.0 * M * N * K))
    return out.check(f"split {c['shape']} / {nsplit}").view(nsplit, M, K)


@gpu
@pytest.mark.parametrize("M,N,K,nsplit,kind", [s[:4] + (k,) for s in SPLIT_CASES for k in _kinds(s[4])])
def test_data_gradient_split_vs_fp64(M, N, K, nsplit, kind, monkeypatch):
    c = dgrad_case(M, N, K, None, None, kind, nsplit)
    outs = []
    with _profile() as take:
        for thr in THRESHOLDS:                          # (the split form has no two-stages-ahead instance)
            monkeypatch.setenv(ENV, thr)
            outs.append(_split_launch(c, nsplit, c["dZ"].to(DEV), take))
    assert torch.equal(outs[0], outs[1])
    _hold(f"split ({M}, {N}, {K}) / {nsplit} {kind} {split_variant(M, K, nsplit)}", outs[1], c)


@gpu
@pytest.mark.parametrize("M,N,K,nsplit", [(130, 96, 64, 3), (5000, 384, 500, 3)])
def test_data_gradient_split_rows_are_independent(M, N, K, nsplit):
    c = dgrad_case(M, N, K, None, None, "plain", nsplit)

    def run(reverse, nan_row):
        dZ = c["dZ"] if nan_row is None else _with_nan(c["dZ"], nan_row, whole=True)            # every chunk reads a NaN of the row
        return _split_launch(c, nsplit, (dZ.flip(0) if reverse else dZ).contiguous().to(DEV), None, cls=_NoCheck)
    _row_checks(run, M, M // 2 + 5)


# ---------------------------------------------------------------- weight gradient
def _wgrad_launch(c, take, layout="plain", ws=None, db=True):
    """dtc_linear_wgrad with the switch off -> (dW, db, workspace): NaN-filled outputs and workspace, a sentinel behind each"""
    _ffi, _ = _lib()
    M, N, K = c["shape"]
    p = _ffi.ptr
    Xs, dZ = _x_operand(c, layout), _inp(c["dZ"], layout)
    kern, red, splits, _rows = wgrad_variant(M, N, _widths(K, c["spec"]))
    with _split_off() as lib:
        need = int(lib.dtc_linear_wgrad_workspace(M, N, K))
        assert need % 4 == 0 and need >= splits * N * part_ld(K) * 4
        if ws is None:
            ws = torch.full((need // 4 + 64,), NAN, device=DEV)
        ws[need // 4:] = SENTINEL
        dW, dB = _Out(1, N * K, "off4" if layout == "off4" else "plain"), _Out(1, N)
        take()
        _ffi.check(lib.dtc_linear_wgrad(p(dZ), dZ.stride(0), Xs, p(dW.t), p(dB.t) if db else None, p(ws), M, N, K, _ffi.stream()),
                   f"wgrad {c['shape']}")
    _expect(take(), linear_wgrad=(1, 2.0 * M * N * K), wgrad_reduce=(1, N * part_ld(K) * 4.0 * (splits + 1)))
    assert bool((ws[need // 4:] == SENTINEL).all()), "a store behind the workspace"
    return dW.check("dW").view(N, K), (dB.check("db").view(N) if db else None), ws


def _hold_wgrad(what, dW, db, c):
    bad = []
    for k, e in (("dW", rr.s_rel(dW, c["dW"], c["dZ"], c["X"])), ("db", rr.s_rel_bias(db, c["db"], c["dZ"]))):
        bd = rr.bound(c["e32"][k])
        print(f"FP32D {what} | {k} | err {e:.3e} | e32 {c['e32'][k]:.3e} | bound {bd:.3e}")
        if not e <= bd:
            bad.append((k, e, c["e32"][k], bd))
    assert not bad, (what, bad)


@gpu
@pytest.mark.parametrize("M,N,K,spec,kind", [s[:4] + (k,) for s in WGRAD_CASES for k in _kinds(s[4])])
def test_weight_gradient_vs_fp64(M, N, K, spec, kind):
    """Also: a second call on the workspace the first one left gives the same bits, and so does a call without db."""
    c = wgrad_case(M, N, K, spec, kind)
    with _profile() as take:
        dW, db, ws = _wgrad_launch(c, take)
        dW2, db2, _ = _wgrad_launch(c, take, ws=ws)
        dW3, _none, _ = _wgrad_launch(c, take, db=False)
    v = wgrad_variant(M, N, _widths(K, spec))
    _hold_wgrad(f"wgrad ({M}, {N}, {K}){' gathered' if spec else ''} {kind} {v[0]} {v[1]} {v[2]} splits", dW, db, c)
    assert torch.equal(dW, dW2) and torch.equal(db, db2) and torch.equal(dW, dW3)


@gpu
@pytest.mark.parametrize("layout", LAYOUTS + ("gather",))
@pytest.mark.parametrize("M,N,K", WGRAD_LAYOUT_SHAPES)
def test_weight_gradient_layouts(M, N, K, layout):
    """lddz and the row stride of X beyond the widths with NaN around them, dW, dZ and X 4 bytes off a 16-byte boundary, odd row strides:
    the bits of the plain layout.  `gather`: X gathered through an index with repeated and out-of-order entries, against float64."""
    with _profile() as take:
        if layout == "gather":
            c = wgrad_case(M, N, K, ((K - 3, 2, K + 4, True), (3, 0, 3, True)), "plain")
            dW, db, _ = _wgrad_launch(c, take)
        else:
            c = wgrad_case(M, N, K, None, "plain")
            plain = _wgrad_launch(c, take)
            dW, db, _ = _wgrad_launch(c, take, layout)
            assert torch.equal(dW, plain[0]) and torch.equal(db, plain[1])
    _hold_wgrad(f"wgrad ({M}, {N}, {K}) plain layout {layout}", dW, db, c)
