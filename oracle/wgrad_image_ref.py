"""Numpy restatement of the image weight gradient's scaling scheme (TEST INFRASTRUCTURE: only tests/ import this; numpy only).

Restates csrc/wgrad_h2i.hip (wgrad_h2i_group_kernel, wgrad_h2i_reduce_kernel; slice rule SLICES_H2I of csrc/wgrad_plan.hpp): dW [N, K] = dZ^T X and db = colsum(dZ)
from two operand images (format: oracle/h2image.py), with exact (float64) accumulation in place of the matrix pipe's fp32 one.

The scheme.  Row m of the images holds (hi, lo) = split(dZ[m] 2^eZ[m]) and split(X[m] 2^eX[m]), one exponent per row and block of
128 columns; HI_EZERO marks a row block without content.  For every 128-row block and 128 x 128 tile of dW:
    live[m] = eZ[m] and eX[m] both set;       T = min over live rows of eZ[m] + eX[m]       (no live row: the predecessor's T)
    f[m]  = fp16(2^max(T - eZ[m] - eX[m], -30)) for live rows, 1 otherwise;  hi', lo' = fp16(hi_X f), fp16(lo_X f)
    acc  += hi_Z^T hi' + hi_Z^T lo' + lo_Z^T hi'     (lo lo' is left out);   dW = sum over blocks of 2^-T acc
    Tz    = min over rows with eZ[m] set of eZ[m];   fb[m] = fp16(2^max(Tz - eZ[m], -30));   db = sum of 2^-Tz (hi_Z + lo_Z)^T fb
A batch slice (slices(): whole 128-row blocks) keeps ONE fp32 accumulator set and multiplies it by 2^(T_new - T_cur) at every block
border; rescale = "as_built" restates that with no limit on the step, rescale = "bounded" with the limit below.

    RESCALE_CAP.  A block with content takes T = min(T_raw, t_lo + RESCALE_CAP), t_lo = the smallest T a block with content of the
    same slice has had so far (the first such block is not limited); the remainder T_raw - T goes into f and fb, which stay <= 1.
    Why the running minimum and not the scale in force: a row of block b adds at most 3 products of |hi hi'| <= 2^30 f <= 2^30 to an
    accumulator held at scale T_b, so at a later scale T_c the accumulator is below rows x 2^30.01 x 2^(T_c - min_b T_b).  A slice
    holds at most 2^22 rows (an image is below 2 GiB and a row takes at least 64 bytes: M < 2^25; at least 8 slices), so with
    T_c - min T_b <= 72 the accumulator stays below 2^(22 + 30.01 + 72) < 2^125 and never reaches inf for finite operands.  A limit
    on single steps alone would let several rising borders in a row multiply up.

What fp16 does to an attenuated row (bits_kept).  The image row's largest |hi| lies in [2^14, 2^15); k = eZ[m] + eX[m] - T >= 0 is
the row's distance below its block's top row.  hi' = hi 2^-k is exact while it stays a normal fp16 number; below 2^-14 it is
rounded to a multiple of 2^-24 (error <= 2^-25), and lo (<= 2^-11 |hi|) gets there 11 octaves earlier.  Relative to the row's
largest element, 2^(14 - k), one such rounding is 2^-(39 - k) and the two of an element (hi', lo') at most 2^-(38 - k): the scaled
row keeps at least min(22, 38 - k) bits -- all 22 the (hi, lo) pair holds up to k = 16, then 21 .. 14 for k = 17 .. 24.  2^-25 is halfway between 0 and the smallest fp16 number 2^-24 and rounds to 0 (ties to even): from k = 25 on f = 0 and the
row adds nothing -- the clamp at 2^-30 is never reached as a value.  The bias factor fb sees k = eZ[m] - Tz alone and is a power of
two or 0: a row is added exactly or not at all.  (The kernel stores 2^15 fb and takes the 2^15 out at the end: the matrix pipe does
not keep product bits below about 2^-24, which (hi + lo) 2^-24 reaches; exact arithmetic, as here, cannot tell the two apart.)

The bound of the scheme against float64 truth dZ^T X (truth of the DECODED operands (hi + lo) 2^-e, so the images' own 22 bits are
not part of it), per element (n, k), rows m of all blocks:
    B_lolo  = sum over kept rows of |lo_Z[m, n]| |lo_X[m, k]| 2^-(eZ + eX)              the product left out; <= 2^-22 (1 + 2^-9) S
    B_round = sum over kept rows of 2^-T ((|hi_Z| + |lo_Z|)[m, n] r(hi_X[m, k] f) + |hi_Z[m, n]| r(lo_X[m, k] f)),
              r(v) = 2^-25 where 0 < |v| < 2^-14 (a subnormal result: half its quantum), 0 elsewhere (a power-of-two factor is exact)
    B_drop  = sum over dropped rows (f = 0) of |dZ[m, n]| |X[m, k]|
    bound   = B_lolo + B_round + B_drop + 2^-40 S_all                                   (the last term: this file's own float64 sums)
and for the bias  bound_b = sum over rows with fb = 0 of |dZ[m, n]| + 2^-40 Sb_all.  Normalisers: S[n, k] = sum over kept rows of
|dZ[m, n]| |X[m, k]|, Sb[n] = sum over rows with fb != 0 of |dZ[m, n]|; *_all: over every row.
"""
from types import SimpleNamespace

import numpy as np

EZERO = 0x7FFF
TILE = 128
F_CLAMP = -30                 # the kernel's clamp of the factors' exponent (never reached as a value: fp16(2^-25) = 0)
DROP_K = 25                   # rows this far below their block's top are multiplied by 0
RESCALE_CAP = 72              # see above
MAX_JOBS = 12


def bits_kept(k):
    """bits of a row, relative to its largest element, that are sure to survive the multiplication by fp16(2^-k): the two subnormal
    roundings of an element (hi', lo') are at most 2^-24 against a top of 2^(14 - k); typically one of them dominates (one bit more)"""
    return 0 if k >= DROP_K else min(22, 38 - k)


def slices(M, tiles_total):
    """(batch slices, rows per slice) of a launch over M rows and `tiles_total` 128 x 128 tiles of all its jobs (wgrad_slices with SLICES_H2I, csrc/wgrad_plan.hpp)"""
    s = max(8, min(24, 768 // max(tiles_total, 1) // 8 * 8))
    s = min(s, -(-(-(-M // 128)) // 8) * 8)
    return s, -(-(-(-M // s)) // 128) * 128


def workspace_bytes(M, shapes):
    """bytes of the partial slabs of a launch over jobs of shapes [(N, K), ...]"""
    tiles = sum(-(-N // 128) * -(-K // 128) for N, K in shapes)
    s, _ = slices(M, tiles)
    return sum(s * (-(-N // 128) * -(-K // 128) * 128 * 128 + -(-K // 128) * -(-N // 128) * 128) * 4 for N, K in shapes)


def planes(A, ex):
    """(hi, lo) float16 [row tiles * 128, k blocks * 128] of A [M, C] under the exponents ex [row tiles, k blocks, 128]"""
    A = np.asarray(A, dtype=np.float64)
    rt, kb = ex.shape[:2]
    P = np.zeros((rt * 128, kb * 128))
    P[:A.shape[0], :A.shape[1]] = A
    e = np.where(ex == EZERO, 0, ex).transpose(0, 2, 1).reshape(rt * 128, kb)
    with np.errstate(over="ignore", invalid="ignore"):
        xs = np.ldexp(P.reshape(rt * 128, kb, 128), e[:, :, None]).reshape(rt * 128, kb * 128).astype(np.float32)
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def decoded(A, ex):
    """what an image of A [M, C] under the exponents ex decodes to: float64 (hi + lo) 2^-e, exactly"""
    hi, lo = planes(A, ex)
    rt, kb = ex.shape[:2]
    e = np.where(ex == EZERO, 0, ex).transpose(0, 2, 1).reshape(rt * 128, kb)
    v = (hi.astype(np.float64) + lo.astype(np.float64)).reshape(rt * 128, kb, 128)
    return np.ldexp(v, -e[:, :, None]).reshape(rt * 128, kb * 128)[:A.shape[0], :A.shape[1]]


def _sub_round(v16, f):
    """r(v f) of the module text: 2^-25 where the fp16 product is a non-zero subnormal, else 0"""
    m = np.abs(v16.astype(np.float64)) * f[:, None]
    return np.where((m > 0) & (m < 2.0 ** -14), 2.0 ** -25, 0.0)


def emulate(dZ, X, eZ, eX, M, rescale="bounded", tiles_total=None, want_bound=True):
    """dZ [M, N], X [M, K]: the decoded operands; eZ / eX: their exponent tables [row tiles, k blocks, 128]; tiles_total: the 128 x
    128 tiles of ALL jobs of the launch (default: this job alone) -- it decides the batch slices.
    want_bound=False leaves `bound` at its float64 term alone (saves half the work where only the emulation is wanted).
    -> dW, db            float64: the scheme under `rescale`'s factors with exact accumulation
       dW32, db32        float32: one accumulator set per slice carried through the block borders in float32 (every block's own sum
                         added exactly, then rounded), slices added in order as the reduce kernel does
       S, Sb, S_all, Sb_all, bound, bound_b     see the module text
       dropped           bool [M]: rows multiplied by 0 in at least one tile;   T [slice-local list]: (tr, tc, block, T, Tz)"""
    assert rescale in ("as_built", "bounded")
    dZ, X = np.asarray(dZ, dtype=np.float64), np.asarray(X, dtype=np.float64)
    N, K = dZ.shape[1], X.shape[1]
    rt, rtn, rtk = -(-M // 128), -(-N // 128), -(-K // 128)
    assert eZ.shape == (rt, rtn, 128) and eX.shape == (rt, rtk, 128) and dZ.shape[0] == M == X.shape[0]
    eZ, eX = np.asarray(eZ, dtype=np.int64), np.asarray(eX, dtype=np.int64)
    splits, rps = slices(M, rtn * rtk if tiles_total is None else tiles_total)
    ah, al = (p.astype(np.float64) for p in planes(dZ, eZ))
    bh16, bl16 = planes(X, eX)
    zp, xp = np.zeros((rt * 128, rtn * 128)), np.zeros((rt * 128, rtk * 128))
    zp[:M, :N], xp[:M, :K] = np.abs(dZ), np.abs(X)
    Np, Kp = rtn * 128, rtk * 128
    out = {k: np.zeros((Np, Kp)) for k in ("dW", "S", "S_all", "bound")}
    outb = {k: np.zeros(Np) for k in ("db", "Sb", "Sb_all", "bound_b")}
    dW32, db32 = np.zeros((Np, Kp), dtype=np.float32), np.zeros(Np, dtype=np.float32)
    dropped, trace = np.zeros(rt * 128, dtype=bool), []
    cap = rescale == "bounded"
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for tr in range(rtn):
            cn = slice(tr * 128, tr * 128 + 128)
            for tc in range(rtk):
                ck = slice(tc * 128, tc * 128 + 128)
                for s in range(splits):
                    b0, b1 = s * rps // 128, min(rt, (s + 1) * rps // 128)
                    if b0 >= b1:
                        continue
                    acc, accb = np.zeros((128, 128), dtype=np.float32), np.zeros(128, dtype=np.float32)
                    t_cur = tz_cur = 0
                    t_lo = tz_lo = None
                    for b in range(b0, b1):
                        rows = slice(b * 128, b * 128 + 128)
                        ez, ex = eZ[b, tr], eX[b, tc]
                        zlive = ez != EZERO
                        live = zlive & (ex != EZERO)
                        esum = np.where(live, ez + ex, 0)
                        T, Tz = t_cur, tz_cur
                        if live.any():
                            T = int(esum[live].min())
                            if cap and t_lo is not None:
                                T = min(T, t_lo + RESCALE_CAP)
                            t_lo = T if t_lo is None else min(t_lo, T)
                        if zlive.any():
                            Tz = int(ez[zlive].min())
                            if cap and tz_lo is not None:
                                Tz = min(Tz, tz_lo + RESCALE_CAP)
                            tz_lo = Tz if tz_lo is None else min(tz_lo, Tz)
                        f16 = np.ldexp(1.0, np.maximum(np.where(live, T - esum, 0), F_CLAMP)).astype(np.float16)
                        fb = np.ldexp(1.0, np.maximum(np.where(zlive, Tz - ez, 0), F_CLAMP)).astype(np.float16).astype(np.float64)
                        f = f16.astype(np.float64)
                        bh = (bh16[rows, ck] * f16[:, None]).astype(np.float64)             # numpy float16 product: one rounding
                        bl = (bl16[rows, ck] * f16[:, None]).astype(np.float64)
                        A_h, A_l = ah[rows, cn] * live[:, None], al[rows, cn] * live[:, None]
                        blk = A_l.T @ bh + A_h.T @ (bl + bh)               # float64: the three products, exactly
                        out["dW"][cn, ck] += np.ldexp(blk, -T)
                        if b > b0:
                            acc = np.ldexp(acc, T - t_cur).astype(np.float32)
                        acc = (acc.astype(np.float64) + blk).astype(np.float32)
                        # normalisers and the bound
                        kept, drop = live & (f != 0), live & (f == 0)
                        dropped[rows] |= drop
                        Zb, Xb = zp[rows, cn], xp[rows, ck]
                        S_blk = (Zb * kept[:, None]).T @ Xb
                        D_blk = (Zb * drop[:, None]).T @ Xb if drop.any() else 0.0
                        out["S"][cn, ck] += S_blk
                        out["S_all"][cn, ck] += S_blk + D_blk               # (a row that is not live has a zero operand row)
                        if want_bound:
                            w = np.ldexp(1.0, -esum) * kept
                            lolo = (np.abs(al[rows, cn]) * w[:, None]).T @ np.abs(bl16[rows, ck].astype(np.float64))
                            kf = np.where(kept, f, 0.0)
                            rh, rl = _sub_round(bh16[rows, ck], kf), _sub_round(bl16[rows, ck], kf)
                            rnd = np.ldexp((np.abs(ah[rows, cn]) + np.abs(al[rows, cn])).T @ rh + np.abs(ah[rows, cn]).T @ rl, -T)
                            out["bound"][cn, ck] += lolo + rnd + D_blk
                        if tc == 0:
                            blkb = (ah[rows, cn] + al[rows, cn]).T @ fb
                            outb["db"][cn] += np.ldexp(blkb, -Tz)
                            if b > b0:
                                accb = np.ldexp(accb, Tz - tz_cur).astype(np.float32)
                            accb = (accb.astype(np.float64) + blkb).astype(np.float32)
                            keptb = zlive & (fb != 0)
                            outb["Sb"][cn] += (Zb * keptb[:, None]).sum(0)
                            outb["Sb_all"][cn] += Zb.sum(0)
                            outb["bound_b"][cn] += (Zb * (zlive & (fb == 0))[:, None]).sum(0)
                        trace.append((tr, tc, b, T, Tz))
                        t_cur, tz_cur = T, Tz
                    dW32[cn, ck] += np.ldexp(acc, -t_cur).astype(np.float32)
                    if tc == 0:
                        db32[cn] += np.ldexp(accb, -tz_cur).astype(np.float32)
    out["bound"] += 2.0 ** -40 * out["S_all"]
    outb["bound_b"] += 2.0 ** -40 * outb["Sb_all"]
    r = {k: v[:N, :K] for k, v in out.items()}
    r.update({k: v[:N] for k, v in outb.items()})
    return SimpleNamespace(dW32=dW32[:N, :K], db32=db32[:N], dropped=dropped[:M], T=trace, splits=splits, rows_per_split=rps, **r)


def truth(dZ, X):
    """float64 dZ^T X and colsum(dZ)"""
    dZ, X = np.asarray(dZ, dtype=np.float64), np.asarray(X, dtype=np.float64)
    return dZ.T @ X, dZ.sum(0)


def rel(err, den):
    """largest err / den over the elements with den > 0; elements with den == 0 must have err == 0 (else inf)"""
    err, den = np.asarray(err, dtype=np.float64), np.asarray(den, dtype=np.float64)
    if err.size == 0:
        return 0.0
    bad = (den <= 0) & ~(err == 0)
    if bad.any():
        return float("inf")
    live = den > 0
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.nan_to_num((err[live] / den[live]), nan=np.inf).max()) if live.any() else 0.0


def chain_tolerance(M, tiles_total):
    """bound of the kernel's fp32 addition chain relative to S: every one of the (stages per slice x 3 MFMAs + slices) additions
    rounds a partial sum that is at most S, by at most 2^-24 of it"""
    s, rps = slices(M, tiles_total)
    return ((rps // 16) * 3 + s) * 2.0 ** -24
