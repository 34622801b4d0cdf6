// Weight gradients from block-scaled two-term fp16 operand images (round 5; format: csrc/h2i_core.hpp): dW [N, K] = dZ^T X and
// db = colsum(dZ) for the nn.Linear stacks of rsl_rl/rsl_rl/modules/actor_critic_decoder.py:98-188, 323-349 under loss.backward()
// (ppo.py:252, 333), with BOTH operands given as the images their producers wrote.
//
// The reduction index is the batch row = the ROW index of both images, so a stage (16 batch rows x 128 columns of each operand) arrives
// by LDS-DMA as 16-byte pieces (8 columns of one batch row) in the sub-block layout
//   stage image [R = row / 4][Q = column / 32][a = row % 4][b = (column / 8) % 4][16 bytes]            (4 KiB per plane and operand)
// and the MFMA fragments (8 consecutive batch rows of ONE column per lane) come out of it by the hardware transpose read
// ds_read_b64_tr_b16 (tools/probes/tr16_dma.hip; conflict free).  The images carry one exponent per batch row and 128-column block:
// row m of dZ is stored times 2^eZ[m], row m of X times 2^eX[m].  Per 128-row block the workgroup forms T = min_m (eZ[m] + eX[m]) and the
// fp16 factors f[m] = 2^(T - eZ[m] - eX[m]) <= 1; the X fragments are multiplied by f (4 v_pk_mul_f16 per fragment), the accumulators hold
// 2^T x the true sums and are rescaled by ONE scalar at the borders of the 128-row blocks (by at most RESCALE_CAP above the slice's
// smallest scale, see there).  The bias gradient is dZ^T x fb on the matrix pipe, fb[m] = 2^(Tz - eZ[m]).
// What a row k = eZ[m] + eX[m] - T octaves below its block's top row keeps (oracle/wgrad_image_ref.py restates the scheme and derives
// the figures, tests/test_hip_wgrad_image.py holds the kernel to them element by element, profiles/wgrad_image_errors.txt has a run):
//   * k <= 16: all 22 bits of the (hi, lo) pair, relative to the ROW's largest element (what lo f loses below 2^-24 is below the
//     pair's own last bit);
//   * 17 <= k <= 24: at least 38 - k bits (21 .. 14): lo f, then hi f too, are fp16 subnormals, multiples of 2^-24 against a top of
//     2^(14 - k) (measured on the CPU with numpy float16: 2^-21.4 at k = 17, 2^-18.4 at 20, 2^-14.5 at 24);
//   * k >= 25: NOTHING -- (_Float16)2^-25 rounds to 0 (halfway to the smallest subnormal, ties to even), the row is multiplied by 0
//     and the clamp at 2^-30 below is never reached as a value.  The bias factor fb sees k = eZ[m] - Tz alone.
// Per ELEMENT of dW that is the error of an fp32 product only where the feature is dense: a feature (row of dW, or input column)
// whose non-zero entries all sit in rows of tier k gets those bits and no more, and one that lives only in rows with k >= 25
// gets a gradient of exactly 0 -- a ReLU unit that fires only on samples whose gradient rows are 2^-25 below their block's largest.
// This is the price of one fp16 multiply per fragment; a wider range for f is a performance trade left open.
// Per wave and stage: 4 LDS-DMA pieces, 16 transpose reads, 2 table reads, 16 v_pk_mul_f16, 12 MFMAs.
// The stage loop is unrolled over three 128-row blocks (24 stages: the period of (position in the block, stage buffer)).
// Partial slabs [batch slice][tile][128][128]; wgrad_h2i_reduce_kernel sums the slices in a fixed order.  The slice rule, the index
// maps, the slab sum and the host plan are shared with the other weight-gradient families: csrc/wgrad_plan.hpp.
#include "h2i_core.hpp"
#include "wgrad_plan.hpp"

namespace {

constexpr int TILE = 128;
// How far a block may raise the accumulators' scale above the smallest scale a block of the same batch slice has had.  A row of block
// b adds at most three products |hi hi'| <= 2^30 f, f <= 1, to accumulators held at scale T_b; at a later scale T_c they are therefore
// below rows x 2^30.01 x 2^(T_c - min_b T_b).  A slice holds at most 2^22 rows: an image is below 2 GiB and a row takes at least 64
// bytes, so M < 2^25, and a launch has at least 8 slices (rows_per_split).  With T_c - min_b T_b <= 72 the accumulators stay below
// 2^(22 + 30.01 + 72) < 2^125: finite operands cannot push them to inf at a border.  (The bias accumulators hold |a| 2^FB_UP fb <= 2^30.01
// per row: the same bound.)  Ordinary data never comes near the cap -- 72 octaves between the top rows of
// two 128-row blocks of one slice -- so its bits do not depend on it; a block beyond it gets the rest of its step as a smaller f / fb,
// i.e. it is attenuated like rows far below a block's top, or dropped (oracle/wgrad_image_ref.py, rescale = "bounded").
constexpr int RESCALE_CAP = 72;
// The bias factors are stored times 2^FB_UP.  v_mfma_f32_32x32x16_f16 does not keep the bits of a product below about 2^-24: with
// fb = 2^-k itself, a feature whose bias gradient comes from rows k octaves below the top came out 2^(k - 40) wrong relative to its
// own sum of magnitudes (measured: 9e-7 at k = 20, 1.3e-5 at k = 24; nothing at k <= 14), although a power-of-two factor promises an
// exact sum.  With 2^15 fb (the largest power of two fp16 holds) the last bit of a 22-bit (hi, lo) pair times fb sits at 2^-16 for
// k = 24, and the products stay below 2^30.01, the bound the cap above was derived for.  (The dW products have the same floor, 25 and
// more octaves below the first bit of hi f: nothing of the bits the factors keep.)
constexpr int FB_UP = 15;
constexpr int T_NONE = 0x3fffffff;           // "no block with content yet" (T_NONE + RESCALE_CAP still fits an int)
typedef __fp16 h16x4 __attribute__((ext_vector_type(4)));
typedef __fp16 h16x8 __attribute__((ext_vector_type(8)));

struct HJob {
    const u32x4* dZ;        // image(M, N)
    const u32x4* X;         // image(M, K)
    const int* ez;          // exps of dZ: [row tile][kbs_n][128]
    const int* ex;
    u32 dz_bytes, x_bytes;
    float* dW;
    float* db;
    float* part;            // [splits][tiles][128][128]
    float* bpart;           // [splits][col_tiles][row_tiles][128]
    long long ldw;
    int N, K, col_tiles, row_tiles, st_n, st_k, kbs_n, kbs_k;
    int tile_end;           // running sum of tiles over the jobs
};
struct HGroup {
    int count, M, mtiles, rows_per_split, splits, tiles_total;
    HJob job[WGRAD_MAX_JOBS];
};

// PASSES = 3: lo hi' + hi lo' + hi hi' per product (the default); PASSES = 1 (opt-in, dtc_set_h2i_passes): plane 0 of both operands alone
// -- 2 LDS-DMA pieces, 8 transpose reads, 8 v_pk_mul_f16 and 4 dW MFMAs per wave and stage, the bias product on the hi plane.  Tables,
// RESCALE_CAP, FB_UP, the slabs and the reduce kernel are the same for both.
template <int PASSES>
__device__ __forceinline__ void wgrad_h2i_group_body(const HGroup& G) {
    constexpr int NP = PASSES == 3 ? 2 : 1;                           // planes of an operand a stage fetches and reads
    // separate objects per stage buffer: an LDS-DMA into one cannot alias the fragment reads of the other
    // (three stage buffers: the transfers run two stages ahead of the MFMAs, see linear_h2i_kernel)
    __shared__ __attribute__((aligned(16))) unsigned char A0[2][4096];
    __shared__ __attribute__((aligned(16))) unsigned char A1[2][4096];
    __shared__ __attribute__((aligned(16))) unsigned char A2[2][4096];
    __shared__ __attribute__((aligned(16))) unsigned char B0[2][4096];
    __shared__ __attribute__((aligned(16))) unsigned char B1[2][4096];
    __shared__ __attribute__((aligned(16))) unsigned char B2[2][4096];
    __shared__ __attribute__((aligned(16))) _Float16 Ft[2][128];      // f[m] of the block in flight / the next one
    __shared__ __attribute__((aligned(16))) _Float16 Fb[2][128];      // fb[m]
    __shared__ int Tt[2][2];                                          // (T, Tz) per table
    __shared__ int Tred[4][2];
#define AS(b) ((b) == 0 ? A0 : (b) == 1 ? A1 : A2)
#define BS(b) ((b) == 0 ? B0 : (b) == 1 ? B1 : B2)
    int split, t;
    if (!slice_tile(G.tiles_total, G.splits, split, t)) return;
    const JobPos jp = tile_job(G, t);
    const int tiles_j = job_tiles(G, jp.j);
    t = jp.t;
    const HJob& J = G.job[jp.j];
    const int tr = t / J.col_tiles, tc = t - tr * J.col_tiles;
    const int m_begin = split * G.rows_per_split;                    // multiples of 128: a slice is a whole number of exponent blocks
    const int m_end = min(G.mtiles * 128, m_begin + G.rows_per_split);
    const int m_live = min(m_end, G.M);                              // batch rows >= M (the tail of the last row tile, h2i_core.hpp) are never fetched: zeros land
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;

    // ---- LDS-DMA geometry: lane t of the workgroup = piece (R = wave, Q, a, b) of the stage image, for A (dZ) and B (X) alike
    const int Q = (tid >> 4) & 3, a4 = (tid >> 2) & 3, b4 = tid & 3;
    const int mrow = 4 * wave + a4;                                          // batch row inside the stage (0..15)
    const u32 slot = (u32)(mrow * 2 + ((b4 & 1) ^ ((mrow >> 3) & 1))) * 16u;   // rslot(row, half) of the source chunk (stage rows are 16-aligned)
    const int sa = tr * 8 + 2 * Q + (b4 >> 1), sb = tc * 8 + 2 * Q + (b4 >> 1);   // source stage (16 columns) of this lane's piece
    const u32 aoff = sa < J.st_n ? (u32)sa * (u32)HI_CHUNK + slot : INVALID;  // columns behind the matrix: zeros land
    const u32 boff = sb < J.st_k ? (u32)sb * (u32)HI_CHUNK + slot : INVALID;
    const rsrc_t ares = make_rsrc_bytes(J.dZ, J.dz_bytes), bres = make_rsrc_bytes(J.X, J.x_bytes);
    // one stage of both operands -> stage buffer nbc: ua / ub = byte offset of its 16 batch rows in the two images, dead = INVALID: zeros land
    auto load_at = [&](auto nbc, u32 ua, u32 ub, u32 dead) {
        constexpr int nbuf = decltype(nbc)::value;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ares, (lds_void*)&AS(nbuf)[p][wave * 1024], 16, aoff | dead, ua + p * HI_PLANE, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(bres, (lds_void*)&BS(nbuf)[p][wave * 1024], 16, boff | dead, ub + p * HI_PLANE, 0, 0);
        }
    };

    // ---- the scale tables of a 128-row block, built by threads < 128 (one batch row each) in three steps that ride on the stages of the
    // block before it: (1) request the two exponents, (2) minima over the block -> Tred (per wave), (3) after a barrier: T, Tz and the
    // factors -> Ft / Fb / Tt of the table the next block reads
    int ez_n = HI_EZERO, ex_n = HI_EZERO;
    int t_lo = T_NONE, tz_lo = T_NONE;      // smallest T / Tz of the slice's blocks with content so far (threads < 128, all the same)
    auto table_request = [&](int mb) {
        if (tid < 128) {
            const int mt = mb >> 7;
            const bool ok = mt < G.mtiles;
            ez_n = ok ? J.ez[((long long)mt * J.kbs_n + tr) * 128 + tid] : HI_EZERO;
            ex_n = ok ? J.ex[((long long)mt * J.kbs_k + tc) * 128 + tid] : HI_EZERO;
        }
    };
    auto table_minima = [&]() {
        if (tid < 128) {
            const bool live = ez_n != HI_EZERO && ex_n != HI_EZERO;
            int tm = live ? ez_n + ex_n : 0x7fffffff, tz = ez_n != HI_EZERO ? ez_n : 0x7fffffff;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                tm = min(tm, __shfl_xor(tm, off, 64));
                tz = min(tz, __shfl_xor(tz, off, 64));
            }
            if (lane == 0) {
                Tred[wave][0] = tm;
                Tred[wave][1] = tz;
            }
        }
    };
    auto table_finish = [&](int which, int t_prev, int tz_prev) {
        if (tid < 128) {
            int T = min(Tred[0][0], Tred[1][0]), Tz = min(Tred[0][1], Tred[1][1]);
            // a block without content keeps the scale (nothing to add, nothing to rescale); one with content raises it to at most
            // RESCALE_CAP above the slice's smallest so far and takes the rest into its factors
            const bool has = T != 0x7fffffff, hasz = Tz != 0x7fffffff;
            T = has ? min(T, t_lo + RESCALE_CAP) : t_prev;
            Tz = hasz ? min(Tz, tz_lo + RESCALE_CAP) : tz_prev;
            t_lo = has ? min(t_lo, T) : t_lo;
            tz_lo = hasz ? min(tz_lo, Tz) : tz_lo;
            const bool live = ez_n != HI_EZERO && ex_n != HI_EZERO;
            const int d = live ? T - (ez_n + ex_n) : 0, dz = ez_n != HI_EZERO ? Tz - ez_n : 0;
            Ft[which][tid] = (_Float16)__builtin_ldexpf(1.0f, d < -30 ? -30 : d);
            // fb carries 2^FB_UP (taken out again in the epilogue) and is 0 from 25 octaves below the top, as f is: see FB_UP
            Fb[which][tid] = dz < -24 ? (_Float16)0.0f : (_Float16)__builtin_ldexpf(1.0f, dz + FB_UP);
            if (tid == 0) {
                Tt[which][0] = T;
                Tt[which][1] = Tz;
            }
        }
    };

    // ---- fragment geometry (ds_read_b64_tr_b16): 16-lane group g: k half g >> 1, 16-column sub-block g & 1 of the 32-column tile;
    // lane i of the group supplies chunk i (row i >> 2, columns 4 (i & 3) .. + 3) and receives column i, rows 0..3
    const int g = lane >> 4, i16 = lane & 15;
    const int khalf = g >> 1, nsub = g & 1;
    const int frag = ((i16 >> 2) * 4 + 2 * nsub + ((i16 & 3) >> 1)) * 16 + 8 * (i16 & 1);          // (a, b, 8-byte half) inside a sub-block
    // sub-block (R, Q) at ((R * 4 + Q) * 256) bytes; R = 2 khalf + r (r = 0, 1: rows 0..3 / 4..7 of the half)
    const int a_base = (2 * khalf * 4 + 2 * wr) * 256 + frag, b_base = (2 * khalf * 4 + 2 * wc) * 256 + frag;
    auto rd = [&](const unsigned char* plane, int off) {
        const h16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h16x4*)(plane + off));
        const h16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h16x4*)(plane + off + 4 * 256));
        return __builtin_bit_cast(f16x8, h16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
    };

    f32x16 acc[2][2], accb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) accb[i][r] = 0.f;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][jj][r] = 0.f;
    }

    const int KT = (m_end - m_begin + BK - 1) / BK;               // stages of this slice (a multiple of 8)
    const bool want_bias = J.db != nullptr;
    int t_cur = 0, tz_cur = 0;                                     // scale of the accumulators (T, Tz of the block in flight)
    if (KT > 0) {
        table_request(m_begin);
        // batch rows mb .. mb + 15 sit in row tile mb >> 7 at local rows (mb & 127) ..; rows >= m_live: nothing valid -> zeros
        const u32 ua = (u32)((m_begin >> 7) * J.st_n) * (u32)HI_CHUNK, ub = (u32)((m_begin >> 7) * J.st_k) * (u32)HI_CHUNK;
        load_at(S0{}, ua, ub, oob_mask(m_begin + mrow, m_live - 1));
        load_at(S1{}, ua + BK * 32u, ub + BK * 32u, oob_mask(m_begin + BK + mrow, m_live - 1));
        table_minima();
        __syncthreads();
        table_finish(0, 0, 0);
        __syncthreads();
        t_cur = Tt[0][0];
        tz_cur = Tt[0][1];
    }
    int bias_phase = 0;
    const int col_tiles_u = __builtin_amdgcn_readfirstlane(J.col_tiles);
    // ---- a stage, with its position inside the 128-row block (ph) and its buffer as compile-time constants: no branch on the phase, the table
    // reads and the transfers' row offsets are immediates, a block's validity is one scalar -- ~80 instructions per stage, 12-16 of them MFMAs
    // (round 6; with ph = kt % 8 and the buffer as run-time / per-trip values the stage had ~130 and five taken branches: -6..9 % for the launch
    // alone, -1.15 ms per bench step, same bits; profiles/r06_wgrad_unroll_*.txt).  Three blocks (24 stages) per trip: stage kt sits in buffer kt % 3.
    // A ragged M ends inside ONE block of a launch (tail / tail_n below).  Whole blocks are fetched by the plain transfers, one scalar
    // dead / dead_n and the offsets hoisted per block; for the block M ends in those transfers are dead as a whole (zeros land) and a second
    // set, issued right behind them in an unlikely uniform branch that lies out of line, fetches its live rows with a per-lane limit (a
    // wave's transfers reach LDS in the order they were issued; the stage waits count them in that order, so a stage with twice the
    // transfers only waits longer).  A whole block's stage is the stage it was plus one scalar test and one branch that is not taken.
    auto tail_dead = [&](int row, int lim) { return oob_mask(mrow + row, lim - 1); };
    struct Blk {
        int kt0, which;
        bool more;
        u32 ua, ub, dead, ua_n, ub_n, dead_n;       // byte offsets of this block's / the next block's row tile in the two images; INVALID: no live row in it
        int lim, lim_n;                             // live batch rows of this block / the next one (<= 0: none -- behind the slice or behind M; >= 128: all)
        bool tail, tail_n;                          // 0 < lim < 128: a ragged M ends inside the block
    };
    auto stage = [&](auto bc, auto phc, const Blk& B) {
        constexpr int buf = decltype(bc)::value, ph = decltype(phc)::value;
        const int which = B.which;
        const bool bias = want_bias && bias_phase == tc;
        bias_phase = bias_phase + 1 == col_tiles_u ? 0 : bias_phase + 1;
        if constexpr (ph == 0) {
            if (B.kt0 > 0) {                                  // (uniform) first stage of a block: the accumulators change scale
                const int tn = Tt[which][0], tzn = Tt[which][1];
                const int d = tn - t_cur, dz = tzn - tz_cur;
                if (d != 0) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[i][jj][r] = __builtin_ldexpf(acc[i][jj][r], d);
                }
                if (dz != 0) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) accb[i][r] = __builtin_ldexpf(accb[i][r], dz);
                }
                t_cur = tn;
                tz_cur = tzn;
            }
        }
        if constexpr (ph == 7) {
            if (B.more) table_finish(which ^ 1, t_cur, tz_cur);
        }
        if constexpr (ph == 6) {
            if (B.more) table_request(m_begin + (B.kt0 + 8) * BK);
        }
        const f16x8 fv = *reinterpret_cast<const f16x8*>(&Ft[which][ph * 16 + 8 * khalf]);
        const f16x8 fbv = *reinterpret_cast<const f16x8*>(&Fb[which][ph * 16 + 8 * khalf]);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ph < 6) {
            load_at(std::integral_constant<int, (buf + 2) % 3>{}, B.ua + (ph + 2) * 512, B.ub + (ph + 2) * 512, B.dead);
            if (__builtin_expect(B.tail, 0))                  // (uniform, once per launch at most) the live rows of the block a ragged M ends in
                load_at(std::integral_constant<int, (buf + 2) % 3>{}, B.ua + (ph + 2) * 512, B.ub + (ph + 2) * 512, tail_dead((ph + 2) * 16, B.lim));
        } else {
            load_at(std::integral_constant<int, (buf + 2) % 3>{}, B.ua_n + (ph - 6) * 512, B.ub_n + (ph - 6) * 512, B.dead_n);
            if (__builtin_expect(B.tail_n, 0))
                load_at(std::integral_constant<int, (buf + 2) % 3>{}, B.ua_n + (ph - 6) * 512, B.ub_n + (ph - 6) * 512, tail_dead((ph - 6) * 16, B.lim_n));
        }
        __builtin_amdgcn_sched_barrier(0);
        f16x8 a[2][2], b[2][2];
#pragma unroll
        for (int p = NP - 1; p >= 0; --p) {
            a[0][p] = rd(AS(buf)[p], a_base);
            b[0][p] = rd(BS(buf)[p], b_base);
            a[1][p] = rd(AS(buf)[p], a_base + 256);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) b[1][p] = rd(BS(buf)[p], b_base + 256);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < NP; ++p) b[0][p] = b[0][p] * fv;
        if constexpr (PASSES == 1) {                         // hi hi' alone: four dW MFMAs
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][0], b[0][0], acc[i][0], 0, 0, 0);
            b[1][0] = b[1][0] * fv;
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][0], b[1][0], acc[i][1], 0, 0, 0);
        } else {
        // smallest terms first: lo hi', hi lo', hi hi'
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][1], b[0][0], acc[i][0], 0, 0, 0);
#pragma unroll
        for (int p = 0; p < 2; ++p) b[1][p] = b[1][p] * fv;
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][0], b[0][1], acc[i][0], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][0], b[0][0], acc[i][0], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][1], b[1][0], acc[i][1], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][0], b[1][1], acc[i][1], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][0], b[1][0], acc[i][1], 0, 0, 0);
        }
        if (bias && wc == 0) {                               // wave-uniform: this tile's share of the column sums of dZ (the wc = 1 waves hold the same rows)
#pragma unroll
            for (int p = NP - 1; p >= 0; --p)
#pragma unroll
                for (int i = 0; i < 2; ++i) accb[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][p], fbv, accb[i], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ph == 6) {
            if (B.more) table_minima();                       // the exponents requested at the stage's head have long arrived
        }
        // this wave's newest stage (4 transfers; one pass: 2) may stay in flight: vmcnt(4) / vmcnt(2), lgkmcnt(0), expcnt untouched
        __builtin_amdgcn_s_waitcnt(0x0070 | (2 * NP));
        __builtin_amdgcn_s_barrier();
    };
    auto block = [&](auto b0c, int kt0) {
        constexpr int b0 = decltype(b0c)::value;              // buffer of the block's first stage
        Blk B;
        B.kt0 = kt0;
        B.which = (kt0 >> 3) & 1;
        B.more = kt0 + 8 < KT;
        const int mb0 = m_begin + kt0 * BK;
        B.ua = (u32)((mb0 >> 7) * J.st_n) * (u32)HI_CHUNK;
        B.ub = (u32)((mb0 >> 7) * J.st_k) * (u32)HI_CHUNK;
        B.ua_n = B.ua + (u32)J.st_n * (u32)HI_CHUNK;
        B.ub_n = B.ub + (u32)J.st_k * (u32)HI_CHUNK;
        B.lim = m_live - mb0;                                 // (slices are whole 128-row blocks; M need not be)
        B.lim_n = B.lim - 128;
        B.dead = B.lim < 128 ? INVALID : 0u;                  // whole blocks alone are fetched by the plain transfers
        B.dead_n = B.lim_n < 128 ? INVALID : 0u;
        B.tail = B.lim > 0 && B.lim < 128;
        B.tail_n = B.lim_n > 0 && B.lim_n < 128;
        stage(std::integral_constant<int, (b0 + 0) % 3>{}, std::integral_constant<int, 0>{}, B);
        stage(std::integral_constant<int, (b0 + 1) % 3>{}, std::integral_constant<int, 1>{}, B);
        stage(std::integral_constant<int, (b0 + 2) % 3>{}, std::integral_constant<int, 2>{}, B);
        stage(std::integral_constant<int, (b0 + 3) % 3>{}, std::integral_constant<int, 3>{}, B);
        stage(std::integral_constant<int, (b0 + 4) % 3>{}, std::integral_constant<int, 4>{}, B);
        stage(std::integral_constant<int, (b0 + 5) % 3>{}, std::integral_constant<int, 5>{}, B);
        stage(std::integral_constant<int, (b0 + 6) % 3>{}, std::integral_constant<int, 6>{}, B);
        stage(std::integral_constant<int, (b0 + 7) % 3>{}, std::integral_constant<int, 7>{}, B);
    };
    for (int kt0 = 0; kt0 < KT; kt0 += 24) {                  // KT is a multiple of 8; stage kt sits in buffer kt % 3
        block(std::integral_constant<int, 0>{}, kt0);
        if (kt0 + 8 < KT) block(std::integral_constant<int, 2>{}, kt0 + 8);
        if (kt0 + 16 < KT) block(std::integral_constant<int, 1>{}, kt0 + 16);
    }

    // ---- epilogue: accumulators (2^T x the sums) -> slab tile [128][128] in logical order (float4 rows through the wave's LDS patch)
    __syncthreads();
    const int half = lane >> 5, l31 = lane & 31;
    float* P = J.part + ((long long)split * tiles_j + t) * (TILE * TILE);
    float* patch = reinterpret_cast<float*>(wave < 2 ? &A0[wave][0] : &A1[wave - 2][0]);
    const int prow = lane >> 3, pc4 = lane & 7;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][jj][r] = __builtin_ldexpf(acc[i][jj][r], -t_cur);
            patch_put(patch, acc[i][jj], half, l31);
            float* q = P + (long long)((2 * wr + i) * 32 + prow) * TILE + (2 * wc + jj) * 32 + 4 * pc4;
#pragma unroll
            for (int p = 0; p < 4; ++p) *reinterpret_cast<f32x4*>(q + (long long)(8 * p) * TILE) = patch_get(patch, prow + 8 * p, pc4);
        }
    if (want_bias && wc == 0 && l31 == 0) {                 // column 0 of accb holds the sums (every column is the same); rows = dZ's columns
        float* bp = J.bpart + (((long long)split * J.col_tiles + tc) * J.row_tiles + tr) * TILE;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) bp[(2 * wr + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half] = __builtin_ldexpf(accb[i][r], -tz_cur - FB_UP);
    }
#undef AS
#undef BS
}

__global__ __launch_bounds__(256, 3) void wgrad_h2i_group_kernel(const HGroup G) { wgrad_h2i_group_body<3>(G); }
__global__ __launch_bounds__(256, 3) void wgrad_h2i_onepass_group_kernel(const HGroup G) { wgrad_h2i_group_body<1>(G); }

// Sum of the batch slices in a fixed order; dW / db written once.  block = (tile, 8 rows); thread = (row, float4 of columns)
__global__ __launch_bounds__(256) void wgrad_h2i_reduce_kernel(const HGroup G) {
    int b = blockIdx.x;
    const int blocks_tiles = G.tiles_total * 16;
    if (b >= blocks_tiles) {                           // bias blocks: four per (job, row tile), 32 features each
        b -= blocks_tiles;
        const int quarter = b & 3;
        int j = 0, rt = b >> 2;
        while (j < G.count - 1 && rt >= G.job[j].row_tiles) { rt -= G.job[j].row_tiles; ++j; }
        const HJob& J = G.job[j];
        if (rt >= J.row_tiles || J.db == nullptr) return;
        // thread = (group g of 8, feature): group g sums the partials q = g, g + 8, ... of the (slice, column tile) pairs -- all its loads
        // in flight at once, a fixed order of additions --, then the eight group sums are added in order
        __shared__ float gsum[8][32];
        const int nl = quarter * 32 + (threadIdx.x & 31), grp = threadIdx.x >> 5;
        const int pairs = G.splits * J.col_tiles;
        const long long stride = (long long)J.row_tiles * TILE;               // between consecutive (slice, column tile) pairs
        const float* src = J.bpart + (long long)rt * TILE + nl;
        float acc = 0.f;
#pragma unroll 16
        for (int q = grp; q < pairs; q += 8) acc += src[(long long)q * stride];
        gsum[grp][threadIdx.x & 31] = acc;
        __syncthreads();
        const int n = rt * TILE + nl;
        if (grp == 0 && n < J.N) {
            float t = gsum[0][threadIdx.x];
#pragma unroll
            for (int g2 = 1; g2 < 8; ++g2) t += gsum[g2][threadIdx.x];
            J.db[n] = t;
        }
        return;
    }
    // eight slabs in flight per thread
    reduce_slab_rows<8>(G, b, [](int r) { return r; }, [](const HJob& J, int n, int tc, int c4, const f32x4& sum) {
        const int k = tc * TILE + 4 * c4;
        float* dst = J.dW + (long long)n * J.ldw + k;
        if (k + 4 <= J.K && (reinterpret_cast<unsigned long long>(dst) & 15ull) == 0) {
            *reinterpret_cast<f32x4*>(dst) = sum;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k + e < J.K) dst[e] = sum[e];
        }
    });
}

using HPlan = WgradPlan<HGroup>;

int plan_h2i(const DtcWgradH2iJob* jobs, int count, int M, void* workspace, HPlan& P) {
    int row_tiles = 0;
    int rc = plan_jobs(P.dev, jobs, count, M, SLICES_H2I, 128, [&](int j, const DtcWgradH2iJob& h, HJob& d, int& tiles) -> int {
        DTC_REQUIRE(h.N > 0 && h.K > 0 && h.dZimg && h.Ximg && h.dW && dtc::aligned16(h.dZimg) && dtc::aligned16(h.Ximg), "job %d: bad shape / null or unaligned pointer", j);
        DTC_REQUIRE(h.ldw >= h.K + h.wcol0 && h.wcol0 >= 0, "job %d: columns [%d, %d) outside the %lld-wide gradient", j, h.wcol0, h.wcol0 + h.K, (long long)h.ldw);
        d.dZ = (const u32x4*)h.dZimg;
        d.X = (const u32x4*)h.Ximg;
        d.st_n = (int)hi_stages(h.N);
        d.st_k = (int)hi_stages(h.K);
        d.kbs_n = (int)hi_kblocks(h.N);
        d.kbs_k = (int)hi_kblocks(h.K);
        DTC_REQUIRE(hi_bytes(M, h.N) < (1ll << 31) && hi_bytes(M, h.K) < (1ll << 31), "job %d: image beyond 2 GiB", j);
        d.dz_bytes = (u32)hi_data_bytes(M, h.N);
        d.x_bytes = (u32)hi_data_bytes(M, h.K);
        d.ez = reinterpret_cast<const int*>(reinterpret_cast<const char*>(h.dZimg) + d.dz_bytes);
        d.ex = reinterpret_cast<const int*>(reinterpret_cast<const char*>(h.Ximg) + d.x_bytes);
        d.dW = h.dW + h.wcol0;
        d.ldw = h.ldw;
        d.db = h.db;
        d.N = h.N;
        d.K = h.K;
        d.col_tiles = (int)dtc::ceil_div(h.K, TILE);
        d.row_tiles = (int)dtc::ceil_div(h.N, TILE);
        tiles = d.row_tiles * d.col_tiles;
        row_tiles += d.row_tiles;
        return DTC_OK;
    });
    if (rc != DTC_OK) return rc;
    P.dev.mtiles = (int)hi_rtiles(M);
    const long long splits = P.dev.splits;
    P.bytes = plan_slabs(P, workspace, [&](HJob& d, int tiles_j, auto take) {
        d.part = take(splits * tiles_j * TILE * TILE * (long long)sizeof(float));
        d.bpart = take(splits * d.col_tiles * d.row_tiles * TILE * (long long)sizeof(float));
    });
    P.red_blocks = P.dev.tiles_total * 16 + 4 * row_tiles;
    return DTC_OK;
}

}  // namespace

extern "C" int64_t dtc_wgrad_group_h2i_workspace(const DtcWgradH2iJob* jobs, int count, int M) {
    HPlan P;
    if (plan_h2i(jobs, count, M, nullptr, P) != DTC_OK) return -1;
    return P.bytes;
}

extern "C" int dtc_wgrad_group_h2i(const DtcWgradH2iJob* jobs, int count, int M, void* workspace, void* stream) {
    DTC_REQUIRE(workspace != nullptr && dtc::aligned16(workspace), "wgrad group workspace must be a 16-byte aligned device buffer");
    HPlan P;
    int rc = plan_h2i(jobs, count, M, workspace, P);
    if (rc != DTC_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const HGroup& G = P.dev;
    return wgrad_launch_pair(P, s, "wgrad_group_h2i",
        [&](int grid) {
            if (dtc_get_h2i_passes() == 1) hipLaunchKernelGGL(wgrad_h2i_onepass_group_kernel, dim3(grid), dim3(256), 0, s, G);
            else hipLaunchKernelGGL(wgrad_h2i_group_kernel, dim3(grid), dim3(256), 0, s, G);
        },
        [&] { hipLaunchKernelGGL(wgrad_h2i_reduce_kernel, dim3(P.red_blocks), dim3(256), 0, s, G); });
}
