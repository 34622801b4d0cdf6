// GRU recurrence on block-scaled two-term fp16 operand images (format: csrc/h2i_core.hpp): the time steps of torch.nn.GRU's forward pass
// and BPTT (rsl_rl/rsl_rl/modules/actor_critic_recurrent.py:92-116 under ppo.py:265-335, padded trajectories of utils/utils.py:33-70)
// with BOTH operands of every per-step product read by LDS-DMA -- no conversion in a K loop, three v_mfma_f32_32x32x16_f16 passes per
// product -- and the results the rest of the policy step consumes written as image rows by the kernels that produce them.  OPT-IN
// (DTC_GRU_H2I=1 / dtc_set_gru_h2i(1)); csrc/gru_s3.hip (three bf16 terms converted from fp32 rows in the K loop, six passes) stays the
// default.
//
//   gru_h2i_wimage_kernel   W_hh -> image, once per pass: forward = gate-interleaved tiles (32 units x (r | z | n), reduction over the
//                           hidden index), backward = W_hh^T (128 columns of dh per tile, reduction over the 3H gate index); one exponent per
//                           image row and block of 128 reduction columns
//   gru_h2i_h0_kernel       h0 -> image of step 0, and the exponent e_r of row r for the WHOLE call: e_r = min(14, 14 - floor(log2 max|h0
//                           row r|)).  |h_t| <= max(1, max|h0 row|) for a GRU (h_t is a convex combination of tanh and h_{t-1}), so every
//                           h_t 2^e_r stays below 2^15: a 128-column block of h_t spans four forward tiles -- no workgroup sees its maximum --
//                           and with a fixed exponent none has to.  An element is exact to 2^-22 of itself or 2^-39 2^(14 - e_r) absolute
//   gru_h2i_kernel<FWD>     gh = h_{t-1} W_hh^T from the two images + torch.nn.GRU's gate math; writes fp32 h_t / gates / gh_n, h_t as the
//                           image rows of step t + 1 and, with a slot map, as rows of the head's valid-row images hx (MLP input) and hp
//                           (h_{t-1} operand of the W_hh weight gradient)
//   gru_h2i_gate_bwd_kernel the gate derivatives (the cell of rnn_cells.hpp, gru_gate_bwd4_kernel's summation order); writes fp32 dgi_t /
//                           dgh_t, dgh_t as image rows with per-row, per-block exponents and, with a slot map, the rows of the head's
//                           weight-gradient images
//   gru_h2i_kernel<BWD>     the chunks of dh_{t-1} += dgh_t W_hh from the dgh_t image and the W_hh^T image -> fp32 part[c]
//
// The products are computed TRANSPOSED: the weight fragment is the MFMA's A operand, the row operand its B operand, so a lane holds one
// batch row and four CONSECUTIVE columns per register group -- 16-byte fp32 and 8-byte image stores straight from the accumulators.
// Accumulator (weight row w, batch row m) carries the scale 2^(ew(w, block) + ea(m, block)); it is rescaled (v_ldexp_f32, exact) at the
// borders of the 128-column blocks: the weight part from a table in LDS, the row part from the lane's exponent.
// Launch shape as gru_s3.hip: one workgroup per CU, a column tile (and chunk) per XCD for all row tiles (gru_xcd_tile, gru_internal.hpp),
// operands two stages ahead.  The gate arithmetic is the cell of rnn_cells.hpp; what is about the image format is in h2i_core.hpp.
#include <stdlib.h>

#include <type_traits>

#include "gru_internal.hpp"
#include "h2i_core.hpp"
#include "rnn_cells.hpp"

namespace {

constexpr int MODE_FWD = 0, MODE_BWD = 1;
constexpr int GH_MAX_TB = 48;        // exponent blocks of one reduction: 3H / 128 <= 48, i.e. H <= 2048
constexpr int GH_MAX_PARTS = dtc::GRU_MAX_PARTS;

__host__ __device__ inline long long gh_wimage_bytes(int H, int backward) {
    const long long tiles = backward ? H / 128 : H / 32, K = backward ? 3ll * H : H;
    return tiles * hi_stages(K) * HI_CHUNK + tiles * hi_kblocks(K) * 512;
}

// block = (tile, exponent block); thread = (image row r, k half h): 8 stages x 8 reduction columns, as h2i_pack_kernel
template <int MODE>
__global__ __launch_bounds__(256) void gru_h2i_wimage_kernel(const float* __restrict__ Whh, u32x4* __restrict__ img, int* __restrict__ exps, int H) {
    const int kbs = (MODE == MODE_FWD ? H : 3 * H) / 128, stages = kbs * HI_KB;
    const int tc = blockIdx.x / kbs, kb = blockIdx.x - tc * kbs;
    const int r = threadIdx.x & 127, h = threadIdx.x >> 7;
    float v[HI_KB][8];
    u32 mx = 0u;
#pragma unroll
    for (int s = 0; s < HI_KB; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = (kb * HI_KB + s) * 16 + 8 * h + e;
            float x;
            if (MODE == MODE_FWD) x = r < 96 ? Whh[((long long)(r >> 5) * H + tc * 32 + (r & 31)) * H + k] : 0.f;
            else x = Whh[(long long)k * H + tc * 128 + r];
            v[s][e] = x;
            const u32 b = finite_bits(x);
            mx = b > mx ? b : mx;
        }
    __shared__ u32 rm[2][128];
    rm[h][r] = mx;
    __syncthreads();
    mx = rm[0][r] > rm[1][r] ? rm[0][r] : rm[1][r];
    const int e = hi_exp(mx);
    if (h == 0) exps[(tc * kbs + kb) * 128 + r] = e;
    const int ee = e == HI_EZERO ? 0 : e;
#pragma unroll
    for (int s = 0; s < HI_KB; ++s) {
        const f32x4 q[2] = {f32x4{v[s][0], v[s][1], v[s][2], v[s][3]}, f32x4{v[s][4], v[s][5], v[s][6], v[s][7]}};
        const HiPiece pc = hi_split8(q, ee);
        u32x4* chunk = img + ((long long)tc * stages + kb * HI_KB + s) * (HI_CHUNK / 16);
        chunk[rslot(r, h)] = pc.p[0];
        chunk[256 + rslot(r, h)] = pc.p[1];
    }
}

// one wave per row: the row's exponent for the call, h0 as the image rows of step 0 (and of hp where slot0 names a valid row), h0 as
// hs_all[0]; the exponent tables of both step images (every block of a row carries e_r)
__global__ __launch_bounds__(256) void gru_h2i_h0_kernel(const float* __restrict__ h0, float* __restrict__ hs0, void* img0, void* img1,
                                                         int* __restrict__ erow, const int* __restrict__ slot0, void* hp_img, int M_valid,
                                                         int R, int H) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    const float* src = h0 + (long long)row * H;
    u32 mx = 0u;
    for (int c = lane * 8; c < H; c += 512) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(src + c), b = *reinterpret_cast<const f32x4*>(src + c + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const u32 x = finite_bits(a[e]), y = finite_bits(b[e]);
            mx = x > mx ? x : mx;
            mx = y > mx ? y : mx;
        }
    }
    mx = wave_max_u32(mx);
    int e = hi_exp(mx);
    e = (e == HI_EZERO || e > 14) ? 14 : e;
    const int s = slot0 ? slot0[row] : -1;
    const bool to_hp = hp_img != nullptr && s >= 0 && s < M_valid;
    for (int c = lane * 8; c < H; c += 512) {
        const f32x4 q[2] = {*reinterpret_cast<const f32x4*>(src + c), *reinterpret_cast<const f32x4*>(src + c + 4)};
        *reinterpret_cast<f32x4*>(hs0 + (long long)row * H + c) = q[0];
        *reinterpret_cast<f32x4*>(hs0 + (long long)row * H + c + 4) = q[1];
        const HiPiece pc = hi_split8(q, e);
        hi_store8(img0, H, row, c, pc);
        if (to_hp) hi_store8(hp_img, H, s, c, pc);
    }
    for (int kb = lane; kb < H / 128; kb += 64) {
        hi_store_exp(img0, R, H, row, kb, e);
        hi_store_exp(img1, R, H, row, kb, e);
        if (to_hp) hi_store_exp(hp_img, M_valid, H, s, kb, e);
    }
    if (lane == 0) erow[row] = e;
}

struct GruH2iArgs {
    const u32x4* aimg;          // row operand [R, K]: the image of h_{t-1} (K = H) / dgh_t (K = 3H)
    const int* aexps;
    long long a_bytes;
    int a_stages, a_kbs;        // stages / exponent blocks of one row tile
    const u32x4* wimg;          // W_hh image (gru_h2i_wimage_kernel)
    const int* wexps;
    long long w_bytes;
    int w_stages, w_kbs;        // ... of one column tile
    int R, H;
    int stages;                 // stages of one block's reduction (H / 16 forward; (3H / nparts) / 16 backward)
    int nparts;
    // forward epilogue
    const float* hprev;
    const float* bhh;
    const float* gi;
    float* hout;
    float* gates;
    float* hn;
    void* hout_img;             // image of h_t [R, H] (exponent tables: gru_h2i_h0_kernel), may be NULL
    const int* erow;            // [R]: exponent of the row's h_t in every image
    const int* slot_x;          // [R]: valid row of (t, r) in hx, or -1 (NULL: no hx rows)
    const int* slot_p;          // [R]: valid row of (t + 1, r) in hp, or -1 (NULL: none)
    void* hx_img;
    void* hp_img;
    int M_valid;
    // backward epilogue: chunk c -> part + c * part_stride, [R, H]
    float* part;
    long long part_stride;
};

// stage ring: separate objects per buffer (an LDS-DMA into one cannot alias the fragment reads of another, see linear_s3_kernel)
__shared__ __attribute__((aligned(16))) u32x2 GAs0[2][128 * 4];
__shared__ __attribute__((aligned(16))) u32x2 GAs1[2][128 * 4];
__shared__ __attribute__((aligned(16))) u32x2 GAs2[2][128 * 4];
__shared__ __attribute__((aligned(16))) u32x2 GWs0[2][128 * 4];
__shared__ __attribute__((aligned(16))) u32x2 GWs1[2][128 * 4];
__shared__ __attribute__((aligned(16))) u32x2 GWs2[2][128 * 4];
__shared__ __attribute__((aligned(16))) short GDw[GH_MAX_TB + 1][128];     // weight rows: exponent delta per block border; [blocks]: -(last exponent)

template <int MODE>
__global__ __launch_bounds__(256, 2) void gru_h2i_kernel(const GruH2iArgs a) {
    constexpr int WW = MODE == MODE_FWD ? 1 : 2;             // waves along the weight rows
    constexpr int TB = MODE == MODE_FWD ? 1 : 2;             // 32-row batch tiles per wave
    constexpr int TW = MODE == MODE_FWD ? 3 : 2;             // 32-row weight tiles per wave
#define GAS(b) ((b) == 0 ? GAs0 : (b) == 1 ? GAs1 : GAs2)
#define GWS(b) ((b) == 0 ? GWs0 : (b) == 1 ? GWs1 : GWs2)
    const dtc::GruXcdTile tile = dtc::gru_xcd_tile(blockIdx.x, (a.R + 127) >> 7, MODE == MODE_FWD ? a.H / 32 : a.H / 128, a.nparts);
    if (!tile.valid) return;
    const int tr = tile.tr, tc = tile.tc, chunk = tile.chunk;
    const int m0 = tr * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int wb_off = (wave / WW) * (32 * TB), ww_off = (wave % WW) * (32 * TW);

    const rsrc_t ares = make_rsrc_bytes(a.aimg, a.a_bytes), wres = make_rsrc_bytes(a.wimg, a.w_bytes);
    const int gs0 = chunk * a.stages;                         // first stage of this block's reduction in both images
    u32 achunk = (u32)(tr * a.a_stages + gs0) * (u32)HI_CHUNK, wchunk = (u32)(tc * a.w_stages + gs0) * (u32)HI_CHUNK;
    int left = a.stages;
    const u32 lane_off = (u32)(tid * 16);
    auto load_stage = [&](auto nbc) {                   // next stage -> LDS[nb]; past the last stage: out-of-range lanes, zeros land
        constexpr int nb = decltype(nbc)::value;
        const u32 voff = lane_off | (left > 0 ? 0u : INVALID);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ares, (lds_void*)&GAS(nb)[p][wave * 128], 16, voff, achunk + p * HI_PLANE, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wres, (lds_void*)&GWS(nb)[p][wave * 128], 16, voff, wchunk + p * HI_PLANE, 0, 0);
        }
        achunk += HI_CHUNK;
        wchunk += HI_CHUNK;
        --left;
    };
    load_stage(S0{});
    load_stage(S1{});

    // ---- exponents.  Blocks kb0 .. kb0 + nblk - 1 of the images take part; a block without content (HI_EZERO) inherits its predecessor's
    // exponent (its products are zero whatever the scale).  Weight rows: thread w < 128 walks the blocks of weight row w into GDw.  Batch
    // rows: a lane's rows are fixed (wb_off + 32 i + l31), their exponents come from the image, the next border's one block ahead.
    const int kb0 = gs0 >> 3, nblk = ((gs0 + a.stages - 1) >> 3) - kb0 + 1;
    if (tid < 128) {
        const int* ex = a.wexps + ((long long)tc * a.w_kbs + kb0) * 128 + tid;
        int prev = 0;
        for (int b = 0; b < nblk; ++b) {
            const int e = ex[b * 128], cur = e == HI_EZERO ? prev : e;
            GDw[b][tid] = (short)(cur - prev);
            prev = cur;
        }
        GDw[nblk][tid] = (short)(-prev);
    }
    const int* __restrict__ aex = a.aexps + ((long long)tr * a.a_kbs + kb0) * 128 + wb_off + l31;
    int acur[TB], anext[TB];
#pragma unroll
    for (int i = 0; i < TB; ++i) {
        const int e0 = aex[32 * i];
        acur[i] = e0 == HI_EZERO ? 0 : e0;
        anext[i] = nblk > 1 ? aex[128 + 32 * i] : HI_EZERO;
    }

    f32x16 acc[TB][TW];
#pragma unroll
    for (int i = 0; i < TB; ++i)
#pragma unroll
        for (int j = 0; j < TW; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // weight rows of this lane's accumulator registers: ww_off + 32 j + 8 g + 4 half + e, register 4 g + e
    auto rescale = [&](int b, const int (&da)[TB]) {
#pragma unroll
        for (int j = 0; j < TW; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int2 d = *reinterpret_cast<const int2*>(&GDw[b][ww_off + 32 * j + 8 * g + 4 * half]);      // four int16
                const int dv[4] = {(d.x << 16) >> 16, d.x >> 16, (d.y << 16) >> 16, d.y >> 16};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TB; ++i) acc[i][j][4 * g + e] = __builtin_ldexpf(acc[i][j][4 * g + e], dv[e] + da[i]);
            }
    };

    int done = 0, blk = 0;
    auto stage = [&](auto bc) {
        constexpr int buf = decltype(bc)::value;
        // (uniform) a block border: rows and weight rows change scale
        if (done > 0 && done < a.stages && ((gs0 + done) & (HI_KB - 1)) == 0) {
            ++blk;
            int da[TB];
#pragma unroll
            for (int i = 0; i < TB; ++i) {
                const int e = anext[i] == HI_EZERO ? acur[i] : anext[i];
                da[i] = e - acur[i];
                acur[i] = e;
            }
            if (blk + 1 < nblk) {
#pragma unroll
                for (int i = 0; i < TB; ++i) anext[i] = aex[(blk + 1) * 128 + 32 * i];
            }
            rescale(blk, da);
        }
        __builtin_amdgcn_sched_barrier(0);
        load_stage(std::integral_constant<int, (buf + 2) % 3>{});
        __builtin_amdgcn_sched_barrier(0);
        u32x4 af[TB][2], wf[TW][2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int i = 0; i < TB; ++i) af[i][p] = reinterpret_cast<const u32x4*>(&GAS(buf)[p][0])[rslot(wb_off + 32 * i + l31, half)];
#pragma unroll
            for (int j = 0; j < TW; ++j) wf[j][p] = reinterpret_cast<const u32x4*>(&GWS(buf)[p][0])[rslot(ww_off + 32 * j + l31, half)];
        }
        using P = Prec<true>;
        // smallest terms first (lo hi', hi lo', hi hi'), term by term over the wave's tiles: consecutive MFMAs never share an accumulator
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int j = 0; j < TW; ++j)
#pragma unroll
                for (int i = 0; i < TB; ++i) acc[i][j] = P::mfma(wf[j][t == 0 ? 1 : 0], af[i][t == 1 ? 1 : 0], acc[i][j]);
        __builtin_amdgcn_sched_barrier(0);
        ++done;
        // stage s + 1 has landed (this wave's four newest transfers -- stage s + 2 -- may still be in flight); then every wave's share has
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0x0F70 | 4);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    __syncthreads();
    for (int trip = (a.stages + 2) / 3; trip > 0; --trip) {
        stage(S0{});
        stage(S1{});
        stage(std::integral_constant<int, 2>{});
    }
    __syncthreads();                                     // the transfers past the last stage (zeros) have landed too

    // back to the values themselves: 2^-(last weight exponent + last row exponent)
    {
        int da[TB];
#pragma unroll
        for (int i = 0; i < TB; ++i) da[i] = -acur[i];
        rescale(nblk, da);
    }

    const int R = a.R, H = a.H;
    if constexpr (MODE == MODE_FWD) {
        // gate math of torch.nn.GRU (rnn_cells.hpp); the lane holds the three pre-activations of batch row `row`, units
        // 32 tc + 8 g + 4 half + (0..3)
        const int row = m0 + wb_off + l31;
        if (row < R) {
            const int er = a.erow ? a.erow[row] : 0;
            const int sx = a.slot_x ? a.slot_x[row] : -1, sp = a.slot_p ? a.slot_p[row] : -1;
            const bool to_x = a.hx_img != nullptr && sx >= 0 && sx < a.M_valid, to_p = a.hp_img != nullptr && sp >= 0 && sp < a.M_valid;
            const float* gir = a.gi + (long long)row * 3 * H;
            float* gtr = a.gates + (long long)row * 3 * H;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int u = tc * 32 + 8 * g + 4 * half;
                f32x4 br, bz, bn;                        // (b_hh is a slice of the parameter arena: 4-byte aligned)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    br[e] = a.bhh[u + e];
                    bz[e] = a.bhh[H + u + e];
                    bn[e] = a.bhh[2 * H + u + e];
                }
                const f32x4 gr = *reinterpret_cast<const f32x4*>(gir + u), gz = *reinterpret_cast<const f32x4*>(gir + H + u),
                            gn = *reinterpret_cast<const f32x4*>(gir + 2 * H + u);
                const f32x4 hp = *reinterpret_cast<const f32x4*>(a.hprev + (long long)row * H + u);
                f32x4 rg, zg, ng, ghn, ho;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ghn[e] = acc[0][2][4 * g + e] + bn[e];
                    const dtc::GruCell c = dtc::gru_cell_fwd(gr[e], gz[e], gn[e], acc[0][0][4 * g + e] + br[e], acc[0][1][4 * g + e] + bz[e], ghn[e], hp[e]);
                    rg[e] = c.r;
                    zg[e] = c.z;
                    ng[e] = c.n;
                    ho[e] = c.h;
                }
                *reinterpret_cast<f32x4*>(a.hout + (long long)row * H + u) = ho;
                *reinterpret_cast<f32x4*>(gtr + u) = rg;
                *reinterpret_cast<f32x4*>(gtr + H + u) = zg;
                *reinterpret_cast<f32x4*>(gtr + 2 * H + u) = ng;
                *reinterpret_cast<f32x4*>(a.hn + (long long)row * H + u) = ghn;
                if (a.hout_img) hi_store4(a.hout_img, H, row, u, ho, er);
                if (to_x) hi_store4(a.hx_img, H, sx, u, ho, er);
                if (to_p) hi_store4(a.hp_img, H, sp, u, ho, er);
            }
            if ((tc & 3) == 0 && half == 0) {            // the first lane of the row's 128-column block: its exponent in the valid-row images
                if (to_x) hi_store_exp(a.hx_img, a.M_valid, H, sx, tc >> 2, er);
                if (to_p) hi_store_exp(a.hp_img, a.M_valid, H, sp, tc >> 2, er);
            }
        }
    } else {
        float* P = a.part + (long long)chunk * a.part_stride;
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            const int row = m0 + wb_off + 32 * i + l31;
            if (row >= R) continue;
#pragma unroll
            for (int j = 0; j < TW; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int col = tc * 128 + ww_off + 32 * j + 8 * g + 4 * half;
                    *reinterpret_cast<f32x4*>(P + (long long)row * H + col) =
                        f32x4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                }
        }
    }
#undef GAS
#undef GWS
}

// ---- gate derivatives.  dh (in/out): on entry the direct part (dh_{t+1} * z_{t+1}) of the gradient flowing into h_t from step t + 1;
// `part`: the chunks of its W_hh part (NULL at t = T - 1); on exit dh_t * z.  Thread = (row, four consecutive units); the 32 threads of
// half a wave hold one row's block of 128 units, so the block maxima behind the exponents are half-wave reductions.
struct GateH2iArgs {
    const float* dhs_t;
    float* dh;
    const float* part;
    const float* gates;
    const float* hn;
    const float* hprev;
    float* dgi;
    float* dgh;
    void* step_img;             // dgh_t as image(R, 3H)
    const int* slot;            // [R] valid row of (t, r) or -1; NULL: no valid-row images
    int M_valid;
    void* drz_img;              // [M, 2H] (da_r | da_z)
    void* dnh_img;              // [M, H]  da_n * r
    void* dni_img;              // [M, H]  da_n
    void* dgh_img;              // [M, 3H]
    void* dgi_img;              // [M, 3H]
    int R, H, nparts;
};
__global__ __launch_bounds__(256) void gru_h2i_gate_bwd_kernel(const GateH2iArgs P) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // group of four units
    const int H = P.H, hq = H >> 2;
    if (q >= (long long)P.R * hq) return;                                       // (whole half waves: hq is a multiple of 32)
    const int row = (int)(q / hq);
    const int j = (int)(q - (long long)row * hq) * 4;
    const long long e = (long long)row * H + j;
    const float* g = P.gates + (long long)row * 3 * H;
    const f32x4 r = *reinterpret_cast<const f32x4*>(g + j), z = *reinterpret_cast<const f32x4*>(g + H + j), n = *reinterpret_cast<const f32x4*>(g + 2 * H + j);
    f32x4 d = *reinterpret_cast<const f32x4*>(P.dhs_t + e) + *reinterpret_cast<const f32x4*>(P.dh + e);
    if (P.part) {
        const long long rh = (long long)P.R * H;
        for (int c = 0; c < P.nparts; ++c) d += *reinterpret_cast<const f32x4*>(P.part + c * rh + e);      // fixed order
    }
    const f32x4 ghn = *reinterpret_cast<const f32x4*>(P.hn + e), hp = *reinterpret_cast<const f32x4*>(P.hprev + e);
    f32x4 da_r, da_z, da_n, da_nr, dz4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const dtc::GruCellGrad c = dtc::gru_cell_bwd(d[k], r[k], z[k], n[k], ghn[k], hp[k]);
        da_r[k] = c.da_r;
        da_z[k] = c.da_z;
        da_n[k] = c.da_n;
        da_nr[k] = c.da_nr;
        dz4[k] = c.dh_z;
    }
    float* gi_o = P.dgi + (long long)row * 3 * H;
    float* gh_o = P.dgh + (long long)row * 3 * H;
    *reinterpret_cast<f32x4*>(gi_o + j) = da_r;
    *reinterpret_cast<f32x4*>(gi_o + H + j) = da_z;
    *reinterpret_cast<f32x4*>(gi_o + 2 * H + j) = da_n;
    *reinterpret_cast<f32x4*>(gh_o + j) = da_r;
    *reinterpret_cast<f32x4*>(gh_o + H + j) = da_z;
    *reinterpret_cast<f32x4*>(gh_o + 2 * H + j) = da_nr;
    *reinterpret_cast<f32x4*>(P.dh + e) = dz4;

    // image rows: true exponents per row and block of 128 columns (gradients span many octaves)
    const int e_r = hi_half_wave_exp(hi_max4_bits(da_r)), e_z = hi_half_wave_exp(hi_max4_bits(da_z)), e_n = hi_half_wave_exp(hi_max4_bits(da_n)),
              e_nr = hi_half_wave_exp(hi_max4_bits(da_nr));
    const int kb = j >> 7, hb = H >> 7;
    const bool first = (threadIdx.x & 31) == 0;
    hi_store4(P.step_img, 3 * H, row, j, da_r, e_r);
    hi_store4(P.step_img, 3 * H, row, H + j, da_z, e_z);
    hi_store4(P.step_img, 3 * H, row, 2 * H + j, da_nr, e_nr);
    if (first) {
        hi_store_exp(P.step_img, P.R, 3 * H, row, kb, e_r);
        hi_store_exp(P.step_img, P.R, 3 * H, row, hb + kb, e_z);
        hi_store_exp(P.step_img, P.R, 3 * H, row, 2 * hb + kb, e_nr);
    }
    const int s = P.slot ? P.slot[row] : -1;
    if (s < 0 || s >= P.M_valid) return;
    const long long M = P.M_valid;
    if (P.drz_img) {
        hi_store4(P.drz_img, 2 * H, s, j, da_r, e_r);
        hi_store4(P.drz_img, 2 * H, s, H + j, da_z, e_z);
        if (first) {
            hi_store_exp(P.drz_img, M, 2 * H, s, kb, e_r);
            hi_store_exp(P.drz_img, M, 2 * H, s, hb + kb, e_z);
        }
    }
    if (P.dnh_img) {
        hi_store4(P.dnh_img, H, s, j, da_nr, e_nr);
        if (first) hi_store_exp(P.dnh_img, M, H, s, kb, e_nr);
    }
    if (P.dni_img) {
        hi_store4(P.dni_img, H, s, j, da_n, e_n);
        if (first) hi_store_exp(P.dni_img, M, H, s, kb, e_n);
    }
    if (P.dgh_img) {
        hi_store4(P.dgh_img, 3 * H, s, j, da_r, e_r);
        hi_store4(P.dgh_img, 3 * H, s, H + j, da_z, e_z);
        hi_store4(P.dgh_img, 3 * H, s, 2 * H + j, da_nr, e_nr);
        if (first) {
            hi_store_exp(P.dgh_img, M, 3 * H, s, kb, e_r);
            hi_store_exp(P.dgh_img, M, 3 * H, s, hb + kb, e_z);
            hi_store_exp(P.dgh_img, M, 3 * H, s, 2 * hb + kb, e_nr);
        }
    }
    if (P.dgi_img) {
        hi_store4(P.dgi_img, 3 * H, s, j, da_r, e_r);
        hi_store4(P.dgi_img, 3 * H, s, H + j, da_z, e_z);
        hi_store4(P.dgi_img, 3 * H, s, 2 * H + j, da_n, e_n);
        if (first) {
            hi_store_exp(P.dgi_img, M, 3 * H, s, kb, e_r);
            hi_store_exp(P.dgi_img, M, 3 * H, s, hb + kb, e_z);
            hi_store_exp(P.dgi_img, M, 3 * H, s, 2 * hb + kb, e_n);
        }
    }
}

bool gh_shapes_ok(int R, int H) {
    return R > 0 && H >= 128 && H % 128 == 0 && 3 * H / 128 <= GH_MAX_TB && (long long)R * 3 * H <= MAX_ELEMS && hi_bytes(R, 3 * H) < (1ll << 31);
}
int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// workspace: [ part: 6 R H floats | dgh_all: T R 3H floats | e_r: R ints | image of h, twice (steps t, t + 1) | image of dgh_t | W_hh image ]
struct GhLayout {
    int64_t dgh_all, erow, himg[2], dimg, wimg, total;
};
GhLayout gh_layout(int T, int R, int H) {
    GhLayout L;
    L.dgh_all = (int64_t)GH_MAX_PARTS * R * H * 4;
    L.erow = align256(L.dgh_all + (int64_t)T * R * 3 * H * 4);
    L.himg[0] = align256(L.erow + (int64_t)R * 4);
    L.himg[1] = align256(L.himg[0] + hi_bytes(R, H));
    L.dimg = align256(L.himg[1] + hi_bytes(R, H));
    L.wimg = align256(L.dimg + hi_bytes(R, 3 * H));
    L.total = align256(L.wimg + gh_wimage_bytes(H, 0));       // (the forward image is the larger one)
    return L;
}

int g_h2i_mode = -1;                 // -1: DTC_GRU_H2I decides (default off), 0 / 1: dtc_set_gru_h2i

}  // namespace

extern "C" void dtc_set_gru_h2i(int on) { g_h2i_mode = on < 0 ? -1 : (on != 0); }
extern "C" int dtc_get_gru_h2i(void) {
    static const bool env_on = getenv("DTC_GRU_H2I") && atoi(getenv("DTC_GRU_H2I")) == 1;
    return g_h2i_mode < 0 ? (env_on ? 1 : 0) : g_h2i_mode;
}

extern "C" int64_t dtc_gru_h2i_image_bytes(int H, int backward) {
    if (H <= 0 || H % 128 != 0) return 0;
    return gh_wimage_bytes(H, backward);
}

extern "C" int dtc_gru_h2i_image(const float* W_hh, void* img, int H, int backward, void* stream) {
    DTC_REQUIRE(W_hh && img && dtc::aligned16(img) && gh_shapes_ok(1, H), "bad arguments (H = %d must be a multiple of 128, at most 2048)", H);
    hipStream_t s = (hipStream_t)stream;
    dtc::ProfScope prof("gru_h2i_wimage", 0.0, s, 24.0 * H * (double)H);
    if (backward) {
        int* exps = (int*)((char*)img + (int64_t)(H / 128) * hi_stages(3 * H) * HI_CHUNK);
        hipLaunchKernelGGL(gru_h2i_wimage_kernel<MODE_BWD>, dim3((unsigned)((H / 128) * (3 * H / 128))), dim3(256), 0, s, W_hh, (u32x4*)img, exps, H);
    } else {
        int* exps = (int*)((char*)img + (int64_t)(H / 32) * hi_stages(H) * HI_CHUNK);
        hipLaunchKernelGGL(gru_h2i_wimage_kernel<MODE_FWD>, dim3((unsigned)((H / 32) * (H / 128))), dim3(256), 0, s, W_hh, (u32x4*)img, exps, H);
    }
    return dtc::check_launch("gru_h2i_image");
}

namespace {
void operand_of(GruH2iArgs& a, const void* aimg, const void* wimg, int R, int H, int backward) {
    const int K = backward ? 3 * H : H;
    a.aimg = (const u32x4*)aimg;
    a.a_bytes = hi_data_bytes(R, K);
    a.aexps = (const int*)((const char*)aimg + a.a_bytes);
    a.a_stages = (int)hi_stages(K);
    a.a_kbs = (int)hi_kblocks(K);
    const int64_t tiles = backward ? H / 128 : H / 32;
    a.wimg = (const u32x4*)wimg;
    a.w_bytes = tiles * hi_stages(K) * HI_CHUNK;
    a.wexps = (const int*)((const char*)wimg + a.w_bytes);
    a.w_stages = a.a_stages;
    a.w_kbs = a.a_kbs;
    a.R = R;
    a.H = H;
}
}  // namespace

// one forward time step.  hprev_img: image(R, H) of h_{t-1} whose rows carry ONE exponent each (row_exp[r], in every block); hout_img (may
// be NULL): image(R, H) that receives h_t with the same exponents -- its exponent table is the caller's (dtc_gru_fwd_h2i writes both tables
// before step 0)
extern "C" int dtc_gru_step_fwd_h2i(const void* hprev_img, const float* hprev, const void* wimg, const float* b_hh, const float* gi_t,
                                    float* hout, float* gates_t, float* hn_t, void* hout_img, const int32_t* row_exp, const int32_t* slot_x,
                                    const int32_t* slot_p, int M_valid, void* hx_img, void* hp_img, int R, int H, void* stream) {
    DTC_REQUIRE(gh_shapes_ok(R, H), "bad shape R=%d H=%d (H must be a multiple of 128, at most 2048)", R, H);
    DTC_REQUIRE(hprev_img && hprev && wimg && b_hh && gi_t && hout && gates_t && hn_t, "null pointer");
    DTC_REQUIRE(row_exp || !(hout_img || hx_img || hp_img), "image outputs need row_exp");
    DTC_REQUIRE((!hx_img || slot_x) && (!hp_img || slot_p) && M_valid >= 0, "valid-row images need their slot maps");
    DTC_REQUIRE(dtc::aligned16(hprev_img) && dtc::aligned16(wimg) && dtc::aligned16(hprev) && dtc::aligned16(gi_t) &&
                    dtc::aligned16(hout) && dtc::aligned16(gates_t) && dtc::aligned16(hn_t),
                "images, hprev, gi_t and the outputs must be 16-byte aligned");
    GruH2iArgs a{};
    operand_of(a, hprev_img, wimg, R, H, 0);
    a.stages = H / 16;
    a.nparts = 1;
    a.hprev = hprev;
    a.bhh = b_hh;
    a.gi = gi_t;
    a.hout = hout;
    a.gates = gates_t;
    a.hn = hn_t;
    a.hout_img = hout_img;
    a.erow = row_exp;
    a.slot_x = hx_img ? slot_x : nullptr;
    a.slot_p = hp_img ? slot_p : nullptr;
    a.hx_img = hx_img;
    a.hp_img = hp_img;
    a.M_valid = M_valid;
    hipStream_t s = (hipStream_t)stream;
    dtc::ProfScope prof(dtc::prof_shape_name("gru_step_fwd_h2i", R, 3 * H, H), 2.0 * R * 3.0 * H * H, s);
    hipLaunchKernelGGL(gru_h2i_kernel<MODE_FWD>, dim3(dtc::gru_xcd_grid((int)dtc::ceil_div(R, 128), H / 32, 1)), dim3(256), 0, s, a);
    return dtc::check_launch("gru_step_fwd_h2i");
}

// the `nparts` chunks of dgh_t [R, 3H] W_hh [3H, H] side by side from the image of dgh_t: chunk c -> part + c * part_stride ([R, H]);
// (3H / nparts) must be a multiple of 16
extern "C" int dtc_gru_dgrad_parts_h2i(const void* dgh_img, const void* wimg, float* part, int64_t part_stride, int R, int H, int nparts,
                                       void* stream) {
    DTC_REQUIRE(gh_shapes_ok(R, H) && nparts >= 1 && nparts <= GH_MAX_PARTS && (3 * H) % nparts == 0 && (3 * H / nparts) % 16 == 0,
                "bad shape R=%d H=%d nparts=%d", R, H, nparts);
    DTC_REQUIRE(dgh_img && wimg && part && part_stride >= (int64_t)R * H, "null pointer / overlapping chunks");
    DTC_REQUIRE(dtc::aligned16(dgh_img) && dtc::aligned16(wimg) && dtc::aligned16(part) && part_stride % 4 == 0, "operands must be 16-byte aligned");
    GruH2iArgs a{};
    operand_of(a, dgh_img, wimg, R, H, 1);
    a.stages = 3 * H / nparts / 16;
    a.nparts = nparts;
    a.part = part;
    a.part_stride = part_stride;
    hipStream_t s = (hipStream_t)stream;
    dtc::ProfScope prof(dtc::prof_shape_name("gru_dgrad_h2i", R, 3 * H, H), 2.0 * R * 3.0 * H * H, s);
    hipLaunchKernelGGL(gru_h2i_kernel<MODE_BWD>, dim3(dtc::gru_xcd_grid((int)dtc::ceil_div(R, 128), H / 128, nparts)), dim3(256), 0, s, a);
    return dtc::check_launch("gru_dgrad_parts_h2i");
}

extern "C" int64_t dtc_gru_h2i_workspace(int T, int R, int H) {
    if (T <= 0 || !gh_shapes_ok(R, H)) return 0;
    return gh_layout(T, R, H).total;
}
extern "C" int64_t dtc_gru_h2i_dgh_offset(int T, int R, int H) {
    if (T <= 0 || !gh_shapes_ok(R, H)) return -1;
    return gh_layout(T, R, H).dgh_all;
}
extern "C" int dtc_gru_fwd_h2i(const float* gi, const float* h0, const float* W_hh, const float* b_hh, float* hs_all, float* gates, float* hn,
                               void* workspace, const int32_t* slot_row, int M_valid, void* hx_img, void* hp_img, int T, int R, int H,
                               void* stream) {
    DTC_REQUIRE(T > 0 && gh_shapes_ok(R, H), "bad shape T=%d R=%d H=%d (H must be a multiple of 128, at most 2048)", T, R, H);
    DTC_REQUIRE(gi && h0 && W_hh && b_hh && hs_all && gates && hn && workspace, "null pointer");
    DTC_REQUIRE(slot_row || !(hx_img || hp_img), "valid-row images need slot_row");
    DTC_REQUIRE(dtc::aligned16(h0) && dtc::aligned16(hs_all) && ((uintptr_t)workspace & 255) == 0, "h0 / hs_all 16-byte, workspace 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const GhLayout L = gh_layout(T, R, H);
    char* ws = (char*)workspace;
    void* himg[2] = {ws + L.himg[0], ws + L.himg[1]};
    int* erow = (int*)(ws + L.erow);
    void* wimg = ws + L.wimg;
    int rc = dtc_gru_h2i_image(W_hh, wimg, H, 0, stream);
    if (rc != DTC_OK) return rc;
    if (!slot_row) hx_img = hp_img = nullptr;
    hipLaunchKernelGGL(gru_h2i_h0_kernel, dim3((unsigned)dtc::ceil_div(R, 4)), dim3(256), 0, s, h0, hs_all, himg[0], himg[1], erow, slot_row, hp_img,
                       M_valid, R, H);
    const size_t RH = (size_t)R * H, R3H = 3 * RH;
    for (int t = 0; t < T; ++t) {
        rc = dtc_gru_step_fwd_h2i(himg[t & 1], hs_all + t * RH, wimg, b_hh, gi + t * R3H, hs_all + (t + 1) * RH, gates + t * R3H, hn + t * RH,
                                  himg[(t + 1) & 1], erow, slot_row ? slot_row + (size_t)t * R : nullptr,
                                  slot_row && t + 1 < T ? slot_row + (size_t)(t + 1) * R : nullptr, M_valid, hx_img, t + 1 < T ? hp_img : nullptr, R, H,
                                  stream);
        if (rc != DTC_OK) return rc;
    }
    return dtc::check_launch("gru_fwd_h2i");
}

extern "C" int dtc_gru_bwd_h2i(const float* dhs, const float* hs_all, const float* gates, const float* hn, const float* W_hh, float* dgi,
                               float* dh0, void* workspace, const int32_t* slot_row, int M_valid, void* drz_img, void* dnh_img, void* dni_img,
                               void* dgh_img, void* dgi_img, int T, int R, int H, void* stream) {
    DTC_REQUIRE(T > 0 && gh_shapes_ok(R, H), "bad shape T=%d R=%d H=%d (H must be a multiple of 128, at most 2048)", T, R, H);
    DTC_REQUIRE(dhs && hs_all && gates && hn && W_hh && dgi && dh0 && workspace, "null pointer");
    DTC_REQUIRE(slot_row || !(drz_img || dnh_img || dni_img || dgh_img || dgi_img), "valid-row images need slot_row");
    DTC_REQUIRE(dtc::aligned16(dhs) && dtc::aligned16(hs_all) && dtc::aligned16(gates) && dtc::aligned16(hn) && dtc::aligned16(dgi) && dtc::aligned16(dh0) &&
                    ((uintptr_t)workspace & 255) == 0,
                "operands 16-byte, workspace 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const GhLayout L = gh_layout(T, R, H);
    char* ws = (char*)workspace;
    float* part = (float*)ws;
    float* dgh_all = (float*)(ws + L.dgh_all);
    void* dimg = ws + L.dimg;
    void* wimg = ws + L.wimg;
    const size_t RH = (size_t)R * H, R3H = 3 * RH;
    const int nparts = dtc::gru_parts(H, true);
    int rc = dtc_gru_h2i_image(W_hh, wimg, H, 1, stream);
    if (rc != DTC_OK) return rc;
    if (hipMemsetAsync(dh0, 0, RH * sizeof(float), s) != hipSuccess) {
        dtc::set_error("gru_bwd_h2i: memset failed");
        return DTC_ERR_LAUNCH;
    }
    const unsigned grid4 = (unsigned)dtc::ceil_div((int64_t)RH / 4, 256);
    for (int t = T - 1; t >= 0; --t) {
        {
            dtc::ProfScope prof("gru_gate_bwd_h2i", (double)RH * 4.0 * 17, s);
            GateH2iArgs g{};
            g.dhs_t = dhs + t * RH;
            g.dh = dh0;
            g.part = t == T - 1 ? nullptr : part;
            g.gates = gates + t * R3H;
            g.hn = hn + t * RH;
            g.hprev = hs_all + t * RH;
            g.dgi = dgi + t * R3H;
            g.dgh = dgh_all + t * R3H;
            g.step_img = dimg;
            g.slot = slot_row ? slot_row + (size_t)t * R : nullptr;
            g.M_valid = M_valid;
            g.drz_img = drz_img;
            g.dnh_img = dnh_img;
            g.dni_img = dni_img;
            g.dgh_img = dgh_img;
            g.dgi_img = dgi_img;
            g.R = R;
            g.H = H;
            g.nparts = nparts;
            hipLaunchKernelGGL(gru_h2i_gate_bwd_kernel, dim3(grid4), dim3(256), 0, s, g);
        }
        rc = dtc_gru_dgrad_parts_h2i(dimg, wimg, part, (int64_t)RH, R, H, nparts, stream);
        if (rc != DTC_OK) return rc;
    }
    dtc::gru_add_parts(dh0, part, (int64_t)RH, nparts, s);
    return dtc::check_launch("gru_bwd_h2i");
}
