// GRU recurrence (forward + BPTT) for gfx950, built on the fp32 MFMA GEMMs of gemm.hip.
//
// Reference: torch.nn.GRU(input, hidden=512, 1 layer) inside `Memory`
// (rsl_rl/rsl_rl/modules/actor_critic_recurrent.py:92-116, twin at actor_critic_decoder.py:584-614), run over
// padded trajectories [T, n_traj, .] with saved initial hidden states during the policy update (BPTT) and
// over [1, N, .] during the rollout.
//
// The gate arithmetic of every kernel here and in the other recurrence sources is the cell of rnn_cells.hpp.
//
// Structure (all launches are issued from this C++ loop -- no Python between time steps):
//   forward  t = 0..T-1 : gh = h_{t-1} W_hh^T + b_hh and the gate math in its epilogue: ONE kernel per step
//                         (dtc_gru_step_fwd in gemm.hip; saves r,z,n and gh_n; DTC_GRU_UNFUSED=1 selects the older
//                         dtc_linear_fwd + gru_gate_fwd_kernel pair)
//   backward t = T-1..0 : gate derivatives                  (gru_gate_bwd_kernel: dgi_t, dgh_t, dh*z)
//                         dh_{t-1} += dgh_t W_hh            (dtc_linear_dgrad_split: the 3H-long reduction runs as three
//                                                            H-long chunks side by side -- one step has only ~12 row
//                                                            tiles -- and the next gate kernel adds the three partial
//                                                            products in a fixed order)
//            after loop : dW_hh, db_hh = [dgh_0..dgh_{T-1}]^T [h_{-1}..h_{T-2}]   (ONE dtc_linear_wgrad over T*R rows)
// The input projection gi = x W_ih^T + b_ih (all T*R rows at once) and its weight gradient are plain
// dtc_linear_fwd / dtc_linear_wgrad calls made by the caller.  Padded steps need no masks: their output
// gradients are zero, so every quantity flowing backwards through them is zero as well.
#include <stdlib.h>

#include "gru_internal.hpp"
#include "rnn_cells.hpp"

namespace {

// one thread per (row, hidden unit)
__global__ __launch_bounds__(256) void gru_gate_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ gh,
                                                           const float* __restrict__ hprev, float* __restrict__ hout,
                                                           float* __restrict__ gates, float* __restrict__ hn, int R,
                                                           int H) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)R * H) return;
    const long long row = e / H;
    const int j = (int)(e - row * H);
    const float* gir = gi + row * 3 * H;
    const float* ghr = gh + row * 3 * H;
    const float ghn = ghr[2 * H + j];
    const dtc::GruCell c = dtc::gru_cell_fwd(gir[j], gir[H + j], gir[2 * H + j], ghr[j], ghr[H + j], ghn, hprev[e]);
    hout[e] = c.h;
    float* g = gates + row * 3 * H;
    g[j] = c.r;
    g[H + j] = c.z;
    g[2 * H + j] = c.n;
    hn[e] = ghn;
}

// dh (in/out): on entry the direct part (dh_{t+1} * z_{t+1}) of the gradient flowing into h_t from step t+1 (zero at
// t = T-1); `part` holds the three chunks of its W_hh part (dgh_{t+1} W_hh, NULL at t = T-1); dhs_t is added here.
// On exit dh holds dh_t * z (the direct path to h_{t-1}); the W_hh path is produced by the following split dgrad.
__global__ __launch_bounds__(256) void gru_gate_bwd_kernel(const float* __restrict__ dhs_t, float* __restrict__ dh,
                                                           const float* __restrict__ part, const float* __restrict__ gates,
                                                           const float* __restrict__ hn, const float* __restrict__ hprev,
                                                           float* __restrict__ dgi, float* __restrict__ dgh, int R, int H, int nparts) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)R * H) return;
    const long long row = e / H;
    const int j = (int)(e - row * H);
    const float* g = gates + row * 3 * H;
    float d = dhs_t[e] + dh[e];
    if (part) {
        const long long rh = (long long)R * H;
        for (int c = 0; c < nparts; ++c) d += part[c * rh + e];              // fixed order
    }
    const dtc::GruCellGrad c = dtc::gru_cell_bwd(d, g[j], g[H + j], g[2 * H + j], hn[e], hprev[e]);
    float* gi_o = dgi + row * 3 * H;
    float* gh_o = dgh + row * 3 * H;
    gi_o[j] = c.da_r;
    gi_o[H + j] = c.da_z;
    gi_o[2 * H + j] = c.da_n;
    gh_o[j] = c.da_r;
    gh_o[H + j] = c.da_z;
    gh_o[2 * H + j] = c.da_nr;
    dh[e] = c.dh_z;
}

// the same with four consecutive hidden units per thread (H % 4 == 0, 16-byte aligned rows): 16-byte loads / stores -- the kernel moves
// 20 floats per (row, unit) and is bound by that traffic (66 MB per launch at R ~ 1470, H = 512)
// (blockIdx.y: which recurrence -- dtc_gru_bwd_multi runs the time step of two recurrences of one shape as one launch)
struct GateBwdPtrs {
    const float* dhs_t;
    float* dh;
    const float* part;
    const float* gates;
    const float* hn;
    const float* hprev;
    float* dgi;
    float* dgh;
};
__global__ __launch_bounds__(256) void gru_gate_bwd4_kernel(const GateBwdPtrs p0, const GateBwdPtrs p1, int R, int H, int nparts) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const GateBwdPtrs P = blockIdx.y == 0 ? p0 : p1;
    const float* __restrict__ dhs_t = P.dhs_t;
    float* __restrict__ dh = P.dh;
    const float* __restrict__ part = P.part;
    const float* __restrict__ gates = P.gates;
    const float* __restrict__ hn = P.hn;
    const float* __restrict__ hprev = P.hprev;
    float* __restrict__ dgi = P.dgi;
    float* __restrict__ dgh = P.dgh;
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // group of four units
    const int hq = H >> 2;
    if (q >= (long long)R * hq) return;
    const long long row = q / hq;
    const int j = (int)(q - row * hq) * 4;
    const long long e = row * H + j;
    const float* g = gates + row * 3 * H;
    const f4 r = *reinterpret_cast<const f4*>(g + j), z = *reinterpret_cast<const f4*>(g + H + j), n = *reinterpret_cast<const f4*>(g + 2 * H + j);
    f4 d = *reinterpret_cast<const f4*>(dhs_t + e) + *reinterpret_cast<const f4*>(dh + e);
    if (part) {
        const long long rh = (long long)R * H;
        for (int c = 0; c < nparts; ++c) d += *reinterpret_cast<const f4*>(part + c * rh + e);      // fixed order
    }
    const f4 ghn = *reinterpret_cast<const f4*>(hn + e), hp = *reinterpret_cast<const f4*>(hprev + e);
    f4 da_r, da_z, da_n, da_nr, dz4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const dtc::GruCellGrad c = dtc::gru_cell_bwd(d[k], r[k], z[k], n[k], ghn[k], hp[k]);
        da_r[k] = c.da_r;
        da_z[k] = c.da_z;
        da_n[k] = c.da_n;
        da_nr[k] = c.da_nr;
        dz4[k] = c.dh_z;
    }
    float* gi_o = dgi + row * 3 * H;
    float* gh_o = dgh + row * 3 * H;
    *reinterpret_cast<f4*>(gi_o + j) = da_r;
    *reinterpret_cast<f4*>(gi_o + H + j) = da_z;
    *reinterpret_cast<f4*>(gi_o + 2 * H + j) = da_n;
    *reinterpret_cast<f4*>(gh_o + j) = da_r;
    *reinterpret_cast<f4*>(gh_o + H + j) = da_z;
    *reinterpret_cast<f4*>(gh_o + 2 * H + j) = da_nr;
    *reinterpret_cast<f4*>(dh + e) = dz4;
}

// dh0 <- dh0 + the chunks of the last W_hh product
__global__ __launch_bounds__(256) void gru_add_parts_kernel(float* __restrict__ dh, const float* __restrict__ part, long long rh, int nparts) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rh) return;
    float d = dh[e];
    for (int c = 0; c < nparts; ++c) d += part[c * rh + e];
    dh[e] = d;
}

}  // namespace

// The dtc_gru_workspace() buffer, as byte offsets from its start -- the only statement of the layout:
//   part     : gh of the GEMM + gate-kernel forward step / the chunks of the W_hh data gradient, GRU_MAX_PARTS * R * H floats
//   dgh_all  : [T, R, 3H] floats (dtc_gru_dgh_offset: the trainers read it there)
//   wgrad_ws : partial sums of the W_hh weight gradient, on a 16-byte boundary
//   wimage   : the image of W_hh / W_hh^T of the split-precision steps (csrc/gru_s3.hip), on a 16-byte boundary
//   seq      : the persistent kernels' exchange buffers (csrc/gru_seq.hip), on a 256-byte boundary
// wgrad_ws and wimage are aligned as ADDRESSES: a `workspace` that itself starts off a 16-byte boundary shifts them inside the
// 16 spare bytes that `total` counts (workspace == NULL: the offsets inside an aligned buffer).
namespace {
using dtc::GRU_MAX_PARTS;
using dtc::gru_parts;
using dtc::plain;

struct GruLayout {
    int64_t part, dgh_all, wgrad_ws, wimage, seq, total;
};
GruLayout gru_layout(int T, int R, int H, const void* workspace = nullptr) {
    const int64_t off = (int64_t)((uintptr_t)workspace & 15), wgrad = (dtc_linear_wgrad_workspace(T * R, 3 * H, H) + 15) & ~(int64_t)15;
    const int64_t img = dtc_s3_planes_bytes(H, 3 * H) > dtc_gru_s3_image_bytes(H) ? dtc_s3_planes_bytes(H, 3 * H) : dtc_gru_s3_image_bytes(H);
    GruLayout L;
    L.part = 0;
    L.dgh_all = (int64_t)GRU_MAX_PARTS * R * H * sizeof(float);
    const int64_t end = L.dgh_all + (int64_t)T * R * 3 * H * sizeof(float);
    L.wgrad_ws = ((off + end + 15) & ~(int64_t)15) - off;
    L.wimage = L.wgrad_ws + wgrad;
    L.seq = (end + 16 + wgrad + img + 255) & ~(int64_t)255;
    L.total = L.seq + dtc_gru_seq_workspace(R, H);
    return L;
}

// the environment's switches, each read once (at the first call that asks)
struct GruSwitches {
    static bool zero(const char* name) { return getenv(name) && atoi(getenv(name)) == 0; }
    const bool unfused = getenv("DTC_GRU_UNFUSED") != nullptr;        // set: two-kernel forward step (GEMM + gate kernel)
    const bool gate_vec = !zero("DTC_GRU_GATE_VEC");                  // 0: one hidden unit per thread in the gate backward
    const bool multi = !zero("DTC_GRU_MULTI");                        // 0: the *_multi calls never advance two recurrences together
    const bool s3 = !zero("DTC_S3_WIMG") && !zero("DTC_GRU_S3");      // 0 (either): no split-precision time steps
};
const GruSwitches& switches() {
    static const GruSwitches sw;
    return sw;
}
bool gru_s3(int H) { return dtc_get_gemm_split() && switches().s3 && H % 128 == 0; }
}  // namespace

extern "C" int64_t dtc_gru_workspace(int T, int R, int H) {
    if (T <= 0 || R <= 0 || H <= 0) return 0;
    return gru_layout(T, R, H).total;
}

// byte offset of dgh_all [T, R, 3H] (the gradient w.r.t. the recurrent pre-activations, written by dtc_gru_bwd) inside the workspace
extern "C" int64_t dtc_gru_dgh_offset(int T, int R, int H) {
    if (R <= 0 || H <= 0) return -1;
    return gru_layout(T, R, H).dgh_all;
}

// ---- the two drivers: `count` recurrences of ONE shape, one launch per time step for all of them (count == 2: the actor's and the
// critic's GRU of ActorCriticRecurrent / ActorCriticDecoderRecurrent: rsl_rl/rsl_rl/modules/actor_critic_recurrent.py:45-46, 92-116).
// A time step of one recurrence is a latency-bound launch of ~190-290 workgroups; two of them on two streams overlap by ~20 %
// (tools/gru_pair_probe.py: 1.12 ms for two forward passes against 0.72 for one).  The same two as ONE launch: 1.09 ms -- a launch with
// twice the workgroups takes 1.5 x as long, and in the trainers the merged chain is slower than two chains on two lanes (DESIGN.md
// 4.3c): an option, not the default.  Results are bit-identical to the single calls (same kernels, same tiles).  Only the split-path
// step kernels (and the persistent kernel) take two recurrences: where the shape or a switch rules them out, two recurrences run as
// the single calls, one after the other.  `who`: the public entry point, for its error messages (which name an item only where the caller
// passed several).
namespace {
int null_pointer(int i, int count) {
    count == 1 ? dtc::set_error("null pointer") : dtc::set_error("item %d: null pointer", i);
    return DTC_ERR_ARG;
}
int gru_fwd_run(const char* who, const DtcGruFwdItem* items, int count, int T, int R, int H, void* stream) {
    DTC_REQUIRE(T > 0 && R > 0 && H > 0, "bad shape T=%d R=%d H=%d", T, R, H);
    const GruSwitches& sw = switches();
    hipStream_t s = (hipStream_t)stream;
    const size_t RH = (size_t)R * H, R3H = (size_t)R * 3 * H;
    bool a16 = true;
    GruLayout L[DTC_GRU_MULTI_MAX];
    for (int i = 0; i < count; ++i) {
        const DtcGruFwdItem& it = items[i];
        if (!(it.gi && it.h0 && it.W_hh && it.b_hh && it.hs_all && it.gates && it.hn && it.workspace)) return null_pointer(i, count);
        L[i] = gru_layout(T, R, H, it.workspace);
        a16 = a16 && dtc::aligned16(it.gi) && dtc::aligned16(it.h0) && dtc::aligned16(it.hs_all) && dtc::aligned16(it.gates) &&
              dtc::aligned16(it.hn) && dtc::aligned16(it.workspace);
    }
    // the whole recurrence as ONE persistent launch (csrc/gru_seq.hip) where the shape is served and the buffers allow 16-byte accesses;
    // two recurrences one after the other inside it -- it may then take every CU
    if (!sw.unfused && dtc_get_gemm_split() && dtc_gru_seq_supported(T, R, H, count == 2) && a16) {
        const DtcGruFwdItem &x = items[0], &y = items[count - 1];
        void* const seq[2] = {(char*)x.workspace + L[0].seq, (char*)y.workspace + L[count - 1].seq};
        if (count == 1) return dtc_gru_seq_fwd(x.gi, x.h0, x.W_hh, x.b_hh, x.hs_all, x.gates, x.hn, seq[0], T, R, H, stream);
        const float *gi[2] = {x.gi, y.gi}, *h0[2] = {x.h0, y.h0}, *W[2] = {x.W_hh, y.W_hh}, *b[2] = {x.b_hh, y.b_hh};
        float *hs[2] = {x.hs_all, y.hs_all}, *gt[2] = {x.gates, y.gates}, *hn[2] = {x.hn, y.hn};
        return dtc_gru_seq_fwd_pair(gi, h0, W, b, hs, gt, hn, seq, T, R, H, stream);
    }
    // split-precision steps (csrc/gru_s3.hip) for the passes of the update (T time steps share ONE image of W_hh); the one-step
    // calls of the rollout keep the single-pass kernel
    const bool s3 = !sw.unfused && T >= 4 && gru_s3(H);
    if (count == 2 && !(sw.multi && s3)) {
        for (int i = 0; i < count; ++i) {
            const DtcGruFwdItem& it = items[i];
            int rc = dtc_gru_fwd(it.gi, it.h0, it.W_hh, it.b_hh, it.hs_all, it.gates, it.hn, it.workspace, T, R, H, stream);
            if (rc != DTC_OK) return rc;
        }
        return DTC_OK;
    }
    DTC_REQUIRE(count == 1 || s3, "%s: %d recurrences without the split-path step", who, count);        // (the steps below take items[0])
    const void* img[DTC_GRU_MULTI_MAX] = {};
    for (int i = 0; i < count; ++i) {
        const DtcGruFwdItem& it = items[i];
        if (hipMemcpyAsync(it.hs_all, it.h0, RH * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
            dtc::set_error("%s: h0 copy failed", who);
            return DTC_ERR_LAUNCH;
        }
        if (!s3) continue;
        void* im = (char*)it.workspace + L[i].wimage;
        img[i] = im;
        int rc = dtc_gru_s3_image(it.W_hh, im, H, 0, stream);
        if (rc != DTC_OK) return rc;
    }
    const DtcGruFwdItem& one = items[0];             // without the split-path step there is one recurrence here
    float* gh = (float*)((char*)one.workspace + L[0].part);
    for (int t = 0; t < T; ++t) {
        if (s3) {
            dtc::GruStepFwd st[DTC_GRU_MULTI_MAX];
            for (int i = 0; i < count; ++i) {
                const DtcGruFwdItem& it = items[i];
                st[i] = dtc::GruStepFwd{it.hs_all + t * RH, img[i], it.b_hh, it.gi + t * R3H, it.hs_all + (t + 1) * RH, it.gates + t * R3H, it.hn + t * RH};
            }
            int rc = dtc::gru_s3_step_fwd(st, count, R, H, stream);
            if (rc != DTC_OK) return rc;
            continue;
        }
        const float* hprev = one.hs_all + t * RH;
        if (!sw.unfused && H % 32 == 0) {
            int rc = dtc_gru_step_fwd(hprev, one.W_hh, one.b_hh, one.gi + t * R3H, one.hs_all + (t + 1) * RH, one.gates + t * R3H, one.hn + t * RH, R, H, stream);
            if (rc != DTC_OK) return rc;
            continue;
        }
        const DtcSegMat X = plain(hprev, H, H, R);
        int rc = dtc_linear_fwd(&X, one.W_hh, one.b_hh, gh, 3 * H, R, 3 * H, H, DTC_ACT_NONE, stream);
        if (rc != DTC_OK) return rc;
        dtc::ProfScope prof("gru_gate_fwd", (double)RH * 4.0 * 12, s);
        hipLaunchKernelGGL(gru_gate_fwd_kernel, dim3((unsigned)dtc::ceil_div((int64_t)RH, 256)), dim3(256), 0, s, one.gi + t * R3H, gh, hprev,
                           one.hs_all + (t + 1) * RH, one.gates + t * R3H, one.hn + t * RH, R, H);
    }
    return dtc::check_launch(who);
}

// BPTT: dgi, dh0 and dgh_all (at the layout's offset) of every item; `wg` (one recurrence only, may be NULL): its W_hh weight gradient
struct GruWgrad {
    float *dW_hh, *db_hh;
    const int64_t* valid_rows;
    int n_valid;
};
int gru_bwd_run(const char* who, const DtcGruBwdItem* items, int count, const GruWgrad* wg, int T, int R, int H, void* stream) {
    DTC_REQUIRE(T > 0 && R > 0 && H > 0, "bad shape T=%d R=%d H=%d", T, R, H);
    const GruSwitches& sw = switches();
    hipStream_t s = (hipStream_t)stream;
    const size_t RH = (size_t)R * H, R3H = (size_t)R * 3 * H;
    const bool s3 = gru_s3(H);
    const int nparts = gru_parts(H, s3);
    // four units per thread when every row of every operand starts on a 16-byte boundary
    bool vec4 = sw.gate_vec && H % 4 == 0;
    float *part[DTC_GRU_MULTI_MAX], *dgh_all[DTC_GRU_MULTI_MAX];
    void *wimage[DTC_GRU_MULTI_MAX], *wgrad_ws = nullptr;
    for (int i = 0; i < count; ++i) {
        const DtcGruBwdItem& it = items[i];
        if (!(it.dhs && it.hs_all && it.gates && it.hn && it.W_hh && it.dgi && it.dh0 && it.workspace)) return null_pointer(i, count);
        const GruLayout L = gru_layout(T, R, H, it.workspace);
        wgrad_ws = (char*)it.workspace + L.wgrad_ws;
        part[i] = (float*)((char*)it.workspace + L.part);              // [nparts][R][H]: the region the forward pass uses for gh
        dgh_all[i] = (float*)((char*)it.workspace + L.dgh_all);
        wimage[i] = (char*)it.workspace + L.wimage;
        vec4 = vec4 && dtc::aligned16(it.dhs) && dtc::aligned16(it.dh0) && dtc::aligned16(part[i]) && dtc::aligned16(it.gates) &&
               dtc::aligned16(it.hn) && dtc::aligned16(it.hs_all) && dtc::aligned16(it.dgi) && dtc::aligned16(dgh_all[i]);
    }
    DTC_REQUIRE(!wg || (wg->dW_hh == nullptr) == (wg->db_hh == nullptr), "dW_hh and db_hh: both or neither");
    if (count == 2 && !(sw.multi && s3 && vec4)) {
        for (int i = 0; i < count; ++i) {
            const DtcGruBwdItem& it = items[i];
            int rc = dtc_gru_bwd(it.dhs, it.hs_all, it.gates, it.hn, it.W_hh, it.dgi, nullptr, nullptr, it.dh0, it.workspace, nullptr, 0, T, R, H, stream);
            if (rc != DTC_OK) return rc;
        }
        return DTC_OK;
    }
    DTC_REQUIRE(count == 1 || (s3 && vec4), "%s: %d recurrences without the split-path step", who, count);   // (the steps below take items[0])
    for (int i = 0; i < count; ++i) {
        if (s3) {               // split path: ONE image of W_hh^T serves all T steps
            int rc = dtc_gru_s3_image(items[i].W_hh, wimage[i], H, 1, stream);
            if (rc != DTC_OK) return rc;
        }
        if (hipMemsetAsync(items[i].dh0, 0, RH * sizeof(float), s) != hipSuccess) {
            dtc::set_error("%s: memset failed", who);
            return DTC_ERR_LAUNCH;
        }
    }
    const unsigned grid = (unsigned)dtc::ceil_div((int64_t)RH, 256), grid4 = (unsigned)dtc::ceil_div((int64_t)RH / 4, 256);
    for (int t = T - 1; t >= 0; --t) {
        GateBwdPtrs gp[DTC_GRU_MULTI_MAX];
        dtc::GruDgradParts dp[DTC_GRU_MULTI_MAX];
        for (int i = 0; i < count; ++i) {
            const DtcGruBwdItem& it = items[i];
            gp[i] = GateBwdPtrs{it.dhs + t * RH, it.dh0, t == T - 1 ? nullptr : part[i], it.gates + t * R3H,
                                it.hn + t * RH, it.hs_all + t * RH, it.dgi + t * R3H, dgh_all[i] + t * R3H};
            dp[i] = dtc::GruDgradParts{gp[i].dgh, wimage[i], part[i]};
        }
        {
            dtc::ProfScope prof("gru_gate_bwd", count * ((double)RH * 4.0 * 17), s);
            const GateBwdPtrs& g = gp[0];
            if (vec4)           // blockIdx.y = the recurrence
                hipLaunchKernelGGL(gru_gate_bwd4_kernel, dim3(grid4, (unsigned)count), dim3(256), 0, s, g, gp[count - 1], R, H, nparts);
            else                // (one recurrence: two advance together on the vec4 kernel only)
                hipLaunchKernelGGL(gru_gate_bwd_kernel, dim3(grid), dim3(256), 0, s, g.dhs_t, g.dh, g.part, g.gates, g.hn, g.hprev, g.dgi, g.dgh, R, H, nparts);
        }
        int rc = s3 ? dtc::gru_s3_dgrad_parts(dp, count, (int64_t)RH, R, H, nparts, stream)
                    : dtc_linear_dgrad_split(dp[0].dgh_t, 3 * H, items[0].W_hh, part[0], H, (int64_t)RH, R, 3 * H, H, nparts, stream);
        if (rc != DTC_OK) return rc;
    }
    for (int i = 0; i < count; ++i) dtc::gru_add_parts(items[i].dh0, part[i], (int64_t)RH, nparts, s);
    // no dW_hh: the caller forms the W_hh weight gradient itself from dgh_all (workspace + dtc_gru_dgh_offset: the operand-image
    // trainers pack it with the other operands of their grouped weight-gradient launch)
    if (!wg || !wg->dW_hh) return dtc::check_launch(who);
    const float* hs_all = items[0].hs_all;
    // the padding slots of the padded trajectory layout have dgh = 0: with the caller's list of valid slots the product skips them
    if (wg->valid_rows && wg->n_valid >= 1024 && wg->n_valid < T * R && dtc_get_gemm_split() && 3ll * H * H >= 128 * 128)
        return dtc_linear_wgrad_rows(dgh_all[0], 3 * H, (int64_t)T * R, hs_all, H, (int64_t)T * R, wg->valid_rows, wg->dW_hh, wg->db_hh, wgrad_ws,
                                     wg->n_valid, 3 * H, H, stream);
    const DtcSegMat Hprev = plain(hs_all, H, H, (int64_t)T * R);
    int rc = dtc_linear_wgrad(dgh_all[0], 3 * H, &Hprev, wg->dW_hh, wg->db_hh, wgrad_ws, T * R, 3 * H, H, stream);
    if (rc != DTC_OK) return rc;
    return dtc::check_launch(who);
}
}  // namespace

void dtc::gru_add_parts(float* dh, const float* part, int64_t rh, int nparts, hipStream_t s) {
    hipLaunchKernelGGL(gru_add_parts_kernel, dim3((unsigned)dtc::ceil_div(rh, 256)), dim3(256), 0, s, dh, part, (long long)rh, nparts);
}

extern "C" int dtc_gru_fwd(const float* gi, const float* h0, const float* W_hh, const float* b_hh, float* hs_all,
                           float* gates, float* hn, void* workspace, int T, int R, int H, void* stream) {
    const DtcGruFwdItem it{gi, h0, W_hh, b_hh, hs_all, gates, hn, workspace};
    return gru_fwd_run("gru_fwd", &it, 1, T, R, H, stream);
}

extern "C" int dtc_gru_fwd_multi(const DtcGruFwdItem* items, int count, int T, int R, int H, void* stream) {
    DTC_REQUIRE(items != nullptr && count >= 1 && count <= DTC_GRU_MULTI_MAX, "count = %d out of range (1..%d)", count, DTC_GRU_MULTI_MAX);
    return gru_fwd_run("gru_fwd_multi", items, count, T, R, H, stream);
}

extern "C" int dtc_gru_bwd(const float* dhs, const float* hs_all, const float* gates, const float* hn, const float* W_hh,
                           float* dgi, float* dW_hh, float* db_hh, float* dh0, void* workspace, const int64_t* valid_rows, int n_valid,
                           int T, int R, int H, void* stream) {
    const DtcGruBwdItem it{dhs, hs_all, gates, hn, W_hh, dgi, dh0, workspace};
    const GruWgrad wg{dW_hh, db_hh, valid_rows, n_valid};
    return gru_bwd_run("gru_bwd", &it, 1, &wg, T, R, H, stream);
}

// BPTT of `count` recurrences without their W_hh weight gradients (dgh_all of item i at its workspace + dtc_gru_dgh_offset, as
// dtc_gru_bwd with dW_hh = NULL leaves it)
extern "C" int dtc_gru_bwd_multi(const DtcGruBwdItem* items, int count, int T, int R, int H, void* stream) {
    DTC_REQUIRE(items != nullptr && count >= 1 && count <= DTC_GRU_MULTI_MAX, "count = %d out of range (1..%d)", count, DTC_GRU_MULTI_MAX);
    return gru_bwd_run("gru_bwd_multi", items, count, nullptr, T, R, H, stream);
}
