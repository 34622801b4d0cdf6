// What the recurrence sources (gru.hip, gru_s3.hip, gru_h2i.hip, lstm.hip and the fused steps of gemm.hip) share besides the cells of
// rnn_cells.hpp: host helpers of the drivers, and two pieces of device code with more than one user -- the GRU epilogue on the 32 x 32
// accumulator layout and the workgroup -> tile map of the per-step GRU kernels, with the grid size that goes with it.  Not part of the
// C ABI.
#pragma once
#include "gemm_core.hpp"      // f32x16 and the buffer loads of the epilogue below (gru.hip / lstm.hip use only the host helpers)
#include "rnn_cells.hpp"

namespace {

// torch.nn.GRU's gate math on the 32 x 32 accumulator layout: the epilogue of the fused forward steps (gru_step_fwd_kernel in gemm.hip,
// gru_s3_kernel<FWD> in gru_s3.hip).  The lane holds unit j and the 16 rows row0 + (r & 3) + 8 * (r >> 2) of acc_*[r] = the three
// gates' h_{t-1} W_hh^T (bias not yet added); ldh = row stride of hprev.  gi / h_{t-1} come in through unconditional buffer loads
// (rows >= R read 0); saves r, z, n and gh_n.
__device__ __forceinline__ void gru_epilogue_32x32(const f32x16& acc_r, const f32x16& acc_z, const f32x16& acc_n, int row0, int j,
                                                   const float* hprev, long long ldh, const float* bhh, const float* gi, float* hout,
                                                   float* gates, float* hn, int R, int H) {
    const float br = bhh[j], bz = bhh[H + j], bn = bhh[2 * H + j];
    const rsrc_t gres = make_rsrc_bytes(gi, (long long)R * 3 * H * 4), hres = make_rsrc_bytes(hprev, (long long)R * ldh * 4);
    float gr[16], gz[16], gn[16], hp[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ro = (r & 3) + 8 * (r >> 2);
        const u32 go = (u32)((row0 + ro) * 3 * H + j) * 4u;
        gr[r] = bload(gres, go, 0u);
        gz[r] = bload(gres, go, (u32)H * 4u);
        gn[r] = bload(gres, go, (u32)H * 8u);
        hp[r] = bload(hres, (u32)((long long)(row0 + ro) * ldh + j) * 4u, 0u);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + (r & 3) + 8 * (r >> 2);
        const float ghn = acc_n[r] + bn;
        const dtc::GruCell c = dtc::gru_cell_fwd(gr[r], gz[r], gn[r], acc_r[r] + br, acc_z[r] + bz, ghn, hp[r]);
        if (row < R) {
            const long long e = (long long)row * H + j;
            float* gp = gates + (long long)row * 3 * H + j;
            hout[e] = c.h;
            gp[0] = c.r;
            gp[H] = c.z;
            gp[2 * H] = c.n;
            hn[e] = ghn;
        }
    }
}

}  // namespace

namespace dtc {

constexpr int GRU_MAX_PARTS = 6;

// chunks of the 3H-long reduction of dh += dgh W_hh that run side by side: 3 on the single-pass path; the split paths run 128 x 128
// tiles (4 column tiles for H = 512), so they take 6 to put ~290 workgroups on the chip where a chunk stays a multiple of 16 long
inline int gru_parts(int H, bool split) { return split && (3 * H / GRU_MAX_PARTS) % 16 == 0 ? GRU_MAX_PARTS : 3; }

// one fp32 matrix [rows, cols] with leading dimension ld as an operand of the dtc_linear_* entry points
inline DtcSegMat plain(const float* p, int64_t ld, int cols, int64_t rows) {
    DtcSegMat m;
    m.nseg = 1;
    m.cols = cols;
    m.idx = nullptr;
    m.seg[0] = DtcSeg{const_cast<float*>(p), ld, 0, cols, 0, 0, rows};
    return m;
}

// The workgroup -> tile map of the per-step GRU kernels (gru_s3_kernel, gru_h2i_kernel) and the grid that goes with it.
// XCD x (= blockIdx.x & 7: workgroups go round-robin over the XCDs) owns a fixed set of (column tile, chunk) pairs and runs them for ALL
// row tiles: its slice of the W_hh image (1/8 of 4.7 MB at H = 512) stays in its 4 MiB L2 over the time steps of a pass, and what it
// fetches from the Infinity Cache per step is the row operand.  With the row-tile map of the general GEMM kernels every XCD walks the
// WHOLE image once per step -- more than its L2 holds -- and a time step's time follows the bytes that miss: two recurrences in one
// launch took 1.6 x the time of one (tools/gru_pair_probe.py).
struct GruXcdTile {
    int tr, tc, chunk;          // row tile, column tile, chunk of the reduction (0 .. nparts - 1)
    bool valid;                 // false: a padding workgroup
};
__device__ __forceinline__ GruXcdTile gru_xcd_tile(int b, int row_tiles, int col_tiles, int nparts) {
    const int combos = col_tiles * nparts, per_xcd = (combos + 7) >> 3;
    const int xcd = b & 7, j = b >> 3, cl = j / row_tiles;
    const int combo = xcd * per_xcd + cl;
    GruXcdTile t;
    t.tr = j - cl * row_tiles;
    t.chunk = combo / col_tiles;
    t.tc = combo - t.chunk * col_tiles;
    t.valid = cl < per_xcd && combo < combos;
    return t;
}
inline unsigned gru_xcd_grid(int row_tiles, int col_tiles, int nparts) {
    return (unsigned)(8 * ceil_div((int64_t)col_tiles * nparts, 8) * row_tiles);
}

// One time step of `count` (1 .. DTC_GRU_MULTI_MAX) recurrences of one shape on the split-precision path as ONE launch (gru_s3.hip);
// img = dtc_gru_s3_image(W_hh, backward = 0 / 1).  The exported dtc_gru_step_fwd_s3 / dtc_gru_dgrad_parts_s3 are the count == 1 case.
struct GruStepFwd {
    const float* hprev;
    const void* img;
    const float* b_hh;
    const float* gi_t;
    float* hout;
    float* gates_t;
    float* hn_t;
};
struct GruDgradParts {
    const float* dgh_t;
    const void* img;
    float* part;
};
// dh <- dh + the nparts chunks [rh] of the last W_hh data gradient of a backward pass, in the gate kernels' order (gru.hip)
void gru_add_parts(float* dh, const float* part, int64_t rh, int nparts, hipStream_t s);

int gru_s3_step_fwd(const GruStepFwd* items, int count, int R, int H, void* stream);
int gru_s3_dgrad_parts(const GruDgradParts* items, int count, int64_t part_stride, int R, int H, int nparts, void* stream);

}  // namespace dtc
