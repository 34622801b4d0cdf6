// What the recurrence sources (gru.hip, gru_s3.hip, gru_h2i.hip, lstm.hip) share on the host side.  Not part of the C ABI.
#pragma once
#include "common.hpp"

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
