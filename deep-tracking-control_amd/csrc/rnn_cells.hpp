// The recurrent cells of torch.nn.GRU / torch.nn.LSTM for one (row, hidden unit): the ONLY statement of their arithmetic.  Every
// recurrence kernel (gru.hip, lstm.hip, gru_s3.hip, gru_h2i.hip, gru_seq.hip, the fused steps of gemm.hip) keeps its own loads, stores
// and layout and calls these; their results are compared bit for bit, so parenthesisation and operand order here are part of the
// contract (the sources compile with the default fp contraction, and contraction follows the expression).
// gi_* = the input projection x W_ih^T + b_ih, gh_* = the recurrent projection h_{t-1} W_hh^T + b_hh (bias included).
#pragma once
#include "common.hpp"

namespace dtc {

// GRU (gate order r, z, n): r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h_t = (1 - z) * n + z * h_{t-1}
struct GruCell {
    float r, z, n, h;
};
__device__ __forceinline__ GruCell gru_cell_fwd(float gi_r, float gi_z, float gi_n, float gh_r, float gh_z, float gh_n, float h_prev) {
    GruCell c;
    c.r = sigmoid(gi_r + gh_r);
    c.z = sigmoid(gi_z + gh_z);
    c.n = tanhf(gi_n + c.r * gh_n);
    c.h = (1.0f - c.z) * c.n + c.z * h_prev;
    return c;
}

// d = the whole gradient flowing into h_t.  da_* = the gradients w.r.t. the gates' pre-activations: dgi = (da_r, da_z, da_n),
// dgh = (da_r, da_z, da_nr); dh_z = the direct path to h_{t-1} (its W_hh path is dgh W_hh)
struct GruCellGrad {
    float da_r, da_z, da_n, da_nr, dh_z;
};
__device__ __forceinline__ GruCellGrad gru_cell_bwd(float d, float r, float z, float n, float gh_n, float h_prev) {
    GruCellGrad g;
    const float dn = d * (1.0f - z);
    const float dz = d * (h_prev - n);
    g.da_n = dn * (1.0f - n * n);
    g.da_z = dz * (z * (1.0f - z));
    g.da_r = (g.da_n * gh_n) * (r * (1.0f - r));
    g.da_nr = g.da_n * r;
    g.dh_z = d * z;
    return g;
}

// LSTM (gate order i, f, g, o): i, f, o = sigmoid(gi + gh), g = tanh(gi_g + gh_g), c_t = f * c_{t-1} + i * g, h_t = o * tanh(c_t)
struct LstmCell {
    float i, f, g, o, c, h;
};
__device__ __forceinline__ LstmCell lstm_cell_fwd(float gi_i, float gi_f, float gi_g, float gi_o, float gh_i, float gh_f, float gh_g, float gh_o,
                                                  float c_prev) {
    LstmCell s;
    s.i = sigmoid(gi_i + gh_i);
    s.f = sigmoid(gi_f + gh_f);
    s.g = tanhf(gi_g + gh_g);
    s.o = sigmoid(gi_o + gh_o);
    // f * c_prev is rounded, i * g is not: stated with fmaf because the compiler may contract `f * c_prev + i * g` around either
    // product, and which one it picks depends on the code around the expression
    s.c = fmaf(s.i, s.g, s.f * c_prev);
    s.h = s.o * tanhf(s.c);
    return s;
}

// dh = the whole gradient flowing into h_t, dc = the gradient flowing into c_t from step t + 1.  da_* = the gradients w.r.t. the gates'
// pre-activations (for an LSTM dgi = dgh), dc_prev = the gradient flowing into c_{t-1}
struct LstmCellGrad {
    float da_i, da_f, da_g, da_o, dc_prev;
};
__device__ __forceinline__ LstmCellGrad lstm_cell_bwd(float dh, float dc, float i, float f, float g, float o, float c_prev, float c_now) {
    LstmCellGrad d;
    const float tc = tanhf(c_now);
    const float dct = dc + dh * o * (1.0f - tc * tc);
    d.da_i = (dct * g) * (i * (1.0f - i));
    d.da_f = (dct * c_prev) * (f * (1.0f - f));
    d.da_g = (dct * i) * (1.0f - g * g);
    d.da_o = (dh * tc) * (o * (1.0f - o));
    d.dc_prev = dct * f;
    return d;
}

}  // namespace dtc
