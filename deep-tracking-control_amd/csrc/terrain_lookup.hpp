// The one definition of the terrain lookup of the surrogate env's kernels (csrc/sim.hip, csrc/sim_contacts.hip).
#pragma once
#include <cstdint>

namespace dtc {

// _get_heights (legged_robot.py:1301-1316) for one world point; the clamp keeps every index inside the table whatever fx, fy hold.
// `t`: a kernel's constants, with int rows, cols (the table's shape) and float border, hscale, vscale.
template <class Table>
__device__ __forceinline__ float terrain_height(const int16_t* __restrict__ hs, const Table& t, float fx, float fy) {
    const float wx = (fx + t.border) / t.hscale;
    const float wy = (fy + t.border) / t.hscale;
    long long cx = (long long)wx, cy = (long long)wy;                              // .long(): truncation toward zero
    cx = cx < 0 ? 0 : (cx > t.rows - 2 ? t.rows - 2 : cx);
    cy = cy < 0 ? 0 : (cy > t.cols - 2 ? t.cols - 2 : cy);
    const int16_t h1 = hs[cx * t.cols + cy], h2 = hs[(cx + 1) * t.cols + cy], h3 = hs[cx * t.cols + cy + 1];
    int16_t h = h1 < h2 ? h1 : h2;
    h = h < h3 ? h : h3;
    return (float)h * t.vscale;
}

}  // namespace dtc
