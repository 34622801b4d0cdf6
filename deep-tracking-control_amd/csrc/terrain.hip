// DTC curriculum terrain for gfx950: the int16 height table the surrogate env (csrc/sim.hip) and the env kernels stand on, generated
// in device memory from one seed.  dtc_terrain_generate (include/dtc_hip.h states every formula; tests/terrain_oracle.py restates
// them in numpy and is the specification) is ONE launch: the first blocks write the table, the last num_rows * num_cols blocks the
// sub-terrain origins.
//
// What is the reference's (legged_gym/utils/terrain.py): the layout (Terrain.__init__, curiculum, randomized_terrain,
// add_terrain_to_map with its origins), the choice of a family from the cumulative proportions and the parameters of make_terrain (the
// "lite3" values that are live there), and the gap and pit sub-terrains, cell for cell.  What is this project's: the cells of the other
// seven families (slopes, stairs, discrete obstacles, stepping stones, stones everywhere).  The reference takes them from
// isaacgym.terrain_utils and from Python loops over numpy's sequential random stream; here every cell is a pure function of
// (config, seed, sub-terrain, cell) with Philox4x32-10 draws, so any thread computes any cell.  They have the reference's parameters, not
// its random sequence, and they are not isaacgym's code.
//
// Arithmetic: the parameters are IEEE doubles in the stated order (-ffp-contract=off, build.py), as the reference's Python floats, so
// every int(x / scale) is the reference's; cells are integers.  Not a hot path (it runs at construction and on request); it is a kernel
// because the env's tensors never leave the device.  Bandwidth bound and small: one thread per cell, eight neighbouring lanes gather
// their cells with wave shuffles and one of them stores 16 bytes where all eight cells lie inside the table, the first and last cells of
// a table that does not start or end on a 16-byte boundary are stored as single int16.  Nothing outside the table is written.  The origin
// blocks recompute the central window of their sub-terrain (they do not read the table, so they do not wait for it) and reduce its
// maximum over the wave with shuffles and over the block through LDS.  No atomics, no scratch.
#include <cstddef>

#include "common.hpp"
#include "philox.hpp"

namespace {

constexpr unsigned TAG = 0x74657272u;       // "terr": word 3 of every counter
enum Purpose : unsigned { P_LAYOUT = 0, P_NODE = 1, P_RECT = 2, P_STEP_SHIFT = 3, P_STONE_SHIFT = 4, P_STONE = 5 };
constexpr int GAP_UNITS = -1000;            // the reference's literal, whatever the vertical scale
constexpr int NUM_RECTANGLES = 20;

struct TerrK {
    double hs, vs, length, width;
    double cum[9];
    int R, C, S, border, rows, cols, x1, x2, curriculum;
    unsigned seed_lo, seed_hi;
    long long total;                        // rows * cols (< 2^31)
    int lead;                               // cells between the 16-byte boundary at or below the table's first cell and that cell (0..7)
    unsigned table_blocks;
};

// the integers of one sub-terrain
struct Sub {
    int fam;
    int emax, w, hstep, g, W;               // pyramids: slopes (0, 1), stairs (2, 3)
    double slope_hs, node_step;
    int full, m0, m1;                       // discrete obstacles
    int m, p, depth, mh;                    // stones (5, 8)
    int px1, px2;                           // the zero platform of 4, 5, 8
    int lo0, hi0, lo1, hi1, inner;          // gap: outer and inner square; pit: lo0, hi0 and the value `inner`
};

__device__ __forceinline__ U4 draw(const TerrK& k, unsigned sub, unsigned purpose, unsigned item) {
    return philox4x32_10(U4{item, sub, purpose, TAG}, k.seed_lo, k.seed_hi);
}

__device__ __forceinline__ int below(unsigned word, int n) { return (int)(((unsigned long long)word * (unsigned long long)(unsigned)n) >> 32); }

// a Python slice bound of a length-S axis
__device__ __forceinline__ int slice_bound(int v, int S) { return v < 0 ? max(v + S, 0) : min(v, S); }

__device__ __forceinline__ void platform(double size, const TerrK& k, int& x1, int& x2) {
    const int P = (int)(size / k.hs);
    if (P < k.S) x1 = (k.S - P) / 2, x2 = (k.S + P) / 2;
    else x1 = 0, x2 = k.S;
}

__device__ __forceinline__ Sub make_sub(const TerrK& k, int i, int j) {
    Sub s{};
    double choice, difficulty;
    if (k.curriculum) {
        difficulty = (double)i / (double)k.R;
        choice = (double)j / (double)k.C + 0.001;
    } else {
        const U4 x = draw(k, (unsigned)(i * k.C + j), P_LAYOUT, 0u);
        choice = (double)x.x * 2.3283064365386963e-10;             // 2^-32
        const unsigned q = x.y >> 30;
        difficulty = q == 0 ? 0.25 : q == 1 ? 0.5 : q == 2 ? 0.75 : 0.9;
    }
    double slope = difficulty * 0.4;
    const double stepping_stones_size = 1.05 - difficulty;
    double step_height = 0.05 + 0.13 * difficulty;
    const double discrete_obstacles_height = 0.05 + difficulty * 0.15;
    const double stone_distance = difficulty == 0.0 ? 0.03 : 0.06;
    const double max_height = 0.02 + 0.03 * difficulty;
    const double stone_size = -0.1 * difficulty + 0.3;
    const double gap_size = .8 * difficulty;
    const double pit_depth = .8 * difficulty;
    const int S = k.S;
    s.emax = max((S - (int)(3. / k.hs)) / 2, 0);
    if (choice < k.cum[0]) {
        if (choice < k.cum[0] / 2) slope *= -1;
        s.fam = 0;
    } else if (choice < k.cum[1]) {
        s.fam = 1;
        s.g = max((int)(0.2 / k.hs), 1);
        s.W = S / s.g + 2;
        s.node_step = 0.005;
    } else if (choice < k.cum[3]) {
        if (choice < k.cum[2]) step_height *= -1, s.fam = 2;
        else s.fam = 3;
        s.w = max((int)(0.31 / k.hs), 1);
        s.hstep = (int)(step_height / k.vs);
    } else if (choice < k.cum[4]) {
        s.fam = 4;
        s.full = (int)(discrete_obstacles_height / k.vs);
        s.m0 = (int)(1. / k.hs), s.m1 = (int)(2. / k.hs);
        platform(3., k, s.px1, s.px2);
    } else if (choice < k.cum[5]) {
        s.fam = 5;
        s.m = (int)(stepping_stones_size / k.hs);
        s.p = max(s.m + (int)(stone_distance / k.hs), 1);
        s.depth = (int)(-2. / k.vs);
        platform(1., k, s.px1, s.px2);
    } else if (choice < k.cum[6]) {
        s.fam = 6;
        const int g = (int)(gap_size / k.hs), P = (int)(1. / k.hs), c = S / 2;
        const int x1 = (S - P) >> 1;                               // Python's floor division
        const int x2 = x1 + g;
        s.lo0 = slice_bound(c - x2, S), s.hi0 = slice_bound(c + x2, S);
        s.lo1 = slice_bound(c - x1, S), s.hi1 = slice_bound(c + x1, S);
    } else if (choice < k.cum[7]) {
        s.fam = 7;
        const int P = (int)(1. / k.hs / 2);
        s.lo0 = slice_bound(S / 2 - P, S), s.hi0 = slice_bound(S / 2 + P, S);
        s.inner = -(int)(pit_depth / k.vs);
    } else {
        s.fam = 8;
        s.m = (int)(stone_size / k.hs);
        s.p = max(s.m + (int)(stone_distance / k.hs), 1);
        s.depth = (int)(-2. / k.vs);
        s.mh = (int)(max_height / k.vs);
        platform(1.3, k, s.px1, s.px2);
    }
    s.slope_hs = slope * k.hs;
    return s;
}

__device__ __forceinline__ double node_units(const TerrK& k, const Sub& s, unsigned sub, int na, int nb) {
    const int k21 = below(draw(k, sub, P_NODE, (unsigned)(na * s.W + nb)).x, 21);
    return ((double)(k21 - 10) * s.node_step) / k.vs;
}

// cell (a, b) of sub-terrain `sub` in units of the vertical scale, before the int16 clamp
__device__ __forceinline__ int cell_units(const TerrK& k, const Sub& s, unsigned sub, int a, int b) {
    const int S = k.S;
    switch (s.fam) {
    case 0:
    case 1: {
        const int e = min(min(min(a, S - 1 - a), min(b, S - 1 - b)), s.emax);
        int z = (int)rint((s.slope_hs * (double)e) / k.vs);
        if (s.fam == 1) {
            const int g = s.g, na = a / g, nb = b / g, fa = a % g, fb = b % g;
            const double t = ((double)((g - fa) * (g - fb)) * node_units(k, s, sub, na, nb) + (double)(fa * (g - fb)) * node_units(k, s, sub, na + 1, nb)) +
                             ((double)((g - fa) * fb) * node_units(k, s, sub, na, nb + 1) + (double)(fa * fb) * node_units(k, s, sub, na + 1, nb + 1));
            z += (int)rint(t / (double)(g * g));
        }
        return z;
    }
    case 2:
    case 3: {
        const int e = min(min(min(a, S - 1 - a), min(b, S - 1 - b)), s.emax);
        return (e / s.w) * s.hstep;
    }
    case 4: {
        if (a >= s.px1 && a < s.px2 && b >= s.px1 && b < s.px2) return 0;
        for (int r = NUM_RECTANGLES - 1; r >= 0; --r) {            // the highest-numbered rectangle over the cell wins
            const U4 x = draw(k, sub, P_RECT, (unsigned)r);
            const int la = min(s.m0 + below(x.x, s.m1 - s.m0 + 1), S), lb = min(s.m0 + below(x.y, s.m1 - s.m0 + 1), S);
            const int pa = below(x.z, S - la + 1), pb = below(x.w, S - lb + 1);
            if (a >= pa && a < pa + la && b >= pb && b < pb + lb) {
                const int mag = (x.y & 1u) ? s.full : s.full / 2;
                return (x.x & 1u) ? -mag : mag;
            }
        }
        return 0;
    }
    case 5:
    case 8: {
        if (a >= s.px1 && a < s.px2 && b >= s.px1 && b < s.px2) return 0;
        const int p = s.p, rb = b / p;
        const int t = a + below(draw(k, sub, s.fam == 5 ? P_STEP_SHIFT : P_STONE_SHIFT, (unsigned)rb).x, p);
        if (s.fam == 5) return (s.m >= S || (s.m >= 1 && b % p < s.m && t % p < s.m)) ? 0 : s.depth;
        const U4 x = draw(k, sub, P_STONE, (unsigned)(rb * 65536 + t / p));
        const int sa = s.m - 1 + below(x.x, 2), sb = s.m - 1 + below(x.y, 2);
        const int height = s.mh >= 1 ? 1 + below(x.z, 2 * s.mh) : 0;
        return (b % p < sb && t % p < sa) ? height : s.depth;
    }
    case 6:
        if (a >= s.lo1 && a < s.hi1 && b >= s.lo1 && b < s.hi1) return 0;
        return (a >= s.lo0 && a < s.hi0 && b >= s.lo0 && b < s.hi0) ? GAP_UNITS : 0;
    default:
        return (a >= s.lo0 && a < s.hi0 && b >= s.lo0 && b < s.hi0) ? s.inner : 0;
    }
}

__device__ __forceinline__ int clamp16(int v) { return min(max(v, -32768), 32767); }

__global__ __launch_bounds__(256) void terrain_kernel(const TerrK k, int16_t* __restrict__ table, float* __restrict__ origins) {
    if (blockIdx.x >= k.table_blocks) {
        // ---- the origin of one sub-terrain: the maximum over its central window (add_terrain_to_map)
        __shared__ int part[4];
        const int sub = (int)(blockIdx.x - k.table_blocks), i = sub / k.C, j = sub % k.C;
        const Sub s = make_sub(k, i, j);
        const int wn = k.x2 - k.x1;
        int top = -32768;
        for (int c = (int)threadIdx.x; c < wn * wn; c += 256)
            top = max(top, clamp16(cell_units(k, s, (unsigned)sub, k.x1 + c / wn, k.x1 + c % wn)));
        for (int d = 32; d >= 1; d >>= 1) top = max(top, __shfl_xor(top, d));
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = top;
        __syncthreads();
        if (threadIdx.x == 0) {
            top = max(max(part[0], part[1]), max(part[2], part[3]));
            origins[3 * sub + 0] = (float)(((double)i + 0.5) * k.length);
            origins[3 * sub + 1] = (float)(((double)j + 0.5) * k.width);
            origins[3 * sub + 2] = (float)((double)top * k.vs);
        }
        return;
    }
    // ---- the table: thread g owns flat cell g - lead, so the cell of a thread with g % 8 == 0 lies on a 16-byte boundary
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x - k.lead;
    const bool inside = idx >= 0 && idx < k.total;
    int v = 0;
    if (inside) {
        const int row = (int)(idx / k.cols) - k.border, col = (int)(idx % k.cols) - k.border;
        if (row >= 0 && row < k.R * k.S && col >= 0 && col < k.C * k.S) {
            const int i = row / k.S, j = col / k.S;
            const Sub s = make_sub(k, i, j);
            v = clamp16(cell_units(k, s, (unsigned)(i * k.C + j), row % k.S, col % k.S));
        }
    }
    // eight neighbouring lanes -> four 32-bit words in the lane whose cell starts the 16 bytes (every lane takes part in the shuffles)
    const unsigned h = (unsigned)v & 0xFFFFu;
    const unsigned pair = h | ((unsigned)__shfl_down((int)h, 1) << 16);
    const unsigned w1 = (unsigned)__shfl_down((int)pair, 2), w2 = (unsigned)__shfl_down((int)pair, 4), w3 = (unsigned)__shfl_down((int)pair, 6);
    const long long first = idx - (threadIdx.x & 7);               // the cell of this group's first lane
    const bool whole = first >= 0 && first + 8 <= k.total;
    if (whole) {
        if ((threadIdx.x & 7) == 0) *reinterpret_cast<uint4*>(table + idx) = make_uint4(pair, w1, w2, w3);
    } else if (inside) {
        table[idx] = (int16_t)v;
    }
}

}  // namespace

extern "C" int dtc_terrain_abi_sizes(int64_t* out, int cap) {
    const int64_t sz[] = {sizeof(DtcTerrainCfg)};
    if (cap > 0 && out) out[0] = sz[0];
    return 1;
}

extern "C" int dtc_terrain_generate(const DtcTerrainCfg* cfg, int16_t* height_samples, float* terrain_origins, void* stream) {
    DTC_REQUIRE(cfg && height_samples && terrain_origins, "null argument");
    const DtcTerrainCfg& c = *cfg;
    DTC_REQUIRE(c.horizontal_scale > 0. && c.vertical_scale > 0. && c.border_size >= 0., "scales must be positive, border_size >= 0");
    DTC_REQUIRE(c.terrain_length == c.terrain_width, "terrain_length %g != terrain_width %g: the sub-terrains are square", c.terrain_length,
                c.terrain_width);
    DTC_REQUIRE(c.terrain_length >= 2. && c.terrain_length / c.horizontal_scale < 32768., "terrain_length %g: at least 2 m, fewer than 32768 cells",
                c.terrain_length);
    DTC_REQUIRE(c.num_rows >= 1 && c.num_cols >= 1 && c.num_rows <= 32768 && c.num_cols <= 32768, "num_rows %d / num_cols %d", c.num_rows, c.num_cols);
    DTC_REQUIRE(c.border_size / c.horizontal_scale < 1073741824., "border_size %g", c.border_size);
    for (int i = 0; i < 9; ++i) DTC_REQUIRE(c.proportions[i] == c.proportions[i], "proportions[%d] is NaN", i);
    const int64_t S = (int64_t)(c.terrain_length / c.horizontal_scale), border = (int64_t)(c.border_size / c.horizontal_scale);
    const int64_t rows = c.num_rows * S + 2 * border, cols = c.num_cols * S + 2 * border;
    DTC_REQUIRE(rows * cols < ((int64_t)1 << 31), "a table of %lld x %lld cells: 2^31 cells or more", (long long)rows, (long long)cols);
    DTC_REQUIRE(rows == c.tot_rows && cols == c.tot_cols, "the table is %d x %d, the geometry gives %lld x %lld", c.tot_rows, c.tot_cols,
                (long long)rows, (long long)cols);
    DTC_REQUIRE((reinterpret_cast<uintptr_t>(height_samples) & 1u) == 0 && (reinterpret_cast<uintptr_t>(terrain_origins) & 3u) == 0, "misaligned output");

    TerrK k{};
    k.hs = c.horizontal_scale, k.vs = c.vertical_scale, k.length = c.terrain_length, k.width = c.terrain_width;
    for (int i = 0; i < 9; ++i) k.cum[i] = c.proportions[i];
    k.R = c.num_rows, k.C = c.num_cols, k.S = (int)S, k.border = (int)border, k.rows = (int)rows, k.cols = (int)cols;
    k.x1 = (int)((c.terrain_length / 2. - 1) / c.horizontal_scale);
    k.x2 = (int)((c.terrain_length / 2. + 1) / c.horizontal_scale);
    if (k.x2 > k.S) k.x2 = k.S;
    DTC_REQUIRE(k.x1 >= 0 && k.x2 > k.x1, "empty origin window %d..%d", k.x1, k.x2);
    k.curriculum = c.curriculum != 0;
    k.seed_lo = (unsigned)c.seed, k.seed_hi = (unsigned)(c.seed >> 32);
    k.total = rows * cols;
    k.lead = (int)((reinterpret_cast<uintptr_t>(height_samples) & 15u) >> 1);
    k.table_blocks = (unsigned)dtc::ceil_div(k.total + k.lead, 256);

    hipStream_t hs = (hipStream_t)stream;
    dtc::ProfScope prof("terrain_generate", 2.0 * (double)k.total, hs);
    hipLaunchKernelGGL(terrain_kernel, dim3(k.table_blocks + (unsigned)(k.R * k.C)), dim3(256), 0, hs, k, height_samples, terrain_origins);
    return dtc::check_launch("terrain_generate");
}
