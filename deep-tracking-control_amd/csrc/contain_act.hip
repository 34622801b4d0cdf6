// Containment of non-finite envs AT THE ROLLOUT STEP (contain_nonfinite_act=True of all three trainers) for gfx950: one launch behind
// the policy step of act(), in front of env.step().
//
//  * dtc_act_contain   env n is BAD iff any fp32 element of any listed item at env n has all exponent bits set (NaN, +-inf).  For a bad
//                      env every element of every mode-1 item is set to +0.0f (the actions that leave act(), the live recurrent state);
//                      act_valid_row[n] = !bad and env_bad[n] = bad are written for EVERY env.  Nothing else is written.
//
// One wavefront owns one env (four envs per 256-thread workgroup): it reads the env's rows of every item, takes a wave-wide any, and
// only a wave that found something runs the stores.  No LDS, no atomics, no barrier, no second launch; the result does not depend on
// scheduling.  A row is read (and zeroed) as an unaligned head of at most 3 elements, whole 16-byte groups, and a tail of at most 3:
// rows of any width and any 4-byte aligned start take 16-byte accesses over their middle (the 1389-wide privileged observations, whose
// 5556-byte rows start at every residue of 16, as well as the 50-wide states), so the host has nothing to decide per item.
#include "common.hpp"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));      // a native vector: one global_load_dwordx4 / global_store_dwordx4

constexpr int MAX_ITEMS = 24;                      // two 2-layer LSTMs (4 state tensors) + actions + 8 scanned row tensors = 13
constexpr int AC_BLOCK = 256;
constexpr int AC_WAVES = AC_BLOCK / 64;            // envs per workgroup

struct ActArgs {
    DtcActItem it[MAX_ITEMS];
    int count;
};

__device__ __forceinline__ unsigned nonfinite_bits(uint32_t x) { return (unsigned)((x & 0x7f800000u) == 0x7f800000u); }

// One row [r, r + width) by the 64 lanes of a wave.  ZERO = false: returns whether this lane saw a non-finite element;
// ZERO = true: stores +0.0f over the row.  Every access lies inside the row.
template <bool ZERO>
__device__ __forceinline__ unsigned walk_row(uint32_t* r, int width, int lane) {
    const int to16 = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(r) >> 2) & 3u)) & 3u);
    const int head = to16 < width ? to16 : width;
    const int nvec = (width - head) >> 2;
    const int tail0 = head + 4 * nvec;
    unsigned hit = 0;
    int e = -1;                                    // lanes 0..2: the head; lanes 4..6: the tail
    if (lane < head) e = lane;
    else if (lane >= 4 && lane - 4 < width - tail0) e = tail0 + lane - 4;
    if (e >= 0) {
        if (ZERO) r[e] = 0u;
        else hit = nonfinite_bits(r[e]);
    }
    u32x4* v = reinterpret_cast<u32x4*>(r + head);
#pragma unroll 4                                   // (several independent 16-byte loads in flight per lane on a wide row)
    for (int g = lane; g < nvec; g += 64) {
        if (ZERO) {
            v[g] = u32x4{0u, 0u, 0u, 0u};
        } else {
            const u32x4 x = v[g];
            hit |= nonfinite_bits(x.x) | nonfinite_bits(x.y) | nonfinite_bits(x.z) | nonfinite_bits(x.w);
        }
    }
    return hit;
}

__global__ __launch_bounds__(AC_BLOCK) void act_contain_kernel(const ActArgs A, long long N, uint8_t* __restrict__ act_valid_row,
                                                               uint8_t* __restrict__ env_bad) {
    const int lane = threadIdx.x & 63;
    const long long n = (long long)blockIdx.x * AC_WAVES + (threadIdx.x >> 6);
    if (n >= N) return;                            // (a whole wave: there is no barrier below)
    unsigned hit = 0;
    for (int q = 0; q < A.count; ++q) {
        const DtcActItem I = A.it[q];
        uint32_t* row = static_cast<uint32_t*>(I.base) + n * I.env_stride_elems;
        for (long long o = 0; o < I.outer; ++o, row += I.outer_stride_elems) hit |= walk_row<false>(row, I.width, lane);
    }
    const bool bad = __builtin_amdgcn_ballot_w64(hit != 0u) != 0ull;
    if (lane == 0) {
        if (act_valid_row) act_valid_row[n] = (uint8_t)!bad;
        if (env_bad) env_bad[n] = (uint8_t)bad;
    }
    if (!bad) return;
    for (int q = 0; q < A.count; ++q) {
        const DtcActItem I = A.it[q];
        if (I.mode != 1) continue;
        uint32_t* row = static_cast<uint32_t*>(I.base) + n * I.env_stride_elems;
        for (long long o = 0; o < I.outer; ++o, row += I.outer_stride_elems) walk_row<true>(row, I.width, lane);
    }
}

}  // namespace

extern "C" int dtc_act_contain_abi_sizes(int64_t* out, int cap) {
    const int64_t sz[] = {sizeof(DtcActItem)};
    const int n = (int)(sizeof(sz) / sizeof(sz[0]));
    for (int i = 0; i < n && i < cap && out; ++i) out[i] = sz[i];
    return n;
}

extern "C" int dtc_act_contain_cap(void) { return MAX_ITEMS; }

extern "C" int dtc_act_contain(const DtcActItem* items, int n_items, int64_t N, uint8_t* act_valid_row, uint8_t* env_bad, void* stream) {
    DTC_REQUIRE(items != nullptr, "act_contain: items is a null pointer");
    DTC_REQUIRE(n_items >= 1 && n_items <= MAX_ITEMS, "act_contain: %d items (1..%d)", n_items, MAX_ITEMS);
    DTC_REQUIRE(N >= 1 && N <= ((int64_t)1 << 31), "act_contain: bad env count N=%lld (1..2^31)", (long long)N);
    ActArgs A;
    bool repairs = false;
    double bytes = 0.0;
    for (int i = 0; i < n_items; ++i) {
        const DtcActItem& c = items[i];
        DTC_REQUIRE(c.base != nullptr, "act_contain: item %d is a null pointer", i);
        DTC_REQUIRE((reinterpret_cast<uintptr_t>(c.base) & 3u) == 0, "act_contain: item %d is not 4-byte aligned", i);
        DTC_REQUIRE(c.width >= 1, "act_contain: item %d has width=%d (>= 1)", i, (int)c.width);
        DTC_REQUIRE(c.outer >= 1 && c.outer <= ((int64_t)1 << 20), "act_contain: item %d has outer=%lld (1..2^20)", i, (long long)c.outer);
        DTC_REQUIRE(c.env_stride_elems >= c.width && c.env_stride_elems <= ((int64_t)1 << 31),
                    "act_contain: item %d: env_stride_elems=%lld is below its width or too large", i, (long long)c.env_stride_elems);
        DTC_REQUIRE(c.outer == 1 || (c.outer_stride_elems >= c.width && c.outer_stride_elems <= ((int64_t)1 << 40)),
                    "act_contain: item %d: outer_stride_elems=%lld is below its width or too large", i, (long long)c.outer_stride_elems);
        DTC_REQUIRE(c.mode == 0 || c.mode == 1, "act_contain: item %d has mode=%d (0: scan, 1: scan and zero)", i, (int)c.mode);
        repairs = repairs || c.mode == 1;
        bytes += 4.0 * (double)c.outer * (double)c.width * (double)N;
        A.it[i] = c;
        if (c.outer == 1) A.it[i].outer_stride_elems = 0;
    }
    DTC_REQUIRE(act_valid_row || env_bad || repairs, "act_contain: no output and no item to zero -- nothing to do");
    for (int i = n_items; i < MAX_ITEMS; ++i) A.it[i] = DtcActItem{nullptr, 0, 0, 0, 0, 0};
    A.count = n_items;
    hipStream_t st = (hipStream_t)stream;
    dtc::ProfScope prof("act_contain", bytes, st, bytes);
    hipLaunchKernelGGL(act_contain_kernel, dim3((unsigned)dtc::ceil_div(N, AC_WAVES)), dim3(AC_BLOCK), 0, st, A, (long long)N, act_valid_row,
                       env_bad);
    return dtc::check_launch("act_contain");
}
