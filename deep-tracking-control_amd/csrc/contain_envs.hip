// Containment of non-finite rollout ENVS (PPO / RecurrentPPO / RecurrentDecoderPPO(contain_nonfinite_envs=True)) for gfx950: the unit is a
// column of the [T, N, ...] storage, the place is the storage itself, before update() reads it.
//
//  * dtc_states_finite        the record over one saved hidden-state tensor [T, L, N, H] (rollout_storage.py:118-132): row t * N + n loses its
//                             1 iff any layer's state of env n at step t has a non-finite element.  The streaming read of dtc_rows_finite
//                             (16 bytes per lane at 64-bit flat indices, four loads in flight, the row worked out on a hit only) with the row
//                             map of this layout; a store is always a 0, so lanes that hit the same row need no reduction among them
//  * dtc_env_fold             env_valid[n] = AND over t of row_valid[t * N + n]: one lane per env, T coalesced byte reads
//  * dtc_env_columns_repair   column env_src[n] copied over column n of every listed buffer, for every invalid env n.  How many there are
//                             is known on the device only: a FIXED grid (a few workgroups per CU) walks the envs in chunks, every workgroup
//                             builds the same ascending list of a chunk's invalid envs in LDS (ballots, no atomics) and takes its share of
//                             the (invalid env, item, block of outer indices) units; a chunk without an invalid env costs one barrier
//
// The sources (env_src) come from dtc_compact_valid + dtc_perm_repair (contain.hip) applied to the identity permutation of length N.
#include "common.hpp"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));      // a native vector: one global_load_dwordx4 / global_store_dwordx4

// ---- hidden-state scan ----------------------------------------------------------------------------------------------------------
constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_BLOCKS = 2048;                  // 8 workgroups per CU x 256 CUs; the rest of the tensor by grid stride

__device__ __forceinline__ bool nonfinite_bits(uint32_t x) { return (x & 0x7f800000u) == 0x7f800000u; }

__device__ __forceinline__ bool any_nonfinite(const u32x4 v) {
    return nonfinite_bits(v.x) | nonfinite_bits(v.y) | nonfinite_bits(v.z) | nonfinite_bits(v.w);
}

// flat element e of [T, L, N, H] -> record row t * N + n
__device__ __forceinline__ long long state_row(long long e, long long H, long long N, long long L) {
    const long long q = e / H;                     // (t * L + l) * N + n
    return (q / (N * L)) * N + q % N;
}

__device__ __forceinline__ void clear_state_rows(const u32x4 v, long long first_elem, long long H, long long N, long long L,
                                                 uint8_t* __restrict__ out) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (nonfinite_bits(v[k])) out[state_row(first_elem + k, H, N, L)] = 0;
}

// Writers only ever store 0 into a record initialised by the caller: plain byte stores, the result does not depend on scheduling.
__global__ __launch_bounds__(SCAN_BLOCK) void states_finite_kernel(const float* __restrict__ p, long long total, long long nvec, int head,
                                                                    long long H, long long N, long long L, uint8_t* __restrict__ out) {
    if (blockIdx.x == 0) {
        // unaligned head and tail of the array: scalar loads (at most 3 + 3 elements)
        const long long tail0 = head + 4 * nvec;
        const int ntail = (int)(total - tail0);
        if ((int)threadIdx.x < head) {
            if (nonfinite_bits(__float_as_uint(p[threadIdx.x]))) out[state_row(threadIdx.x, H, N, L)] = 0;
        } else if ((int)threadIdx.x >= 64 && (int)threadIdx.x - 64 < ntail) {
            const long long e = tail0 + ((int)threadIdx.x - 64);
            if (nonfinite_bits(__float_as_uint(p[e]))) out[state_row(e, H, N, L)] = 0;
        }
    }
    const u32x4* __restrict__ pv = reinterpret_cast<const u32x4*>(p + head);
    const long long stride = (long long)gridDim.x * SCAN_BLOCK;
    long long g = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    // four independent 16-byte loads in flight per lane
    for (; g + 3 * stride < nvec; g += 4 * stride) {
        const u32x4 v0 = __builtin_nontemporal_load(pv + g);
        const u32x4 v1 = __builtin_nontemporal_load(pv + g + stride);
        const u32x4 v2 = __builtin_nontemporal_load(pv + g + 2 * stride);
        const u32x4 v3 = __builtin_nontemporal_load(pv + g + 3 * stride);
        if (any_nonfinite(v0)) clear_state_rows(v0, head + 4 * g, H, N, L, out);
        if (any_nonfinite(v1)) clear_state_rows(v1, head + 4 * (g + stride), H, N, L, out);
        if (any_nonfinite(v2)) clear_state_rows(v2, head + 4 * (g + 2 * stride), H, N, L, out);
        if (any_nonfinite(v3)) clear_state_rows(v3, head + 4 * (g + 3 * stride), H, N, L, out);
    }
    for (; g < nvec; g += stride) {
        const u32x4 v = __builtin_nontemporal_load(pv + g);
        if (any_nonfinite(v)) clear_state_rows(v, head + 4 * g, H, N, L, out);
    }
}

// ---- fold: rows -> envs ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void env_fold_kernel(const uint8_t* __restrict__ row_valid, long long T, long long N,
                                                       uint8_t* __restrict__ env_valid) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    uint8_t ok = 1;
    for (long long t = 0; t < T; ++t) ok &= (uint8_t)(row_valid[t * N + n] != 0);
    env_valid[n] = ok;
}

// ---- repair: valid columns over invalid ones ------------------------------------------------------------------------------------
constexpr int MAX_ITEMS = 32;
constexpr int RP_BLOCK = 256;
constexpr int RP_WAVES = RP_BLOCK / 64;
constexpr int RP_PER = 8;                          // envs per lane and chunk
constexpr int RP_CHUNK = RP_BLOCK * RP_PER;        // envs per chunk: its invalid envs fit an 8 KiB list in LDS
constexpr int RP_UNIT_BYTES = 4096;                // a unit copies about this much: several outer indices of a narrow item at once
constexpr int RP_BLOCKS_PER_CU = 4;

struct RepairItem {
    char* base;
    long long outer, outer_stride, env_stride;
    int width;               // bytes of one (outer index, env) row
    int elem;                // bytes per access: 16, 4 or 1 (what base, strides and width allow)
    int rpu;                 // outer indices per unit
    int unit0;               // first unit of this item among the units of one env
};
struct RepairArgs {
    RepairItem it[MAX_ITEMS];
    int count;
    int units;               // units of one env over all items
};

template <typename V>
__device__ __forceinline__ void copy_rows(char* __restrict__ dst, const char* __restrict__ src, long long outer_stride, int rows,
                                          unsigned per_row) {
    const unsigned total = (unsigned)rows * per_row;           // rows > 1 only where rows * width <= 2 * RP_UNIT_BYTES
    for (unsigned e = threadIdx.x; e < total; e += RP_BLOCK) {
        const unsigned r = e / per_row, c = e - r * per_row;
        const long long o = (long long)r * outer_stride + (long long)c * (long long)sizeof(V);
        *reinterpret_cast<V*>(dst + o) = *reinterpret_cast<const V*>(src + o);
    }
}

// Source columns belong to valid envs and are never written, destination columns to invalid ones: no read / write overlap between
// units, and every unit is taken by exactly one workgroup (every workgroup derives the same lists from the same record).
__global__ __launch_bounds__(RP_BLOCK) void env_columns_repair_kernel(const RepairArgs A, const uint8_t* __restrict__ env_valid,
                                                                      const long long* __restrict__ env_src, long long N) {
    __shared__ int s_list[RP_CHUNK];
    __shared__ int s_cnt[RP_PER * RP_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long G = gridDim.x;
    long long rot = 0;                             // units handed out so far, modulo G: the next chunk's first unit goes to the next workgroup
    for (long long c0 = 0; c0 < N; c0 += RP_CHUNK) {
        unsigned inv = 0;
#pragma unroll
        for (int k = 0; k < RP_PER; ++k) {
            const long long n = c0 + k * RP_BLOCK + threadIdx.x;
            bool bad = n < N && env_valid[n] == 0;
            if (bad) {
                const long long s = env_src[n];    // (no valid env at all: the identity -- nothing can be repaired, nothing is copied)
                bad = s >= 0 && s < N && s != n;
            }
            inv |= (unsigned)bad << k;
        }
        if (!__syncthreads_or((int)inv)) continue;
        int pos[RP_PER];
#pragma unroll
        for (int k = 0; k < RP_PER; ++k) {
            const unsigned long long m = __ballot((inv >> k) & 1u);
            pos[k] = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) s_cnt[k * RP_WAVES + wave] = __popcll(m);
        }
        __syncthreads();
        int found = 0;
#pragma unroll
        for (int k = 0; k < RP_PER; ++k) {
#pragma unroll
            for (int w = 0; w < RP_WAVES; ++w) {
                if (w == wave && ((inv >> k) & 1u)) s_list[found + pos[k]] = (int)(k * RP_BLOCK + threadIdx.x);
                found += s_cnt[k * RP_WAVES + w];
            }
        }
        __syncthreads();
        found = __builtin_amdgcn_readfirstlane(found);           // (the same in every lane: keeps the unit loop and the item look-up scalar)
        const long long total = (long long)found * A.units;
        for (long long u = ((long long)blockIdx.x + G - rot) % G; u < total; u += G) {
            const int i = __builtin_amdgcn_readfirstlane((int)(u / A.units)), j = __builtin_amdgcn_readfirstlane((int)(u % A.units));
            const long long n = c0 + s_list[i];
            const long long s = env_src[n];
            int q = 0;
            while (q + 1 < A.count && j >= A.it[q + 1].unit0) ++q;
            const RepairItem I = A.it[q];
            const long long r0 = (long long)(j - I.unit0) * I.rpu;
            const int rows = (int)(I.outer - r0 < I.rpu ? I.outer - r0 : I.rpu);
            char* row0 = I.base + r0 * I.outer_stride;
            char* dst = row0 + n * I.env_stride;
            const char* src = row0 + s * I.env_stride;
            if (I.elem == 16)
                copy_rows<u32x4>(dst, src, I.outer_stride, rows, (unsigned)I.width / 16u);
            else if (I.elem == 4)
                copy_rows<uint32_t>(dst, src, I.outer_stride, rows, (unsigned)I.width / 4u);
            else
                copy_rows<uint8_t>(dst, src, I.outer_stride, rows, (unsigned)I.width);
        }
        rot = (rot + total) % G;
        __syncthreads();                           // the list is rebuilt by the next chunk
    }
}

int repair_grid() {
    static int blocks = 0;                         // (the CU count of the current device, read once)
    if (blocks == 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
            return 0;
        blocks = cus * RP_BLOCKS_PER_CU;
    }
    return blocks;
}

}  // namespace

extern "C" int dtc_contain_envs_abi_sizes(int64_t* out, int cap) {
    const int64_t sz[] = {sizeof(DtcEnvColumn)};
    const int n = (int)(sizeof(sz) / sizeof(sz[0]));
    for (int i = 0; i < n && i < cap && out; ++i) out[i] = sz[i];
    return n;
}

extern "C" int dtc_env_columns_cap(void) { return MAX_ITEMS; }

extern "C" int dtc_states_finite(const float* s, int64_t T, int64_t L, int64_t N, int64_t H, uint8_t* row_valid, void* stream) {
    DTC_REQUIRE(s && row_valid, "states_finite: null pointer");
    DTC_REQUIRE(T >= 0 && L >= 1 && N >= 1 && H >= 1, "states_finite: bad shape T=%lld L=%lld N=%lld H=%lld", (long long)T, (long long)L,
                (long long)N, (long long)H);
    DTC_REQUIRE((reinterpret_cast<uintptr_t>(s) & 3u) == 0, "states_finite: the tensor is not 4-byte aligned");
    const int64_t lim = (int64_t)1 << 20;
    DTC_REQUIRE(T <= lim && L <= lim && N <= ((int64_t)1 << 31) && H <= lim && T * L <= ((int64_t)1 << 60) / (N * H),
                "states_finite: T * L * N * H overflows");
    if (T == 0) return DTC_OK;
    const long long total = (long long)(T * L * N * H);
    const long long to16 = (long long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(s) & 15u)) & 15u) / 4u);
    const int head = (int)(to16 < total ? to16 : total);
    const long long nvec = (total - head) / 4;
    const long long want = dtc::ceil_div(nvec, (long long)SCAN_BLOCK * 4);       // four groups per lane and pass
    const int blocks = (int)(want < 1 ? 1 : (want < SCAN_BLOCKS ? want : SCAN_BLOCKS));
    hipStream_t st = (hipStream_t)stream;
    const double bytes = 4.0 * (double)total;
    dtc::ProfScope prof("states_finite", bytes, st, bytes);
    hipLaunchKernelGGL(states_finite_kernel, dim3(blocks), dim3(SCAN_BLOCK), 0, st, s, total, nvec, head, (long long)H, (long long)N,
                       (long long)L, row_valid);
    return dtc::check_launch("states_finite");
}

extern "C" int dtc_env_fold(const uint8_t* row_valid, int64_t T, int64_t N, uint8_t* env_valid, void* stream) {
    DTC_REQUIRE(row_valid && env_valid, "env_fold: null pointer");
    DTC_REQUIRE(T >= 1 && N >= 1 && N <= ((int64_t)1 << 31) && T <= ((int64_t)1 << 60) / N, "env_fold: bad shape T=%lld N=%lld", (long long)T,
                (long long)N);
    hipLaunchKernelGGL(env_fold_kernel, dim3((unsigned)dtc::ceil_div(N, 256)), dim3(256), 0, (hipStream_t)stream, row_valid, (long long)T,
                       (long long)N, env_valid);
    return dtc::check_launch("env_fold");
}

extern "C" int dtc_env_columns_repair(const DtcEnvColumn* items, int n_items, const uint8_t* env_valid, const int64_t* env_src, int64_t N,
                                      void* stream) {
    DTC_REQUIRE(n_items >= 1 && n_items <= MAX_ITEMS, "env_columns_repair: %d items (1..%d)", n_items, MAX_ITEMS);
    DTC_REQUIRE(items && env_valid && env_src, "env_columns_repair: null pointer");
    DTC_REQUIRE(N >= 1 && N <= ((int64_t)1 << 31), "env_columns_repair: bad env count N=%lld", (long long)N);
    RepairArgs A;
    long long units = 0;
    for (int i = 0; i < n_items; ++i) {
        const DtcEnvColumn& c = items[i];
        DTC_REQUIRE(c.base != nullptr, "env_columns_repair: item %d is a null pointer", i);
        DTC_REQUIRE(c.width_bytes >= 1, "env_columns_repair: item %d has width_bytes=%d (>= 1)", i, (int)c.width_bytes);
        DTC_REQUIRE(c.outer >= 1 && c.outer <= ((int64_t)1 << 30), "env_columns_repair: item %d has outer=%lld (1..2^30)", i, (long long)c.outer);
        DTC_REQUIRE(c.env_stride_bytes >= c.width_bytes && c.env_stride_bytes <= ((int64_t)1 << 40),
                    "env_columns_repair: item %d: env_stride_bytes=%lld is below its width or too large", i, (long long)c.env_stride_bytes);
        DTC_REQUIRE(c.outer_stride_bytes >= 0 && c.outer_stride_bytes <= ((int64_t)1 << 50) && (c.outer == 1 || c.outer_stride_bytes >= c.width_bytes),
                    "env_columns_repair: item %d: bad outer_stride_bytes=%lld", i, (long long)c.outer_stride_bytes);
        RepairItem& r = A.it[i];
        r.base = (char*)c.base;
        r.outer = c.outer;
        r.outer_stride = c.outer_stride_bytes;
        r.env_stride = c.env_stride_bytes;
        r.width = c.width_bytes;
        const uint64_t all = (uint64_t)reinterpret_cast<uintptr_t>(c.base) | (uint64_t)c.outer_stride_bytes | (uint64_t)c.env_stride_bytes |
                             (uint64_t)c.width_bytes;
        r.elem = (all & 15u) == 0 ? 16 : (all & 3u) == 0 ? 4 : 1;
        const long long fit = dtc::ceil_div(RP_UNIT_BYTES, (long long)c.width_bytes);
        r.rpu = (int)(fit < c.outer ? fit : c.outer);
        r.unit0 = (int)units;
        units += dtc::ceil_div(c.outer, r.rpu);
        DTC_REQUIRE(units < ((long long)1 << 31), "env_columns_repair: too many outer indices in all");
    }
    for (int i = n_items; i < MAX_ITEMS; ++i) A.it[i] = RepairItem{nullptr, 1, 0, 0, 1, 1, 1, (int)units};
    A.count = n_items;
    A.units = (int)units;
    const int blocks = repair_grid();
    if (blocks < 1) {
        dtc::set_error("env_columns_repair: no device to size the grid from");
        return DTC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(env_columns_repair_kernel, dim3(blocks), dim3(RP_BLOCK), 0, (hipStream_t)stream, A, env_valid,
                       (const long long*)env_src, (long long)N);
    return dtc::check_launch("env_columns_repair");
}
