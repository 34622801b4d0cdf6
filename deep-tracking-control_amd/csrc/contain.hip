// Containment of non-finite rollout rows (PPO(contain_nonfinite=True)) for gfx950: the per-row validity record of the stored rollout,
// its compaction into the ascending list of valid rows, and the repair of a mini-batch permutation.
//
//  * dtc_rows_finite     the record over the stored tensors of rollout_storage.py:57-97: row r keeps its 1 iff every element of row r
//                        of every matrix is finite (exponent field not all ones).  The only kernel here that moves real bytes
//                        (7.2 KB per row): a streaming read, 16 bytes per lane at 64-bit flat indices, rows worked out on a hit only
//  * dtc_compact_valid   record -> valid_list (ascending flat rows t * N + n) and n_valid, on the device: per-block counts, one
//                        single-block scan of the block counts, a scatter.  No atomics: the list is the same on every run
//  * dtc_perm_repair     rollout_storage.py:165 (`torch.randperm`) restricted to the valid rows: an entry that names an invalid
//                        row is replaced by valid_list[entry % n_valid]; the mini-batch size stays
//
// The contained GAE scan and advantage statistics live in gae.hip beside the kernels whose reduction order they keep.
#include "common.hpp"

namespace {

constexpr int MAX_MATS = 16;
constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_BLOCKS_PER_MAT = 2048;          // 8 workgroups per CU x 256 CUs; the rest of a matrix by grid stride

struct ScanMat {
    const float* ptr;        // 4-byte aligned base of the flat [R * w] array
    long long w;             // row width in floats
    long long total;         // R * w
    long long nvec;          // 16-byte groups between the unaligned head and the tail
    int head;                // floats in front of the first 16-byte boundary (0..3, <= total)
    int blk0;                // first block of the 1-D grid that works on this matrix
};
struct ScanArgs {
    ScanMat m[MAX_MATS];
    int count;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));      // a native vector: one global_load_dwordx4, and the nontemporal builtin takes it

__device__ __forceinline__ bool nonfinite_bits(uint32_t x) { return (x & 0x7f800000u) == 0x7f800000u; }

// a 16-byte group with a non-finite element (rare): the rows its four elements lie in -- two when w % 4 != 0 and the group straddles
__device__ __forceinline__ void clear_rows(const u32x4 v, long long first_elem, long long w, uint8_t* __restrict__ out) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (nonfinite_bits(v[k])) out[(first_elem + k) / w] = 0;
}

__device__ __forceinline__ bool any_nonfinite(const u32x4 v) {
    return nonfinite_bits(v.x) | nonfinite_bits(v.y) | nonfinite_bits(v.z) | nonfinite_bits(v.w);
}

// Writers only ever store 0 into a record initialised to 1: plain byte stores, the result does not depend on scheduling.
__global__ __launch_bounds__(SCAN_BLOCK) void rows_finite_kernel(const ScanArgs A, uint8_t* __restrict__ out) {
    int mi = 0;
    while (mi + 1 < A.count && (int)blockIdx.x >= A.m[mi + 1].blk0) ++mi;
    const float* __restrict__ p = A.m[mi].ptr;
    const long long w = A.m[mi].w, total = A.m[mi].total, nvec = A.m[mi].nvec;
    const int head = A.m[mi].head;
    const int nblk = (mi + 1 < A.count ? A.m[mi + 1].blk0 : (int)gridDim.x) - A.m[mi].blk0;
    const int blk = (int)blockIdx.x - A.m[mi].blk0;
    if (blk == 0) {
        // unaligned head and tail of the array: scalar loads (at most 3 + 3 elements)
        const long long tail0 = head + 4 * nvec;
        const int ntail = (int)(total - tail0);
        if ((int)threadIdx.x < head) {
            if (nonfinite_bits(__float_as_uint(p[threadIdx.x]))) out[(long long)threadIdx.x / w] = 0;
        } else if ((int)threadIdx.x >= 64 && (int)threadIdx.x - 64 < ntail) {
            const long long e = tail0 + ((int)threadIdx.x - 64);
            if (nonfinite_bits(__float_as_uint(p[e]))) out[e / w] = 0;
        }
    }
    const u32x4* __restrict__ pv = reinterpret_cast<const u32x4*>(p + head);
    const long long stride = (long long)nblk * SCAN_BLOCK;
    long long g = (long long)blk * SCAN_BLOCK + threadIdx.x;
    // four independent 16-byte loads in flight per lane
    for (; g + 3 * stride < nvec; g += 4 * stride) {
        const u32x4 v0 = __builtin_nontemporal_load(pv + g);
        const u32x4 v1 = __builtin_nontemporal_load(pv + g + stride);
        const u32x4 v2 = __builtin_nontemporal_load(pv + g + 2 * stride);
        const u32x4 v3 = __builtin_nontemporal_load(pv + g + 3 * stride);
        if (any_nonfinite(v0)) clear_rows(v0, head + 4 * g, w, out);
        if (any_nonfinite(v1)) clear_rows(v1, head + 4 * (g + stride), w, out);
        if (any_nonfinite(v2)) clear_rows(v2, head + 4 * (g + 2 * stride), w, out);
        if (any_nonfinite(v3)) clear_rows(v3, head + 4 * (g + 3 * stride), w, out);
    }
    for (; g < nvec; g += stride) {
        const u32x4 v = __builtin_nontemporal_load(pv + g);
        if (any_nonfinite(v)) clear_rows(v, head + 4 * g, w, out);
    }
}

// ---- compaction: record -> ascending list of valid rows -------------------------------------------------------------------------
constexpr int CP_BLOCK = 256;
constexpr int CP_ITEMS = 4;                        // consecutive rows per thread
constexpr int CP_TILE = CP_BLOCK * CP_ITEMS;       // rows per block

__device__ __forceinline__ int tile_flags(const uint8_t* __restrict__ valid, long long n, long long base, bool f[CP_ITEMS]) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < CP_ITEMS; ++k) {
        f[k] = base + k < n && valid[base + k] != 0;
        c += (int)f[k];
    }
    return c;
}

// inclusive scan of one int per thread over the block (Hillis-Steele in LDS)
__device__ __forceinline__ int block_inclusive_scan(int v, int* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < CP_BLOCK; off <<= 1) {
        const int add = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    return sh[threadIdx.x];
}

__global__ __launch_bounds__(CP_BLOCK) void compact_count_kernel(const uint8_t* __restrict__ valid, long long n,
                                                                 long long* __restrict__ block_off) {
    __shared__ int sh[CP_BLOCK];
    bool f[CP_ITEMS];
    const int c = tile_flags(valid, n, (long long)blockIdx.x * CP_TILE + (long long)threadIdx.x * CP_ITEMS, f);
    const int incl = block_inclusive_scan(c, sh);
    if (threadIdx.x == CP_BLOCK - 1) block_off[blockIdx.x] = incl;
}

// block_off[b] = number of valid rows in front of block b (in place, from the per-block counts); *n_valid = their total.
// ONE block: every thread sums a contiguous run of block counts, the 256 run sums are scanned, the runs are rewritten.
__global__ __launch_bounds__(CP_BLOCK) void compact_scan_kernel(long long* __restrict__ block_off, long long nb,
                                                                long long* __restrict__ n_valid) {
    __shared__ long long sh[CP_BLOCK];
    const long long per = (nb + CP_BLOCK - 1) / CP_BLOCK;
    const long long lo = (long long)threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    long long sum = 0;
    for (long long i = lo; i < hi; ++i) sum += block_off[i];
    sh[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < CP_BLOCK; off <<= 1) {
        const long long add = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    long long run = sh[threadIdx.x] - sum;             // exclusive
    for (long long i = lo; i < hi; ++i) {
        const long long c = block_off[i];
        block_off[i] = run;
        run += c;
    }
    if (threadIdx.x == CP_BLOCK - 1) *n_valid = sh[CP_BLOCK - 1];
}

__global__ __launch_bounds__(CP_BLOCK) void compact_scatter_kernel(const uint8_t* __restrict__ valid, long long n,
                                                                   const long long* __restrict__ block_off,
                                                                   long long* __restrict__ valid_list) {
    __shared__ int sh[CP_BLOCK];
    bool f[CP_ITEMS];
    const long long base = (long long)blockIdx.x * CP_TILE + (long long)threadIdx.x * CP_ITEMS;
    const int c = tile_flags(valid, n, base, f);
    const int incl = block_inclusive_scan(c, sh);
    long long pos = block_off[blockIdx.x] + (incl - c);        // pos + c <= number of valid rows <= n: inside valid_list
#pragma unroll
    for (int k = 0; k < CP_ITEMS; ++k)
        if (f[k]) valid_list[pos++] = base + k;
}

__global__ __launch_bounds__(256) void perm_repair_kernel(const long long* __restrict__ perm, long long len,
                                                          const uint8_t* __restrict__ valid, long long R,
                                                          const long long* __restrict__ valid_list,
                                                          const long long* __restrict__ n_valid, long long* __restrict__ out) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= len) return;
    const long long p = perm[j], nv = *n_valid;
    long long r = p;
    // (an entry outside [0, R) names no row of the record and no valid row can stand in for all rows when there is none: both pass through)
    if (p >= 0 && p < R && nv > 0 && nv <= R && valid[p] == 0) r = valid_list[p % nv];
    out[j] = r;
}

}  // namespace

extern "C" int dtc_rows_finite(const float* const* mats, const int64_t* widths, int count, int64_t R, uint8_t* row_valid,
                               void* stream) {
    DTC_REQUIRE(count >= 1 && count <= MAX_MATS, "rows_finite: %d matrices (1..%d)", count, MAX_MATS);
    DTC_REQUIRE(mats && widths && row_valid, "rows_finite: null pointer");
    DTC_REQUIRE(R >= 0, "rows_finite: bad row count R=%lld", (long long)R);
    for (int i = 0; i < count; ++i) {
        DTC_REQUIRE(mats[i] != nullptr, "rows_finite: matrix %d is a null pointer", i);
        DTC_REQUIRE(widths[i] >= 1, "rows_finite: matrix %d has width w=%lld (w >= 1)", i, (long long)widths[i]);
        DTC_REQUIRE((reinterpret_cast<uintptr_t>(mats[i]) & 3u) == 0, "rows_finite: matrix %d is not 4-byte aligned", i);
        DTC_REQUIRE(widths[i] <= (int64_t)1 << 40 && R <= ((int64_t)1 << 60) / widths[i], "rows_finite: matrix %d: R * w overflows", i);
    }
    if (R == 0) return DTC_OK;
    ScanArgs A;
    A.count = count;
    int blocks = 0;
    double bytes = 0.0;
    for (int i = 0; i < count; ++i) {
        ScanMat& m = A.m[i];
        m.ptr = mats[i];
        m.w = widths[i];
        m.total = R * widths[i];
        const long long to16 = (long long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(mats[i]) & 15u)) & 15u) / 4u);
        m.head = (int)(to16 < m.total ? to16 : m.total);
        m.nvec = (m.total - m.head) / 4;
        m.blk0 = blocks;
        const long long want = dtc::ceil_div(m.nvec, (long long)SCAN_BLOCK * 4);     // four groups per lane and pass
        blocks += (int)(want < 1 ? 1 : (want < SCAN_BLOCKS_PER_MAT ? want : SCAN_BLOCKS_PER_MAT));
        bytes += 4.0 * (double)m.total;
    }
    for (int i = count; i < MAX_MATS; ++i) A.m[i] = ScanMat{nullptr, 1, 0, 0, 0, blocks};
    hipStream_t s = (hipStream_t)stream;
    dtc::ProfScope prof("rows_finite", bytes, s, bytes);
    hipLaunchKernelGGL(rows_finite_kernel, dim3(blocks), dim3(SCAN_BLOCK), 0, s, A, row_valid);
    return dtc::check_launch("rows_finite");
}

extern "C" int64_t dtc_compact_workspace(int64_t n) {
    return n < 0 ? 0 : (int64_t)sizeof(long long) * (dtc::ceil_div(n, CP_TILE) > 1 ? dtc::ceil_div(n, CP_TILE) : 1);
}

extern "C" int dtc_compact_valid(const uint8_t* row_valid, int64_t n, int64_t* valid_list, int64_t* n_valid, void* workspace,
                                 void* stream) {
    DTC_REQUIRE(row_valid && valid_list && n_valid && workspace, "compact_valid: null pointer");
    DTC_REQUIRE(n > 0 && dtc::ceil_div(n, CP_TILE) < ((int64_t)1 << 31), "compact_valid: bad row count n=%lld", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    const long long nb = dtc::ceil_div(n, CP_TILE);
    long long* block_off = (long long*)workspace;
    hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)nb), dim3(CP_BLOCK), 0, s, row_valid, (long long)n, block_off);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(CP_BLOCK), 0, s, block_off, nb, (long long*)n_valid);
    hipLaunchKernelGGL(compact_scatter_kernel, dim3((unsigned)nb), dim3(CP_BLOCK), 0, s, row_valid, (long long)n, block_off,
                       (long long*)valid_list);
    return dtc::check_launch("compact_valid");
}

extern "C" int dtc_perm_repair(const int64_t* perm, int64_t len, const uint8_t* row_valid, int64_t R, const int64_t* valid_list,
                               const int64_t* n_valid, int64_t* out, void* stream) {
    DTC_REQUIRE(len >= 0 && R >= 0, "perm_repair: bad shape len=%lld R=%lld", (long long)len, (long long)R);
    DTC_REQUIRE(perm && row_valid && valid_list && n_valid && out, "perm_repair: null pointer");
    if (len == 0) return DTC_OK;
    DTC_REQUIRE(dtc::ceil_div(len, 256) < ((int64_t)1 << 31), "perm_repair: len=%lld too large", (long long)len);
    hipLaunchKernelGGL(perm_repair_kernel, dim3((unsigned)dtc::ceil_div(len, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)perm, (long long)len, row_valid, (long long)R, (const long long*)valid_list,
                       (const long long*)n_valid, (long long*)out);
    return dtc::check_launch("perm_repair");
}
