// What the three weight-gradient families (csrc/wgrad.hip: fp32 MFMA, csrc/wgrad_s3.hip: bf16 x 3 / two-term fp16, csrc/wgrad_h2i.hip:
// operand images) share -- everything that is not arithmetic.  dW[N,K] = dZ[M,N]^T X[M,K] reduces over the mini-batch while the output
// is small, so every family cuts the batch into slices: workgroup (slice, tile) writes the partial product of its slice into a slab, a
// reduce kernel adds the slabs in a fixed order (deterministic, no atomics).  Here, once:
//   device: workgroup -> (slice, tile) | tile -> (job, tile of the job) | column tile -> (segment of X, tile of the segment) | the two
//           slab sums (fp32 rows with the bias column; 128 x 128 slab tiles);
//   host:   the slice-count rule with each family's constants, the walk over a group's jobs (tile sums), the slab layout in the
//           workspace with the flop / byte bookkeeping, the partial + reduce launch pair.
// tests/test_wgrad_plan_host.py pins the host half through the workspace sizes, without a GPU.
#pragma once
#include "gemm_core.hpp"

namespace {

constexpr int WGRAD_MAX_JOBS = 12;          // layers per grouped launch (the group structs travel as kernel arguments)

// ---- device: index maps ----------------------------------------------------------------------------------------------------------
// Workgroup b runs on XCD b % 8 and takes batch slice xcd + 8 * (b / 8 / tiles), tile (b / 8) % tiles: every XCD owns whole slices, so
// each slice of dZ / X is pulled from HBM into ONE L2 and shared there by all output tiles of all layers (dZ of layer l is X-adjacent
// data of layer l - 1).  The grid (wgrad_grid) holds whole groups of eight slices; false: a padding workgroup of the last group.
__device__ __forceinline__ bool slice_tile(int tiles, int splits, int& split, int& t) {
    const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
    split = xcd + 8 * (jb / tiles);
    t = jb % tiles;
    return split < splits;
}

// Position `t` in the running sums end(job[0]) <= end(job[1]) <= ... of a group -> (job, position inside the job)
struct JobPos {
    int j, t;
};
template <class Group, class End>
__device__ __forceinline__ JobPos job_pos(const Group& G, int t, End end) {
    int j = 0;
    while (j < G.count - 1 && t >= end(G.job[j])) ++j;
    if (j > 0) t -= end(G.job[j - 1]);
    return {j, t};
}
template <class Group>
__device__ __forceinline__ JobPos tile_job(const Group& G, int t) {
    return job_pos(G, t, [](const auto& J) { return J.tile_end; });
}
// tiles of job j = slab tiles per batch slice.  (Asked for where it is used: held across the K loop of wgrad_s3_group_kernel it cost
// two registers, 170 instead of 168 = two instead of three workgroups per CU)
template <class Group>
__host__ __device__ __forceinline__ int job_tiles(const Group& G, int j) {
    return G.job[j].tile_end - (j > 0 ? G.job[j - 1].tile_end : 0);
}

// Column tiles are aligned to the segments of X, so every workgroup reads ONE source matrix: column tile tc of `width` columns ->
// (segment, tile inside the segment)
struct SegTile {
    int seg, tc;
};
__device__ __forceinline__ SegTile seg_tile(const SegMatDev& X, int tc, int width) {
    int seg = 0;
    for (; seg < X.nseg - 1; ++seg) {
        const int nt = (X.s[seg].width + width - 1) / width;
        if (tc < nt) break;
        tc -= nt;
    }
    return {seg, tc};
}

// ---- device: the slab sums -------------------------------------------------------------------------------------------------------
// fp32 family: part[slice][n][part_ld(K)], column K = the bias-gradient partial.  Workgroup = 64 float4 columns (lane) x G slice groups:
// group g adds slices g, g + G, g + 2 G, ... (4 loads in flight), the groups are then added in order 0..G-1 through LDS.
template <int G>
__device__ __forceinline__ void reduce_row(const float* __restrict__ part, float* __restrict__ dW, float* __restrict__ db, int N, int K,
                                           int splits, int n, int c4, int g, int lane, float4 (*red)[64]) {
    const int ldp = part_ld(K);
    const long long total = (long long)N * ldp;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 * 4 < ldp) {
        const float4* p = reinterpret_cast<const float4*>(part + (long long)n * ldp) + c4;
        const long long step = total / 4;
        int s = g;
        for (; s + 3 * G < splits; s += 4 * G) {
            const float4 v0 = p[(long long)s * step], v1 = p[(long long)(s + G) * step];
            const float4 v2 = p[(long long)(s + 2 * G) * step], v3 = p[(long long)(s + 3 * G) * step];
            acc.x = (((acc.x + v0.x) + v1.x) + v2.x) + v3.x;
            acc.y = (((acc.y + v0.y) + v1.y) + v2.y) + v3.y;
            acc.z = (((acc.z + v0.z) + v1.z) + v2.z) + v3.z;
            acc.w = (((acc.w + v0.w) + v1.w) + v2.w) + v3.w;
        }
        for (; s < splits; s += G) {
            const float4 v = p[(long long)s * step];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    red[g][lane] = acc;
    __syncthreads();
    if (g == 0 && c4 * 4 < ldp) {
        for (int j = 1; j < G; ++j) {
            const float4 v = red[j][lane];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        const float out[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = c4 * 4 + i;
            if (c < K) dW[(long long)n * K + c] = out[i];
            else if (c == K && db) db[n] = out[i];
        }
    }
}

// 128 x 128 families: part[slice][tile of the job][128][128].  Workgroup b = (tile b / 16, 8 slab rows); thread = (slab row, float4 of
// slab columns).  The slices are added one after the other from 0, U loads in flight: the bits do not depend on U.  row_of: slab row ->
// row of the tile (the slabs of wgrad_s3.hip are in physical order); store(J, n, tc, c4, sum): the four columns 4 c4 .. of tile column tc.
template <int U, class Group, class RowOf, class Store>
__device__ __forceinline__ void reduce_slab_rows(const Group& G, int b, RowOf row_of, Store store) {
    constexpr int TILE = 128;
    const JobPos jp = tile_job(G, b >> 4);
    const int tiles_j = job_tiles(G, jp.j);
    const auto& J = G.job[jp.j];
    const int tr = jp.t / J.col_tiles, tc = jp.t - tr * J.col_tiles;
    const int pr = (b & 15) * 8 + (threadIdx.x >> 5), c4 = threadIdx.x & 31;
    const int n = tr * TILE + row_of(pr);
    if (n >= J.N) return;
    const f32x4* p = reinterpret_cast<const f32x4*>(J.part + (long long)jp.t * (TILE * TILE) + (long long)pr * TILE) + c4;
    const long long step = (long long)tiles_j * (TILE * TILE / 4);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int sp = 0;
    for (; sp + U - 1 < G.splits; sp += U) {
        f32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = p[(long long)(sp + u) * step];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += v[u][e];
    }
    for (; sp < G.splits; ++sp) {
        const f32x4 v0 = p[(long long)sp * step];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += v0[e];
    }
    store(J, n, tc, c4, acc);
}

// ---- host: how many batch slices ---------------------------------------------------------------------------------------------------
// target / tiles workgroups' worth of slices, in whole groups of eight (one slice per XCD: measured 10-20 % faster than filling the chip
// with an arbitrary count -- 44 tiles x 23 slices = 1012 workgroups ran slower than 44 x 16 = 704), at least 8, at most `cap` (0: none)
// and no more than leave min_rows batch rows per slice.
struct SliceRule {
    int target, cap, min_rows;
};
inline int wgrad_slices(int M, long long tiles, SliceRule r) {
    int s = (int)(r.target / (tiles > 0 ? tiles : 1)) / 8 * 8;
    if (s < 8) s = 8;
    if (r.cap > 0 && s > r.cap) s = r.cap;
    const int max_s = (int)dtc::ceil_div(dtc::ceil_div(M, r.min_rows), 8) * 8;
    if (s > max_s) s = max_s;
    return s;
}
// dtc_linear_wgrad, fp32 kernels: one layer per launch
constexpr SliceRule SLICES_LAYER = {1024, 0, BK * 8};
// dtc_wgrad_group: one count for all jobs (every workgroup then reduces the same number of batch rows).  Sweep 1024 ... 4096 with
// bench.py: 3072 best (24 batch slices per layer)
constexpr SliceRule SLICES_GROUP = {3072, 0, BK * 8};
// dtc_wgrad_group_s3 / _h2.  768: eight batch slices for the 61..70-tile groups of the bench step.  Measured (tools/jobs/r3_sweep2.sh):
// 512..1536 within 0.5 % of each other in step time, 2048 (32 slices) no faster; the partial slabs are HBM traffic written and read
// once per slice, so the smallest count that still fills the chip wins (family traffic 1.30 -> 1.15 x the algorithmic bytes).
// (Round 4, two-term fp16 kernels -- half the matrix work per workgroup: 1536 = 24 slices for the 61..64-tile groups, 16 for the
// 70-tile one: 57.4 vs 60.2 ms per step; 2048 / 3072 with a higher cap: 59.7 / 61.0 vs 59.1 on another box.)  The cap bounds the slab
// traffic of small groups (64 KiB per tile and slice, written and re-read).
constexpr SliceRule SLICES_S3 = {1536, 24, BK * 8};
// What dtc_linear_wgrad_workspace assumes of a one-layer launch of that family (csrc/wgrad.hip: s3_one_layer_bound)
constexpr SliceRule SLICES_S3_ONE_LAYER = {2048, 0, 16 * 8};
// dtc_wgrad_group_h2i.  768 (round 5; 8 batch slices for the 61..70-tile buckets of the bench step): with both operands arriving by
// LDS-DMA the slices need not be short to hide their loads -- 1024 / 1536 / 2048 workgroups: 50.3 / 50.1 / 50.2 ms per step on one
// box, 512 / 768 / 1024: 46.67 / 46.70 / 46.94 on another (interleaved pairs; round 4's converting kernel wanted 1536) -- and a third
// of the partial slabs is a third of the reduce traffic (again on round 6's kernel: 8 / 16 / 24 slices 46.3 / 46.8 / 47.2 ms per step,
// three interleaved rounds).  A slice holds at least one 128-row exponent block.
constexpr SliceRule SLICES_H2I = {768, 24, 128};

// ---- host: the plan of a grouped launch ------------------------------------------------------------------------------------------
// Group: {count, M, rows_per_split, splits, tiles_total, job[WGRAD_MAX_JOBS]}, every job with N, K, part and tile_end
template <class Group>
struct WgradPlan {
    Group dev;
    long long bytes;           // of the workspace
    int red_blocks;
    double flop, algo_bytes;   // algo_bytes: dZ, X read once, dW + db written once (the partial slabs are overhead)
};

// Pass 1: describe(j, host job, device job, tiles of the job) fills the operand descriptors of job j.  Sets the tile sums, then the slice
// count by `rule` and the slice length, a multiple of `row_step` batch rows.
template <class Group, class HostJob, class Describe>
int plan_jobs(Group& G, const HostJob* jobs, int count, int M, SliceRule rule, int row_step, Describe describe) {
    DTC_REQUIRE(jobs != nullptr && count >= 1 && count <= WGRAD_MAX_JOBS, "job count %d outside 1..%d", count, WGRAD_MAX_JOBS);
    DTC_REQUIRE(M > 0, "bad M=%d", M);
    G.count = count;
    G.M = M;
    int tiles = 0;
    for (int j = 0; j < count; ++j) {
        int tiles_j = 0;
        const int rc = describe(j, jobs[j], G.job[j], tiles_j);
        if (rc != DTC_OK) return rc;
        tiles += tiles_j;
        G.job[j].tile_end = tiles;
    }
    G.tiles_total = tiles;
    G.splits = wgrad_slices(M, tiles, rule);
    G.rows_per_split = (int)dtc::ceil_div(dtc::ceil_div(M, G.splits), row_step) * row_step;
    return DTC_OK;
}

// Pass 2: the slabs of every job, one behind the other in the workspace (null: sizes only).  slabs(device job, tiles of the job, take):
// take(bytes) hands out the next slab, 16-byte aligned.  Returns the offset behind the last slab.
template <class Plan, class Slabs>
long long plan_slabs(Plan& P, void* workspace, Slabs slabs) {
    auto& G = P.dev;
    long long off = 0;
    auto take = [&](long long bytes) {
        float* p = workspace ? (float*)((char*)workspace + off) : nullptr;
        off += (bytes + 15) & ~15ll;
        return p;
    };
    P.flop = P.algo_bytes = 0.0;
    for (int j = 0; j < G.count; ++j) {
        auto& d = G.job[j];
        slabs(d, job_tiles(G, j), take);
        P.flop += 2.0 * G.M * (double)d.N * d.K;
        P.algo_bytes += 4.0 * ((double)G.M * d.N + (double)G.M * d.K + (double)d.N * (d.K + 1));
    }
    return off;
}

// what plan_group and plan_s3 ask of a DtcWgradJob alike, and the part of its device twin that does not depend on the family
inline int check_job(const DtcWgradJob& h, int j) {
    DTC_REQUIRE(h.N > 0 && h.K > 0 && h.lddz >= h.N, "job %d: bad shape N=%d K=%d lddz=%lld", j, h.N, h.K, (long long)h.lddz);
    DTC_REQUIRE(h.dZ && h.dW, "job %d: null pointer", j);
    return DTC_OK;
}
template <class Job>
int describe_job(const DtcWgradJob& h, Job& d, int M, int tile_cols, const char* who) {
    const int rc = to_dev(&h.X, d.X, h.K, false, M, who);
    if (rc != DTC_OK) return rc;
    d.dZ = h.dZ;
    d.lddz = h.lddz;
    d.dW = h.dW;
    d.db = h.db;
    d.N = h.N;
    d.K = h.K;
    d.col_tiles = 0;
    for (int i = 0; i < d.X.nseg; ++i) d.col_tiles += (int)dtc::ceil_div(d.X.s[i].width, tile_cols);
    return DTC_OK;
}

// whole groups of eight slices (slice_tile)
inline int wgrad_grid(int tiles, int splits) { return tiles * 8 * (int)dtc::ceil_div(splits, 8); }

// The launch pair of a grouped call under its two profiler scopes: partial(grid) and reduce() launch on stream s
template <class Plan, class Partial, class Reduce>
int wgrad_launch_pair(const Plan& P, hipStream_t s, const char* who, Partial partial, Reduce reduce) {
    const auto& G = P.dev;
    {
        dtc::ProfScope prof(dtc::prof_shape_name("linear_wgrad", G.M, G.tiles_total, G.count), P.flop, s, P.algo_bytes);
        partial(wgrad_grid(G.tiles_total, G.splits));
    }
    {
        dtc::ProfScope prof(dtc::prof_shape_name("wgrad_reduce", G.splits, G.tiles_total, G.count), (double)P.bytes + P.bytes / (double)G.splits, s);
        reduce();
    }
    return dtc::check_launch(who);
}

}  // namespace
