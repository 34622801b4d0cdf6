// Env reset for gfx950: LeggedRobot.reset_idx (legged_gym/envs/base/legged_robot.py:200-272) with _update_terrain_curriculum
// (:690-711), _reset_dofs (:632-641), LeggedRobotDTC._reset_root_states (legged_robot_dtc.py:291-311), _resample_commands (:567-593),
// _randomize_dof_props (:465-481), the buffer clears and the extras["episode"] means, driven by reset_buf itself (dtc_env_reset,
// include/dtc_hip.h): no nonzero(), no host read, two launches whatever the mask.
//
// Launch 1, one 256-thread workgroup per 256 envs, thread t owns env n = 256 b + t:
//   * the block's offset into env_ids is the popcount of the reset_buf bytes in front of it (<= 32 KB at 32768 envs, L2-resident; N is capped at 2^18,
//     recomputed by every block: no scan across blocks, no dependence on dispatch order); ranks inside the block come from ballots,
//     so env_ids is ascending;
//   * the terrain curriculum of its env (reads the pre-reset root_states / env_origins / commands that launch 2 overwrites) and its
//     column of episode_sums [n_sums, N] (coalesced): read, zeroed;
//   * per-block float64 partials (one per episode-sum row, the terrain-level sum, the count) go to the workspace: xor-butterflies
//     inside a wavefront, the four wavefronts added in order.
// Launch 2, one wavefront per env (4 per workgroup, as csrc/rewards.hip): the wavefront of an env that resets writes its rows (dofs,
// root state, commands, dof props, height-noise row, the clear tables), lanes along the row, every load ahead of the first store;
// the others read one flag byte and leave.  Workgroup 0 also folds the partials over the blocks in order and writes the means and
// the count.  The kernel boundary is the only cross-block synchronisation; every store is an ordinary vector store.
//
// Latency bound: 1-2 KB written per reset env, one flag byte read per other env.  -ffp-contract=off (build.py): every fp32
// operation of the reference expressions is rounded once, in the reference's operand order.
#include "common.hpp"
#include "philox.hpp"

namespace {

struct Span { float span, lo; };            // a range [lo, hi] as the reference's fp32 scalars: float32(hi - lo), float32(lo)

struct ResetK {
    int D, B, C, P, S;
    int curriculum, init_done, custom_origins, heading, play, rnd_strength, rnd_kp, rnd_kd;
    int max_level, t_rows, t_cols;
    float move_up_distance, episode_length_s_f, height_noise;
    double episode_length_s;
    float base_init[13];
    Span origin, cmd_x, cmd_y, cmd_third, strength, kp, kd;
    unsigned seed_lo, seed_hi, ctr_lo, ctr_hi;
    int nblocks;
};

// draw `slot` of env n: the caller's u[n, slot], or word slot & 3 of Philox(counter = (n, slot >> 2, call counter), key = seed)
__device__ __forceinline__ float draw(const DtcResetStep& s, const ResetK& k, int n, int slot) {
    if (s.u) return s.u[(long long)n * k.S + slot];
    const U4 x = philox4x32_10(U4{(unsigned)n, (unsigned)(slot >> 2), k.ctr_lo, k.ctr_hi}, k.seed_lo, k.seed_hi);
    const unsigned w = (slot & 2) ? ((slot & 1) ? x.w : x.z) : ((slot & 1) ? x.y : x.x);
    return (float)(w >> 8) * 5.9604644775390625e-08f;                              // [0, 1): 24 uniform bits
}

__device__ __forceinline__ long long draw_level(const DtcResetStep& s, const ResetK& k, int n) {
    if (s.level_draw) return s.level_draw[n];
    const U4 x = philox4x32_10(U4{(unsigned)n, 0xFFFFFFFFu, k.ctr_lo, k.ctr_hi}, k.seed_lo, k.seed_hi);
    return (long long)(x.x % (unsigned)k.max_level);
}

__device__ __forceinline__ double wave_sum_f64(double v) {                         // xor-butterfly, fixed order
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// zero `bytes` bytes at p with the 64 lanes of a wavefront: words when pointer and length allow it, bytes otherwise
__device__ __forceinline__ void wave_clear(void* p, int bytes, int lane) {
    if (((reinterpret_cast<uintptr_t>(p) | (uintptr_t)bytes) & 3u) == 0) {
        uint32_t* q = static_cast<uint32_t*>(p);
        for (int i = lane; i < (bytes >> 2); i += 64) q[i] = 0u;
    } else {
        uint8_t* q = static_cast<uint8_t*>(p);
        for (int i = lane; i < bytes; i += 64) q[i] = 0;
    }
}

// Launch 1: flags -> env_ids, the terrain curriculum and the episode-sum column of this thread's env, the block's partial sums.
__global__ __launch_bounds__(256) void env_reset_scan_kernel(const DtcResetStep s, const ResetK k, int N) {
    __shared__ int wave_cnt[4], wave_before[4];
    __shared__ double red[DTC_RESET_MAX_SUMS + 2][4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int base = blockIdx.x * 256;
    const int n = base + t;

    // reset flags in front of this block (bytes [0, base) of reset_buf): words where aligned, at most 3 + 3 single bytes
    int before = 0;
    {
        const uint8_t* p = s.reset_buf;
        const int head = min(base, (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 3u)) & 3u));
        const int nw = (base - head) >> 2;
        const uint32_t* pw = reinterpret_cast<const uint32_t*>(p + head);
        for (int i = t; i < nw; i += 256) {
            const uint32_t v = pw[i];
            before += __popc((((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u);        // bytes != 0
        }
        const int tail = head + 4 * nw;
        if (t < head) before += p[t] != 0;
        if (tail + t < base) before += p[tail + t] != 0;
    }
    before = wave_sum_i32(before);
    const bool f = n < N && s.reset_buf[n] != 0;
    const unsigned long long m = __ballot(f);
    if (lane == 0) {
        wave_cnt[w] = __popcll(m);
        wave_before[w] = before;
    }
    __syncthreads();
    const int offset = ((wave_before[0] + wave_before[1]) + wave_before[2]) + wave_before[3];
    const int total = ((wave_cnt[0] + wave_cnt[1]) + wave_cnt[2]) + wave_cnt[3];
    int rank = __popcll(m & ((1ull << lane) - 1ull));
    for (int i = 0; i < w; ++i) rank += wave_cnt[i];
    if (f) s.env_ids[offset + rank] = n;                                           // ascending: what nonzero() gives

    // 1. _update_terrain_curriculum (:690-711) of this thread's env, from its pre-reset root state, origin and commands (launch 2
    //    overwrites them); the new origin is what launch 2 adds to the root state
    long long level = 0;
    if (k.curriculum && n < N) level = s.terrain_levels[n];
    if (f && k.curriculum && k.init_done) {
        float* o = s.env_origins + (long long)n * 3;
        const float* r = s.root_states + (long long)n * 13;
        const float* c = s.commands + (long long)n * k.C;
        const float dx = r[0] - o[0], dy = r[1] - o[1];
        const float dist = sqrtf(dx * dx + dy * dy);
        const bool up = dist > k.move_up_distance;
        const float cn = sqrtf(c[0] * c[0] + c[1] * c[1]);
        const bool down = (dist < cn * k.episode_length_s_f * 0.5f) && !up;
        level = level + (up ? 1 : 0) - (down ? 1 : 0);
        level = level >= k.max_level ? draw_level(s, k, n) : (level < 0 ? 0 : level);
        s.terrain_levels[n] = level;
        // the table index is clamped for the address only (a level_draw outside [0, rows) must not read outside the table)
        const long long ty = s.terrain_types[n];
        const int li = (int)(level < 0 ? 0 : (level >= k.t_rows ? k.t_rows - 1 : level));
        const int ti = (int)(ty < 0 ? 0 : (ty >= k.t_cols ? k.t_cols - 1 : ty));
        const float* src = s.terrain_origins + ((long long)li * k.t_cols + ti) * 3;
        const float ox = src[0], oy = src[1], oz = src[2];
        o[0] = ox, o[1] = oy, o[2] = oz;
    }

    // 8. per-block float64 partials: episode sums of the reset envs (read, then zeroed), terrain levels of all envs, the count
    for (int r = 0; r < s.n_sums; ++r) {
        double v = 0.0;
        if (total > 0) {
            if (f) {
                float* e = s.episode_sums + (long long)r * N + n;
                v = (double)*e;
                *e = 0.f;
            }
            v = wave_sum_f64(v);
        }
        if (lane == 0) red[r][w] = v;
    }
    {
        const double lv = wave_sum_f64((k.curriculum && n < N) ? (double)(float)level : 0.0);
        if (lane == 0) {
            red[s.n_sums][w] = lv;
            red[s.n_sums + 1][w] = (double)wave_cnt[w];
        }
    }
    __syncthreads();
    if (t < s.n_sums + 2)
        static_cast<double*>(s.workspace)[(long long)blockIdx.x * (s.n_sums + 2) + t] = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
}

// 2-7 for one env, by one wavefront, lanes along the rows.  Every load is issued before the first store: the work of one env is a
// handful of memory latencies, not one per tensor.
__device__ __forceinline__ void reset_rows(const DtcResetStep& s, const ResetK& k, int N, int en, int lane) {
    const long long e = en;
    const int D = k.D, C = k.C;
    const bool dof = lane < D, vel = lane >= 7 && lane < 13, xy = lane < 2 && k.custom_origins;
    float u_dof = 0.f, dflt = 0.f, u_root = 0.f, org = 0.f, u_x = 0.f, u_y = 0.f, u_th = 0.f, u_ms = 0.f, u_kp = 0.f, u_kd = 0.f;
    if (dof) {
        u_dof = draw(s, k, en, lane);
        dflt = s.default_dof_pos[lane];
        if (k.rnd_strength) u_ms = draw(s, k, en, D + 11);
        if (k.rnd_kp) u_kp = draw(s, k, en, D + 12);
        if (k.rnd_kd) u_kd = draw(s, k, en, D + 13);
    }
    if (xy || vel) u_root = draw(s, k, en, vel ? D + 2 + (lane - 7) : D + lane);
    if (lane < 3) org = s.env_origins[e * 3 + lane];                               // the NEW origin (launch 1)
    if (lane == 0) {
        u_x = draw(s, k, en, D + 8);
        u_y = draw(s, k, en, D + 9);
        u_th = draw(s, k, en, D + 10);
    }
    float* h = s.height_noise_offset ? s.height_noise_offset + e * k.P : nullptr;
    const bool h_regs = h && k.P <= 12 * 64;
    float hv[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) hv[i] = (h_regs && lane + 64 * i < k.P) ? h[lane + 64 * i] : 0.f;

    if (dof) {                                                                     // _reset_dofs, :640-641
        s.dof_pos[e * s.dof_pos_row_stride + lane * s.dof_pos_elem_stride] = dflt * (1.0f * u_dof + 0.5f);
        s.dof_vel[e * s.dof_vel_row_stride + lane * s.dof_vel_elem_stride] = 0.f;
        // _randomize_dof_props, :465-481 (u * (max - min) + min)
        if (k.rnd_strength) s.motor_strengths[e * D + lane] = u_ms * k.strength.span + k.strength.lo;
        if (k.rnd_kp) s.Kp_factors[e * D + lane] = u_kp * k.kp.span + k.kp.lo;
        if (k.rnd_kd) s.Kd_factors[e * D + lane] = u_kd * k.kd.span + k.kd.lo;
    }
    if (lane < 13) {                                                               // _reset_root_states, dtc.py:299-311
        float v = k.base_init[lane];
        if (lane < 3) v = v + org;
        if (xy) v = v + (k.origin.span * u_root + k.origin.lo);
        if (vel) v = 1.0f * u_root + -0.5f;
        s.root_states[e * 13 + lane] = v;
    }
    if (lane == 0) {                                                               // _resample_commands, :573-591
        float* c = s.commands + e * C;
        float x = k.cmd_x.span * u_x + k.cmd_x.lo;
        float y = k.cmd_y.span * u_y + k.cmd_y.lo;
        float th = k.cmd_third.span * u_th + k.cmd_third.lo;
        if (k.play) x = 0.5f, y = 0.0f, th = 0.0f;
        c[k.heading ? 3 : 2] = th;
        const float keep = sqrtf(x * x + y * y) > 0.1f ? 1.f : 0.f;
        c[0] = x * keep;
        c[1] = y * keep;
    }
    if (s.forces) wave_clear(s.forces + e * k.B * 3, k.B * 12, lane);              // :592
    if (h_regs) {                                                                  // :229-230
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (lane + 64 * i < k.P) h[lane + 64 * i] = hv[i] * 0.0f + k.height_noise;
    } else if (h) {
        for (int p = lane; p < k.P; p += 64) h[p] = h[p] * 0.0f + k.height_noise;
    }
    for (int j = 0; j < s.n_rows; ++j)                                             // :233-251, :267-268
        wave_clear(static_cast<uint8_t*>(s.rows[j].ptr) + e * s.rows[j].row_bytes, s.rows[j].row_bytes, lane);
    for (int j = 0; j < s.n_time_rows; ++j) {                                      // :270-272
        const int rb = s.time_rows[j].row_bytes;
        for (int tt = 0; tt < s.time_rows[j].T; ++tt)
            wave_clear(static_cast<uint8_t*>(s.time_rows[j].ptr) + ((long long)tt * N + e) * rb, rb, lane);
    }
}

// Launch 2: one wavefront per env (4 per workgroup) writes the rows of the envs that reset; workgroup 0 also folds the partials of
// launch 1 over the blocks, in order, and writes the means and the count.
__global__ __launch_bounds__(256) void env_reset_rows_kernel(const DtcResetStep s, const ResetK k, int N) {
    __shared__ double count_s;
    const int t = threadIdx.x;
    const int n = blockIdx.x * 4 + (t >> 6);
    if (n < N && s.reset_buf[n] != 0) reset_rows(s, k, N, n, t & 63);
    if (blockIdx.x != 0) return;
    const int cols = s.n_sums + 2;
    double acc = 0.0;
    if (t < cols) {
        const double* ws = static_cast<const double*>(s.workspace);
#pragma unroll 8
        for (int b = 0; b < k.nblocks; ++b) acc = acc + ws[(long long)b * cols + t];
    }
    if (t == cols - 1) {
        count_s = acc;
        *s.count = (int)acc;
    }
    __syncthreads();
    const double count = count_s;
    if (count == 0.0) return;                                                      // :210-211: extras["episode"] stays as it was
    if (t < s.n_sums) s.episode_means[t] = (float)((acc / count) / k.episode_length_s);           // :255
    if (t == s.n_sums && k.curriculum) *s.terrain_level_mean = (float)(acc / (double)N);          // :259
}

Span span_of(const double r[2]) { return Span{(float)(r[1] - r[0]), (float)r[0]}; }

}  // namespace

extern "C" int64_t dtc_env_reset_workspace(int N, int n_sums) {
    if (N <= 0 || n_sums < 0 || n_sums > DTC_RESET_MAX_SUMS) return -1;
    return dtc::ceil_div(N, 256) * (int64_t)(n_sums + 2) * (int64_t)sizeof(double);
}

extern "C" int dtc_env_reset_abi_sizes(int64_t* out, int cap) {
    const int64_t sz[] = {sizeof(DtcResetRows), sizeof(DtcResetCfg), sizeof(DtcResetStep)};
    for (int i = 0; i < 3 && i < cap && out; ++i) out[i] = sz[i];
    return 3;
}

extern "C" int dtc_env_reset(const DtcResetStep* st, const DtcResetCfg* cfg, int N, void* stream) {
    DTC_REQUIRE(st && cfg, "null descriptor");
    DTC_REQUIRE(N > 0 && N <= (1 << 18), "N %d outside 1..2^18", N);
    const DtcResetStep& s = *st;
    const DtcResetCfg& c = *cfg;
    DTC_REQUIRE(c.num_dof >= 1 && c.num_dof <= 64, "num_dof %d outside 1..64", c.num_dof);
    DTC_REQUIRE(c.num_commands >= (c.heading_command ? 4 : 3), "num_commands %d", c.num_commands);
    DTC_REQUIRE(s.n_sums >= 0 && s.n_sums <= DTC_RESET_MAX_SUMS, "n_sums %d outside 0..%d", s.n_sums, DTC_RESET_MAX_SUMS);
    DTC_REQUIRE(s.n_rows >= 0 && s.n_rows <= DTC_RESET_MAX_ROWS, "%d row items (at most %d)", s.n_rows, DTC_RESET_MAX_ROWS);
    DTC_REQUIRE(s.n_time_rows >= 0 && s.n_time_rows <= DTC_RESET_MAX_TIME_ROWS, "%d time-major items (at most %d)", s.n_time_rows,
                DTC_RESET_MAX_TIME_ROWS);
    DTC_REQUIRE(s.reset_buf && s.env_ids && s.count && s.workspace, "reset_buf / env_ids / count / workspace");
    DTC_REQUIRE((reinterpret_cast<uintptr_t>(s.workspace) & 7u) == 0, "workspace must be 8-byte aligned");
    DTC_REQUIRE(s.dof_pos && s.dof_vel && s.default_dof_pos && s.root_states && s.env_origins && s.commands, "dof / root / command tensors");
    // strided dof tensors: positive strides, rows that do not overlap
    DTC_REQUIRE(s.dof_pos_elem_stride >= 1 && s.dof_pos_row_stride >= (c.num_dof - 1) * s.dof_pos_elem_stride + 1 &&
                s.dof_vel_elem_stride >= 1 && s.dof_vel_row_stride >= (c.num_dof - 1) * s.dof_vel_elem_stride + 1, "dof_pos / dof_vel strides");
    DTC_REQUIRE(s.n_sums == 0 || (s.episode_sums && s.episode_means), "episode_sums / episode_means");
    const bool levels = c.terrain_curriculum != 0;
    DTC_REQUIRE(!levels || (s.terrain_levels && s.terrain_level_mean), "terrain_levels / terrain_level_mean");
    DTC_REQUIRE(!(levels && c.init_done) || (s.terrain_origins && s.terrain_types && c.max_terrain_level >= 1 && c.terrain_rows >= 1 &&
                                             c.terrain_cols >= 1), "terrain curriculum inputs");
    DTC_REQUIRE(!c.randomize_motor_strength || s.motor_strengths, "motor_strengths");
    DTC_REQUIRE(!c.randomize_kp || s.Kp_factors, "Kp_factors");
    DTC_REQUIRE(!c.randomize_kd || s.Kd_factors, "Kd_factors");
    DTC_REQUIRE(!s.forces || c.num_bodies >= 1, "num_bodies %d", c.num_bodies);
    DTC_REQUIRE(!s.height_noise_offset || c.num_points >= 1, "num_points %d", c.num_points);
    for (int i = 0; i < s.n_rows; ++i) DTC_REQUIRE(s.rows[i].ptr && s.rows[i].row_bytes > 0, "row item %d", i);
    for (int i = 0; i < s.n_time_rows; ++i)
        DTC_REQUIRE(s.time_rows[i].ptr && s.time_rows[i].row_bytes > 0 && s.time_rows[i].T > 0, "time-major item %d", i);

    ResetK k{};
    k.D = c.num_dof, k.B = c.num_bodies, k.C = c.num_commands, k.P = c.num_points, k.S = c.num_dof + DTC_RESET_FIXED_DRAWS;
    k.curriculum = levels, k.init_done = c.init_done != 0, k.custom_origins = c.custom_origins != 0;
    k.heading = c.heading_command != 0, k.play = c.play_command != 0;
    k.rnd_strength = c.randomize_motor_strength != 0, k.rnd_kp = c.randomize_kp != 0, k.rnd_kd = c.randomize_kd != 0;
    k.max_level = c.max_terrain_level, k.t_rows = c.terrain_rows, k.t_cols = c.terrain_cols;
    k.move_up_distance = c.move_up_distance;
    k.episode_length_s = c.max_episode_length_s, k.episode_length_s_f = (float)c.max_episode_length_s;
    k.height_noise = c.height_noise;
    for (int i = 0; i < 13; ++i) k.base_init[i] = c.base_init_state[i];
    k.origin = span_of(c.origin_xy), k.cmd_x = span_of(c.lin_vel_x), k.cmd_y = span_of(c.lin_vel_y);
    k.cmd_third = span_of(c.heading_command ? c.heading : c.ang_vel_yaw);
    k.strength = span_of(c.motor_strength), k.kp = span_of(c.kp_range), k.kd = span_of(c.kd_range);
    k.seed_lo = (unsigned)c.seed, k.seed_hi = (unsigned)(c.seed >> 32), k.ctr_lo = (unsigned)c.counter, k.ctr_hi = (unsigned)(c.counter >> 32);
    k.nblocks = (int)dtc::ceil_div(N, 256);

    hipStream_t hs = (hipStream_t)stream;
    {
        dtc::ProfScope prof("env_reset_scan", (double)N * (1.0 + 4.0 * s.n_sums), hs);
        hipLaunchKernelGGL(env_reset_scan_kernel, dim3((unsigned)k.nblocks), dim3(256), 0, hs, s, k, N);
        const int rc = dtc::check_launch("env_reset_scan");
        if (rc != DTC_OK) return rc;
    }
    dtc::ProfScope prof("env_reset_rows", (double)N, hs);
    hipLaunchKernelGGL(env_reset_rows_kernel, dim3((unsigned)dtc::ceil_div(N, 4)), dim3(256), 0, hs, s, k, N);
    return dtc::check_launch("env_reset_rows");
}
