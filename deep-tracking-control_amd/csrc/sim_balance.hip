// Support-polygon balance and falls of the surrogate legged env for gfx950 (opt-in): dtc_sim_balance, a launch of its own that runs
// directly behind dtc_sim_step* (csrc/sim.hip) and in front of dtc_sim_contacts, on what the step wrote, once per env step.
// include/dtc_hip.h states every operation and its order (B1..B9), tests/sim_balance_oracle.py restates them in numpy float32 bit
// for bit.  A point-mass inverted pendulum about the edge of the support polygon of the stance feet: a lean vector p (world frame,
// radians) and its rate per env, accelerated away from the support when the base's xy lies outside it, restored when inside, and
// laid over the base's attitude, height and angular velocity as the step wrote them.  |p| > fall_angle is a fall: the base row
// of contact_forces takes fall_force and check_termination ends the episode.
//
// What it is NOT: an overlay, not attitude dynamics.  The link positions are not rotated (feet and hips stay where the step put
// them, so the planner and dtc_sim_contacts see the un-leaned positions; only the knee of dtc_sim_contacts, which that launch turns
// with base_quat, follows the lean), pushes do not feed the lean rate, there is no
// friction and no slipping pivot, crossed feet are neglected (the stance feet are taken in the fixed order FL, FR, HR, HL), and
// control types "V" / "T" and `forces` stay absent.  Every constant is a free choice, fitted to nothing.
//
// Not a ninth template axis of sim_step_kernel: that kernel's eight instantiations stand at up to 99 VGPRs with SGPR spills, and
// the lean is integrated once per env step, after the last substep.
//
// One lane per env, 64-thread workgroups (one wavefront each, so 4096 envs spread over 64 CUs): an env is ~40 values in and ~40
// out with a few hundred flops between, and no value is shared between lanes.  No LDS, no atomics, no scratch: the packing of the
// stance feet and the edge loop are unrolled with constant indices, so the four points stay in registers.  Every store is a
// per-lane vector store.  Latency bound: ~0.3 KB read and ~0.2 KB written per env.
// -ffp-contract=off (build.py): every value is one single-rounded fp32 operation in the stated order; no libm call (sqrtf is the
// correctly rounded v_sqrt sequence, as in csrc/sim.hip).
//
// Resources (compiler resource-usage remarks, gfx950): VGPRs / SGPRs / SGPRs spilled / scratch
//   sim_balance_kernel  76 / 62 / 0 / 0
#include "common.hpp"

namespace {

struct BalK {
    float *root_states, *base_pos, *base_quat, *projected_gravity, *base_lin_vel, *base_ang_vel, *rigid_body_state, *contact_forces;
    const uint8_t* contact_filt;
    const long long* episode_length_buf;
    float* lean;
    uint8_t* fallen;
    int B, feet[4];
    float gravity, h_min, lean_eps, fall_angle, fall_force, dt, ox, oy;
};

// rot(q, v) of dtc_sim_contacts C1: t = 2 * (qv x v); c = qv x t; rot.i = (v.i + q.w * t.i) + c.i
__device__ __forceinline__ void rot(const float q[4], const float v[3], float o[3]) {
    const float tx = 2.0f * (q[1] * v[2] - q[2] * v[1]), ty = 2.0f * (q[2] * v[0] - q[0] * v[2]), tz = 2.0f * (q[0] * v[1] - q[1] * v[0]);
    const float cx = q[1] * tz - q[2] * ty, cy = q[2] * tx - q[0] * tz, cz = q[0] * ty - q[1] * tx;
    o[0] = (v[0] + q[3] * tx) + cx, o[1] = (v[1] + q[3] * ty) + cy, o[2] = (v[2] + q[3] * tz) + cz;
}

__global__ __launch_bounds__(64) void sim_balance_kernel(const BalK k, int N) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const long long e = n;
    float* rs = k.root_states + e * 13;
    float* rb = k.rigid_body_state + e * k.B * 13;
    float* cfz = k.contact_forces + e * k.B * 3 + 2;                               // the base row's z

    // ---- the env's rows, as the step just wrote them
    const float Bx = k.base_pos[e * 3], By = k.base_pos[e * 3 + 1], Bz = k.base_pos[e * 3 + 2];
    const float q[4] = {k.base_quat[e * 4], k.base_quat[e * 4 + 1], k.base_quat[e * 4 + 2], k.base_quat[e * 4 + 3]};
    const bool fresh = k.episode_length_buf[e] == 1;
    const float px = k.lean[e * 4], py = k.lean[e * 4 + 1], vx = k.lean[e * 4 + 2], vy = k.lean[e * 4 + 3];

    // B1. the stance feet in the order FL, FR, HR, HL, packed to the front
    float V[4][3] = {};
    int cnt = 0;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int l = o == 2 ? 3 : (o == 3 ? 2 : o);
        const bool s = k.contact_filt[e * 4 + l] != 0;
        const float* f = rb + (long long)k.feet[l] * 13;
        const float P[3] = {f[0], f[1], f[2]};
#pragma unroll
        for (int slot = 0; slot < 4; ++slot) {
            const bool put = s && cnt == slot;
#pragma unroll
            for (int i = 0; i < 3; ++i) V[slot][i] = put ? P[i] : V[slot][i];
        }
        cnt += s ? 1 : 0;
    }
    const int kc = cnt;

    // B2. the centre of mass over the ground
    const float ry = sqrtf(q[2] * q[2] + q[3] * q[3]);
    const float zy = q[2] / ry, wy = q[3] / ry;
    const float cy_ = 1.0f - 2.0f * (zy * zy), sy_ = 2.0f * (zy * wy);
    const float cx = Bx + (cy_ * k.ox - sy_ * k.oy);
    const float cyy = By + (sy_ * k.ox + cy_ * k.oy);

    // B3. the nearest boundary point, edge by edge, and the side of every edge the centre lies on
    float best = __builtin_inff(), nx = V[0][0], ny = V[0][1];
    float area = (V[1][0] - V[0][0]) * (V[2][1] - V[0][1]) - (V[1][1] - V[0][1]) * (V[2][0] - V[0][0]);
    {
        const float a2 = area + ((V[2][0] - V[0][0]) * (V[3][1] - V[0][1]) - (V[2][1] - V[0][1]) * (V[3][0] - V[0][0]));
        area = kc == 4 ? a2 : area;
    }
    bool left = true, right = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool last = j < 3 && kc == j + 1;
        const float Ex = (j == 3 || last) ? V[0][0] : V[j < 3 ? j + 1 : 0][0];
        const float Ey = (j == 3 || last) ? V[0][1] : V[j < 3 ? j + 1 : 0][1];
        const bool active = j == 0 ? kc >= 1 : (kc >= 2 && j < (kc == 2 ? 1 : kc));
        const float ex = Ex - V[j][0], ey = Ey - V[j][1];
        const float wx = cx - V[j][0], wy_ = cyy - V[j][1];
        const float ee = ex * ex + ey * ey;
        float t = (wx * ex + wy_ * ey) / ee;
        t = t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f;
        const float gx = V[j][0] + t * ex, gy = V[j][1] + t * ey;
        const float rx = cx - gx, ry_ = cyy - gy;
        const float d2 = rx * rx + ry_ * ry_;
        const bool take = active && d2 < best;
        best = take ? d2 : best, nx = take ? gx : nx, ny = take ? gy : ny;
        const float cr = ex * wy_ - ey * wx;
        left = left && (!active || cr >= 0.0f), right = right && (!active || cr <= 0.0f);
    }
    const bool inside = kc >= 3 && ((area > 0.0f && left) || (area < 0.0f && right));
    const float dist = sqrtf(best);
    const float d = inside ? -dist : dist;
    const float ux = (cx - nx) / dist, uy = (cyy - ny) / dist;

    // B4. the pendulum's length
    float top = V[0][2];
#pragma unroll
    for (int slot = 1; slot < 4; ++slot) top = (kc > slot && V[slot][2] > top) ? V[slot][2] : top;
    const float h0 = Bz - top;
    const float h = h0 > k.h_min ? h0 : k.h_min;

    // B5. the acceleration of the lean
    const float den = h * h + d * d;
    const float out_x = (k.gravity * (d * ux + h * px)) / den, out_y = (k.gravity * (d * uy + h * py)) / den;
    const float m0 = sqrtf(px * px + py * py);
    const float gin = k.gravity * (-d);
    const float in_x = -((gin * px) / (m0 * den)), in_y = -((gin * py) / (m0 * den));
    const bool outside = kc >= 1 && d > 0.0f;
    const bool within = kc >= 1 && !outside;
    const bool restoring = within && m0 > 0.0f;
    const float ax = outside ? out_x : (restoring ? in_x : 0.0f), ay = outside ? out_y : (restoring ? in_y : 0.0f);

    // B6. semi-implicit Euler, the landing, the step after a reset
    float v1x = vx + ax * k.dt, v1y = vy + ay * k.dt;
    float p1x = px + v1x * k.dt, p1y = py + v1y * k.dt;
    const float dot = p1x * px + p1y * py;
    const float m1 = sqrtf(p1x * p1x + p1y * p1y);
    const bool lands = within && (!(m0 > 0.0f) || dot <= 0.0f || m1 < k.lean_eps);
    const bool clear = lands || fresh;
    p1x = clear ? 0.0f : p1x, p1y = clear ? 0.0f : p1y, v1x = clear ? 0.0f : v1x, v1y = clear ? 0.0f : v1y;

    // B7. the fall
    const float m = sqrtf(p1x * p1x + p1y * p1y);
    const bool fell = m > k.fall_angle;
    const float f0 = *cfz;

    // B8. the lean's rotation, composed on the left, and the body-frame vectors in the leaned frame
    const float lx = -(p1y * 0.5f), ly = p1x * 0.5f;
    const float ln = sqrtf((lx * lx + ly * ly) + 1.0f);
    const float Lx = lx / ln, Ly = ly / ln, Lw = 1.0f / ln;
    const float qn[4] = {(Lw * q[0] + Lx * q[3]) + Ly * q[2], (Lw * q[1] - Lx * q[2]) + Ly * q[3], (Lw * q[2] + Lx * q[1]) - Ly * q[0],
                         (Lw * q[3] - Lx * q[0]) - Ly * q[1]};
    const float qc[4] = {-qn[0], -qn[1], -qn[2], qn[3]};
    const float down[3] = {0.0f, 0.0f, 0.0f - 1.0f};
    const float lv0[3] = {k.base_lin_vel[e * 3], k.base_lin_vel[e * 3 + 1], k.base_lin_vel[e * 3 + 2]};
    const float av0[3] = {k.base_ang_vel[e * 3], k.base_ang_vel[e * 3 + 1], k.base_ang_vel[e * 3 + 2]};
    float g[3], lw[3], lv[3], ww[3], av[3];
    rot(qc, down, g);
    rot(q, lv0, lw);
    rot(qc, lw, lv);
    rot(q, av0, ww);
    const float wl[3] = {ww[0] + (-v1y), ww[1] + v1x, ww[2]};
    rot(qc, wl, av);
    const float z1 = Bz - (h * (m * m)) * 0.5f;
    const bool on = m > 0.0f;

    // B9. the stores.  Without a lean (on == false) every tensor but the base row of rigid_body_state, lean and fallen keeps its bytes.
    k.lean[e * 4] = p1x, k.lean[e * 4 + 1] = p1y, k.lean[e * 4 + 2] = v1x, k.lean[e * 4 + 3] = v1y;
    k.fallen[e] = fell ? 1 : 0;
    if (fell) *cfz = f0 < k.fall_force ? k.fall_force : f0;
    const float zz = on ? z1 : Bz;
    rb[0] = Bx, rb[1] = By, rb[2] = zz;
#pragma unroll
    for (int i = 0; i < 4; ++i) rb[3 + i] = on ? qn[i] : q[i];
    if (!on) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) k.base_quat[e * 4 + i] = qn[i], rs[3 + i] = qn[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) k.projected_gravity[e * 3 + i] = g[i], k.base_lin_vel[e * 3 + i] = lv[i], k.base_ang_vel[e * 3 + i] = av[i];
    rs[10] = rs[10] + (-v1y);
    rs[11] = rs[11] + v1x;
    rs[2] = z1;
    k.base_pos[e * 3 + 2] = z1;
}

bool finite_pos(float v) { return v > 0.f && v <= 3.0e38f; }                      // false for a NaN and for an infinity
bool finite_nonneg(float v) { return v >= 0.f && v <= 3.0e38f; }
bool finite(float v) { return v >= -3.0e38f && v <= 3.0e38f; }

}  // namespace

extern "C" int dtc_sim_balance_abi_sizes(int64_t* out, int cap) {
    const int64_t sz[] = {sizeof(DtcSimBalance)};
    if (cap > 0 && out) out[0] = sz[0];
    return 1;
}

extern "C" int dtc_sim_balance(const DtcSimStep* st, const DtcSimCfg* cfg, const DtcSimBalance* bal, int N, void* stream) {
    DTC_REQUIRE(st && cfg && bal, "null descriptor");
    DTC_REQUIRE(N > 0 && N <= (1 << 24), "N %d outside 1..2^24", N);
    const DtcSimStep& s = *st;
    const DtcSimCfg& c = *cfg;
    const DtcSimBalance& b = *bal;
    DTC_REQUIRE(c.num_bodies >= 2 && c.num_bodies <= (1 << 16), "num_bodies %d", c.num_bodies);
    for (int l = 0; l < 4; ++l)
        DTC_REQUIRE(c.feet[l] >= 1 && c.feet[l] < c.num_bodies, "leg %d: foot body %d outside 1..%d (body 0 is the base)", l, c.feet[l],
                    c.num_bodies - 1);
    DTC_REQUIRE(s.root_states && s.base_pos && s.base_quat && s.projected_gravity && s.base_lin_vel && s.base_ang_vel && s.rigid_body_state &&
                    s.contact_forces && s.contact_filt && s.episode_length_buf,
                "null tensor of the step");
    DTC_REQUIRE(b.lean && b.fallen, "null lean / fallen");
    // comparisons written so that a NaN is refused
    DTC_REQUIRE(finite_pos(b.h_min) && finite_pos(b.fall_angle) && finite_pos(b.dt),
                "h_min %g, fall_angle %g, dt %g must be positive and finite", (double)b.h_min, (double)b.fall_angle, (double)b.dt);
    DTC_REQUIRE(b.fall_force > 100.0f && b.fall_force <= 3.0e38f, "fall_force %g must exceed the termination threshold of 100 N",
                (double)b.fall_force);
    DTC_REQUIRE(finite_nonneg(b.gravity) && finite_nonneg(b.lean_eps), "gravity %g, lean_eps %g must be finite and not negative",
                (double)b.gravity, (double)b.lean_eps);
    DTC_REQUIRE(finite(b.com_offset[0]) && finite(b.com_offset[1]), "com_offset (%g, %g) must be finite", (double)b.com_offset[0],
                (double)b.com_offset[1]);

    BalK k{};
    k.root_states = s.root_states, k.base_pos = s.base_pos, k.base_quat = s.base_quat, k.projected_gravity = s.projected_gravity;
    k.base_lin_vel = s.base_lin_vel, k.base_ang_vel = s.base_ang_vel, k.rigid_body_state = s.rigid_body_state;
    k.contact_forces = s.contact_forces, k.contact_filt = s.contact_filt, k.episode_length_buf = (const long long*)s.episode_length_buf;
    k.lean = b.lean, k.fallen = b.fallen;
    k.B = c.num_bodies;
    for (int l = 0; l < 4; ++l) k.feet[l] = c.feet[l];
    k.gravity = b.gravity, k.h_min = b.h_min, k.lean_eps = b.lean_eps, k.fall_angle = b.fall_angle, k.fall_force = b.fall_force;
    k.dt = b.dt, k.ox = b.com_offset[0], k.oy = b.com_offset[1];

    hipStream_t hs = (hipStream_t)stream;
    const dim3 grid((unsigned)dtc::ceil_div(N, 64)), block(64);
    dtc::ProfScope prof("sim_balance", (double)N * 500.0, hs);
    hipLaunchKernelGGL(sim_balance_kernel, grid, block, 0, hs, k, N);
    return dtc::check_launch("sim_balance");
}
