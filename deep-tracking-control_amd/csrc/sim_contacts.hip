// Leg collisions and foot stumbles of the surrogate legged env for gfx950 (opt-in): dtc_sim_contacts, a launch of its own that runs
// directly behind dtc_sim_step* (csrc/sim.hip) on what that launch wrote, once per env step.  include/dtc_hip.h states every
// operation and its order, tests/sim_contact_oracle.py restates them in numpy float32 bit for bit.  It writes the contact-force rows
// of the thighs and shanks (a penetration spring over sample points along the two links), the horizontal contact force of a swing
// foot that flies into a riser, the knee positions (shank rows of rigid_body_state) and two flag tensors.
//
// What it is NOT: the forces feed the rewards (collision, stumble, feet_stumble, foot_clearance) and nothing else.  A colliding
// shank is not held back, a stumbling foot is not stopped (the support rule still lifts it onto the riser), nothing topples, the
// torso has no contact of its own (its row belongs to flight's crash force).  Every constant is a free choice, fitted to nothing.
//
// Not a ninth template axis of sim_step_kernel: that kernel's eight instantiations stand at up to 99 VGPRs with SGPR spills, and
// contact forces are read once per env step, after the last substep.
//
// One 64-lane wavefront per env, 4 envs per 256-thread workgroup (as csrc/sim.hip).  Lane 8 l + j serves leg l: j = 0..2 the thigh
// samples, j = 3..6 the shank samples; lanes 32..63 idle.  Every lane of a group computes its leg's knee and the probe ahead of
// its foot itself (the same loads, one cache line; a wavefront pays per instruction, not per lane), the seven penetrations go
// round the group by __shfl, and the eight lanes share the stores.
// No LDS, no atomics, no scratch; every store is a per-lane vector store.  Latency bound: ~0.4 KB read and ~0.2 KB written per env.
// -ffp-contract=off (build.py): every value is one single-rounded fp32 operation in the stated order.
//
// Resources (compiler resource-usage remarks, gfx950): VGPRs / SGPRs / SGPRs spilled / scratch
//   sim_contacts_kernel  42 / 35 / 0 / 0
#include "common.hpp"
#include "terrain_lookup.hpp"

namespace {

struct ConK {
    const float *base_pos, *base_quat, *dof_pos, *default_dof_pos, *knee_nominal, *knee_jacobian;
    const int16_t* hs;
    float *rigid_body_state, *contact_forces;
    uint8_t *leg_contact, *stumbled;
    long long row_stride, elem_stride;
    int B, feet[4], thighs[4], shanks[4];
    int rows, cols;
    float border, hscale, vscale;
    float body_radius, stiffness, max_force, probe, stumble_height, wall_damping, min_speed;
};

__global__ __launch_bounds__(256) void sim_contacts_kernel(const ConK k, int N) {
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (n >= N) return;
    const long long e = n;
    const bool live = lane < 32;
    const int l = live ? lane >> 3 : 0, j = lane & 7, g0 = l * 8;                  // idle lanes shadow leg 0 and store nothing
    int foot = k.feet[0], thigh = k.thighs[0], shank = k.shanks[0];
#pragma unroll
    for (int m = 1; m < 4; ++m)                                                    // constant index into the by-value struct
        if (l == m) foot = k.feet[m], thigh = k.thighs[m], shank = k.shanks[m];

    // ---- the env's rows, as the step just wrote them
    const float Bx = k.base_pos[e * 3], By = k.base_pos[e * 3 + 1], Bz = k.base_pos[e * 3 + 2];
    const float qx = k.base_quat[e * 4], qy = k.base_quat[e * 4 + 1], qz = k.base_quat[e * 4 + 2], qw = k.base_quat[e * 4 + 3];
    float dq[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) dq[i] = k.dof_pos[e * k.row_stride + (l * 3 + i) * k.elem_stride] - k.default_dof_pos[l * 3 + i];
    const float* hrow = k.rigid_body_state + (e * k.B + thigh) * 13;
    const float* frow = k.rigid_body_state + (e * k.B + foot) * 13;
    const float H[3] = {hrow[0], hrow[1], hrow[2]}, F[3] = {frow[0], frow[1], frow[2]};
    const float Vx = frow[7], Vy = frow[8];

    // C1. the knee: linear in the joint angles, then the base's rotation
    float v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float* J = k.knee_jacobian + (l * 3 + i) * 3;
        v[i] = k.knee_nominal[l * 3 + i] + ((J[0] * dq[0] + J[1] * dq[1]) + J[2] * dq[2]);
    }
    const float tx = 2.0f * (qy * v[2] - qz * v[1]), ty = 2.0f * (qz * v[0] - qx * v[2]), tz = 2.0f * (qx * v[1] - qy * v[0]);
    const float cx = qy * tz - qz * ty, cy = qz * tx - qx * tz, cz = qx * ty - qy * tx;
    const float K[3] = {Bx + ((v[0] + qw * tx) + cx), By + ((v[1] + qw * ty) + cy), Bz + ((v[2] + qw * tz) + cz)};

    // C2, C3. this lane's sample and its penetration (lane 7 of a group: the shank's last sample once more, not used)
    const bool on_thigh = j < 3;
    const float s = on_thigh ? (j == 0 ? 0.25f : (j == 1 ? 0.5f : 0.75f)) : (j == 3 ? 0.0f : (j == 4 ? 0.25f : (j == 5 ? 0.5f : 0.75f)));
    float X[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float A = on_thigh ? H[i] : K[i], E = on_thigh ? K[i] : F[i];
        X[i] = A + s * (E - A);
    }
    const float pen = (dtc::terrain_height(k.hs, k, X[0], X[1]) + k.body_radius) - X[2];
    float dt = 0.0f, ds = 0.0f;                                                    // every lane of the group, in sample order
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const float p = __shfl(pen, g0 + m, 64);
        dt = p > dt ? p : dt;
    }
#pragma unroll
    for (int m = 3; m < 7; ++m) {
        const float p = __shfl(pen, g0 + m, 64);
        ds = p > ds ? p : ds;
    }
    // C4. the body forces
    const float ft = k.stiffness * dt, fs = k.stiffness * ds;
    const float Ft = dt > 0.0f ? (ft < k.max_force ? ft : k.max_force) : 0.0f;
    const float Fs = ds > 0.0f ? (fs < k.max_force ? fs : k.max_force) : 0.0f;
    // C5. the stumble (every lane computes its leg's; one lookup more)
    const float sp = sqrtf(Vx * Vx + Vy * Vy);
    const float ex = Vx / sp, ey = Vy / sp;
    const float rise = dtc::terrain_height(k.hs, k, F[0] + ex * k.probe, F[1] + ey * k.probe) - F[2];
    const bool hit = sp > k.min_speed && rise > k.stumble_height;
    const float m0 = k.wall_damping * sp;
    const float mag = m0 < k.max_force ? m0 : k.max_force;
    const float fx = hit ? -(mag * ex) : 0.0f, fy = hit ? -(mag * ey) : 0.0f;

    // ---- the stores: lanes j = 0..2 the thigh's force row and the knee position, 3..5 the shank's force row, 6, 7 the foot's x, y
    if (!live) return;
    float* cf = k.contact_forces + e * k.B * 3;
    if (j < 3) {
        cf[thigh * 3 + j] = j == 2 ? Ft : 0.0f;
        k.rigid_body_state[(e * k.B + shank) * 13 + j] = j == 0 ? K[0] : (j == 1 ? K[1] : K[2]);
    } else if (j < 6) {
        cf[shank * 3 + (j - 3)] = j == 5 ? Fs : 0.0f;
    } else {
        cf[foot * 3 + (j - 6)] = j == 6 ? fx : fy;
    }
    if (j == 0) k.leg_contact[e * 8 + 2 * l] = dt > 0.0f ? 1 : 0;
    if (j == 1) k.leg_contact[e * 8 + 2 * l + 1] = ds > 0.0f ? 1 : 0;
    if (j == 2) k.stumbled[e * 4 + l] = hit ? 1 : 0;
}

bool finite_pos(float v) { return v > 0.f && v <= 3.0e38f; }                      // false for a NaN and for an infinity
bool finite_nonneg(float v) { return v >= 0.f && v <= 3.0e38f; }

}  // namespace

extern "C" int dtc_sim_contact_abi_sizes(int64_t* out, int cap) {
    const int64_t sz[] = {sizeof(DtcSimContacts)};
    if (cap > 0 && out) out[0] = sz[0];
    return 1;
}

extern "C" int dtc_sim_contacts(const DtcSimStep* st, const DtcSimCfg* cfg, const DtcSimContacts* con, int N, void* stream) {
    DTC_REQUIRE(st && cfg && con, "null descriptor");
    DTC_REQUIRE(N > 0 && N <= (1 << 24), "N %d outside 1..2^24", N);
    const DtcSimStep& s = *st;
    const DtcSimCfg& c = *cfg;
    const DtcSimContacts& t = *con;
    DTC_REQUIRE(c.num_dof == 12, "num_dof %d: the surrogate has four legs of three joints", c.num_dof);
    DTC_REQUIRE(c.num_bodies >= 1 && c.num_bodies <= (1 << 16), "num_bodies %d", c.num_bodies);
    for (int l = 0; l < 4; ++l)
        DTC_REQUIRE(c.feet[l] >= 0 && c.feet[l] < c.num_bodies && c.thighs[l] >= 0 && c.thighs[l] < c.num_bodies,
                    "leg %d: foot body %d / thigh body %d outside 0..%d", l, c.feet[l], c.thighs[l], c.num_bodies - 1);
    DTC_REQUIRE(c.rows >= 2 && c.cols >= 2 && (int64_t)c.rows * c.cols < ((int64_t)1 << 31) && c.horizontal_scale > 0.f, "terrain table %d x %d",
                c.rows, c.cols);
    DTC_REQUIRE(s.base_pos && s.base_quat && s.dof_pos && s.default_dof_pos && s.height_samples && s.rigid_body_state && s.contact_forces,
                "null tensor of the step");
    DTC_REQUIRE(s.dof_pos_elem_stride >= 1 && s.dof_pos_row_stride >= (c.num_dof - 1) * s.dof_pos_elem_stride + 1, "dof_pos strides");
    DTC_REQUIRE(t.knee_nominal && t.knee_jacobian, "null knee table");
    DTC_REQUIRE(t.leg_contact && t.stumbled, "null leg_contact / stumbled");
    // comparisons written so that a NaN is refused
    DTC_REQUIRE(finite_pos(t.stiffness) && finite_pos(t.max_force) && finite_pos(t.probe) && finite_pos(t.wall_damping),
                "stiffness %g, max_force %g, probe %g, wall_damping %g must be positive and finite", (double)t.stiffness, (double)t.max_force,
                (double)t.probe, (double)t.wall_damping);
    DTC_REQUIRE(finite_nonneg(t.body_radius) && finite_nonneg(t.stumble_height) && finite_nonneg(t.min_speed),
                "body_radius %g, stumble_height %g, min_speed %g must be finite and not negative", (double)t.body_radius,
                (double)t.stumble_height, (double)t.min_speed);
    for (int l = 0; l < 4; ++l) {
        DTC_REQUIRE(t.shanks[l] >= 1 && t.shanks[l] < c.num_bodies, "leg %d: shank body %d outside 1..%d (body 0 is the base)", l, t.shanks[l],
                    c.num_bodies - 1);
        for (int m = 0; m < 4; ++m)
            DTC_REQUIRE(t.shanks[l] != c.feet[m] && t.shanks[l] != c.thighs[m] && (m == l || t.shanks[l] != t.shanks[m]),
                        "leg %d: shank body %d is a foot, a thigh or another leg's shank", l, t.shanks[l]);
    }

    ConK k{};
    k.base_pos = s.base_pos, k.base_quat = s.base_quat, k.dof_pos = s.dof_pos, k.default_dof_pos = s.default_dof_pos;
    k.knee_nominal = t.knee_nominal, k.knee_jacobian = t.knee_jacobian, k.hs = s.height_samples;
    k.rigid_body_state = s.rigid_body_state, k.contact_forces = s.contact_forces, k.leg_contact = t.leg_contact, k.stumbled = t.stumbled;
    k.row_stride = s.dof_pos_row_stride, k.elem_stride = s.dof_pos_elem_stride;
    k.B = c.num_bodies;
    for (int l = 0; l < 4; ++l) k.feet[l] = c.feet[l], k.thighs[l] = c.thighs[l], k.shanks[l] = t.shanks[l];
    k.rows = c.rows, k.cols = c.cols, k.border = c.border_size, k.hscale = c.horizontal_scale, k.vscale = c.vertical_scale;
    k.body_radius = t.body_radius, k.stiffness = t.stiffness, k.max_force = t.max_force, k.probe = t.probe;
    k.stumble_height = t.stumble_height, k.wall_damping = t.wall_damping, k.min_speed = t.min_speed;

    hipStream_t hs = (hipStream_t)stream;
    const dim3 grid((unsigned)dtc::ceil_div(N, 4)), block(256);
    dtc::ProfScope prof("sim_contacts", (double)N * 600.0, hs);
    hipLaunchKernelGGL(sim_contacts_kernel, grid, block, 0, hs, k, N);
    return dtc::check_launch("sim_contacts");
}
