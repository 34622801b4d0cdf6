// Surrogate legged env for gfx950: the state the env kernels (csrc/foothold.hip, rewards.hip, reset.hip, envstep.hip) run on when no
// simulator stands behind them.  dtc_sim_step (include/dtc_hip.h states every operation and its order) is one env step as ONE launch:
// `decimation` substeps of the PD law of LeggedRobot._compute_torques, control type "P" (legged_gym/envs/base/legged_robot.py:610-630),
// explicit joint integration with hard position limits, legs that are linear in the joint angles around the default pose, a base that
// only yaws and rides on its stance feet over the int16 terrain table (_get_heights, :1301-1316), its planar twist as the
// least-squares fit of "stance feet do not slip", then the bookkeeping of post_physics_step up to the planner
// (legged_robot_dtc.py:66-91, legged_robot.py:534-535 with _resample_commands :573-591, and :562-564).
//
// It is a surrogate, not physics.  dtc_sim_step keeps the base level (quaternion x = y = 0, projected gravity (0, 0, -1));
// dtc_sim_step_tilt, the other instantiation of the same kernel, lets roll and pitch follow the least-squares plane through the
// support points the terrain asks of the stance feet -- kinematically: after a reset (identity quaternion) the first fit is one
// substep with a tilt-rate spike.  dtc_sim_step_act, two further instantiations (either base), adds the reference's two training
// disturbances: the PD goal comes from a six-slot lag buffer of scaled actions, shifted at every substep, at a slot the host draws per
// substep for all envs (legged_robot.py:608-618), and a random planar velocity (:546-553, :673-678) that rides on the base twist as a
// slip velocity with a chosen exponential decay -- kinematic, not a contact dynamics; its decay and floor are free constants fitted
// to nothing.  dtc_sim_step_fly, four further instantiations (any of the above), gives the base a vertical degree of freedom: a base
// whose support falls away falls under gravity and lands when it reaches a support, and a support that rises by more than max_step_up
// within a substep is a crash, reported as the base's own contact force so that dtc_check_termination ends the episode; max_step_up,
// crash_force and the take-off rule are free constants.  Without it at least one foot is always in contact.  Deliberately absent from
// all: control types "V" and "T", `forces` (never touched), contact dynamics, anything that topples the robot, and the heading
// command's yaw law (legged_robot.py:537-539), which stays with the caller.  Contact with anything but the soles of the feet is not
// here either: dtc_sim_contacts (csrc/sim_contacts.hip, opt-in, a launch of its own behind this one) writes thigh, shank and
// stumble forces for the rewards, and holds nothing back.
//
// One 64-lane wavefront per env, 4 envs per 256-thread workgroup (as csrc/envstep.hip).  Lanes 0..11 own the joints (leg l owns
// 3l..3l+2) and lane 3l+i computes component i of foot l; the twelve foot components are then broadcast with v_readlane and every lane
// carries the same base state
// through the substep, so the whole decimation loop runs in registers: each env row is loaded once, ahead of the loop, and stored once,
// after it.  Only the terrain table is read inside the loop.  No atomics, no LDS, no scratch (every register array is indexed by
// unrolled constants).  Latency bound: ~0.8 KB read and ~1.2 KB written per env (dtc_sim_step_act: ~0.3 KB more each way).
// -ffp-contract=off (build.py): every value is one single-rounded fp32 operation in the stated order, sums over legs run in leg order
// from 0.0f, and tests/sim_oracle.py restates the step in numpy float32 bit for bit (tests/sim_tilt_oracle.py and
// tests/sim_actuator_oracle.py: the other instantiations; tests/sim_flight_oracle.py: all four with FLY).
//
// Resources of the eight instantiations (compiler resource-usage remarks, gfx950): VGPRs / SGPRs / SGPRs spilled to VGPR lanes / scratch
//   yaw  60 /  98 /  0 / 0    tilt  89 / 106 /  8 / 0    yaw + act  70 / 104 / 0 / 0    tilt + act  99 / 106 / 16 / 0
//   with FLY:  64 / 104 /  0 / 0          87 / 106 / 16 / 0               76 / 106 / 6 / 0                96 / 106 / 24 / 0
// Scratch must stay 0 for all eight (tests/test_abi_and_host.py pins it for every kernel).
#include <cstddef>

#include "common.hpp"
#include "philox.hpp"
#include "terrain_lookup.hpp"

namespace {

struct Span { float span, lo; };            // a range [lo, hi] as fp32 scalars: float32(hi - lo), float32(lo)

struct SimK {
    int B, C, dec, heading, T;
    int feet[4], thighs[4];
    long long resample;
    float dt, half_dt, action_scale, clip, inertia, eps, weight, rmin2;
    int rows, cols;
    float border, hscale, vscale;
    Span cmd_x, cmd_y, cmd_third;
    unsigned seed_lo, seed_hi, ctr_lo, ctr_hi;
    float max_slope, min_det;                   // dtc_sim_step_tilt only
};

__device__ __forceinline__ float bcast(float v, int src_lane) {                    // src_lane is wave-uniform
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}

// _get_heights (legged_robot.py:1301-1316) for one world point: the lookup rule lives in terrain_lookup.hpp, shared with sim_contacts.hip
__device__ __forceinline__ float terrain_height(const int16_t* __restrict__ hs, const SimK& k, float fx, float fy) {
    return dtc::terrain_height(hs, k, fx, fy);
}

// The tilt rotation Rt, the minimal rotation that takes z to n = (nx, ny, nz): third column n, third row (-nx, -ny, nz), and the
// three entries computed here (Rt[0][1] = Rt[1][0]).
struct TiltR { float r00, r01, r11; };
__device__ __forceinline__ TiltR tilt_entries(float nx, float ny, float nz) {
    const float k1 = 1.0f + nz;
    return TiltR{1.0f - (nx * nx) / k1, -((nx * ny) / k1), 1.0f - (ny * ny) / k1};
}
__device__ __forceinline__ void tilt_rotate(const TiltR& R, float nx, float ny, float nz, const float v[3], float out[3]) {       // Rt v
    out[0] = (R.r00 * v[0] + R.r01 * v[1]) + nx * v[2];
    out[1] = (R.r01 * v[0] + R.r11 * v[1]) + ny * v[2];
    out[2] = (-(nx * v[0]) - ny * v[1]) + nz * v[2];
}
__device__ __forceinline__ void tilt_rotate_t(const TiltR& R, float nx, float ny, float nz, const float v[3], float out[3]) {     // Rt^T v
    out[0] = (R.r00 * v[0] + R.r01 * v[1]) - nx * v[2];
    out[1] = (R.r01 * v[0] + R.r11 * v[1]) - ny * v[2];
    out[2] = (nx * v[0] + ny * v[1]) + nz * v[2];
}

// INVARIANTS of this kernel's signature and launch:
//  * the descriptor is the FIRST parameter (`d`, whose first member is the DtcSimStep `s`), so it lies at offset 0 of the
//    kernel-argument segment: the rows written after the loop take their pointers from there (see below).  A parameter put in front
//    of it breaks that silently; keep the order.  (ACT: lag_state and push_vel are needed ahead of the loop and come from `d`
//    itself; after the loop they, u_push and the push constants come from the segment like the rest.)
//  * one wavefront owns one env row and no other wavefront touches it (grid = ceil(N / 4) workgroups of 4 wavefronts, n from the
//    wavefront's index): the ring-buffer shift below has lanes load slot t + 1 and store slot t of the same env, which is right
//    only because a wavefront's loads issue ahead of its stores and nobody else writes those slots.
static_assert(offsetof(DtcSimStep, actions_in) == 0 && sizeof(DtcSimStep) % 8 == 0, "descriptor layout the late loads rely on");
// The first parameter: the descriptor alone, or (ACT) the descriptor with the actuator's by-value struct behind it, so that the late
// loads find both at offsets the language fixes (0 and offsetof(SimDesc<true>, a)) whatever follows in the argument list.
// (FLY: the flight struct comes last, found alike.)
template <bool ACT, bool FLY = false> struct SimDesc { DtcSimStep s; };
template <> struct SimDesc<true, false> { DtcSimStep s; DtcSimActuator a; };
template <> struct SimDesc<false, true> { DtcSimStep s; DtcSimFlight f; };
template <> struct SimDesc<true, true> { DtcSimStep s; DtcSimActuator a; DtcSimFlight f; };
static_assert(offsetof(SimDesc<true>, s) == 0 && offsetof(SimDesc<true>, a) % 8 == 0 && sizeof(SimDesc<false>) == sizeof(DtcSimStep),
              "descriptor layout the late loads rely on");
using SimDescFly = SimDesc<false, true>;
using SimDescActFly = SimDesc<true, true>;
static_assert(offsetof(SimDescFly, s) == 0 && offsetof(SimDescActFly, s) == 0 && offsetof(SimDescFly, f) % 8 == 0 &&
              offsetof(SimDescActFly, f) % 8 == 0 && offsetof(SimDescActFly, a) == offsetof(SimDesc<true>, a),
              "descriptor layout the late loads rely on");
// TILT = false is dtc_sim_step, the yaw-only base; TILT = true is dtc_sim_step_tilt: the body z-axis n (yaw frame) lives in the
// quaternion between steps and in three registers through the loop, and r = Rt p, sv = Rt u stand where the yaw-only step has p, u.
// ACT = true is dtc_sim_step_act (either base): the PD goal comes from the six-slot lag buffer of scaled actions, which lanes 0..11
// hold in registers through the loop, and a pending push (two wave-uniform registers) rides on the base twist and decays.
// FLY = true is dtc_sim_step_fly (any of the four above): the base has a vertical degree of freedom.  Its z velocity, its world-frame
// planar velocity and its yaw rate are carried from substep to substep (between calls: in root_states[7:10] and [12]); a substep
// whose ballistic candidate stays clear of the support is airborne, every other one is grounded and computed as without FLY.  The
// grounded values are always computed and an airborne env takes the carried ones by selects, so no division by a contact count of
// zero reaches an output and a grounded env keeps the arithmetic of the other instantiations.
template <bool TILT, bool ACT, bool FLY>
__global__ __launch_bounds__(256) void sim_step_kernel(const SimDesc<ACT, FLY> d, const SimK k, int N) {
    const DtcSimStep& s = d.s;
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (n >= N) return;
    const long long e = n;
    const int D = 12;
    const bool joint = lane < D;

    // ---- the env's rows and the tables, once
    float act = 0.f, kp = 0.f, kd = 0.f, strength = 0.f, off = 0.f, limit = 0.f, lo = 0.f, hi = 0.f, dflt = 0.f, q = 0.f, qd = 0.f;
    float J0 = 0.f, J1 = 0.f, J2 = 0.f, nom = 0.f;                                 // lane 3 l + i: row i of leg l's Jacobian, foot_nominal[l][i]
    if (joint) {
        act = s.actions_in[e * D + lane];
        kp = s.p_gains[lane] * s.Kp_factors[e * D + lane];
        kd = s.d_gains[lane] * s.Kd_factors[e * D + lane];
        strength = s.motor_strengths[e * D + lane];
        off = s.motor_offsets[e * D + lane];
        limit = s.torque_limits[lane];
        lo = s.dof_pos_limits[lane * 2];
        hi = s.dof_pos_limits[lane * 2 + 1];
        dflt = s.default_dof_pos[lane];
        q = s.dof_pos[e * s.dof_pos_row_stride + lane * s.dof_pos_elem_stride];
        qd = s.dof_vel[e * s.dof_vel_row_stride + lane * s.dof_vel_elem_stride];
        J0 = s.leg_jacobian[lane * 3], J1 = s.leg_jacobian[lane * 3 + 1], J2 = s.leg_jacobian[lane * 3 + 2];
        nom = s.foot_nominal[lane];
    }
    const int leg0 = joint ? (lane / 3) * 3 : 0;                                   // first joint lane of this lane's leg
    const float* rs = s.root_states + e * 13;
    float x = rs[0], y = rs[1], z = rs[2], qz = rs[5], qw = rs[6];
    float nx = 0.f, ny = 0.f, nz = 1.f, wx = 0.f, wy = 0.f;                        // TILT: body z-axis in the yaw frame, its rate
    if constexpr (TILT) {                                                          // twist about z (the yaw pair) and swing (n)
        const float qx = rs[3], qy = rs[4];
        const float ry = sqrtf(qz * qz + qw * qw);
        const float zy = qz / ry, wyw = qw / ry;
        const float c = 1.0f - 2.0f * (zy * zy), sn = 2.0f * (zy * wyw);
        const float ax = 2.0f * (qx * qz + qw * qy), ay = 2.0f * (qy * qz - qw * qx), az = 1.0f - 2.0f * (qx * qx + qy * qy);
        const float mx = c * ax + sn * ay, my = c * ay - sn * ax;
        const float rn = sqrtf((mx * mx + my * my) + az * az);
        nx = mx / rn, ny = my / rn, nz = az / rn;
        qz = zy, qw = wyw;
    }
    float old_ang = 0.f;
    if (lane < 3) old_ang = s.base_ang_vel[e * 3 + lane];
    const long long elen = s.episode_length_buf[e] + 1;
    unsigned char last_c = 0;
    if (lane < 4) last_c = s.last_contacts[e * 4 + lane];

    const float a = fminf(fmaxf(act, -k.clip), k.clip);
    const float goal = fminf(fmaxf(a * k.action_scale + dflt, lo), hi);
    float lg[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, px = 0.f, py = 0.f;              // ACT: the joint's lag slots, the pending push (world)
    if constexpr (ACT) {
        if (joint) {
#pragma unroll
            for (int i = 0; i < 6; ++i) lg[i] = d.a.lag_state[(e * 6 + i) * D + lane];
        }
        if (d.a.push) px = d.a.push_vel[e * 2], py = d.a.push_vel[e * 2 + 1];
    }

    float tau = 0.f, p[4][3], u[4][3], w = 0.f, vbx = 0.f, vby = 0.f, vz = 0.f, nc = 0.f;
    bool ct[4];
    float Vwx = 0.f, Vwy = 0.f, gdt = 0.f;                                         // FLY: the carried planar velocity (world), g * dt
    bool air = false, crashed = false;
    if constexpr (FLY) Vwx = rs[7], Vwy = rs[8], vz = rs[9], w = rs[12], gdt = d.f.gravity * k.dt;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        ct[l] = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) p[l][i] = 0.f, u[l][i] = 0.f;
    }
    for (int it = 0; it < k.dec; ++it) {
        // 0. (ACT) the lag buffer shifts, takes the scaled action, and slot choice[it] (wave-uniform) is the PD goal
        float g = goal;
        if constexpr (ACT) {
#pragma unroll
            for (int i = 0; i < 5; ++i) lg[i] = lg[i + 1];
            lg[5] = a * k.action_scale;
            const int ch = d.a.lag_choice[it];
            float sel = lg[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) sel = ch == i ? lg[i] : sel;
            const float gl = fminf(fmaxf(sel + dflt, lo), hi);
            g = d.a.lag ? gl : goal;
        }
        // 1. PD law, 2. joint integration with hard limits (joint lanes)
        tau = fminf(fmaxf(((kp * ((g - q) + off)) - kd * qd) * strength, -limit), limit);
        qd = qd + (tau / k.inertia) * k.dt;
        q = q + qd * k.dt;
        if (q < lo) q = lo, qd = 0.f;
        if (q > hi) q = hi, qd = 0.f;
        const float dq = q - dflt;
        // 3. linear leg kinematics: lane 3 l + i computes component i of leg l, then every lane takes all twelve
        const float a0 = __shfl(dq, leg0, 64), a1 = __shfl(dq, leg0 + 1, 64), a2 = __shfl(dq, leg0 + 2, 64);
        const float v0 = __shfl(qd, leg0, 64), v1 = __shfl(qd, leg0 + 1, 64), v2 = __shfl(qd, leg0 + 2, 64);
        const float pl = nom + ((J0 * a0 + J1 * a1) + J2 * a2);
        const float ul = (J0 * v0 + J1 * v1) + J2 * v2;
#pragma unroll
        for (int l = 0; l < 4; ++l)
#pragma unroll
            for (int i = 0; i < 3; ++i) p[l][i] = bcast(pl, 3 * l + i), u[l][i] = bcast(ul, 3 * l + i);
        // the feet in the yaw frame: r = Rt p, sv = Rt u (TILT), or p, u themselves
        float r[4][3], sv[4][3];
        if constexpr (TILT) {
            const TiltR R = tilt_entries(nx, ny, nz);
#pragma unroll
            for (int l = 0; l < 4; ++l) tilt_rotate(R, nx, ny, nz, p[l], r[l]), tilt_rotate(R, nx, ny, nz, u[l], sv[l]);
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l)
#pragma unroll
                for (int i = 0; i < 3; ++i) r[l][i] = p[l][i], sv[l][i] = u[l][i];
        }
        // 4. yaw, 5. terrain under each foot, 6. support and contact
        const float c = 1.0f - 2.0f * (qz * qz), sn = 2.0f * (qz * qw);
        float h[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const float fx = x + (c * r[l][0] - sn * r[l][1]);
            const float fy = y + (sn * r[l][0] + c * r[l][1]);
            h[l] = terrain_height(s.height_samples, k, fx, fy);
        }
        float bz = h[0] - r[0][2];
#pragma unroll
        for (int l = 1; l < 4; ++l) bz = fmaxf(bz, h[l] - r[l][2]);
        nc = 0.f;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            ct[l] = ((bz + r[l][2]) - h[l]) <= k.eps;
            nc = nc + (ct[l] ? 1.0f : 0.0f);
        }
        // 7. base twist: planar least squares of v_b + w z^ x r_l + sv_l = 0 over the stance feet
        float spx = 0.f, spy = 0.f, sux = 0.f, suy = 0.f;
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (ct[l]) spx = spx + r[l][0], spy = spy + r[l][1], sux = sux + sv[l][0], suy = suy + sv[l][1];
        const float pmx = spx / nc, pmy = spy / nc, umx = sux / nc, umy = suy / nc;
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (ct[l]) {
                const float dpx = r[l][0] - pmx, dpy = r[l][1] - pmy, dux = sv[l][0] - umx, duy = sv[l][1] - umy;
                num = num + (dpx * duy - dpy * dux);
                den = den + (dpx * dpx + dpy * dpy);
            }
        const float w_air = w;                                                     // FLY: the yaw rate an airborne substep keeps
        w = den > k.rmin2 ? -(num / den) : 0.0f;
        vbx = (-umx) + w * pmy;
        vby = (-umy) - w * pmx;
        const float n_air[3] = {nx, ny, nz};                                       // FLY: the tilt an airborne substep keeps
        if constexpr (TILT) {
            // the new tilt.  Stance legs: those extended to within eps of the most extended one (body frame: the legs the env stands
            // on, whether or not the current plane has them on the ground).  Centred least squares of d_l = h_l - p_l.z =
            // c0 + a p_l.x + b p_l.y over them, every d_l relative to the first stance leg's; then the tilt rate, the small-angle
            // reading of dn/dt = omega x n
            float zmin = p[0][2];
#pragma unroll
            for (int l = 1; l < 4; ++l) zmin = p[l][2] < zmin ? p[l][2] : zmin;
            bool sl[4];
            float ns = 0.f, d[4];
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                sl[l] = (p[l][2] - zmin) <= k.eps;
                ns = ns + (sl[l] ? 1.0f : 0.0f);
                d[l] = h[l] - p[l][2];
            }
            const float d0 = sl[0] ? d[0] : (sl[1] ? d[1] : (sl[2] ? d[2] : d[3]));
            float tpx = 0.f, tpy = 0.f, te = 0.f;
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (sl[l]) tpx = tpx + p[l][0], tpy = tpy + p[l][1], te = te + (d[l] - d0);
            const float mx = tpx / ns, my = tpy / ns, me = te / ns;
            float sxx = 0.f, sxy = 0.f, syy = 0.f, sxe = 0.f, sye = 0.f;
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (sl[l]) {
                    const float dx = p[l][0] - mx, dy = p[l][1] - my, de = (d[l] - d0) - me;
                    sxx = sxx + dx * dx, sxy = sxy + dx * dy, syy = syy + dy * dy;
                    sxe = sxe + dx * de, sye = sye + dy * de;
                }
            const float det = sxx * syy - sxy * sxy;
            const float sa = (sxe * syy - sye * sxy) / det, sb = (sye * sxx - sxe * sxy) / det;
            const float ca = sa < -k.max_slope ? -k.max_slope : (sa > k.max_slope ? k.max_slope : sa);
            const float cb = sb < -k.max_slope ? -k.max_slope : (sb > k.max_slope ? k.max_slope : sb);
            const float rr = sqrtf((ca * ca + cb * cb) + 1.0f);
            const bool fit = ns >= 3.0f && det > k.min_det;
            const float nnx = fit ? (-ca) / rr : nx, nny = fit ? (-cb) / rr : ny, nnz = fit ? 1.0f / rr : nz;
            wx = -((nny - ny) / k.dt);
            wy = (nnx - nx) / k.dt;
            nx = nnx, ny = nny, nz = nnz;
        }
        // 7p. (ACT) a pending push rides on the twist: a select, so that an env without one keeps the bits above (the sign of a
        // zero included)
        if constexpr (ACT) {
            const bool pushed = px != 0.0f || py != 0.0f;
            const float ax = vbx + (c * px + sn * py), ay = vby + (c * py - sn * px);
            vbx = pushed ? ax : vbx;
            vby = pushed ? ay : vby;
        }
        // 8. integrate the base
        if constexpr (FLY) {
            // F1 the ballistic candidate, F2 the airborne test, F3 the take-off velocity of a grounded substep, F4 the crash,
            // F5 the selects (include/dtc_hip.h)
            const float vzb = vz - gdt;
            const float zb = z + vzb * k.dt;
            air = (zb - bz) > k.eps;
            float suz = 0.f;
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (ct[l]) suz = suz + sv[l][2];
            const float vzg = -(suz / nc);
            crashed = crashed || (!air && (bz - z) > d.f.max_step_up && elen != 1);
            const float gx = c * vbx - sn * vby, gy = sn * vbx + c * vby;
            Vwx = air ? Vwx : gx, Vwy = air ? Vwy : gy;
            w = air ? w_air : w;
            vz = air ? vzb : vzg;
            z = air ? zb : bz;
            nc = air ? 0.0f : nc;
#pragma unroll
            for (int l = 0; l < 4; ++l) ct[l] = ct[l] && !air;
            if constexpr (TILT) {
                nx = air ? n_air[0] : nx, ny = air ? n_air[1] : ny, nz = air ? n_air[2] : nz;
                wx = air ? 0.0f : wx, wy = air ? 0.0f : wy;
            }
            x = x + Vwx * k.dt;
            y = y + Vwy * k.dt;
        } else {
            x = x + (c * vbx - sn * vby) * k.dt;
            y = y + (sn * vbx + c * vby) * k.dt;
            vz = (bz - z) / k.dt;
            z = bz;
        }
        const float ee = k.half_dt * w;
        const float zn = qz + ee * qw, wn = qw - ee * qz;
        const float rq = sqrtf(zn * zn + wn * wn);
        qz = zn / rq;
        qw = wn / rq;
        if constexpr (ACT) {                                                       // 8p. the push decays, and ends below the floor
            px = px * d.a.keep, py = py * d.a.keep;
            if (px * px + py * py < d.a.floor2) px = 0.0f, py = 0.0f;
        }
    }

    // ---- the env's rows, once.  Every load of the bookkeeping below that another lane's store could change is issued first.
    // The 39 pointers of the descriptor and the constants do not fit the scalar registers at once: the rows written from here on take
    // their pointers from the kernel-argument segment (the descriptor is its first member) behind a barrier the compiler cannot
    // hoist the loads across, so they are not held through the loop above.
    unsigned long long args = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(args));
    const __attribute__((address_space(4))) DtcSimStep* o = (const __attribute__((address_space(4))) DtcSimStep*)args;
    using DescFly = SimDesc<ACT, true>;
    constexpr size_t fly_at = offsetof(DescFly, f);                                // FLY: where the flight struct lies in the segment
    const int C = k.C, T = k.T;
    const float cmd_old = lane < C ? o->commands[e * C + lane] : 0.f;               // the commands as they stand (cmd_buffer[-1])
    const float c = 1.0f - 2.0f * (qz * qz), sn = 2.0f * (qz * qw);
    float Vx = c * vbx - sn * vby, Vy = sn * vbx + c * vby;
    float fz = k.weight / nc;
    if constexpr (FLY) {                                                           // airborne: the carried world velocity, seen from the new yaw
        const float ax = c * Vwx + sn * Vwy, ay = c * Vwy - sn * Vwx;
        Vx = air ? Vwx : Vx, Vy = air ? Vwy : Vy;
        vbx = air ? ax : vbx, vby = air ? ay : vby;
        fz = air ? 0.0f : fz;
    }
    // ACT: a new push (the host's flag, legged_robot.py:546-553, :673-678) is the pending push of the next step and overwrites the
    // root's planar velocity, after base_lin_vel and the foot velocities took the old one.  Every lane draws the same two values.
    float rvx = Vx, rvy = Vy;
    if constexpr (ACT) {
        const __attribute__((address_space(4))) DtcSimActuator* oa =
            (const __attribute__((address_space(4))) DtcSimActuator*)(args + offsetof(SimDesc<true>, a));
        if (oa->push && oa->push_now) {
            float u0, u1;
            if (oa->u_push) {
                u0 = oa->u_push[e * 2], u1 = oa->u_push[e * 2 + 1];
            } else {
                const U4 r = philox4x32_10(U4{(unsigned)n, 1u, k.ctr_lo, k.ctr_hi}, k.seed_lo, k.seed_hi);
                u0 = (float)(r.x >> 8) * 5.9604644775390625e-08f;
                u1 = (float)(r.y >> 8) * 5.9604644775390625e-08f;
            }
            px = oa->push_span * u0 + oa->push_lo;
            py = oa->push_span * u1 + oa->push_lo;
            rvx = px, rvy = py;
        }
        if (joint) {
#pragma unroll
            for (int i = 0; i < 6; ++i) oa->lag_state[(e * 6 + i) * D + lane] = lg[i];
        }
        if (oa->push && lane < 2) oa->push_vel[e * 2 + lane] = lane == 0 ? px : py;
    }
    // TILT: everything below takes the NEW tilt, as it takes the new yaw.  bl, ba: the base velocities in the body frame (Rt^T);
    // oq: q_yaw (x) q_tilt, q_tilt = (-ny, nx, 0, 1 + nz) / sqrt(2 (1 + nz))
    TiltR R{1.f, 0.f, 1.f};
    float bl[3] = {vbx, vby, vz}, ba[3] = {0.0f, 0.0f, w}, Wx = 0.f, Wy = 0.f, oq[4] = {0.0f, 0.0f, qz, qw};
    if constexpr (TILT) {
        R = tilt_entries(nx, ny, nz);
        const float vv[3] = {vbx, vby, vz}, wv[3] = {wx, wy, w};
        tilt_rotate_t(R, nx, ny, nz, vv, bl);
        tilt_rotate_t(R, nx, ny, nz, wv, ba);
        Wx = c * wx - sn * wy, Wy = sn * wx + c * wy;
        const float k1 = 1.0f + nz;
        const float dn = sqrtf(2.0f * k1);
        const float tx = (-ny) / dn, ty = nx / dn, tw = k1 / dn;
        oq[0] = qw * tx - qz * ty, oq[1] = qw * ty + qz * tx, oq[2] = qz * tw, oq[3] = qw * tw;
    }

    if (joint) {
        o->dof_pos[e * o->dof_pos_row_stride + lane * o->dof_pos_elem_stride] = q;
        o->dof_vel[e * o->dof_vel_row_stride + lane * o->dof_vel_elem_stride] = qd;
        o->torques[e * D + lane] = tau;
        o->actions[e * D + lane] = a;
    }
    if (lane < 13) {
        float v = 0.f;
        v = lane == 0 ? x : v, v = lane == 1 ? y : v, v = lane == 2 ? z : v, v = lane == 5 ? oq[2] : v, v = lane == 6 ? oq[3] : v;
        v = lane == 7 ? rvx : v, v = lane == 8 ? rvy : v, v = lane == 9 ? vz : v, v = lane == 12 ? w : v;
        if constexpr (TILT) v = lane == 3 ? oq[0] : v, v = lane == 4 ? oq[1] : v, v = lane == 10 ? Wx : v, v = lane == 11 ? Wy : v;
        o->root_states[e * 13 + lane] = v;
    }
    if (lane < 3) {
        o->base_lin_vel[e * 3 + lane] = lane == 0 ? bl[0] : (lane == 1 ? bl[1] : bl[2]);
        o->last_base_ang_vel[e * 3 + lane] = old_ang;
        o->base_ang_vel[e * 3 + lane] = lane == 0 ? ba[0] : (lane == 1 ? ba[1] : ba[2]);
        if constexpr (TILT) o->projected_gravity[e * 3 + lane] = lane == 0 ? nx : (lane == 1 ? ny : -nz);
        else o->projected_gravity[e * 3 + lane] = lane == 2 ? -1.0f : 0.0f;
        o->base_pos[e * 3 + lane] = lane == 0 ? x : (lane == 1 ? y : z);
    }
    if (lane < 4) o->base_quat[e * 4 + lane] = lane == 0 ? oq[0] : (lane == 1 ? oq[1] : (lane == 2 ? oq[2] : oq[3]));
    // foot rows (lanes 16 + 6 l + i: position i < 3, velocity i >= 3) and thigh rows (lanes 40 + 3 l + i) of rigid_body_state
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        float r[3] = {p[l][0], p[l][1], p[l][2]}, sv[3] = {u[l][0], u[l][1], u[l][2]};
        if constexpr (TILT) tilt_rotate(R, nx, ny, nz, p[l], r), tilt_rotate(R, nx, ny, nz, u[l], sv);
        float rx = sv[0] - w * r[1], ry = sv[1] + w * r[0], rz = sv[2];
        if constexpr (TILT) rx = rx + wy * r[2], ry = ry - wx * r[2], rz = rz + (wx * r[1] - wy * r[0]);      // the tilt rate's lever arm
        const float f0 = x + (c * r[0] - sn * r[1]), f1 = y + (sn * r[0] + c * r[1]), f2 = z + r[2];
        const float g0 = Vx + (c * rx - sn * ry), g1 = Vy + (sn * rx + c * ry), g2 = vz + rz;
        const int i = lane - (16 + 6 * l);
        if (i >= 0 && i < 6) {
            const float v = i == 0 ? f0 : (i == 1 ? f1 : (i == 2 ? f2 : (i == 3 ? g0 : (i == 4 ? g1 : g2))));
            o->rigid_body_state[(e * k.B + k.feet[l]) * 13 + (i < 3 ? i : i + 4)] = v;
        }
    }
    if (lane >= 40 && lane < 52) {
        const int l = (lane - 40) / 3, m = lane - 40 - 3 * l;
        float hp[3] = {o->hip_offset[l * 3], o->hip_offset[l * 3 + 1], o->hip_offset[l * 3 + 2]};
        if constexpr (TILT) {
            const float hb[3] = {hp[0], hp[1], hp[2]};
            tilt_rotate(R, nx, ny, nz, hb, hp);
        }
        const float t0 = x + (c * hp[0] - sn * hp[1]), t1 = y + (sn * hp[0] + c * hp[1]), t2 = z + hp[2];
        const float v = m == 0 ? t0 : (m == 1 ? t1 : t2);
#pragma unroll
        for (int ll = 0; ll < 4; ++ll)                                             // constant index into the by-value struct
            if (l == ll) o->rigid_body_state[(e * k.B + k.thighs[ll]) * 13 + m] = v;
    }
    for (int i = lane; i < k.B * 3; i += 64) {
        float v = 0.f;
#pragma unroll
        for (int l = 0; l < 4; ++l) v = (i == k.feet[l] * 3 + 2 && ct[l]) ? fz : v;
        if constexpr (FLY) {                                                       // a crash: the base's own contact force (body 0, z)
            const __attribute__((address_space(4))) DtcSimFlight* of = (const __attribute__((address_space(4))) DtcSimFlight*)(args + fly_at);
            v = (crashed && i == 2) ? of->crash_force : v;
        }
        o->contact_forces[e * k.B * 3 + i] = v;
    }
    if constexpr (FLY) {
        const __attribute__((address_space(4))) DtcSimFlight* of = (const __attribute__((address_space(4))) DtcSimFlight*)(args + fly_at);
        if (lane == 0) of->airborne[e] = air ? 1 : 0;
        if (lane == 1) of->crashed[e] = crashed ? 1 : 0;
    }

    // ---- bookkeeping, in the reference's order: episode length, the ring buffers [T, N, .] (each env shifts its own T entries:
    // 64 entries are loaded, then stored one slot down), the command resample, the contact filter
    for (int i0 = 0; i0 < T * 2; i0 += 64) {
        const int i = i0 + lane, t = i >> 1, col = i & 1;
        if (i < T * 2) {
            const float v = t + 1 < T ? o->lin_vel_buffer[((long long)(t + 1) * N + e) * 2 + col] : (col == 0 ? bl[0] : bl[1]);
            o->lin_vel_buffer[((long long)t * N + e) * 2 + col] = v;
        }
    }
    for (int i0 = 0; i0 < T; i0 += 64) {
        const int t = i0 + lane;
        if (t < T) {
            const float v = t + 1 < T ? o->ang_vel_buffer[(long long)(t + 1) * N + e] : ba[2];
            o->ang_vel_buffer[(long long)t * N + e] = v;
        }
    }
    for (int i0 = 0; i0 < T * C; i0 += 64) {
        const int i = i0 + lane, t = i / C, col = i - t * C;
        const float newest = __shfl(cmd_old, col, 64);                             // by every lane: the source lanes must be active
        if (i < T * C) {
            const float v = t + 1 < T ? o->cmd_buffer[((long long)(t + 1) * N + e) * C + col] : newest;
            o->cmd_buffer[((long long)t * N + e) * C + col] = v;
        }
    }
    if (lane == 0) {
        o->episode_length_buf[e] = elen;
        if (elen % k.resample == 0) {                                              // _resample_commands, :573-591
            float u0, u1, u2;
            if (o->u_cmd) {
                u0 = o->u_cmd[e * 3], u1 = o->u_cmd[e * 3 + 1], u2 = o->u_cmd[e * 3 + 2];
            } else {
                const U4 r = philox4x32_10(U4{(unsigned)n, 0u, k.ctr_lo, k.ctr_hi}, k.seed_lo, k.seed_hi);
                u0 = (float)(r.x >> 8) * 5.9604644775390625e-08f;                  // [0, 1): 24 uniform bits
                u1 = (float)(r.y >> 8) * 5.9604644775390625e-08f;
                u2 = (float)(r.z >> 8) * 5.9604644775390625e-08f;
            }
            const float cx = k.cmd_x.span * u0 + k.cmd_x.lo;
            const float cy = k.cmd_y.span * u1 + k.cmd_y.lo;
            const float keep = sqrtf(cx * cx + cy * cy) > 0.1f ? 1.f : 0.f;
            float* cm = o->commands + e * C;
            cm[k.heading ? 3 : 2] = k.cmd_third.span * u2 + k.cmd_third.lo;
            cm[0] = cx * keep;
            cm[1] = cy * keep;
        }
    }
    if (lane < 4) {                                                                // legged_robot.py:562-564
        const unsigned stance = (ct[0] ? 1u : 0u) | (ct[1] ? 2u : 0u) | (ct[2] ? 4u : 0u) | (ct[3] ? 8u : 0u);
        const bool contact = (((stance >> lane) & 1u) ? fz : 0.0f) > 1.0f;
        o->contact_filt[e * 4 + lane] = (contact || last_c != 0) ? 1 : 0;
        o->last_contacts[e * 4 + lane] = contact ? 1 : 0;
    }
}

Span span_of(const double r[2]) { return Span{(float)(r[1] - r[0]), (float)r[0]}; }

}  // namespace

extern "C" int dtc_sim_tilt_abi_sizes(int64_t* out, int cap) {
    const int64_t sz[] = {sizeof(DtcSimTilt)};
    if (cap > 0 && out) out[0] = sz[0];
    return 1;
}

extern "C" int dtc_sim_abi_sizes(int64_t* out, int cap) {
    const int64_t sz[] = {sizeof(DtcSimCfg), sizeof(DtcSimStep)};
    for (int i = 0; i < 2 && i < cap && out; ++i) out[i] = sz[i];
    return 2;
}

extern "C" int dtc_sim_act_abi_sizes(int64_t* out, int cap) {
    const int64_t sz[] = {sizeof(DtcSimActuator)};
    if (cap > 0 && out) out[0] = sz[0];
    return 1;
}

extern "C" int dtc_sim_fly_abi_sizes(int64_t* out, int cap) {
    const int64_t sz[] = {sizeof(DtcSimFlight)};
    if (cap > 0 && out) out[0] = sz[0];
    return 1;
}

// dtc_sim_step (tilt == nullptr), dtc_sim_step_tilt, dtc_sim_step_act (act != nullptr, either base) and dtc_sim_step_fly
// (fly != nullptr, any of the four): one validation, one descriptor, the eight instantiations of one kernel
static int sim_step_launch(const DtcSimStep* st, const DtcSimCfg* cfg, const DtcSimTilt* tilt, const DtcSimActuator* act, const DtcSimFlight* fly,
                           int N, void* stream) {
    DTC_REQUIRE(st && cfg, "null descriptor");
    DTC_REQUIRE(N > 0 && N <= (1 << 24), "N %d outside 1..2^24", N);
    const DtcSimStep& s = *st;
    const DtcSimCfg& c = *cfg;
    DTC_REQUIRE(c.num_dof == 12, "num_dof %d: the surrogate has four legs of three joints", c.num_dof);
    DTC_REQUIRE(c.num_bodies >= 1 && c.num_bodies <= (1 << 16), "num_bodies %d", c.num_bodies);
    for (int l = 0; l < 4; ++l)
        DTC_REQUIRE(c.feet[l] >= 0 && c.feet[l] < c.num_bodies && c.thighs[l] >= 0 && c.thighs[l] < c.num_bodies,
                    "leg %d: foot body %d / thigh body %d outside 0..%d", l, c.feet[l], c.thighs[l], c.num_bodies - 1);
    DTC_REQUIRE(c.num_commands >= (c.heading_command ? 4 : 3) && c.num_commands <= 64, "num_commands %d", c.num_commands);
    DTC_REQUIRE(c.decimation >= 1 && c.decimation <= 64, "decimation %d outside 1..64", c.decimation);
    DTC_REQUIRE(c.buffer_len >= 1 && c.buffer_len <= 64, "buffer_len %d outside 1..64", c.buffer_len);
    DTC_REQUIRE(c.resampling_steps >= 1, "resampling_steps %lld", (long long)c.resampling_steps);
    DTC_REQUIRE(c.sim_dt > 0.f && c.joint_inertia > 0.f && c.clip_actions >= 0.f && c.r_min >= 0.f, "sim_dt / joint_inertia / clip_actions / r_min");
    DTC_REQUIRE(c.rows >= 2 && c.cols >= 2 && (int64_t)c.rows * c.cols < ((int64_t)1 << 31) && c.horizontal_scale > 0.f, "terrain table %d x %d",
                c.rows, c.cols);
    DTC_REQUIRE(s.actions_in && s.Kp_factors && s.Kd_factors && s.motor_strengths && s.motor_offsets && s.height_samples, "null per-env input");
    DTC_REQUIRE(s.p_gains && s.d_gains && s.torque_limits && s.default_dof_pos && s.dof_pos_limits && s.hip_offset && s.foot_nominal &&
                s.leg_jacobian, "null table");
    DTC_REQUIRE(s.dof_pos && s.dof_vel && s.root_states && s.base_ang_vel && s.commands && s.episode_length_buf && s.last_contacts &&
                s.lin_vel_buffer && s.ang_vel_buffer && s.cmd_buffer, "null state tensor");
    DTC_REQUIRE(s.rigid_body_state && s.contact_forces && s.torques && s.actions && s.base_lin_vel && s.last_base_ang_vel &&
                s.projected_gravity && s.base_pos && s.base_quat && s.contact_filt, "null output tensor");
    // strided dof tensors: positive strides, rows that do not overlap
    DTC_REQUIRE(s.dof_pos_elem_stride >= 1 && s.dof_pos_row_stride >= (c.num_dof - 1) * s.dof_pos_elem_stride + 1 &&
                s.dof_vel_elem_stride >= 1 && s.dof_vel_row_stride >= (c.num_dof - 1) * s.dof_vel_elem_stride + 1, "dof_pos / dof_vel strides");

    SimK k{};
    k.B = c.num_bodies, k.C = c.num_commands, k.dec = c.decimation, k.heading = c.heading_command != 0, k.T = c.buffer_len;
    for (int l = 0; l < 4; ++l) k.feet[l] = c.feet[l], k.thighs[l] = c.thighs[l];
    k.resample = c.resampling_steps;
    k.dt = c.sim_dt, k.half_dt = 0.5f * c.sim_dt, k.action_scale = c.action_scale, k.clip = c.clip_actions, k.inertia = c.joint_inertia;
    k.eps = c.contact_eps, k.weight = c.weight, k.rmin2 = c.r_min * c.r_min;
    k.rows = c.rows, k.cols = c.cols, k.border = c.border_size, k.hscale = c.horizontal_scale, k.vscale = c.vertical_scale;
    k.cmd_x = span_of(c.lin_vel_x), k.cmd_y = span_of(c.lin_vel_y), k.cmd_third = span_of(c.heading_command ? c.heading : c.ang_vel_yaw);
    k.seed_lo = (unsigned)c.seed, k.seed_hi = (unsigned)(c.seed >> 32), k.ctr_lo = (unsigned)c.counter, k.ctr_hi = (unsigned)(c.counter >> 32);

    if (tilt) {
        DTC_REQUIRE(tilt->max_slope > 0.f && tilt->max_slope <= 1e3f && tilt->min_det >= 0.f, "max_slope %g outside (0, 1000] or min_det %g < 0",
                    (double)tilt->max_slope, (double)tilt->min_det);
        k.max_slope = tilt->max_slope, k.min_det = tilt->min_det;
    }
    if (act) {                                                                     // comparisons written so that a NaN is refused
        DTC_REQUIRE(act->lag_state, "null lag_state");
        DTC_REQUIRE(!act->push || act->push_vel, "null push_vel with pushes configured");
        for (int it = 0; it < c.decimation; ++it)
            DTC_REQUIRE(act->lag_choice[it] <= 5, "lag_choice[%d] = %d outside 0..5", it, (int)act->lag_choice[it]);
        DTC_REQUIRE(act->keep > 0.f && act->keep <= 1.f, "keep %g outside (0, 1]", (double)act->keep);
        DTC_REQUIRE(act->floor2 >= 0.f && act->push_span >= 0.f, "negative push floor %g or span %g", (double)act->floor2, (double)act->push_span);
    }

    if (fly) {                                                                     // comparisons written so that a NaN is refused
        DTC_REQUIRE(fly->airborne && fly->crashed, "null airborne / crashed");
        DTC_REQUIRE(fly->gravity >= 0.f && fly->max_step_up > 0.f, "gravity %g < 0 or max_step_up %g <= 0", (double)fly->gravity,
                    (double)fly->max_step_up);
        DTC_REQUIRE(fly->crash_force > 100.f, "crash_force %g not above the termination threshold of 100 N", (double)fly->crash_force);
        for (int l = 0; l < 4; ++l) DTC_REQUIRE(c.feet[l] != 0, "leg %d: foot body 0 is the base, which takes the crash force", l);
    }

    hipStream_t hs = (hipStream_t)stream;
    const dim3 grid((unsigned)dtc::ceil_div(N, 4)), block(256);
    if (fly) {
        const char* name = act ? (tilt ? "sim_step_tilt_act_fly" : "sim_step_act_fly") : (tilt ? "sim_step_tilt_fly" : "sim_step_fly");
        dtc::ProfScope prof(name, (double)N * (2050.0 + 12.0 * c.num_bodies + 8.0 * c.buffer_len * (3 + c.num_commands) + (act ? 592.0 : 0.0)), hs);
        if (act) {
            const SimDesc<true, true> d{s, *act, *fly};
            if (tilt) hipLaunchKernelGGL((sim_step_kernel<true, true, true>), grid, block, 0, hs, d, k, N);
            else hipLaunchKernelGGL((sim_step_kernel<false, true, true>), grid, block, 0, hs, d, k, N);
        } else {
            const SimDesc<false, true> d{s, *fly};
            if (tilt) hipLaunchKernelGGL((sim_step_kernel<true, false, true>), grid, block, 0, hs, d, k, N);
            else hipLaunchKernelGGL((sim_step_kernel<false, false, true>), grid, block, 0, hs, d, k, N);
        }
        return dtc::check_launch(name);
    }
    const char* name = act ? (tilt ? "sim_step_tilt_act" : "sim_step_act") : (tilt ? "sim_step_tilt" : "sim_step");
    dtc::ProfScope prof(name, (double)N * (2048.0 + 12.0 * c.num_bodies + 8.0 * c.buffer_len * (3 + c.num_commands) + (act ? 592.0 : 0.0)), hs);
    if (act) {
        const SimDesc<true> d{s, *act};
        if (tilt) hipLaunchKernelGGL((sim_step_kernel<true, true, false>), grid, block, 0, hs, d, k, N);
        else hipLaunchKernelGGL((sim_step_kernel<false, true, false>), grid, block, 0, hs, d, k, N);
    } else {
        const SimDesc<false> d{s};
        if (tilt) hipLaunchKernelGGL((sim_step_kernel<true, false, false>), grid, block, 0, hs, d, k, N);
        else hipLaunchKernelGGL((sim_step_kernel<false, false, false>), grid, block, 0, hs, d, k, N);
    }
    return dtc::check_launch(name);
}

extern "C" int dtc_sim_step(const DtcSimStep* st, const DtcSimCfg* cfg, int N, void* stream) {
    return sim_step_launch(st, cfg, nullptr, nullptr, nullptr, N, stream);
}

extern "C" int dtc_sim_step_tilt(const DtcSimStep* st, const DtcSimCfg* cfg, const DtcSimTilt* tilt, int N, void* stream) {
    DTC_REQUIRE(tilt, "null DtcSimTilt");
    return sim_step_launch(st, cfg, tilt, nullptr, nullptr, N, stream);
}

extern "C" int dtc_sim_step_act(const DtcSimStep* st, const DtcSimCfg* cfg, const DtcSimTilt* tilt, const DtcSimActuator* act, int N, void* stream) {
    DTC_REQUIRE(act, "null DtcSimActuator");
    return sim_step_launch(st, cfg, tilt, act, nullptr, N, stream);
}

extern "C" int dtc_sim_step_fly(const DtcSimStep* st, const DtcSimCfg* cfg, const DtcSimTilt* tilt, const DtcSimActuator* act, const DtcSimFlight* fly,
                                int N, void* stream) {
    DTC_REQUIRE(fly, "null DtcSimFlight");
    return sim_step_launch(st, cfg, tilt, act, fly, N, stream);
}
