// Env rewards for gfx950: LeggedRobot.compute_reward (legged_gym/envs/base/legged_robot.py:274-291) with all 34 `_reward_*` terms of
// LeggedRobotDTC (legged_robot.py:1321-1622, legged_robot_dtc.py:522-586) in ONE launch (dtc_env_rewards, include/dtc_hip.h).
//
// One 64-lane wavefront per env row, 4 rows per 256-thread workgroup.  Lanes hold one dof (lane < D), one foot (lane < 4), one
// penalised body, one ring-buffer row or one stride of the 693-point height row, as each term needs; every reduction is the DPP
// xor-butterfly of wave.hpp (fixed order: two launches give the same bits) or a ballot.  Terms run in the reference's order
// (alphabetical, termination after the clip), each behind `scale != 0` -- uniform over the launch, so no per-term arrays and no
// scratch; the state they change (feet_air_time, last_contacts, the stumble history, pitch_est) lives in registers between them.
//
// HBM / latency bound.  Algorithmic bytes per env with every term on (Lite3: D = 12, B = 17, 693 height points):
//   measured_heights row 2772 | root/base vel/gravity/commands 13+3+3+3+4 floats 104 | 8 [N,D] dof tensors 384 | contact_forces
//   B*12 = 204 | 4 [N,4,3] foot tensors 192 | contact_filt, last_contacts, stumble, reset, time_out 14 | feet_air_time 16 |
//   clearance 16 | mass, pitch_est 8 | terrain level 8 | ring buffers (4 rows of cmd, 1 of lin vel, 4 of yaw rate) 100 ->
//   ~3.8 KB read; written: rew_buf 4, state 4*4 + 4 + 4 + 4, episode sums read+write 2*4*n_active (24 terms: 192) -> ~0.2 KB.
//   About 3.9 KB/env, 16 MB at 4096 envs; the plane-fit coefficients [2,693] are shared by all envs (L2-resident).
//
// Numerics: -ffp-contract=off (build.py), each op a single fp32 op in the reference's order where that is cheap; the plane fit
// uses the constant least-squares rows instead of the reference's batched fp32 inverse (tests bound the difference).
#include "common.hpp"
#include "wave.hpp"

namespace {

__device__ __forceinline__ float foot_sum(float v, int lane) { return wave_sum(lane < 4 ? v : 0.f); }
__device__ __forceinline__ bool wave_any(bool p) { return __ballot(p) != 0ull; }
__device__ __forceinline__ float wave_count(bool p) { return (float)__popcll(__ballot(p)); }

// _reward_orientation / _reward_orientation_roll after the plane fit (legged_robot.py:1559-1596): pitch_est EMA, then the gravity
// direction (0, 0, -1) rotated into quat_from_euler_xyz(roll_clip, pitch_est, 0) by quat_rotate_inverse, in closed form.
__device__ __forceinline__ void plane_gravity(float pitch_c, float roll_c, float& pitch_est, float& px, float& py) {
    pitch_est = pitch_est * 0.2f + 0.8f * pitch_c;
    const float cr = cosf(roll_c * 0.5f), sr = sinf(roll_c * 0.5f);
    const float cp = cosf(pitch_est * 0.5f), sp = sinf(pitch_est * 0.5f);
    const float qx = sr * cp, qy = cr * sp, qz = -(sr * sp), qw = cr * cp;
    px = qy * qw * 2.0f - qx * qz * 2.0f;            // -(cross(q, g) * w * 2) + q * (q . g) * 2 with g = (0, 0, -1)
    py = -(qx * qw * 2.0f) - qy * qz * 2.0f;
}

__global__ __launch_bounds__(256) void env_rewards_kernel(const DtcRewardStep s, const DtcRewardCfg c, int N) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const int D = c.num_dof, C = s.num_commands;
    const long long nd = (long long)n * D;
    const bool is_dof = lane < D, is_foot = lane < 4;
    const int fl = is_foot ? lane : 0;                       // foot of this lane (lanes >= 4 read foot 0 and are masked)
    const long long nf = (long long)n * 4 + fl;
    const float* cmd = s.commands + (long long)n * C;
    const float cx = cmd[0], cy = cmd[1], cz = cmd[2];
    const float cmd_norm = sqrtf(cx * cx + cy * cy);
    const float* cf = s.contact_forces + ((long long)n * s.num_bodies + c.feet[fl]) * 3;
    const float fx = cf[0], fy = cf[1], fz = cf[2];
    const float fxy = sqrtf(fx * fx + fy * fy);
    // reward state of this lane's foot
    bool last_contact = s.last_contacts[nf] != 0;
    float air = 0.f;
    unsigned hist = 0;
    float pitch_est = 0.f;
    const float* sc = c.scale;
    float rew = 0.f;
    auto emit = [&](int id, float v) {
        const float r = v * sc[id];
        if (id != DTC_REW_TERMINATION) rew = rew + r;
        if (lane == 0) {
            const long long o = (long long)c.row[id] * N + n;
            s.episode_sums[o] = s.episode_sums[o] + r;
            if (s.per_term) s.per_term[o] = r;
        }
    };
    const float dpos = is_dof ? s.dof_pos[nd + lane] : 0.f;
    const float dvel = is_dof ? s.dof_vel[nd + lane] : 0.f;
    const float tau = is_dof ? s.torques[nd + lane] : 0.f;

    if (sc[DTC_REW_ACTION_RATE] != 0.f) {                                  // :1620
        const float d = is_dof ? s.last_actions[nd + lane] - s.actions[nd + lane] : 0.f;
        emit(DTC_REW_ACTION_RATE, wave_sum(d * d));
    }
    if (sc[DTC_REW_ANG_VEL_XY] != 0.f) {                                   // :1325
        const float* w = s.base_ang_vel + (long long)n * 3;
        emit(DTC_REW_ANG_VEL_XY, w[0] * w[0] + w[1] * w[1]);
    }
    if (sc[DTC_REW_BASE_HEIGHT] != 0.f) {                                  // dtc.py:531
        const float mean = foot_sum(s.foot_positions[nf * 3 + 2], lane) / 4.0f;
        const float d = (s.root_states[(long long)n * 13 + 2] - mean) - c.base_height_target;
        emit(DTC_REW_BASE_HEIGHT, d * d);
    }
    if (sc[DTC_REW_BIG_PITCH] != 0.f)                                      // dtc.py:522
        emit(DTC_REW_BIG_PITCH, fabsf(s.projected_gravity[(long long)n * 3]) > 0.6f ? 1.f : 0.f);
    if (sc[DTC_REW_COLLISION] != 0.f) {                                    // :1350
        bool hit = false;
        if (lane < c.n_penalised) {
            const float* b = s.contact_forces + ((long long)n * s.num_bodies + c.penalised[lane]) * 3;
            hit = sqrtf((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]) > 0.1f;
        }
        emit(DTC_REW_COLLISION, wave_count(hit));
    }
    if (sc[DTC_REW_DOF_ACC] != 0.f) {                                      // :1342
        const float a = is_dof ? (s.last_dof_vel[nd + lane] - dvel) / c.dt : 0.f;
        emit(DTC_REW_DOF_ACC, wave_sum(a * a));
    }
    if (sc[DTC_REW_DOF_POS_LIMITS] != 0.f) {                               // :1358
        float o = 0.f;
        if (is_dof) {
            o = -fminf(dpos - s.dof_pos_limits[lane * 2], 0.f);
            o = o + fmaxf(dpos - s.dof_pos_limits[lane * 2 + 1], 0.f);
        }
        emit(DTC_REW_DOF_POS_LIMITS, wave_sum(o));
    }
    if (sc[DTC_REW_DOF_VEL] != 0.f) emit(DTC_REW_DOF_VEL, wave_sum(dvel * dvel));      // :1338
    if (sc[DTC_REW_DOF_VEL_LIMITS] != 0.f) {                               // :1364
        const float o = is_dof ? fminf(fmaxf(fabsf(dvel) - s.dof_vel_limits[lane] * c.soft_dof_vel_limit, 0.f), 1.f) : 0.f;
        emit(DTC_REW_DOF_VEL_LIMITS, wave_sum(o));
    }
    if (sc[DTC_REW_FEET_AIR_TIME] != 0.f) {                                // :1386-1412
        air = s.feet_air_time[nf];
        const bool contact = fz > 1.0f;
        const bool filt = contact || last_contact;
        last_contact = contact;
        const bool first = air > 0.f && filt;
        air = air + c.dt;
        float r = foot_sum((air - 0.5f) * (first ? 1.f : 0.f), lane);
        r = r * (cmd_norm > 0.1f ? 1.f : 0.f);
        air = air * (filt ? 0.f : 1.f);
        emit(DTC_REW_FEET_AIR_TIME, r);
    }
    if (sc[DTC_REW_FEET_CONTACT_FORCES] != 0.f) {                          // :1426
        const float f = sqrtf((fx * fx + fy * fy) + fz * fz);
        emit(DTC_REW_FEET_CONTACT_FORCES, foot_sum(fmaxf(f - c.max_contact_force, 0.f), lane));
    }
    if (sc[DTC_REW_FEET_SLIP] != 0.f) {                                    // :1494 (sees the last_contacts of feet_air_time)
        const bool filt = fz > 1.0f || last_contact;
        const float* v = s.foot_velocities + nf * 3;
        const float sp = sqrtf(v[0] * v[0] + v[1] * v[1]);
        emit(DTC_REW_FEET_SLIP, foot_sum((filt ? 1.f : 0.f) * (sp * sp), lane));
    }
    if (sc[DTC_REW_FEET_STUMBLE] != 0.f)                                   // dtc.py:526
        emit(DTC_REW_FEET_STUMBLE, wave_any(is_foot && fxy > 3.0f * fabsf(fz)) ? 1.f : 0.f);
    if (sc[DTC_REW_FOOT_ACC] != 0.f) {                                     // :1525
        const float mask = s.terrain_levels[n] > 5 ? 0.2f : 1.0f;
        const float* v = s.foot_velocities + nf * 3;
        const float* lv = s.last_foot_velocities + nf * 3;
        const float ax = (lv[0] - v[0]) / c.dt, ay = (lv[1] - v[1]) / c.dt, az = (lv[2] - v[2]) / c.dt;
        const float a = sqrtf((ax * ax + ay * ay) + az * az);
        emit(DTC_REW_FOOT_ACC, foot_sum(fmaxf(mask * (a - c.max_acc), 0.f), lane));
    }
    if (sc[DTC_REW_FOOT_CLEARANCE] != 0.f) {                               // :1474-1492
        float clr;
        if (s.height_samples) {                                            // _get_foot_clearance, :1443-1472
            const float* p = s.foot_positions + nf * 3;
            const float x = (p[0] + s.border_size) / s.horizontal_scale, y = (p[1] + s.border_size) / s.horizontal_scale;
            const int xmax = s.rows - 3, ymax = s.cols - 3;
            const int px = !(x >= 1.0f) ? 1 : (x >= (float)xmax ? xmax : (int)x);      // .long() then clip(1, dim - 3); NaN -> 1
            const int py = !(y >= 1.0f) ? 1 : (y >= (float)ymax ? ymax : (int)y);
            const int16_t* t = s.height_samples;
            const long long cl = s.cols;
            // px, py >= 1 and <= dim - 3, so i, j lie in [-1, dim - 1]: the reference's index -1 (px - 2 at px == 1) wraps to the
            // last row / column, as torch indexing does
            auto at = [&](int i, int j) {
                i = i < 0 ? i + s.rows : i;
                j = j < 0 ? j + s.cols : j;
                return (int)t[(long long)i * cl + j];
            };
            int h = at(px, py);
            h = max(h, at(px + 1, py));
            h = max(h, at(px, py + 1));
            h = max(h, at(px + 2, py));
            h = max(h, at(px, py + 2));
            h = max(h, at(px + 1, py + 1));
            h = max(h, at(px - 1, py));
            h = max(h, at(px, py - 1));
            h = max(h, at(px - 2, py));
            h = max(h, at(px, py - 2));
            clr = p[2] - (float)h * s.vertical_scale;
            if (s.foot_clearance && is_foot) s.foot_clearance[nf] = clr;
        } else {
            clr = s.foot_clearance[nf];
        }
        hist = s.stumble[nf];
        const bool stumb = fxy > 4.0f * fabsf(fz);
        hist = ((hist << 1) | (stumb ? 1u : 0u)) & 0x1Fu;
        emit(DTC_REW_FOOT_CLEARANCE, wave_count(is_foot && hist == 0u && clr > 0.18f));
    }
    if (sc[DTC_REW_FOOTHOLD_MISS] != 0.f)                                  // dtc.py:536
        emit(DTC_REW_FOOTHOLD_MISS, wave_any(is_foot && s.foot_positions[nf * 3 + 2] < 0.f) ? 1.f : 0.f);
    if (sc[DTC_REW_HIP_POS] != 0.f) {                                      // :1504
        const float q = lane < c.n_hip ? s.dof_pos[nd + c.hip[lane]] : 0.f;
        emit(DTC_REW_HIP_POS, wave_sum(q * q));
    }
    if (sc[DTC_REW_LIN_VEL_Z] != 0.f) {                                    // :1321
        const float v = s.base_lin_vel[(long long)n * 3 + 2];
        emit(DTC_REW_LIN_VEL_Z, v * v);
    }
    if (sc[DTC_REW_ORIENTATION] != 0.f || sc[DTC_REW_ORIENTATION_ROLL] != 0.f) {          // get_plane_norm, :1535-1557
        const float* h = s.measured_heights + (long long)n * c.num_points;
        float ax = 0.f, by = 0.f;
        for (int p = lane; p < c.num_points; p += 64) {
            const float v = h[p];
            ax = ax + v * c.plane[p];
            by = by + v * c.plane[c.num_points + p];
        }
        ax = wave_sum(ax);
        by = wave_sum(by);
        const float nrm = sqrtf((ax * ax + by * by) + 1.0f);
        const float pitch = atanf(-ax / nrm), roll = -atanf(-by / nrm);                // p_norm = -plane_vector
        const float pitch_c = (pitch >= -0.1f && pitch <= 0.1f) ? 0.f : pitch;
        const float roll_c = (roll >= -0.1f && roll <= 0.1f) ? 0.f : roll;
        pitch_est = s.pitch_est[n];
        const float* g = s.projected_gravity + (long long)n * 3;
        float px, py;
        if (sc[DTC_REW_ORIENTATION] != 0.f) {                              // :1559
            plane_gravity(pitch_c, roll_c, pitch_est, px, py);
            const float d = g[0] - px;
            emit(DTC_REW_ORIENTATION, d * d);
        }
        if (sc[DTC_REW_ORIENTATION_ROLL] != 0.f) {                         // :1579
            plane_gravity(pitch_c, roll_c, pitch_est, px, py);
            emit(DTC_REW_ORIENTATION_ROLL, fabsf(g[1] - py));
        }
    }
    if (sc[DTC_REW_POS_ACC] != 0.f) {                                      // :1600 (the later definition: half-extents / 2)
        float e = 0.f;
        if (lane < 8) {
            const float* v = s.base_lin_vel + (long long)n * 3;
            const float* w = s.base_ang_vel + (long long)n * 3;
            const float rx = (lane & 4) ? 0.15f : -0.15f, ry = (lane & 2) ? 0.1f : -0.1f, rz = (lane & 1) ? 0.075f : -0.075f;
            const float vx = v[0] + (w[1] * rz - w[2] * ry), vy = v[1] + (w[2] * rx - w[0] * rz), vz = v[2] + (w[0] * ry - w[1] * rx);
            const float m = sqrtf((vx * vx + vy * vy) + vz * vz);
            e = m * m;
        }
        emit(DTC_REW_POS_ACC, wave_sum(e));
    }
    if (sc[DTC_REW_POWER] != 0.f || sc[DTC_REW_POWERCHANGE] != 0.f) {
        const float p = wave_sum(fmaxf(tau * dvel, 0.f));
        if (sc[DTC_REW_POWER] != 0.f) emit(DTC_REW_POWER, p);              // :1435
        if (sc[DTC_REW_POWERCHANGE] != 0.f) {                              // :1613
            const float q = p / ((s.robot_mass[n] * 9.815f) * fmaxf(cx, 1.0f));
            emit(DTC_REW_POWERCHANGE, q * q);
        }
    }
    if (sc[DTC_REW_SMOOTH] != 0.f) {                                       // :1440
        const float d = is_dof ? (s.actions[nd + lane] - 2.0f * s.last_actions[nd + lane]) + s.last_actions_2[nd + lane] : 0.f;
        emit(DTC_REW_SMOOTH, wave_sum(d * d));
    }
    if (sc[DTC_REW_SOFT_TRACKING_ANG_VEL] != 0.f) {                        // dtc.py:555: last 4 rows, 0 / 1 at tolerance 0.15
        float e = 0.f;
        if (lane < 4) {
            const long long r = 6 + lane;
            const float d = (s.cmd_buffer[(r * N + n) * C + 2] - s.ang_vel_buffer[r * N + n]) / c.ang_vel_yaw_max;
            const float d2 = (d * d <= 0.0225f) ? 0.f : 1.f;
            e = expf(-d2 / c.tracking_sigma);
        }
        emit(DTC_REW_SOFT_TRACKING_ANG_VEL, wave_sum(e) / 4.0f);
    }
    if (sc[DTC_REW_SOFT_TRACKING_LIN_VEL] != 0.f) {                        // dtc.py:542 (sic: ONE velocity row, buffer[-3])
        float e = 0.f;
        if (lane < 3) {
            const long long r = 7 + lane;
            const float* v = s.lin_vel_buffer + (7ll * N + n) * 2;
            const float dx = (s.cmd_buffer[(r * N + n) * C] - v[0]) / c.lin_vel_x_max;
            const float dy = (s.cmd_buffer[(r * N + n) * C + 1] - v[1]) / c.lin_vel_x_max;
            e = expf(-(dx * dx + dy * dy) / c.tracking_sigma);
        }
        emit(DTC_REW_SOFT_TRACKING_LIN_VEL, wave_sum(e) / 3.0f);
    }
    if (sc[DTC_REW_STAND_STILL] != 0.f) {                                  // :1422
        const float d = is_dof ? fabsf(dpos - s.default_dof_pos[lane]) : 0.f;
        emit(DTC_REW_STAND_STILL, wave_sum(d) * (cmd_norm < 0.1f ? 1.f : 0.f));
    }
    if (sc[DTC_REW_STUMBLE] != 0.f)                                        // :1417
        emit(DTC_REW_STUMBLE, wave_any(is_foot && fxy > 5.0f * fabsf(fz)) ? 1.f : 0.f);
    if (sc[DTC_REW_TORQUE_LIMITS] != 0.f) {                                // :1369
        const float o = is_dof ? fmaxf(fabsf(tau) - s.torque_limits[lane] * c.soft_torque_limit, 0.f) : 0.f;
        emit(DTC_REW_TORQUE_LIMITS, wave_sum(o));
    }
    if (sc[DTC_REW_TORQUES] != 0.f) emit(DTC_REW_TORQUES, wave_sum(tau * tau));        // :1334
    if (sc[DTC_REW_TRACKING_ANG_VEL] != 0.f) {                             // dtc.py:571
        const float d = cz - s.base_ang_vel[(long long)n * 3 + 2];
        emit(DTC_REW_TRACKING_ANG_VEL, expf(-(d * d) / c.tracking_sigma));
    }
    if (sc[DTC_REW_TRACKING_LIN_VEL] != 0.f) {                             // :1373
        const float* v = s.base_lin_vel + (long long)n * 3;
        const float dx = (cx - v[0]) / c.lin_vel_x_max, dy = (cy - v[1]) / c.lin_vel_x_max;
        emit(DTC_REW_TRACKING_LIN_VEL, expf(-(dx * dx + dy * dy) / c.tracking_sigma));
    }
    if (sc[DTC_REW_TRACKING_OPTIMAL_FOOTHOLDS] != 0.f) {                   // dtc.py:577
        const float* p = s.foot_positions + nf * 3;
        const float* o = s.optimal_footholds_world + nf * 3;
        const float dx = p[0] - o[0], dy = p[1] - o[1];
        const float r = -logf(0.8f + sqrtf(dx * dx + dy * dy));
        emit(DTC_REW_TRACKING_OPTIMAL_FOOTHOLDS, foot_sum(s.contact_filt[nf] ? r : 0.f, lane));
    }
    if (c.only_positive_rewards) rew = rew < 0.f ? 0.f : rew;             // torch.clip(min=0) keeps NaN
    if (sc[DTC_REW_TERMINATION] != 0.f) {                                  // :1354, after the clip
        const float t = (s.reset_buf[n] && !s.time_out_buf[n]) ? 1.f : 0.f;
        emit(DTC_REW_TERMINATION, t);
        rew = rew + t * sc[DTC_REW_TERMINATION];
    }
    if (lane == 0) {
        s.rew_buf[n] = rew;
        if (sc[DTC_REW_ORIENTATION] != 0.f || sc[DTC_REW_ORIENTATION_ROLL] != 0.f) s.pitch_est[n] = pitch_est;
    }
    if (is_foot) {
        if (sc[DTC_REW_FEET_AIR_TIME] != 0.f) {
            s.feet_air_time[nf] = air;
            s.last_contacts[nf] = last_contact ? 1 : 0;
        }
        if (sc[DTC_REW_FOOT_CLEARANCE] != 0.f) s.stumble[nf] = (uint8_t)hist;
    }
}

}  // namespace

extern "C" int dtc_env_rewards(const DtcRewardStep* st, const DtcRewardCfg* cfg, int N, void* stream) {
    DTC_REQUIRE(st && cfg, "null descriptor");
    DTC_REQUIRE(N >= 0, "N < 0");
    const DtcRewardCfg& c = *cfg;
    const DtcRewardStep& s = *st;
    DTC_REQUIRE(c.num_dof >= 1 && c.num_dof <= 64, "num_dof %d outside 1..64", c.num_dof);
    DTC_REQUIRE(c.n_penalised >= 0 && c.n_penalised <= 32 && c.n_hip >= 0 && c.n_hip <= 16, "index lists too long");
    DTC_REQUIRE(s.num_bodies >= 1 && s.num_commands >= 3, "num_bodies %d, num_commands %d", s.num_bodies, s.num_commands);
    int n_active = 0;
    for (int i = 0; i < DTC_REWARD_TERMS; ++i)
        if (c.scale[i] != 0.f) ++n_active;
    for (int i = 0; i < DTC_REWARD_TERMS; ++i)
        DTC_REQUIRE(c.scale[i] != 0.f ? (c.row[i] >= 0 && c.row[i] < n_active) : c.row[i] == -1, "bad row of term %d", i);
    for (int i = 0; i < 4; ++i) DTC_REQUIRE(c.feet[i] >= 0 && c.feet[i] < s.num_bodies, "foot index out of range");
    for (int i = 0; i < c.n_penalised; ++i) DTC_REQUIRE(c.penalised[i] >= 0 && c.penalised[i] < s.num_bodies, "penalised index out of range");
    for (int i = 0; i < c.n_hip; ++i) DTC_REQUIRE(c.hip[i] >= 0 && c.hip[i] < c.num_dof, "hip index out of range");
    if (N == 0) return DTC_OK;
    DTC_REQUIRE(s.rew_buf && s.episode_sums && s.commands && s.contact_forces && s.last_contacts, "null pointer");
    auto on = [&](int id) { return c.scale[id] != 0.f; };
    const bool orient = on(DTC_REW_ORIENTATION) || on(DTC_REW_ORIENTATION_ROLL);
    DTC_REQUIRE(!orient || (s.measured_heights && s.pitch_est && s.projected_gravity && c.plane && c.num_points > 0), "plane-fit inputs");
    DTC_REQUIRE(!on(DTC_REW_FOOT_CLEARANCE) || (s.stumble && (s.height_samples || s.foot_clearance)), "foot_clearance inputs");
    DTC_REQUIRE(!s.height_samples || (s.rows >= 5 && s.cols >= 5 && (int64_t)s.rows * s.cols < (1ll << 31)), "bad height table shape");
    DTC_REQUIRE(!on(DTC_REW_FEET_AIR_TIME) || s.feet_air_time, "feet_air_time state");
    DTC_REQUIRE(!(on(DTC_REW_SOFT_TRACKING_LIN_VEL) || on(DTC_REW_SOFT_TRACKING_ANG_VEL)) ||
                (s.cmd_buffer && s.lin_vel_buffer && s.ang_vel_buffer), "ring buffers");
    const bool dofs = on(DTC_REW_ACTION_RATE) || on(DTC_REW_DOF_ACC) || on(DTC_REW_DOF_POS_LIMITS) || on(DTC_REW_DOF_VEL) ||
                      on(DTC_REW_DOF_VEL_LIMITS) || on(DTC_REW_HIP_POS) || on(DTC_REW_POWER) || on(DTC_REW_POWERCHANGE) ||
                      on(DTC_REW_SMOOTH) || on(DTC_REW_STAND_STILL) || on(DTC_REW_TORQUE_LIMITS) || on(DTC_REW_TORQUES);
    DTC_REQUIRE(!dofs || (s.dof_pos && s.dof_vel && s.torques), "dof inputs");
    DTC_REQUIRE(!(on(DTC_REW_ACTION_RATE) || on(DTC_REW_SMOOTH)) || (s.actions && s.last_actions && (!on(DTC_REW_SMOOTH) || s.last_actions_2)),
                "action inputs");
    DTC_REQUIRE(!on(DTC_REW_DOF_ACC) || s.last_dof_vel, "last_dof_vel");
    DTC_REQUIRE(!on(DTC_REW_DOF_POS_LIMITS) || s.dof_pos_limits, "dof_pos_limits");
    DTC_REQUIRE(!on(DTC_REW_DOF_VEL_LIMITS) || s.dof_vel_limits, "dof_vel_limits");
    DTC_REQUIRE(!on(DTC_REW_TORQUE_LIMITS) || s.torque_limits, "torque_limits");
    DTC_REQUIRE(!on(DTC_REW_STAND_STILL) || s.default_dof_pos, "default_dof_pos");
    DTC_REQUIRE(!on(DTC_REW_POWERCHANGE) || s.robot_mass, "robot_mass");
    DTC_REQUIRE(!(on(DTC_REW_ANG_VEL_XY) || on(DTC_REW_POS_ACC) || on(DTC_REW_TRACKING_ANG_VEL)) || s.base_ang_vel, "base_ang_vel");
    DTC_REQUIRE(!(on(DTC_REW_LIN_VEL_Z) || on(DTC_REW_POS_ACC) || on(DTC_REW_TRACKING_LIN_VEL)) || s.base_lin_vel, "base_lin_vel");
    DTC_REQUIRE(!on(DTC_REW_BIG_PITCH) || s.projected_gravity, "projected_gravity");
    DTC_REQUIRE(!(on(DTC_REW_BASE_HEIGHT) || on(DTC_REW_FOOTHOLD_MISS) || on(DTC_REW_TRACKING_OPTIMAL_FOOTHOLDS) ||
                  (on(DTC_REW_FOOT_CLEARANCE) && s.height_samples)) || s.foot_positions, "foot_positions");
    DTC_REQUIRE(!on(DTC_REW_BASE_HEIGHT) || s.root_states, "root_states");
    DTC_REQUIRE(!(on(DTC_REW_FEET_SLIP) || on(DTC_REW_FOOT_ACC)) || s.foot_velocities, "foot_velocities");
    DTC_REQUIRE(!on(DTC_REW_FOOT_ACC) || (s.last_foot_velocities && s.terrain_levels), "foot_acc inputs");
    DTC_REQUIRE(!on(DTC_REW_TRACKING_OPTIMAL_FOOTHOLDS) || (s.optimal_footholds_world && s.contact_filt), "foothold inputs");
    DTC_REQUIRE(!on(DTC_REW_TERMINATION) || (s.reset_buf && s.time_out_buf), "reset_buf / time_out_buf");
    DTC_REQUIRE(N <= 400000000, "N too large");
    hipStream_t hs = (hipStream_t)stream;
    const double bytes = (double)N * (3900.0 + 8.0 * n_active);
    dtc::ProfScope prof("env_rewards", bytes, hs);
    hipLaunchKernelGGL(env_rewards_kernel, dim3((unsigned)dtc::ceil_div(N, 4)), dim3(256), 0, hs, s, c, N);
    return dtc::check_launch("env_rewards");
}
