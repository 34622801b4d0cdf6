/* dtc_hip.h -- C ABI of libdtc_hip.so, the MI355X (gfx950) hot path of Deep-Tracking-Control.
 *
 * The reference has no FFI: its hot path is Python calling torch.  Each entry
 * point below replaces the torch op sequence of the cited reference lines; the Python classes
 * in deep-tracking-control_amd/dtc_amd keep the reference's signatures and call these through
 * ctypes with `tensor.data_ptr()` (INTEGRATION.md shows the binding).
 *
 * One entry point has no counterpart in the reference: dtc_sim_step, a kinematic surrogate of the simulator behind env.step()
 * that fills the Isaac Gym tensors the env-side entry points read, so they can run closed loop on one GPU.  It is not physics;
 * its section lists what is absent.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter is documented as host;
 *   - the caller owns all buffers; nothing is retained after return;
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); calls are
 *     asynchronous on it and never synchronise the host;
 *   - return 0 on success, a negative DTC_ERR_* otherwise (bad argument / launch failure);
 *     no exception crosses the boundary;
 *   - all matrices are row-major fp32; `ld*` are leading dimensions in elements.
 */
#ifndef DTC_HIP_H
#define DTC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTC_OK 0
#define DTC_ERR_ARG (-1)      /* null pointer / bad shape / unsupported size            */
#define DTC_ERR_LAUNCH (-2)   /* hipGetLastError() != hipSuccess after a launch           */
#define DTC_ERR_ALIGN (-3)    /* a pointer that must be 16-byte aligned is not            */

#define DTC_ACT_NONE 0
#define DTC_ACT_RELU 1
#define DTC_ACT_ELU 2
/* the remaining entries of the reference's get_activation table (actor_critic_decoder.py:565-582; 'crelu' is nn.ReLU there) */
#define DTC_ACT_SELU 3
#define DTC_ACT_LRELU 4    /* nn.LeakyReLU(): negative slope 0.01 */
#define DTC_ACT_TANH 5
#define DTC_ACT_SIGMOID 6

/* library / device info ------------------------------------------------------------------ */
#define DTC_ABI_VERSION 25                  /* bumped whenever a signature or a by-value struct layout changes       */
int dtc_version(void);                       /* == DTC_ABI_VERSION of the build; the host binding refuses a mismatch   */
/* sizeof() of the structs that cross the boundary, in the order DtcGridCfg, DtcObsCfg, DtcRowCopy, DtcSeg, DtcSegMat,
   DtcFwdLayer, DtcWgradJob, DtcPpoCfg, DtcProfRec, DtcWimgJob, DtcH2iWJob, DtcH2iOperand, DtcWgradH2iJob, DtcEnvStep, DtcH2iFwdLayer, DtcH2iDgradLayer, DtcGruFwdItem, DtcGruBwdItem: the binding compares them with its own layouts at load time (a library
   built from another revision -- e.g. a stale DTC_LIB override -- must not receive descriptors it would misread).
   Returns the number of entries (written up to `cap`). */
int dtc_abi_sizes(int64_t* out, int cap);
const char* dtc_last_error(void);            /* host string describing the last failure   */
/* A non-blocking HIP stream owned by the caller (high_priority != 0: the device's greatest priority).  The trainers run their second compute
 * lane and their weight-gradient lanes on such streams instead of entries of torch's shared stream pool (dtc_amd/algorithms/ppo.py:_Lanes). */
int dtc_stream_create(int high_priority, void** out);
int dtc_stream_destroy(void* stream);

/* ---- foothold planner: legged_gym/envs/base/legged_robot_dtc.py:98-201 ----------------- */
typedef struct DtcGridCfg {
    int nx, ny;            /* 33, 21: cfg.terrain.measured_points_{x,y} (lite3_dtc_config.py:32-36) */
    float t_stance;        /* cfg.sim.dt * cfg.control.decimation = 0.02 (legged_robot_dtc.py:106)  */
    float fdbk_gain;       /* 0.03 (legged_robot_dtc.py:107)                                        */
    float x[64];           /* host copies of the grid coordinates                                   */
    float y[32];
} DtcGridCfg;

/* One call = lines :98-201 for N envs.  idx is the reference's optimal_foothold_indice [N,1,4]
 * (int64).  Optional outputs may be NULL: score [N,P,4] (self.foothold_score),
 * nominal_idx [N,4] int64, slope [N,nx,ny], heights_world [N,P,3].  cfg is a HOST pointer. */
int dtc_foothold_plan(const float* measured_heights /*[N,P]*/, const float* root_states /*[N,13]*/,
                      const float* thigh_pos /*[N,4,3]*/, const float* commands /*[N,4]*/,
                      const DtcGridCfg* cfg, int64_t* idx /*[N,4]*/, float* foothold_obs /*[N,8]*/,
                      float* opt_world /*[N,4,3]*/, float* pred /*[N,4,3]*/, float* pred_to_robot /*[N,4,3]*/,
                      float* score_or_null, int64_t* nominal_idx_or_null, float* slope_or_null,
                      float* heights_world_or_null, int N, void* stream);

/* Host only (no device needed): which path a grid takes.  out[0] = 1 if the 8 x 8 candidate patch may be placed (the disc of
 * 0.16 m fits into 8 cells on both axes AND both tables are strictly increasing and uniform to 0.03 cells; the generic kernel
 * uses the patch only where ny >= 8, every other grid takes the exact full scan), out[1] = P = nx * ny, out[2] = bytes of
 * dynamic LDS per workgroup of the generic kernel ((2 * 4 * P + 96) * 4: 65 920 B at the largest grid, 64 x 32;
 * dtc_foothold_plan refuses a grid whose request exceeds the device's per-workgroup limit before it launches anything),
 * out[3] = 1 if the call without debug outputs takes the 33 x 21 fast kernel. */
int dtc_foothold_grid_info(const DtcGridCfg* cfg, int32_t out[4]);

/* Consumers of the planner output in the same env step (legged_robot_dtc.py:577-586 and :536-539):
 * tracking[n] = sum_legs contact ? -log(0.8 + ||foot_xy - optimal_xy||) : 0   (_reward_tracking_optimal_footholds)
 * miss[n]     = min_legs foot_z < 0 ? 1 : 0                                    (_reward_foothold_miss)
 * contact is the env's contact_filt as uint8 [N,4]; either output may be NULL. */
int dtc_foothold_rewards(const float* foot_positions /*[N,4,3]*/, const float* opt_world /*[N,4,3]*/,
                         const uint8_t* contact /*[N,4]*/, float* tracking /*[N]*/, float* miss /*[N]*/, int N,
                         void* stream);

/* LeggedRobot._get_heights: legged_gym/envs/base/legged_robot.py:1279-1317 (row f1). */
int dtc_get_heights(const int16_t* height_samples /*[rows,cols]*/, int rows, int cols,
                    const float* root_states /*[N,13]*/, const DtcGridCfg* cfg, float border_size,
                    float horizontal_scale, float vertical_scale, float* measured_heights /*[N,P]*/,
                    int N, void* stream);

/* Rows f1 + c fused: sample the terrain table (legged_robot.py:1279-1317), write measured_heights [N,P] (the observations
 * consume it) and plan the footholds (legged_robot_dtc.py:98-201) from the freshly sampled rows in ONE launch -- no
 * read-back of the [N,P] matrix.  Bit-identical to dtc_get_heights followed by dtc_foothold_plan (any grid other than
 * the reference's 33 x 21 runs exactly those two). */
int dtc_foothold_plan_from_table(const int16_t* height_samples /*[rows,cols]*/, int rows, int cols, float border_size,
                                 float horizontal_scale, float vertical_scale, const float* root_states /*[N,13]*/,
                                 const float* thigh_pos /*[N,4,3]*/, const float* commands /*[N,4]*/,
                                 const DtcGridCfg* cfg, float* measured_heights /*out [N,P]*/, int64_t* idx /*[N,4]*/,
                                 float* foothold_obs /*[N,8]*/, float* opt_world /*[N,4,3]*/, float* pred /*[N,4,3]*/,
                                 float* pred_to_robot /*[N,4,3]*/, int N, void* stream);

/* ---- env-step consumers of the planner output (row f3) ----------------------------------
 * LeggedRobotDTC.compute_observations, legged_gym/envs/base/legged_robot_dtc.py:255-288, and
 * LeggedRobotDTC.check_termination, legged_gym/envs/base/legged_robot_dtc.py:229-248. */
typedef struct DtcObsCfg {
    float ang_vel, dof_pos, dof_vel, height_measurements, force;   /* cfg.normalization.obs_scales (legged_robot_config.py:181-188) */
    float commands_scale[3];     /* [lin_vel, lin_vel, ang_vel] (legged_robot.py:810)                                    */
    float base_height_target;    /* cfg.rewards.base_height_target (lite3_dtc_config.py:139)                             */
    float height_noise;          /* 0.1: amplitude of the uniform height noise of the privileged obs (:278)              */
    float term_height;           /* 0.15: base-height termination threshold (:244-246)                                   */
    int num_dof, num_foothold_obs, num_points;      /* 12, 8, 693                                                        */
    int term_row0, term_row1;    /* slice of measured_heights averaged by the height test: 10*21, (33-10)*21             */
} DtcObsCfg;

/* obs_buf [N, 9 + 3*num_dof + num_foothold_obs] = cat(ang_vel*s, gravity, commands[:, :3]*s, (dof_pos-default)*s,
 * dof_vel*s, actions, foothold_obs) (+ (2*u_obs-1)*noise_scale_vec when u_obs != NULL: the torch.rand_like draw of :287
 * is an INPUT); heights [N,P] = clip(root_z - target - measured_heights, -1, 1)*s (may be NULL);
 * privileged_obs_buf [N, 2P+3] = cat(heights + (2*u_heights-1)*0.1 + height_noise_offset, forces[:,0,:]*s, heights)
 * (u_heights / height_noise_offset may be NULL = term omitted).  forces: first body's force of env n at
 * forces + n*ld_forces.  commands is [N,4].  cfg is a HOST pointer. */
int dtc_compute_observations(const float* base_ang_vel, const float* projected_gravity, const float* commands,
                             const float* dof_pos, const float* default_dof_pos /*[num_dof]*/, const float* dof_vel,
                             const float* actions, const float* foothold_obs, const float* root_states /*[N,13]*/,
                             const float* measured_heights /*[N,P]*/, const float* forces, int64_t ld_forces,
                             const float* height_noise_offset /*[N,P]*/, const float* u_obs, const float* noise_scale_vec,
                             const float* u_heights /*[N,P]*/, const DtcObsCfg* cfg, float* obs_buf,
                             float* privileged_obs_buf, float* heights, int N, void* stream);

/* reset_buf[n] = any_j |contact_forces[n, idx_j]| > 100  |  episode_length > max  |  gravity_z > 0.2  |
 * mean(root_z - max(measured_heights[n, term_row0:term_row1], 0)) < term_height;  time_out_buf[n] = episode_length > max.
 * contact_forces [N,num_bodies,3]; indices int32 (device); episode_length_buf int64; outputs uint8. */
int dtc_check_termination(const float* contact_forces, int num_bodies, const int32_t* termination_contact_indices,
                          int n_term, const int64_t* episode_length_buf, int64_t max_episode_length,
                          const float* projected_gravity /*[N,3]*/, const float* root_states /*[N,13]*/,
                          const float* measured_heights /*[N,P]*/, const DtcObsCfg* cfg, uint8_t* reset_buf,
                          uint8_t* time_out_buf /*or NULL*/, float* height_mean_or_null, int N, void* stream);

/* Same as dtc_compute_observations for the rows with where[n] != 0 only (the other rows of the three outputs are left untouched):
 * the observation pass AFTER `reset_idx` (legged_robot_dtc.py:209-211) when dtc_env_post_physics has already written the rows
 * of the envs that were not reset.  where == NULL: all rows. */
int dtc_compute_observations_where(const float* base_ang_vel, const float* projected_gravity, const float* commands,
                                   const float* dof_pos, const float* default_dof_pos, const float* dof_vel,
                                   const float* actions, const float* foothold_obs, const float* root_states,
                                   const float* measured_heights, const float* forces, int64_t ld_forces,
                                   const float* height_noise_offset, const float* u_obs, const float* noise_scale_vec,
                                   const float* u_heights, const DtcObsCfg* cfg, float* obs_buf, float* privileged_obs_buf,
                                   float* heights, const uint8_t* where, int N, void* stream);

/* ---- one env step's post-physics block as ONE launch (BASELINE configs[3]: 4096 envs, launch-bound) -----------------------
 * LeggedRobotDTC.post_physics_step, legged_gym/envs/base/legged_robot_dtc.py:98-211, on the env's own buffers:
 *   [measured_heights = _get_heights() (legged_robot.py:1279-1317) when height_samples != NULL]
 *   foothold block :98-201  ->  check_termination :229-248  ->  foothold rewards :577-586 / :536-539  ->  compute_observations :255-288
 * = dtc_foothold_plan[_from_table] + dtc_check_termination + dtc_foothold_rewards + dtc_compute_observations with the same
 * arguments, same bits, one launch (each env's height row is read once and stays in LDS for all four).  The reference resets
 * envs (`reset_idx`, simulator state) BETWEEN the rewards and the observations: the observation rows written here are those of
 * the state passed in; after resetting (dtc_env_reset below), refresh the rows of the reset envs with
 * dtc_compute_observations_where(..., where = reset_buf).  All pointers are device pointers; optional ones may be NULL where the separate entry points allow it.
 * Grids other than 33 x 21 run the separate launches in that order.  `st`, `grid`, `obs` are HOST pointers. */
typedef struct DtcEnvStep {
    /* planner */
    const int16_t* height_samples;   /* terrain table [rows, cols] or NULL (then measured_heights is an input) */
    int rows, cols;
    float border_size, horizontal_scale, vertical_scale;
    const float *root_states, *thigh_pos, *commands;
    float* measured_heights;         /* [N,P]: written when height_samples != NULL, read otherwise */
    int64_t* idx;
    float *foothold_obs, *opt_world, *pred, *pred_to_robot;
    /* check_termination */
    const float* contact_forces;
    const int32_t* termination_contact_indices;
    const int64_t* episode_length_buf;
    const float* projected_gravity;
    int64_t max_episode_length;
    int num_bodies, n_term;
    uint8_t *reset_buf, *time_out_buf;
    float* height_mean;
    /* rewards */
    const float* foot_positions;
    const uint8_t* contact_filt;
    float *rew_tracking, *rew_miss;
    /* compute_observations (commands, root_states, projected_gravity, foothold_obs, measured_heights: the ones above) */
    const float *base_ang_vel, *dof_pos, *default_dof_pos, *dof_vel, *actions, *forces;
    int64_t ld_forces;
    const float *height_noise_offset, *u_obs, *noise_scale_vec, *u_heights;
    float *obs_buf, *privileged_obs_buf, *heights;
} DtcEnvStep;
int dtc_env_post_physics(const DtcEnvStep* st, const DtcGridCfg* grid, const DtcObsCfg* obs, int N, void* stream);

/* ---- env rewards: LeggedRobot.compute_reward, legged_gym/envs/base/legged_robot.py:274-291 ----------------------------------
 * Every `_reward_*` term of LeggedRobotDTC (legged_robot.py:1321-1622, legged_robot_dtc.py:522-586) in ONE launch, accumulated in
 * the reference's order: rew_buf = 0; for each active term but termination, in alphabetical order (the order class_to_dict gives
 * the scales, legged_robot.py:929-952 / utils/helpers.py:11-26): r = term * scale, rew_buf += r, episode_sums[term] += r; clip
 * rew_buf at 0 if only_positive_rewards; then the termination term.  The state the reference's terms change is updated in the same
 * order: feet_air_time / last_contacts (_reward_feet_air_time, :1386-1412 -- feet_slip and foot_acc after it see the new
 * last_contacts), the 5-step stumble history of _reward_foot_clearance (:1474-1492) and pitch_est (_reward_orientation,
 * _reward_orientation_roll, :1559-1596; updated twice when both are on).  Term indices are the DTC_REW_* below. */
#define DTC_REWARD_TERMS 34
enum {
    DTC_REW_ACTION_RATE, DTC_REW_ANG_VEL_XY, DTC_REW_BASE_HEIGHT, DTC_REW_BIG_PITCH, DTC_REW_COLLISION, DTC_REW_DOF_ACC,
    DTC_REW_DOF_POS_LIMITS, DTC_REW_DOF_VEL, DTC_REW_DOF_VEL_LIMITS, DTC_REW_FEET_AIR_TIME, DTC_REW_FEET_CONTACT_FORCES,
    DTC_REW_FEET_SLIP, DTC_REW_FEET_STUMBLE, DTC_REW_FOOT_ACC, DTC_REW_FOOT_CLEARANCE, DTC_REW_FOOTHOLD_MISS, DTC_REW_HIP_POS,
    DTC_REW_LIN_VEL_Z, DTC_REW_ORIENTATION, DTC_REW_ORIENTATION_ROLL, DTC_REW_POS_ACC, DTC_REW_POWER, DTC_REW_POWERCHANGE,
    DTC_REW_SMOOTH, DTC_REW_SOFT_TRACKING_ANG_VEL, DTC_REW_SOFT_TRACKING_LIN_VEL, DTC_REW_STAND_STILL, DTC_REW_STUMBLE,
    DTC_REW_TERMINATION, DTC_REW_TORQUE_LIMITS, DTC_REW_TORQUES, DTC_REW_TRACKING_ANG_VEL, DTC_REW_TRACKING_LIN_VEL,
    DTC_REW_TRACKING_OPTIMAL_FOOTHOLDS
};

typedef struct DtcRewardCfg {
    float scale[DTC_REWARD_TERMS];  /* float32(scale * dt), dt = sim.dt * decimation in double (legged_robot.py:929-938); 0 = off */
    int32_t row[DTC_REWARD_TERMS];  /* row of the term in episode_sums / per_term (its rank in the scales dict), -1 = off          */
    float dt;                       /* cfg.sim.dt * cfg.control.decimation: dof_acc, foot_acc divide by it, feet_air_time adds it   */
    float tracking_sigma;           /* cfg.rewards.tracking_sigma (legged_robot_config.py:174)                                      */
    float soft_dof_vel_limit, soft_torque_limit;    /* cfg.rewards (legged_robot.py:1364-1371)                                     */
    float base_height_target;       /* cfg.rewards.base_height_target (legged_robot_dtc.py:531-534)                                 */
    float max_contact_force;        /* cfg.rewards.max_contact_force (legged_robot.py:1426-1428)                                    */
    float max_acc;                  /* cfg.rewards.max_acc (legged_robot.py:1525-1531)                                              */
    float lin_vel_x_max, ang_vel_yaw_max;   /* command_ranges["lin_vel_x"][1], ["ang_vel_yaw"][1] (:1373-1378, dtc.py:542-568) */
    int32_t only_positive_rewards;  /* cfg.rewards.only_positive_rewards (legged_robot.py:284-285)                                  */
    int32_t num_dof;                /* 12 (<= 64)                                                                                   */
    int32_t n_penalised, n_hip;     /* lengths of the two index lists below                                                         */
    int32_t feet[4];                /* self.feet_indices: bodies of contact_forces (legged_robot.py:1183)                           */
    int32_t penalised[32];          /* self.penalised_contact_indices: bodies (:1187)                                               */
    int32_t hip[16];                /* self.hip_indices: columns of dof_pos (:1108-1111, :1504-1505)                                */
    int32_t num_points;             /* 693: columns of measured_heights                                                             */
    const float* plane;             /* DEVICE [2, num_points]: rows 0, 1 of (A^T A)^-1 A^T, A = [x, y, 1] over height_points -- the
                                       constant part of get_plane_norm's batched least squares (:1535-1557); fp32 of float64     */
} DtcRewardCfg;

typedef struct DtcRewardStep {
    /* inputs (device; shapes and dtypes of the reference's attributes; N envs, D dofs, B bodies, C = num_commands) */
    const float *root_states;                         /* [N,13]                                                                */
    const float *base_lin_vel, *base_ang_vel, *projected_gravity;    /* [N,3]                                                   */
    const float *commands;                            /* [N,C], C >= 3                                                          */
    const float *dof_pos, *default_dof_pos;           /* [N,D], [D]                                                             */
    const float *dof_vel, *last_dof_vel, *torques, *actions, *last_actions, *last_actions_2;   /* [N,D]                        */
    const float *contact_forces;                      /* [N,B,3]                                                                */
    const float *foot_positions, *foot_velocities, *last_foot_velocities, *optimal_footholds_world;   /* [N,4,3]              */
    const uint8_t *contact_filt;                      /* [N,4] bool: set by _post_physics_step_callback (:561-564)              */
    const float *measured_heights;                    /* [N,num_points]                                                         */
    const uint8_t *reset_buf, *time_out_buf;          /* [N] bool                                                               */
    const float *robot_mass;                          /* [N]                                                                    */
    const int64_t *terrain_levels;                    /* [N]                                                                    */
    const float *dof_pos_limits;                      /* [D,2]                                                                  */
    const float *dof_vel_limits, *torque_limits;      /* [D]                                                                    */
    /* ring buffers, time-major as the reference holds them (legged_robot.py:844-846) */
    const float *cmd_buffer;                          /* [10,N,C]                                                               */
    const float *lin_vel_buffer;                      /* [10,N,2]                                                               */
    const float *ang_vel_buffer;                      /* [10,N,1]                                                               */
    /* foot clearance (_get_foot_clearance, :1443-1472): from the int16 height table when height_samples != NULL (then written to
       foot_clearance if that is not NULL), else read from foot_clearance = the env's measured_foot_clearance [N,4] */
    const int16_t *height_samples;
    int32_t rows, cols;
    float border_size, horizontal_scale, vertical_scale;
    float *foot_clearance;
    /* state, read and written */
    float *feet_air_time;                             /* [N,4]                                                                  */
    uint8_t *last_contacts;                           /* [N,4] bool: as the env holds it after the callback; written only when
                                                         feet_air_time is on (the reference rebinds it there)                    */
    uint8_t *stumble;                                 /* [N,4]: bit k = the stumble mask pushed k steps ago (the 5-list of :1485) */
    float *pitch_est;                                 /* [N]                                                                    */
    /* outputs */
    float *rew_buf;                                   /* [N]                                                                    */
    float *episode_sums;                              /* [n_active, N], row DtcRewardCfg.row[term]: accumulated                 */
    float *per_term;                                  /* [n_active, N] term * scale, or NULL                                    */
    int32_t num_bodies, num_commands;
} DtcRewardStep;
/* One launch for all N envs.  Pointers of terms that are off may be NULL.  `st`, `cfg` are HOST pointers. */
int dtc_env_rewards(const DtcRewardStep* st, const DtcRewardCfg* cfg, int N, void* stream);

/* ---- env reset: LeggedRobot.reset_idx, legged_gym/envs/base/legged_robot.py:200-272, and what it calls ----------------------------
 * For every env n with reset_buf[n] != 0, on the env's own tensors, in the reference's order (all arithmetic fp32, one rounding per
 * operation, operands in the reference's order):
 *   1. _update_terrain_curriculum (legged_robot.py:690-711; when terrain_curriculum and init_done), from the PRE-reset root_states[n,:2],
 *      the PRE-update env_origins[n,:2] and the PRE-resample commands[n,:2]: distance = |root_xy - origin_xy|; move_up = distance >
 *      move_up_distance; move_down = distance < |commands_xy| * max_episode_length_s * 0.5 and not move_up; terrain_levels[n] += move_up -
 *      move_down; then level >= max_terrain_level ? level_draw[n] : max(level, 0); env_origins[n] = terrain_origins[level, terrain_types[n]].
 *   2. _reset_dofs (:632-641): dof_pos[n] = default_dof_pos * ((1.5 - 0.5) * u + 0.5); dof_vel[n] = 0.
 *   3. LeggedRobotDTC._reset_root_states (legged_robot_dtc.py:291-311): root_states[n] = base_init_state; [:3] += the NEW env_origins[n];
 *      with custom_origins [:2] += (hi - lo) * u + lo over origin_xy (DTC: -0.5..0.5; LeggedRobot, legged_robot.py:659: -1..1);
 *      [7:13] = (0.5 - -0.5) * u + -0.5.
 *   4. _resample_commands (:567-593): commands[n,0], [n,1] drawn from lin_vel_x / lin_vel_y, then commands[n,3] from heading
 *      (heading_command) or commands[n,2] from ang_vel_yaw; with play_command 0.5, 0.0 and 0 instead; commands[n,:2] *= (|commands_xy|
 *      > 0.1); forces[n,:,:] = 0.
 *   5. _randomize_dof_props (:465-481): motor_strengths / Kp_factors / Kd_factors [n,:] = u * (max - min) + min, one draw per env, for
 *      each flag that is on.
 *   6. height_noise_offset[n,:] = old * 0.0 + height_noise (:229-230; the caller draws np.random.normal(0, 0.02) once per call).
 *   7. the buffer clears of :233-251 and :267-272, table driven: `rows` items are [N, row_bytes] tensors whose row n is zeroed
 *      (last_actions, ..., episode_length_buf, the lag buffers, the stumble masks or the stumble bits of dtc_env_rewards, contact_filt,
 *      last_contacts), `time_rows` items are [T, N, row_bytes] tensors whose rows [:, n] are zeroed (lin_vel_buffer, ang_vel_buffer,
 *      cmd_buffer).  reset_buf[n] = 1 (:238) changes nothing and is not written.
 *   8. the episode log (:253-259): episode_means[r] = mean over the reset envs of episode_sums[r, n] / max_episode_length_s, read BEFORE
 *      episode_sums[r, n] = 0; with terrain_curriculum terrain_level_mean = mean over ALL N envs of terrain_levels after step 1.  Sums are
 *      accumulated in float64 in a fixed order (per 256-env block, then over the blocks in order) and rounded to fp32 once: no
 *      floating-point atomics, the same bits from run to run.
 *   9. the hand-over to the simulator: env_ids[0 .. count) = the reset envs in ascending order (what reset_buf.nonzero() gives), count[0]
 *      their number -- device memory, for the caller of set_dof_state_tensor_indexed / set_actor_root_state_tensor_indexed.
 * count == 0 is the reference's early return (:210-211): no env tensor is written and episode_means / terrain_level_mean keep their
 * contents (count[0] = 0 is written).  `force_positions = rb_positions.clone()` (:593) and update_command_curriculum (:717-726) are
 * host-side decisions and stay with the caller.
 *
 * Draws.  u [N, num_dof + 14] fp32 in [0, 1): row n holds the draws env n uses IF it resets (the reference draws one row per reset env,
 * in env_ids order); slots: [0, D) dof_pos | D, D+1 origin x, y | D+2 .. D+7 root_states[7:13] | D+8, D+9, D+10 command x, y,
 * heading-or-yaw | D+11, D+12, D+13 motor strength, Kp, Kd.  level_draw [N] int64: torch.randint_like(levels, max_terrain_level).
 * With u == NULL (level_draw == NULL) the kernel draws them itself: Philox4x32-10 (csrc/philox.hpp, as dtc_randn), key = seed, counter = (n, slot group,
 * call counter), 24 bits per uniform; level = word % max_terrain_level.  One env's draws do not depend on which other envs reset.  That
 * stream has torch's distribution, not torch's bits.  A range [lo, hi] enters as float32(hi - lo) (difference in double) and float32(lo).
 *
 * N <= 2^18: every 256-env block of launch 1 recounts the reset_buf bytes in front of it (16 KB on average at 32768 envs, the
 * largest env count the design is meant for); that is quadratic in N, so larger N is refused rather than run slowly.
 * Two launches per call whatever the mask, both sized by N alone (one workgroup per 256 envs: env_ids, terrain curriculum, episode
 * sums and their per-block partial sums; then one wavefront per env: the rows of the envs that reset, and the fold of the partials);
 * the launch function allocates, copies and waits for nothing.  `st`, `cfg` are HOST pointers holding DEVICE pointers. */
#define DTC_RESET_MAX_ROWS 32
#define DTC_RESET_MAX_TIME_ROWS 8
#define DTC_RESET_MAX_SUMS 64
#define DTC_RESET_FIXED_DRAWS 14               /* u has num_dof + 14 columns */

typedef struct DtcResetRows {
    void* ptr;                       /* [N, row_bytes] (time_rows: [T, N, row_bytes]), dense */
    int32_t T;                       /* rows: ignored; time_rows: the leading dimension (10)  */
    int32_t row_bytes;
} DtcResetRows;

typedef struct DtcResetCfg {
    int32_t num_dof;                 /* D: 12 (<= 64)                                                                     */
    int32_t num_bodies;              /* B: rows of forces[n]                                                              */
    int32_t num_commands;            /* C: columns of commands (>= 3; >= 4 with heading_command)                          */
    int32_t num_points;              /* columns of height_noise_offset (693)                                              */
    int32_t terrain_curriculum;      /* cfg.terrain.curriculum (legged_robot.py:213, :258)                                */
    int32_t init_done;               /* self.init_done (:697)                                                             */
    int32_t custom_origins;          /* self.custom_origins (:1206 / :1219)                                               */
    int32_t heading_command;         /* cfg.commands.heading_command (:575)                                               */
    int32_t play_command;            /* cfg.env.play_commond (:580)                                                       */
    int32_t randomize_motor_strength, randomize_kp, randomize_kd;       /* cfg.domain_rand (:466-477)                     */
    int32_t max_terrain_level;       /* cfg.terrain.num_rows (:1213)                                                      */
    int32_t terrain_rows, terrain_cols;      /* shape of terrain_origins [rows, cols, 3]                                  */
    float move_up_distance;          /* float32(terrain.env_length * 0.6) (:702)                                          */
    double max_episode_length_s;     /* cfg.env.episode_length_s (:704 as fp32, :255 divides the float64 mean by it)      */
    float base_init_state[13];       /* self.base_init_state (:1132)                                                      */
    float height_noise;              /* the np.random.normal(0, 0.02) of this call (:230)                                 */
    double origin_xy[2];             /* [lo, hi] of the xy offset under custom_origins                                    */
    double lin_vel_x[2], lin_vel_y[2], ang_vel_yaw[2], heading[2];      /* self.command_ranges, as they are at this call  */
    double motor_strength[2], kp_range[2], kd_range[2];                 /* cfg.domain_rand [min, max]                     */
    uint64_t seed, counter;          /* generated draws only: key and call counter                                        */
} DtcResetCfg;

typedef struct DtcResetStep {
    const uint8_t* reset_buf;        /* [N] bool                                                                          */
    const float* u;                  /* [N, D + 14] or NULL (generated)                                                   */
    const int64_t* level_draw;       /* [N] or NULL (generated)                                                           */
    const float* terrain_origins;    /* [terrain_rows, terrain_cols, 3]                                                   */
    const int64_t* terrain_types;    /* [N]                                                                               */
    const float* default_dof_pos;    /* [D]                                                                               */
    /* read and written */
    int64_t* terrain_levels;         /* [N]                                                                               */
    float* env_origins;              /* [N,3]                                                                             */
    float* root_states;              /* [N,13]                                                                            */
    float* commands;                 /* [N,C]                                                                             */
    float *dof_pos, *dof_vel;        /* [N,D], strided: element (n, d) at n * dof_row_stride + d * dof_elem_stride floats.  The
                                        reference's are the two interleaved views of dof_state [N,D,2] (legged_robot.py:774-775):
                                        row stride 2 D, element stride 2; a dense [N,D] tensor has D and 1                 */
    int64_t dof_pos_row_stride, dof_pos_elem_stride, dof_vel_row_stride, dof_vel_elem_stride;
    float* forces;                   /* [N,B,3] or NULL                                                                   */
    float *motor_strengths, *Kp_factors, *Kd_factors;   /* [N,D]; needed when their flag is on                             */
    float* height_noise_offset;      /* [N,num_points] or NULL                                                            */
    float* episode_sums;             /* [n_sums, N] (the layout of dtc_env_rewards)                                       */
    int32_t n_sums, n_rows, n_time_rows, pad_;
    DtcResetRows rows[DTC_RESET_MAX_ROWS];
    DtcResetRows time_rows[DTC_RESET_MAX_TIME_ROWS];
    /* outputs */
    int32_t* env_ids;                /* [N]: entries [0, count) written                                                   */
    int32_t* count;                  /* [1]                                                                               */
    float* episode_means;            /* [n_sums]                                                                          */
    float* terrain_level_mean;       /* [1]; needed with terrain_curriculum                                               */
    void* workspace;                 /* dtc_env_reset_workspace(N, n_sums) bytes, 8-byte aligned; contents need not be kept */
} DtcResetStep;
int64_t dtc_env_reset_workspace(int N, int n_sums);
/* sizeof() of DtcResetRows, DtcResetCfg, DtcResetStep, as dtc_abi_sizes gives them for the older structs: compared by the binding at
   load time.  Returns the number of entries (written up to `cap`). */
int dtc_env_reset_abi_sizes(int64_t* out, int cap);
int dtc_env_reset(const DtcResetStep* st, const DtcResetCfg* cfg, int N, void* stream);

/* ---- surrogate legged env: the state the env kernels above run on, with no simulator ------
 * dtc_sim_step (csrc/sim.hip) stands where the reference calls Isaac Gym: `decimation` substeps of _compute_torques, control type "P"
 * (legged_robot.py:610-630, the current action where the reference takes a randomly lagged one), a kinematic quadruped, and the
 * bookkeeping of post_physics_step up to the planner (legged_robot_dtc.py:66-91, legged_robot.py:534-535, :562-564), as ONE launch,
 * one wavefront per env, each env row loaded once and stored once.  It is a surrogate, not physics: state that is consistent,
 * evolves, responds to actions and can terminate.  In dtc_sim_step the base only yaws (the quaternion keeps x = y = 0,
 * projected_gravity is (0, 0, -1)); dtc_sim_step_tilt, below, adds a kinematic roll and pitch.  Absent on purpose from both:
 * attitude and base dynamics (the base rides on its stance feet; free flight, landing and crashes: dtc_sim_step_fly, below), lag
 * buffers and pushes (dtc_sim_step_act, below; `forces` are never touched), control types "V" and "T", contact dynamics, anything
 * that topples the robot, and the heading command's yaw law (legged_robot.py:537-539 stays with the caller).  Contact with anything
 * but the soles of the feet: dtc_sim_contacts, below, a launch of its own, whose forces feed the rewards and hold nothing back.
 *
 * Every value is a single-rounded fp32 operation in the order below (-ffp-contract=off; tests/sim_oracle.py restates it in numpy
 * float32, bit for bit).  Joint j = 3 l + k is joint k of leg l; sums over legs run in leg order 0..3 from 0.0f.  Once per step:
 *   a = min(max(action, -clip_actions), clip_actions)                      -> actions
 *   goal = min(max(a * action_scale + default, lo), hi);   kp = p_gain * Kp_factor;   kd = d_gain * Kd_factor
 * One substep:
 *   1. tau = min(max(((kp * ((goal - q) + offset)) - kd * qd) * strength, -limit), limit)
 *   2. qd = qd + (tau / joint_inertia) * dt;  q = q + qd * dt;  q < lo: q = lo, qd = 0;  q > hi: q = hi, qd = 0
 *   3. p_l[i] = foot_nominal[l][i] + ((J[l][i][0] * dq0 + J[l][i][1] * dq1) + J[l][i][2] * dq2),  dq = q - default;
 *      u_l[i] = (J[l][i][0] * qd0 + J[l][i][1] * qd1) + J[l][i][2] * qd2
 *   4. c = 1 - 2 * (qz * qz);  s = 2 * (qz * qw);  foot world xy: fx = x + (c * p.x - s * p.y),  fy = y + (s * p.x + c * p.y)
 *   5. h_l: the _get_heights rule (legged_robot.py:1301-1316) at (fx, fy): index = clamp((long)((f + border) / hscale), 0, size - 2),
 *      min of the three samples, times vertical_scale
 *   6. base_z = max_l(h_l - p_l.z);  contact_l = ((base_z + p_l.z) - h_l) <= contact_eps;  n_c = number of contacts (>= 1)
 *   7. pm = (sum of stance p.xy) / n_c;  um = (sum of stance u.xy) / n_c;  over the stance legs, dp = p - pm, du = u - um:
 *      num = sum(dp.x * du.y - dp.y * du.x);  den = sum(dp.x * dp.x + dp.y * dp.y);  w = den > r_min * r_min ? -(num / den) : 0
 *      vb.x = (-um.x) + w * pm.y;  vb.y = (-um.y) - w * pm.x             (the least-squares twist of "stance feet do not slip")
 *   8. x = x + (c * vb.x - s * vb.y) * dt;  y = y + (s * vb.x + c * vb.y) * dt;  vz = (base_z - z) / dt;  z = base_z
 *      e = (0.5 * dt) * w;  z' = qz + e * qw;  w' = qw - e * qz;  r = sqrt(z' * z' + w' * w');  qz = z' / r;  qw = w' / r
 * After the last substep, with c, s of the NEW quaternion and V = (c * vb.x - s * vb.y, s * vb.x + c * vb.y):
 *   root_states = [x, y, z, 0, 0, qz, qw, V.x, V.y, vz, 0, 0, w];  dof_pos, dof_vel, torques (the last substep's);
 *   base_lin_vel = (vb.x, vb.y, vz);  last_base_ang_vel = the base_ang_vel found;  base_ang_vel = (0, 0, w);
 *   projected_gravity = (0, 0, -1);  base_quat = (0, 0, qz, qw);  base_pos = (x, y, z);
 *   rigid_body_state[foot_l]: columns 0..2 = (x + (c p.x - s p.y), y + (s p.x + c p.y), z + p.z), columns 7..9 = (V.x + (c r.x - s r.y),
 *   V.y + (s r.x + c r.y), vz + u.z) with r = (u.x - w * p.y, u.y + w * p.x);  rigid_body_state[thigh_l]: columns 0..2 = base + R hip_offset_l;
 *   the other columns and bodies of rigid_body_state are left alone;
 *   contact_forces[n] = 0 except [foot_l][2] = contact_l ? weight / n_c : 0.
 * Then: episode_length_buf += 1; the three time-major ring buffers [T, N, .] shift by one and take (vb.x, vb.y), w and the commands
 * as they stand; envs with episode_length_buf % resampling_steps == 0 resample their commands as _resample_commands does
 * (:573-591: x, y, and heading (column 3) or yaw rate (column 2); xy zeroed when their norm is <= 0.1) from u_cmd [N,3] in [0, 1),
 * or with u_cmd == NULL from Philox4x32-10 (key = seed, counter = (n, 0, call counter), words x, y, z, 24 bits each, as
 * dtc_env_reset draws); contact = contact_forces[foot, 2] > 1;  contact_filt = contact | last_contacts;  last_contacts = contact.
 * `st`, `cfg` are HOST pointers; every pointer inside is a DEVICE pointer and, except u_cmd, required. */
typedef struct DtcSimCfg {
    int32_t num_dof;                 /* 12: four legs of three joints                                                     */
    int32_t num_bodies;              /* B: rows of rigid_body_state[n] / contact_forces[n]                                */
    int32_t num_commands;            /* C: columns of commands / cmd_buffer (>= 3; >= 4 with heading_command)             */
    int32_t decimation;              /* substeps per env step (1..64)                                                     */
    int32_t heading_command;         /* the third draw goes to column 3, not 2                                            */
    int32_t buffer_len;              /* T of the ring buffers (10)                                                        */
    int32_t feet[4], thighs[4];      /* body indices, leg order                                                           */
    int64_t resampling_steps;        /* int(cfg.commands.resampling_time / dt) (>= 1)                                     */
    float sim_dt, action_scale, clip_actions, joint_inertia, contact_eps, weight, r_min;
    int32_t rows, cols;              /* terrain table [rows, cols] int16 (both >= 2)                                      */
    float border_size, horizontal_scale, vertical_scale;
    double lin_vel_x[2], lin_vel_y[2], ang_vel_yaw[2], heading[2];      /* [lo, hi], entering as float32(hi - lo), float32(lo) */
    uint64_t seed, counter;          /* generated draws only                                                              */
} DtcSimCfg;

typedef struct DtcSimStep {
    /* inputs */
    const float* actions_in;         /* [N,D] the policy's actions                                                        */
    const float *Kp_factors, *Kd_factors, *motor_strengths, *motor_offsets;       /* [N,D]                                */
    const int16_t* height_samples;   /* [rows, cols]                                                                      */
    const float* u_cmd;              /* [N,3] or NULL (generated)                                                         */
    const float *p_gains, *d_gains, *torque_limits, *default_dof_pos;             /* [D]                                  */
    const float* dof_pos_limits;     /* [D,2]                                                                             */
    const float *hip_offset, *foot_nominal;      /* [4,3] base frame                                                      */
    const float* leg_jacobian;       /* [4,3,3]: d foot_l[i] / d q[3 l + k] at the default pose                           */
    /* read and written */
    float *dof_pos, *dof_vel;        /* [N,D] strided as in DtcResetStep                                                  */
    int64_t dof_pos_row_stride, dof_pos_elem_stride, dof_vel_row_stride, dof_vel_elem_stride;
    float* root_states;              /* [N,13]                                                                            */
    float* base_ang_vel;             /* [N,3]                                                                             */
    float* commands;                 /* [N,C]                                                                             */
    int64_t* episode_length_buf;     /* [N]                                                                               */
    uint8_t* last_contacts;          /* [N,4] bool                                                                        */
    float *lin_vel_buffer, *ang_vel_buffer, *cmd_buffer;       /* [T,N,2], [T,N,1], [T,N,C]                               */
    /* written */
    float* rigid_body_state;         /* [N,B,13]: foot and thigh rows                                                     */
    float* contact_forces;           /* [N,B,3]                                                                           */
    float *torques, *actions;        /* [N,D]                                                                             */
    float *base_lin_vel, *last_base_ang_vel, *projected_gravity, *base_pos;       /* [N,3]                                */
    float* base_quat;                /* [N,4]                                                                             */
    uint8_t* contact_filt;           /* [N,4] bool                                                                        */
} DtcSimStep;
/* sizeof() of DtcSimCfg, DtcSimStep, in a table of their own (dtc_abi_sizes keeps its 18 entries): compared by the binding at load
   time.  Returns the number of entries (written up to `cap`). */
int dtc_sim_abi_sizes(int64_t* out, int cap);
int dtc_sim_step(const DtcSimStep* st, const DtcSimCfg* cfg, int N, void* stream);

/* ---- surrogate legged env with roll and pitch (opt-in) ------------------------------------
 * dtc_sim_step_tilt is dtc_sim_step with a body plane that follows the support points of the stance feet over the terrain table.
 * Still kinematic, still ONE launch (the other instantiation of the same kernel), still not physics: there are no attitude dynamics,
 * the tilt is a least-squares plane through where the terrain asks the stance feet to be.  No new tensor: the tilt lives in the
 * quaternion of root_states[:, 3:7] between steps.  Absent as before: base dynamics and free flight, lag buffers, pushes, control
 * types "V" and "T", the heading command's yaw law.  After a reset the quaternion is the identity, so the first fit on sloped ground
 * is one step whose tilt rate (w.x, w.y below) is the whole tilt divided by sim_dt: a spike by construction.
 *
 * Only + - * /, sqrt and comparisons, each a single-rounded fp32 operation in the order below (tests/sim_tilt_oracle.py restates it
 * in numpy float32, bit for bit, and is the specification).  Rt(n), for a unit vector n, is the minimal rotation that takes z to n:
 *   k1 = 1 + n.z;   Rt = [[1 - (n.x * n.x) / k1,  -((n.x * n.y) / k1),  n.x],
 *                         [-((n.x * n.y) / k1),   1 - (n.y * n.y) / k1, n.y],
 *                         [-n.x,                  -n.y,                 n.z]]
 *   Rt v   = ((R00 * v.x + R01 * v.y) + n.x * v.z,  (R01 * v.x + R11 * v.y) + n.y * v.z,  (-(n.x * v.x) - n.y * v.y) + n.z * v.z)
 *   Rt^T v = ((R00 * v.x + R01 * v.y) - n.x * v.z,  (R01 * v.x + R11 * v.y) - n.y * v.z,  (n.x * v.x + n.y * v.y) + n.z * v.z)
 * At load, q = (qx, qy, qz, qw) = root_states[3:7] is split into its twist about z and the remaining swing:
 *   ry = sqrt(qz * qz + qw * qw);  the yaw pair (zy, wy) = (qz / ry, qw / ry) stands where dtc_sim_step has (qz, qw);
 *   c = 1 - 2 * (zy * zy);  s = 2 * (zy * wy);
 *   the body z-axis in the world: A = (2 * (qx * qz + qw * qy),  2 * (qy * qz - qw * qx),  1 - 2 * (qx * qx + qy * qy));
 *   in the yaw frame: m = (c * A.x + s * A.y,  c * A.y - s * A.x,  A.z);  n = m / sqrt((m.x * m.x + m.y * m.y) + m.z * m.z)
 *   (the identity quaternion, and every quaternion with qx = qy = 0, gives n = (0, 0, 1) exactly).
 * One substep: steps 1..3 of dtc_sim_step give p_l, u_l (body frame); then
 *   T1. r_l = Rt(n) p_l;  sv_l = Rt(n) u_l.  Steps 4..8 run as stated above with r_l, sv_l in place of p_l, u_l: the terrain lookup
 *       under each foot, base_z = max_l(h_l - r_l.z), contact_l = ((base_z + r_l.z) - h_l) <= contact_eps, the no-slip twist fit.
 *   T2. the new tilt, after step 7.  The stance legs of the fit are those extended to within contact_eps of the most extended leg, in the
 *       body frame: zmin = min_l p_l.z (by comparisons);  stance_l = (p_l.z - zmin) <= contact_eps;  n_s = their number.  (The contact
 *       test of step 6 cannot choose them: it is taken under the CURRENT tilt, so a level base on a slope has only its uphill feet
 *       in contact and its plane would never move.  Legs the policy lifts leave the fit; the contacts of step 6 stay what they are.)
 *       d_l = h_l - p_l.z;  d0 = d of the first stance leg;  over the stance legs, from 0.0f in leg order:
 *       tp = sum p_l.xy;  te = sum (d_l - d0);  m = tp / n_s;  me = te / n_s;  dx = p_l.x - m.x;  dy = p_l.y - m.y;  de = (d_l - d0) - me;
 *       Sxx = sum dx * dx;  Sxy = sum dx * dy;  Syy = sum dy * dy;  Sxe = sum dx * de;  Sye = sum dy * de;
 *       det = Sxx * Syy - Sxy * Sxy;  a = (Sxe * Syy - Sye * Sxy) / det;  b = (Sye * Sxx - Sxe * Sxy) / det
 *       (the centred least-squares fit d = c0 + a p.x + b p.y; equal d_l give a = b = 0 exactly);
 *       a, b clamped by comparisons to [-max_slope, max_slope];  rr = sqrt((a * a + b * b) + 1);
 *       n_new = n_s >= 3 and det > min_det ? ((-a) / rr, (-b) / rr, 1 / rr) : n
 *   T3. the tilt rate in the yaw frame: w.x = -((n_new.y - n.y) / dt);  w.y = (n_new.x - n.x) / dt: the small-angle reading of
 *       dn/dt = omega x n (at n = z it is exact; the error grows with the square of the tilt).  Then n = n_new, then step 8.
 * After the last substep, with c, s of the NEW yaw pair, Rt of the NEW n, r_l = Rt p_l, sv_l = Rt u_l, V as in dtc_sim_step:
 *   k1 = 1 + n.z;  dn = sqrt(2 * k1);  q_tilt = (tx, ty, 0, tw) = ((-n.y) / dn, n.x / dn, 0, k1 / dn);
 *   q = q_yaw (x) q_tilt = (wy * tx - zy * ty,  wy * ty + zy * tx,  zy * tw,  wy * tw)         -> root_states[3:7], base_quat;
 *   root_states[7:13] = (V.x, V.y, vz, c * w.x - s * w.y, s * w.x + c * w.y, w)  (both velocities in the world frame);
 *   base_lin_vel = Rt^T (vb.x, vb.y, vz);  base_ang_vel = Rt^T (w.x, w.y, w);  projected_gravity = (n.x, n.y, -n.z);
 *   rigid_body_state[foot_l]: columns 0..2 = (x + (c r.x - s r.y), y + (s r.x + c r.y), z + r.z), columns 7..9 = (V.x + (c g.x - s g.y),
 *   V.y + (s g.x + c g.y), vz + g.z) with g = ((sv.x - w * r.y) + w.y * r.z, (sv.y + w * r.x) - w.x * r.z, sv.z + (w.x * r.y - w.y * r.x));
 *   rigid_body_state[thigh_l]: columns 0..2 = base + Rz (Rt hip_offset_l);
 *   lin_vel_buffer takes base_lin_vel[0:2] and ang_vel_buffer base_ang_vel[2] (legged_robot_dtc.py:76-79).
 * Everything else is exactly as in dtc_sim_step. */
typedef struct DtcSimTilt {
    float max_slope;                 /* bound of the fitted slopes a, b (> 0)                                             */
    float min_det;                   /* m^4: a stance whose centred xy scatter has det <= min_det keeps the tilt (>= 0)   */
} DtcSimTilt;
/* sizeof() of DtcSimTilt, in a table of its own (dtc_sim_abi_sizes keeps its 2 entries). */
int dtc_sim_tilt_abi_sizes(int64_t* out, int cap);
int dtc_sim_step_tilt(const DtcSimStep* st, const DtcSimCfg* cfg, const DtcSimTilt* tilt, int N, void* stream);

/* ---- surrogate legged env with actuator lag and random pushes (opt-in) ---------------------
 * dtc_sim_step_act is dtc_sim_step (tilt == NULL) or dtc_sim_step_tilt (tilt != NULL) under the two disturbances the reference trains
 * every DTC policy with: the lagged PD goal of _compute_torques (legged_robot.py:608-618, :827, :248-249) and the random pushes of
 * _push_robots (:546-553, :673-678).  Still ONE launch (two further instantiations of the same kernel), still not physics: a push here
 * is a kinematic slip velocity of the base with a chosen exponential decay, not a contact dynamics -- the stance feet of a pushed env
 * slide over the ground, nothing resists, nothing topples.  push_decay_s and the floor (keep, floor2 below) are free constants of
 * the surrogate, fitted to nothing.  `forces` stay untouched (max_push_force_xy is 0 in every reference config); control types "V"
 * and "T" stay absent.  tests/sim_actuator_oracle.py restates everything below in numpy float32, bit for bit, and is the specification.
 *
 * New per-env state: lag_state [N,6,12] fp32, the scaled actions of the last six substeps, slot 0 the oldest, slot 5 the newest;
 * push_vel [N,2] fp32, the pending push in the world frame.  Both are loaded once ahead of the substeps and stored once after them.
 * Every value is a single-rounded fp32 operation in this order; everything not named is exactly as in dtc_sim_step / dtc_sim_step_tilt.
 * Substep `it` (0-based), ahead of step 1:
 *   L1. lag[i] = lag[i + 1] for i = 0..4
 *   L2. lag[5] = a * action_scale                                           (a: the clipped action of this step)
 *   L3. with `lag` set: goal = min(max(lag[lag_choice[it]] + default, lo), hi) stands where step 1 has goal; lag_choice[it] is the
 *       same for every env, as the reference's one np.random.randint(1, 5) per substep is; slot 5 is the current action, and
 *       with every choice 5 the step is dtc_sim_step's bit for bit.  With `lag` clear the goal is dtc_sim_step's, and L1, L2 still run.
 * After step 7 (and T2, T3), ahead of step 8, with the c, s of step 4, for an env with push_vel != (0, 0) (a select: an env
 * with no pending push keeps every bit of dtc_sim_step, the sign of a zero included):
 *   P1. vb.x = vb.x + (c * p.x + s * p.y);   vb.y = vb.y + (c * p.y - s * p.x)          (p = push_vel, rotated into the yaw frame)
 * After step 8:
 *   P2. p.x = p.x * keep;   p.y = p.y * keep
 *   P3. (p.x * p.x + p.y * p.y) < floor2: p.x = p.y = 0.0f
 * Everything downstream follows from vb without further change: x, y, root_states[7:9], base_lin_vel, the foot velocities, the ring
 * buffers.  After the last substep, with `push_now` set (the host sets it when common_step_counter % push_interval is 0 or 1,
 * push_interval = ceil(push_interval_s / dt), legged_robot.py:1240, :673):
 *   N1. pv = (push_span * u[0] + push_lo, push_span * u[1] + push_lo), with u = u_push[n] in [0, 1), or with u_push == NULL the words
 *       x, y (24 bits each) of Philox4x32-10, key = seed, counter = (n, 1, call counter) -- the command resample draws (n, 0, ..)
 *   N2. push_vel = pv;   root_states[7:9] = pv   (as the reference overwrites the root velocity after base_lin_vel was taken:
 *       base_lin_vel, the foot rows and the ring buffers keep this step's twist; the push acts on the base from the next step on).
 * lag_state and push_vel are then written.  With `push` clear push_vel and u_push are not touched (they may be NULL) and no push is
 * ever pending.  DTC_ERR_ARG before any launch: act == NULL, lag_state == NULL, push set with push_vel == NULL, a lag_choice[it]
 * (it < decimation) outside 0..5, keep outside (0, 1], a negative floor2 or push_span; and everything dtc_sim_step refuses. */
typedef struct DtcSimActuator {
    float* lag_state;                /* [N,6,12], read and written                                                        */
    float* push_vel;                 /* [N,2], read and written (NULL allowed when push == 0)                             */
    const float* u_push;             /* [N,2] or NULL (generated); read only when push_now                                */
    uint8_t lag_choice[64];          /* the first `decimation` entries: the slot of substep `it` (0..5)                   */
    int32_t lag;                     /* 1: L3 takes the lagged goal                                                       */
    int32_t push;                    /* 1: pushes are configured (push_vel is live)                                       */
    int32_t push_now;                /* 1: this step draws a new push (needs push)                                        */
    float keep;                      /* float32(exp(-sim_dt / push_decay_s)), in (0, 1]                                   */
    float floor2;                    /* float32(push_floor * push_floor) [m^2/s^2] (>= 0)                                 */
    float push_span, push_lo;        /* float32(2 * max_push_vel_xy), float32(-max_push_vel_xy)                           */
    int32_t reserved;
} DtcSimActuator;
/* sizeof() of DtcSimActuator, in a table of its own (the older tables keep their entries). */
int dtc_sim_act_abi_sizes(int64_t* out, int cap);
int dtc_sim_step_act(const DtcSimStep* st, const DtcSimCfg* cfg, const DtcSimTilt* tilt_or_null, const DtcSimActuator* act, int N, void* stream);

/* ---- surrogate legged env with free flight, landing and wall crashes (opt-in) --------------
 * dtc_sim_step_fly is any of the four steps above (tilt_or_null, act_or_null) with a vertical degree of freedom of the base: a base
 * whose support falls away falls under gravity, lands when it reaches a support, and a support that rises by more than max_step_up
 * within one substep is a collision that ends the episode through the reference's own rule, a base contact force above the
 * termination threshold (dtc_check_termination: 100 N).  Still ONE launch (four further instantiations of the same kernel), still not
 * physics: the flight is a point mass on a parabola, a landing dissipates whatever velocity the base arrives with, nothing tumbles.
 * The take-off rule F3, max_step_up and crash_force are choices of the surrogate, fitted to nothing.  Still absent: control types
 * "V" and "T", `forces`, contact dynamics (stance feet neither slip under load nor push back), and anything that topples the robot.
 * tests/sim_flight_oracle.py restates everything below in numpy float32, bit for bit, and is the specification.
 *
 * Carried state, no new fp32 tensor: vz, the base's z velocity, V = (V.x, V.y), its planar velocity in the world frame, and w, its yaw
 * rate.  At the first substep of a call they are root_states[9], root_states[7:9] and root_states[12]; the step writes them back there.
 * fresh = (episode_length_buf == 0 on entry): the step after a reset, which places the base on its support as dtc_sim_step does.
 * Every value is a single-rounded fp32 operation in this order; everything not named is exactly as in the step underneath.
 * One substep: steps 1..7 (T1..T3, L1..L3, P1) run as stated above and give base_z, contact_l, n_c, sv_l (= u_l without tilt), vb
 * (with a pending push), w', n_new, the tilt rate.  Then, in place of "vz = (base_z - z) / dt; z = base_z" of step 8:
 *   F1. vzb = vz - (gravity * dt);   zb = z + vzb * dt                                      (the ballistic candidate)
 *   F2. airborne = (zb - base_z) > contact_eps
 *   F3. vzg = -((sum over contact legs of sv_l.z, leg order, from 0.0f) / n_c): the take-off velocity the stance legs give the
 *       base.  It is not (base_z - z) / dt: a terrain discontinuity moves a grounded base, but gives it no momentum.
 *   F4. crashed = crashed or (not airborne and (base_z - z) > max_step_up and not fresh)    (sticky through the call)
 *   F5. grounded: V = (c * vb.x - s * vb.y, s * vb.x + c * vb.y);  w = w';  vz = vzg;  z = base_z;  n = n_new
 *       airborne: V, w and (tilt) n keep their values, the tilt rate is 0;  vz = vzb;  z = zb;  every contact_l is false, n_c = 0;
 *       a pending push (P1) adds nothing; it still decays (P2, P3).  All by selects: the grounded values are computed for every
 *       env, so no division by n_c = 0 reaches an output and a grounded env keeps the arithmetic of the step underneath.
 *   F6. x = x + V.x * dt;   y = y + V.y * dt;   the yaw pair is integrated with w as in step 8.
 * After the last substep, with c, s of the NEW yaw pair: a grounded env continues as in the step underneath, with the carried vz
 * wherever that step has vz (root_states[9], base_lin_vel through Rt^T with tilt, the foot velocities).  An airborne env (the last
 * substep's flag) takes V itself for root_states[7:9] and the foot velocities, vb = (c * V.x + s * V.y, c * V.y - s * V.x) for
 * base_lin_vel and lin_vel_buffer, and weight / n_c is replaced by 0: no foot force, contact = false.  N1, N2 overwrite
 * root_states[7:9] as before, so a push drawn in the air is the planar velocity the next call starts from.
 *   contact_forces[n][0] = (0, 0, crash_force) for a crashed env (body 0, the base: the env's termination_contact_indices);
 *   airborne[n] = the last substep's flag;   crashed[n] = the sticky flag.
 * DTC_ERR_ARG before any launch: fly == NULL, airborne or crashed NULL, gravity < 0, max_step_up <= 0, crash_force <= 100, a foot
 * that is body 0; and everything the step underneath refuses. */
typedef struct DtcSimFlight {
    float gravity;                   /* m/s^2 (>= 0)                                                                      */
    float max_step_up;               /* m: a grounded substep whose support rises by more is a crash (> 0)                */
    float crash_force;               /* N: written to contact_forces[n][0][2] of a crashed env (> 100)                    */
    uint8_t* airborne;               /* [N], written                                                                      */
    uint8_t* crashed;                /* [N], written                                                                      */
} DtcSimFlight;
/* sizeof() of DtcSimFlight, in a table of its own (the older tables keep their entries). */
int dtc_sim_fly_abi_sizes(int64_t* out, int cap);
int dtc_sim_step_fly(const DtcSimStep* st, const DtcSimCfg* cfg, const DtcSimTilt* tilt_or_null, const DtcSimActuator* act_or_null,
                     const DtcSimFlight* fly, int N, void* stream);

/* ---- surrogate legged env: leg collisions and foot stumbles on the terrain (opt-in) --------
 * dtc_sim_contacts (csrc/sim_contacts.hip) is a launch of its own that runs directly behind any dtc_sim_step* on what that launch
 * wrote, once per env step (the env kernels read contact forces once per step, after the last substep, as the reference refreshes
 * them at the top of post_physics_step).  It gives the contact-force rows of the thighs and shanks and the horizontal force of the
 * feet a content, so that the reward terms `collision`, `stumble`, `feet_stumble` and `foot_clearance` (csrc/rewards.hip) see
 * non-zero inputs in a closed-loop run.  One wavefront per env, lanes 8 l + j serve leg l: j = 0..2 the thigh samples, j = 3..6 the
 * shank samples; the eight lanes share the leg's stores.  No LDS, no atomics, no scratch.
 *
 * What this model is NOT: the forces feed the rewards and nothing else.  A colliding shank is not held back, a stumbling foot is
 * not stopped (it is still lifted onto the riser by the support rule of step 6), nothing topples, the torso has no contact of its
 * own (its row belongs to the crash of dtc_sim_step_fly), and `forces`, friction and control types "V" and "T" stay absent.  Every
 * constant of DtcSimContacts is a free choice of the surrogate, fitted to nothing.
 *
 * Inputs, as the step just wrote them: B = base_pos, q = base_quat (x, y, z, w), dof_pos (strides as in DtcSimStep),
 * H_l = rigid_body_state[thigh_l][0:3] (the hip point), F_l = rigid_body_state[foot_l][0:3], V_l = rigid_body_state[foot_l][7:9],
 * the height table, default_dof_pos, and two tables of dtc_amd.sim.knee_tables: knee_nominal [4,3] and knee_jacobian [4,3,3], the
 * knee of a leg (hip + (-l1 sin t1, l1 cos t1 sin a, -l1 cos t1 cos a)) linearised at the default pose as leg_jacobian is.
 * Every value is a single-rounded fp32 operation in the order below (-ffp-contract=off); tests/sim_contact_oracle.py restates it in
 * numpy float32, bit for bit, and is the specification.  Per leg l, with dq = dof_pos[3 l .. 3 l + 2] - default:
 *   C1. k[i] = knee_nominal[l][i] + ((Jk[l][i][0] * dq0 + Jk[l][i][1] * dq1) + Jk[l][i][2] * dq2)
 *       rot(q, v): qv = (q.x, q.y, q.z);  t = 2 * (qv x v), t.x = 2 * (q.y * v.z - q.z * v.y), t.y = 2 * (q.z * v.x - q.x * v.z),
 *       t.z = 2 * (q.x * v.y - q.y * v.x);  c = qv x t likewise;  rot.i = (v.i + q.w * t.i) + c.i
 *       K = (B.x + rot.x, B.y + rot.y, B.z + rot.z)            -> rigid_body_state[shank_l][0:3] (the other columns are left alone)
 *   C2. sample j: X = A + s * (E - A), per component, with (A, E, s) = (H, K, (j + 1) / 4) for j = 0..2 and (K, F, (j - 3) / 4)
 *       for j = 3..6 (s = 0 gives K + 0 * (F - K)); the foot point itself stays the step's business
 *   C3. pen_j = (terrain_height(X.x, X.y) + body_radius) - X.z, the lookup rule of step 5 of dtc_sim_step
 *       d = 0.0f, then in sample order d = pen_j > d ? pen_j : d (a NaN is never selected): d_thigh over j = 0..2, d_shank over 3..6
 *   C4. f = stiffness * d;  Fb = d > 0 ? (f < max_force ? f : max_force) : 0
 *       contact_forces[thigh_l] = (0, 0, Fb_thigh);  contact_forces[shank_l] = (0, 0, Fb_shank);
 *       leg_contact[n][2 l] = d_thigh > 0;  leg_contact[n][2 l + 1] = d_shank > 0
 *   C5. sp = sqrt(V.x * V.x + V.y * V.y);  e = (V.x / sp, V.y / sp);  P = (F.x + e.x * probe, F.y + e.y * probe);
 *       rise = terrain_height(P.x, P.y) - F.z;  hit = sp > min_speed && rise > stumble_height;
 *       m = wall_damping * sp;  mag = m < max_force ? m : max_force;
 *       contact_forces[foot_l][0] = hit ? -(mag * e.x) : 0;  contact_forces[foot_l][1] = hit ? -(mag * e.y) : 0;
 *       stumbled[n][l] = hit.  contact_forces[foot_l][2] is NOT written.
 * Everything else stays byte for byte: the base row of contact_forces (flight's crash force), the hip rows, every other row and
 * column of rigid_body_state.  Every comparison is false for a NaN, so an env row of NaN gives no flag and zero forces, and the
 * lookup's clamp keeps every index inside the table.
 * `st`, `cfg`: the descriptor and constants of the dtc_sim_step* call this one follows; of `st` only base_pos, base_quat, dof_pos
 * with its strides, default_dof_pos, height_samples, rigid_body_state and contact_forces are read here (the others may be NULL).
 * DTC_ERR_ARG before any launch (comparisons written so that a NaN is refused): a null descriptor or a null pointer among those
 * named, among the two tables or the two flag tensors; N outside 1..2^24; stiffness, max_force, probe or wall_damping not > 0 or
 * not finite; body_radius, stumble_height or min_speed negative or not finite; a shank that is body 0, a foot, a thigh, another
 * leg's shank or outside 0..num_bodies - 1; and what dtc_sim_step refuses of num_dof, num_bodies, feet, thighs, the table's shape
 * and scale and the dof_pos strides. */
typedef struct DtcSimContacts {
    const float* knee_nominal;       /* [4,3] base frame                                                                  */
    const float* knee_jacobian;      /* [4,3,3]: d knee_l[i] / d q[3 l + k] at the default pose                           */
    uint8_t* leg_contact;            /* [N,8], written: (thigh, shank) of leg 0, 1, 2, 3                                  */
    uint8_t* stumbled;               /* [N,4], written                                                                    */
    int32_t shanks[4];               /* body rows, leg order; the knee position is written there                         */
    float body_radius;               /* m, capsule radius of thigh and shank (>= 0)                                       */
    float stiffness;                 /* N/m, penetration spring (> 0)                                                     */
    float max_force;                 /* N, cap of every force this kernel writes (> 0)                                    */
    float probe;                     /* m, look-ahead of a moving foot (> 0)                                              */
    float stumble_height;            /* m, a face this much above the foot point is a riser (>= 0)                        */
    float wall_damping;              /* N s/m, horizontal force per foot speed at a riser (> 0)                           */
    float min_speed;                 /* m/s, below it a foot does not stumble (>= 0)                                      */
    int32_t reserved;
} DtcSimContacts;
/* sizeof() of DtcSimContacts, in a table of its own (the older tables keep their entries). */
int dtc_sim_contact_abi_sizes(int64_t* out, int cap);
int dtc_sim_contacts(const DtcSimStep* st, const DtcSimCfg* cfg, const DtcSimContacts* con, int N, void* stream);

/* ---- surrogate legged env: support-polygon balance and falls (opt-in) ----------------------
 * dtc_sim_balance (csrc/sim_balance.hip) is a launch of its own that runs directly behind any dtc_sim_step*, and in front of
 * dtc_sim_contacts, on what the step wrote, once per env step.  It is an overlay: a point-mass inverted pendulum about the edge of
 * the support polygon of the stance feet.  Per env it owns lean [N,4] fp32 = (p.x, p.y, v.x, v.y): p is the world-frame horizontal
 * direction in which the body tips times the tip angle [rad], v its rate; and fallen [N] uint8.  One lane per env, 64-thread
 * workgroups.  No LDS, no atomics, no scratch.  The ABI version stays: no existing signature or struct changes.
 *
 * What this model is NOT: attitude dynamics.  The link positions are not rotated with the lean: the feet and hips in
 * rigid_body_state stay where the step put them, so the planner and dtc_sim_contacts see the un-leaned positions (dtc_sim_contacts
 * runs behind this launch and turns its knee, C1, with the leaned base_quat about the lowered base_pos: its sample points run from
 * the un-leaned hip through that knee to the un-leaned foot).  Pushes do not
 * feed the lean rate.  There is no friction and no slipping pivot.  The stance feet are joined in the fixed order FL, FR, HR, HL
 * (legs 0, 1, 3, 2); crossed feet are neglected, a self-intersecting outline gives whatever the rule below gives.  Control types
 * "V" / "T" and `forces` stay absent.  Every constant of DtcSimBalance is a free choice of the surrogate, fitted to nothing.
 * The next step reads what this launch wrote where it carries state in root_states: the yaw pair (renormalised there; L below
 * scales q.z and q.w alike, so the yaw is kept), under dtc_sim_step_tilt the plane normal n, which a stance of three or more
 * extended legs replaces by its fit and a smaller one KEEPS, lean included (the lean is then composed onto it again: in that
 * case the attitude tips faster than |p| says), and under dtc_sim_step_fly z (lower by the drop of B8).
 *
 * Inputs, as the step just wrote them: B = base_pos, q = base_quat (x, y, z, w), F_l = rigid_body_state[foot_l][0:3],
 * stance_l = contact_filt[l] != 0, fresh = (episode_length_buf == 1: the step after a reset), projected_gravity, base_lin_vel,
 * base_ang_vel, root_states[10:12], contact_forces[0][2], lean.  Only + - * /, sqrt and comparisons, each a single-rounded fp32
 * operation in the order below (-ffp-contract=off, no libm call); tests/sim_balance_oracle.py restates it in numpy float32, bit for
 * bit, and is the specification.  Every comparison is false for a NaN.
 *   B1. V[0 .. k - 1]: the F_l of the stance legs in the order 0, 1, 3, 2, packed to the front; k = their number; V[k ..] = 0.
 *   B2. ry = sqrt(q.z * q.z + q.w * q.w);  zy = q.z / ry;  wy = q.w / ry;  cy = 1 - 2 * (zy * zy);  sy = 2 * (zy * wy);
 *       c = (B.x + (cy * ox - sy * oy),  B.y + (sy * ox + cy * oy)),  (ox, oy) = com_offset
 *   B3. area = (V1.x - V0.x) * (V2.y - V0.y) - (V1.y - V0.y) * (V2.x - V0.x), for k = 4 plus
 *       ((V2.x - V0.x) * (V3.y - V0.y) - (V2.y - V0.y) * (V3.x - V0.x)).   best = +inf, N = V0.xy; then edge j = 0..3 from V[j] to E,
 *       E = V[0] for j = 3 or j + 1 == k, else V[j + 1];  active: j == 0 ? k >= 1 : (k >= 2 and j < (k == 2 ? 1 : k)):
 *       e = E - V[j];  w = c - V[j];  ee = e.x * e.x + e.y * e.y;  t = (w.x * e.x + w.y * e.y) / ee;
 *       t = t > 0 ? (t < 1 ? t : 1) : 0  (one foot: 0 / 0 gives 0, the point itself);  G = V[j] + t * e;  r = c - G;
 *       d2 = r.x * r.x + r.y * r.y;  active and d2 < best: best = d2, N = G.   cr = e.x * w.y - e.y * w.x;
 *       left = every active edge has cr >= 0;  right = every active edge has cr <= 0.
 *       inside = k >= 3 and ((area > 0 and left) or (area < 0 and right));  dist = sqrt(best);  d = inside ? -dist : dist;
 *       u = ((c.x - N.x) / dist, (c.y - N.y) / dist)
 *   B4. top = V0.z, then for slot 1..3: k > slot and V[slot].z > top: top = V[slot].z;  h0 = B.z - top;  h = h0 > h_min ? h0 : h_min
 *   B5. den = h * h + d * d;  m0 = sqrt(p.x * p.x + p.y * p.y);  outside = k >= 1 and d > 0;  within = k >= 1 and not outside;
 *       outside:              a.i = (gravity * (d * u.i + h * p.i)) / den
 *       within and m0 > 0:    a.i = -(((gravity * (-d)) * p.i) / (m0 * den))                              (restoring)
 *       else (k = 0: airborne, no torque; or upright over the support):  a = 0
 *   B6. v' = v + a * dt;  p' = p + v' * dt;  dot = p'.x * p.x + p'.y * p.y;  m1 = sqrt(p'.x * p'.x + p'.y * p'.y);
 *       lands = within and (not (m0 > 0) or dot <= 0 or m1 < lean_eps);  lands or fresh: p' = v' = 0 (the arrival rate is
 *       dissipated, as a landing of dtc_sim_step_fly is).  A lean only lands over its support: outside it passes through zero.
 *   B7. m = sqrt(p'.x * p'.x + p'.y * p'.y);  fell = m > fall_angle;  fallen[n] = fell;
 *       fell: contact_forces[n][0][2] = (f0 < fall_force ? fall_force : f0), f0 its value (a crash force of dtc_sim_step_fly is
 *       never lowered); dtc_check_termination then ends the episode by the reference's rule.  Otherwise the row is not written.
 *   B8. l = (-(p'.y * 0.5), p'.x * 0.5);  ln = sqrt((l.x * l.x + l.y * l.y) + 1);  L = (l.x / ln, l.y / ln, 0, 1 / ln): the rotation
 *       about the horizontal axis z x p' by 2 atan(m / 2) (m - m^3 / 12: at fall_angle 0.8 it is 0.761).  q' = L (x) q:
 *       q'.x = (L.w * q.x + L.x * q.w) + L.y * q.z;   q'.y = (L.w * q.y - L.x * q.z) + L.y * q.w;
 *       q'.z = (L.w * q.z + L.x * q.y) - L.y * q.x;   q'.w = (L.w * q.w - L.x * q.x) - L.y * q.y;   qc = (-q'.x, -q'.y, -q'.z, q'.w);
 *       with rot(q, v) of C1 above:  g = rot(qc, (0, 0, -1));  lv = rot(qc, rot(q, base_lin_vel));
 *       ww = rot(q, base_ang_vel);  av = rot(qc, (ww.x + (-v'.y), ww.y + v'.x, ww.z))   (the lean rate is omega = z x v');
 *       z1 = B.z - (h * (m * m)) * 0.5
 *   B9. lean[n] = (p'.x, p'.y, v'.x, v'.y).  rigid_body_state[n][0][0:7] = (B.x, B.y, zz, qq) with (zz, qq) = (z1, q') if m > 0, else
 *       (B.z, q).  With m > 0 only: base_quat = root_states[3:7] = q';  projected_gravity = g;  base_lin_vel = lv;  base_ang_vel = av;
 *       root_states[10] += -v'.y;  root_states[11] += v'.x;  root_states[2] = base_pos[2] = z1.  With m > 0 false (upright, or
 *       a NaN) those tensors keep their bytes.
 * Everything else stays byte for byte: every other row and column of rigid_body_state and contact_forces, every input.
 * `st`, `cfg`: the descriptor and constants of the dtc_sim_step* call this one follows; of `st` only the tensors named above are
 * read here (the others may be NULL), of `cfg` num_bodies and feet.  DTC_ERR_ARG before any launch (comparisons written so that a
 * NaN is refused): a null descriptor or a null pointer among those named or lean / fallen; N outside 1..2^24; h_min, fall_angle or
 * dt not > 0 or not finite; fall_force not > 100 (the termination threshold) or not finite; gravity or lean_eps negative or not
 * finite; a com_offset that is not finite; num_bodies < 2; a foot that is body 0 or outside 1..num_bodies - 1. */
typedef struct DtcSimBalance {
    float* lean;                     /* [N,4], read and written: (p.x, p.y, v.x, v.y)                                     */
    uint8_t* fallen;                 /* [N], written                                                                      */
    float gravity;                   /* m/s^2 (>= 0)                                                                      */
    float h_min;                     /* m, floor of the pendulum's length (> 0)                                           */
    float lean_eps;                  /* rad, a lean over its support shorter than this lands (>= 0)                       */
    float fall_angle;                /* rad, |p| above it is a fall (> 0)                                                 */
    float fall_force;                /* N, raised into contact_forces[n][0][2] of a fallen env (> 100)                    */
    float dt;                        /* s, float32(sim_dt * decimation): one integration step per env step (> 0)          */
    float com_offset[2];             /* m, base frame: the centre of mass relative to the base's origin                   */
} DtcSimBalance;
/* sizeof() of DtcSimBalance, in a table of its own (the older tables keep their entries). */
int dtc_sim_balance_abi_sizes(int64_t* out, int cap);
int dtc_sim_balance(const DtcSimStep* st, const DtcSimCfg* cfg, const DtcSimBalance* bal, int N, void* stream);

/* ---- DTC curriculum terrain, generated on the device (opt-in) ------------------------------
 * dtc_terrain_generate (csrc/terrain.hip) fills the int16 height table [tot_rows, tot_cols] (border included: zeros) and
 * terrain_origins [R, C, 3] fp32 from one seed, as ONE launch: the first blocks write the table, the last R * C blocks the origins
 * (each recomputes its sub-terrain's central window; the table is not read back).  No second launch, no atomics, nothing outside the
 * two outputs is written.  tests/terrain_oracle.py restates everything below in numpy and is the specification; the kernel equals it
 * bit for bit.
 *
 * The reference's (legged_gym/utils/terrain.py): the layout, the choice of a family, the parameters, the origins, and families 6 (gap)
 * and 7 (pit) cell for cell.  This project's: the cells of families 0..5 and 8.  The reference takes those from isaacgym.terrain_utils
 * and from Python loops over numpy's random stream; here they are pure functions of (cfg, seed, i, j, cell) with the reference's
 * parameters -- not its random sequence, and not isaacgym's code.
 *
 * Arithmetic: parameters are IEEE doubles in the order written (-ffp-contract=off), as the reference's Python floats, so every
 * int(x / scale) below is the reference's (int() truncates toward zero); cells are integers; `//` is Python's floor division.
 * Geometry (terrain.py:20-30), hs = horizontal_scale, vs = vertical_scale, R = num_rows, C = num_cols:
 *   S = int(terrain_length / hs) cells per sub-terrain side (terrain_length == terrain_width, else DTC_ERR_ARG; at least 2 m);
 *   border = int(border_size / hs);  tot_rows = R * S + 2 * border;  tot_cols = C * S + 2 * border (< 2^31 cells, else DTC_ERR_ARG);
 *   sub-terrain (i, j) occupies rows border + i * S .., columns border + j * S ..; (a, b) is a cell inside it.
 * Origins (terrain.py:143-160): x = (i + 0.5) * terrain_length;  y = (j + 0.5) * terrain_width;  z = the maximum of the cells
 *   [x1, x2) x [x1, x2), x1 = int((terrain_length / 2 - 1) / hs), x2 = min(int((terrain_length / 2 + 1) / hs), S), times vs; each a
 *   double rounded once to fp32.
 * Draws: Philox4x32-10, key = (seed low, seed high), counter = (item, sub-terrain index i * C + j, purpose, 0x74657272), so no two
 *   draws share a counter; words x, y, z, w;  below(word, n) = (word * n) >> 32 in 64 bits.  Purposes: 0 layout (item 0), 1 noise node
 *   (item na * W + nb), 2 rectangle (item r), 3 stepping-stone row shift (item b // p), 4 stones-everywhere row shift (item b // p),
 *   5 stones-everywhere stone (item (b // p) * 65536 + (a + shift) // p).
 * Family and difficulty (terrain.py:45-62): curriculum: difficulty = i / R, choice = j / C + 0.001; else choice = x * 2^-32 and
 *   difficulty = {0.25, 0.5, 0.75, 0.9}[y >> 30] of the layout draw.  `proportions` are the CUMULATIVE sums of terrain_proportions as
 *   Terrain.__init__ takes them, padded to nine entries with 2.0.  make_terrain (terrain.py:79-141, the "lite3" values):
 *   slope = difficulty * 0.4;  stepping_stones_size = 1.05 - difficulty;  step_height = 0.05 + 0.13 * difficulty;
 *   discrete_obstacles_height = 0.05 + difficulty * 0.15;  stone_distance = difficulty == 0 ? 0.03 : 0.06;
 *   max_height = 0.02 + 0.03 * difficulty;  stone_size = -0.1 * difficulty + 0.3;  gap_size = pit_depth = 0.8 * difficulty;
 *   choice < p[0]: family 0 (slope negated when choice < p[0] / 2);  < p[1]: 1;  < p[3]: stairs, 2 (step_height negated) when
 *   choice < p[2], else 3;  < p[4]: 4;  < p[5]: 5;  < p[6]: 6;  < p[7]: 7;  else 8.
 * Cells, in units of vs (clamped to int16 at the end).  e = min(a, S - 1 - a, b, S - 1 - b);  e_max = max((S - int(3 / hs)) // 2, 0);
 * platform(size): P = int(size / hs);  the square [(S - P) // 2, (S + P) // 2) in a and b (P >= S: the whole sub-terrain).
 *   0 smooth slope:  rint(((slope * hs) * min(e, e_max)) / vs)                      (a pyramid; its flat top is the 3 m platform)
 *   1 rough slope:   family 0 plus lattice noise: g = max(int(0.2 / hs), 1), W = S // g + 2, node (na, nb) carries
 *                    n = ((below(x, 21) - 10) * 0.005) / vs;  with na = a // g, nb = b // g, fa = a % g, fb = b % g:
 *                    t = (((g - fa) * (g - fb)) * n[na][nb] + (fa * (g - fb)) * n[na + 1][nb]) +
 *                        (((g - fa) * fb) * n[na][nb + 1] + (fa * fb) * n[na + 1][nb + 1]);   noise = rint(t / (g * g))
 *   2 / 3 stairs:    (min(e, e_max) // max(int(0.31 / hs), 1)) * int(step_height / vs)
 *   4 discrete:      20 rectangles r: la = min(int(1 / hs) + below(x, int(2 / hs) - int(1 / hs) + 1), S), lb likewise from y,
 *                    pa = below(z, S - la + 1), pb = below(w, S - lb + 1);  full = int(discrete_obstacles_height / vs);
 *                    mag = y & 1 ? full : full // 2;  value = x & 1 ? -mag : mag;  the highest r whose rectangle
 *                    [pa, pa + la) x [pb, pb + lb) holds the cell gives its value, no rectangle: 0;  platform(3): 0
 *   5 stepping:      s = int(stepping_stones_size / hs);  p = max(s + int(stone_distance / hs), 1);  shift = below(x, p) of row b // p;
 *                    stone when s >= S, or s >= 1 and b % p < s and (a + shift) % p < s: 0;  else int(-2 / vs);  platform(1): 0
 *   6 gap:           gap_terrain (terrain.py:162-173), its two slice assignments with Python's slice rules (a negative start counts
 *                    from the end): -1000 in the outer square, 0 in the inner
 *   7 pit:           pit_terrain (terrain.py:175-182): -int(pit_depth / vs) in the square S // 2 -+ int(1 / hs / 2)
 *   8 stones:        m = int(stone_size / hs);  p = max(m + int(stone_distance / hs), 1);  shift as in 5 (purpose 4);  t = a + shift;
 *                    the stone (b // p, t // p) has sa = m - 1 + below(x, 2), sb = m - 1 + below(y, 2) and height
 *                    1 + below(z, 2 * int(max_height / vs)) (0 when int(max_height / vs) < 1);  b % p < sb and t % p < sa: that height;
 *                    else int(-2 / vs);  platform(1.3): 0
 * `cfg` is a HOST pointer; height_samples (2-byte aligned) and terrain_origins are DEVICE pointers of tot_rows * tot_cols int16 and
 * R * C * 3 floats.  A bad argument returns DTC_ERR_ARG before any launch. */
typedef struct DtcTerrainCfg {
    double horizontal_scale, vertical_scale, border_size, terrain_length, terrain_width;      /* [m]                     */
    double proportions[9];           /* cumulative terrain_proportions, padded with 2.0                                   */
    int32_t num_rows, num_cols;      /* R (levels), C (types)                                                             */
    int32_t curriculum;              /* 1: curiculum(), 0: randomized_terrain()                                           */
    int32_t tot_rows, tot_cols;      /* the table as the caller allocated it: must equal the geometry above               */
    int32_t reserved;                /* 0                                                                                 */
    uint64_t seed;
} DtcTerrainCfg;
/* sizeof() of DtcTerrainCfg, in a table of its own (the other tables keep their lengths). */
int dtc_terrain_abi_sizes(int64_t* out, int cap);
int dtc_terrain_generate(const DtcTerrainCfg* cfg, int16_t* height_samples, float* terrain_origins, void* stream);

/* ---- rollout-side store (row f2) ---------------------------------------------------------
 * RolloutStorage.add_transitions, rsl_rl/rsl_rl/storage/rollout_storage.py:99-116: the 13 `copy_` of one env step as
 * ONE launch (each item: N rows of width_bytes, source row stride src_stride_bytes -- 0 for a broadcast row such as
 * action_sigma -- into a dense destination), plus the time-out bootstrap of PPO.process_env_step, ppo.py:162-163:
 * rewards_dst[n] = rewards[n] + gamma * values[n] * time_outs[n] (time_outs NULL = plain copy; rewards_dst NULL = skip).
 * `items` is a HOST array of at most 16 descriptors holding DEVICE pointers. */
typedef struct DtcRowCopy {
    const void* src;
    void* dst;
    int64_t src_stride_bytes;
    int32_t width_bytes;
} DtcRowCopy;
int dtc_store_transition(const DtcRowCopy* items, int n_items, const float* rewards, const float* values,
                         const uint8_t* time_outs_or_null, float gamma, float* rewards_dst, int N, void* stream);

/* HistoryWrapper.step / get_observations, rsl_rl/rsl_rl/env/wrappers/history_wrapper.py:23,37:
 * out = cat(obs_history[:, num_obs:], obs) ([N, history_len*num_obs] <= 1024 floats per row); `out` may alias
 * `obs_history`.  The reference builds a NEW tensor every step and callers keep the old one until the transition is
 * stored, so the host wrapper ping-pongs two buffers.  Rows with reset[n] != 0 are cleared first (reset_idx, :42). */
int dtc_history_roll(const float* obs_history, const float* obs, float* out, const uint8_t* reset_or_null, int N,
                     int history_len, int num_obs, void* stream);

/* ---- RolloutStorage.compute_returns: rsl_rl/rsl_rl/storage/rollout_storage.py:138-152 --- */
/* GAE scan; writes returns and the UN-normalised advantages (returns - values) and
 * stats[0] = sum(advantages) (double).  stats is double[4] on the device. */
int dtc_gae(const float* rewards, const float* values, const uint8_t* dones, const float* last_values,
            float gamma, float lam, float* returns, float* advantages, double* stats, int T, int N,
            void* stream);
/* stats[1] = sum((adv - stats[0]/count)^2).  `count` is the GLOBAL sample count (data-parallel
 * callers all-reduce stats[0] first and pass world_size*T*N). */
int dtc_adv_sqdev(const float* advantages, double* stats, int64_t n_local, double count, void* stream);
/* adv = (adv - mean) / (std_unbiased + 1e-8) with mean = stats[0]/count, std from stats[1]. */
int dtc_adv_normalize(float* advantages, const double* stats, int64_t n_local, double count, void* stream);

/* ---- containment of non-finite rollout rows (PPO(contain_nonfinite=True)): rollout_storage.py:138-152, 165 --------------------
 * Row (t, n) of the stored rollout is VALID iff every element of its row is finite (exponent field not all ones: denormals, +-0 and
 * +-FLT_MAX are finite) in every stored fp32 tensor, and its return and un-normalised advantage are finite.  The record is one byte
 * per flat row t * N + n (1 = valid). */
/* The record of the stored tensors (rollout_storage.py:57-97, the buffers the sums of :138-152 and the mini-batches of :165 read):
 * `mats` / `widths` are HOST arrays of `count` (1..16) device pointers to contiguous fp32 [R, widths[i]] matrices (4-byte aligned, any
 * width >= 1, any size: 64-bit flat indices) -- row_valid[r] &= every element of row r of every matrix is finite.  row_valid is
 * read-modify-write in the sense that the kernel only ever stores 0: the caller initialises it (to 1, or to an earlier record). */
int dtc_rows_finite(const float* const* mats, const int64_t* widths, int count, int64_t R, uint8_t* row_valid, void* stream);
/* dtc_gae (rollout_storage.py:138-150) with the record: the same scan statement for statement (a NaN travels backwards through an
 * env's earlier steps, also across a done); row_valid[o] <- row_valid[o] AND finite(return) AND finite(advantage);
 * stats[0] = sum(advantages) and stats[1] = count over the rows that are valid afterwards.  stats is double[4] on the device. */
int dtc_gae_contained(const float* rewards, const float* values, const uint8_t* dones, const float* last_values, float gamma,
                      float lam, float* returns, float* advantages, uint8_t* row_valid, double* stats, int T, int N, void* stream);
/* rollout_storage.py:151-152 over the valid rows: stats[2] = sum((adv - stats[0]/stats[1])^2); then adv = (adv - mean) /
 * (std_unbiased + 1e-8) on the valid rows (invalid rows keep what the scan wrote).  The count is READ FROM stats[1] on the device
 * (data-parallel callers all-reduce stats[0..1] in one collective first, stats[2] in a second); reductions in the order of
 * dtc_adv_sqdev / dtc_adv_normalize, so with no invalid row the results are theirs bit for bit. */
int dtc_adv_sqdev_contained(const float* advantages, const uint8_t* row_valid, double* stats, int64_t n_local, void* stream);
int dtc_adv_normalize_contained(float* advantages, const uint8_t* row_valid, const double* stats, int64_t n_local, void* stream);
/* The rows a permutation of rollout_storage.py:165 may name: record -> valid_list[0 .. *n_valid) = the valid flat rows in ascending
 * order, *n_valid = their number (both on the device;
 * valid_list has room for n entries, those behind *n_valid are not written).  Deterministic (counts, one single-block scan, scatter);
 * `workspace`: dtc_compact_workspace(n) bytes. */
int64_t dtc_compact_workspace(int64_t n);
int dtc_compact_valid(const uint8_t* row_valid, int64_t n, int64_t* valid_list, int64_t* n_valid, void* workspace, void* stream);
/* The permutation of rollout_storage.py:165 over valid rows only: out[j] = perm[j] where row perm[j] is valid, else
 * valid_list[perm[j] % *n_valid].  The length does not change; with no invalid row out == perm.  (*n_valid == 0, or an entry outside
 * [0, R): the entry passes through.) */
int dtc_perm_repair(const int64_t* perm, int64_t len, const uint8_t* row_valid, int64_t R, const int64_t* valid_list,
                    const int64_t* n_valid, int64_t* out, void* stream);

/* ---- containment of non-finite rollout ENVS (contain_nonfinite_envs=True of all three trainers) -------------------------------
 * The unit is an env, a column of the [T, N, ...] storage: env n is VALID iff every row t * N + n of the record above is, the record
 * now also covering the saved hidden states (rollout_storage.py:118-132).  Invalid columns are overwritten in the storage by valid
 * ones before rollout_storage.py:138-152 runs; the sources are dtc_compact_valid + dtc_perm_repair over the identity permutation:
 * env_src[n] = n where env n is valid, else valid_list[n % *n_valid] (no valid env: the identity). */
/* The record of one saved hidden-state tensor, contiguous fp32 [T, L, N, H] (4-byte aligned, any H >= 1, 64-bit flat indices):
 * row_valid[t * N + n] &= every element of [t, l, n, :] is finite for every layer l -- the finiteness rule and the store-0-only
 * contract of dtc_rows_finite. */
int dtc_states_finite(const float* s, int64_t T, int64_t L, int64_t N, int64_t H, uint8_t* row_valid, void* stream);
/* env_valid[n] = AND over t of row_valid[t * N + n] (every entry written; deterministic). */
int dtc_env_fold(const uint8_t* row_valid, int64_t T, int64_t N, uint8_t* env_valid, void* stream);
/* One per-env buffer of the storage as `outer` rows per env: row (o, n) is the width_bytes bytes at
 * base + o * outer_stride_bytes + n * env_stride_bytes.  [T, N, w]: outer = T; saved states [T, L, N, H]: outer = T * L; [N, w]: outer = 1. */
typedef struct DtcEnvColumn {
    void* base;
    int64_t outer;
    int64_t outer_stride_bytes;
    int64_t env_stride_bytes;
    int32_t width_bytes;
} DtcEnvColumn;
/* For every env n with env_valid[n] == 0 and env_src[n] another env of [0, N): rows (o, env_src[n]) copied over rows (o, n) of every
 * item, bit for bit.  `items` is a HOST array of n_items (1..dtc_env_columns_cap()) descriptors; env_valid / env_src are on the device,
 * and so is the number of invalid envs: the launch is a fixed grid sized from the device's CU count, which ends after one pass over
 * env_valid when there is nothing to repair.  16-byte accesses where base, strides and width of an item allow them, else 4-byte or
 * 1-byte ones; 64-bit byte offsets.  Source columns (valid envs) are never written: the result does not depend on scheduling.
 * The kernel trusts the descriptors (as dtc_store_transition does); null pointers, n_items outside 1..cap, width_bytes < 1,
 * outer < 1 and an env stride below the width are rejected with DTC_ERR_ARG before any launch. */
int dtc_env_columns_cap(void);
int dtc_env_columns_repair(const DtcEnvColumn* items, int n_items, const uint8_t* env_valid, const int64_t* env_src, int64_t N,
                           void* stream);
/* sizeof() of DtcEnvColumn, as dtc_abi_sizes gives them for the older structs (whose table keeps its 18 entries): compared by the
 * binding at load time. */
int dtc_contain_envs_abi_sizes(int64_t* out, int cap);

/* ---- containment of non-finite envs AT THE ROLLOUT STEP (contain_nonfinite_act=True of all three trainers) ----------------------
 * One launch behind the policy step of act(), in front of env.step(): an env whose step consumed or produced anything non-finite
 * leaves act() with finite (zero) actions and a cleared live recurrent state, and is named in two device-side masks. */
/* One fp32 tensor with an env dimension as `outer` rows per env: element (o, n, j), j < width, sits at
 * base + o * outer_stride_elems + n * env_stride_elems + j (counted in 4-byte elements).  [N]: outer = 1, width = 1; [N, w]: outer = 1;
 * live states [L, N, H]: outer = L.  mode 0: the item is scanned only; mode 1: scanned, then zeroed at every bad env. */
typedef struct DtcActItem {
    void* base;
    int64_t outer;
    int64_t outer_stride_elems;              /* not read where outer == 1 */
    int64_t env_stride_elems;
    int32_t width;
    int32_t mode;
} DtcActItem;
/* For every env n of [0, N): bad(n) = any element of any item at env n, over all outer indices, has all exponent bits set (NaN,
 * +-inf).  act_valid_row[n] = !bad(n) and env_bad[n] = bad(n) (uint8 on the device, each may be NULL, each written for EVERY env, 0 or
 * 1); where bad(n), every element of every mode-1 item at env n becomes +0.0f.  Nothing else is written: a good env's bytes stay as
 * they are in every item, a mode-0 item is never written.  `items` is a HOST array of n_items (1..dtc_act_contain_cap()) descriptors.
 * One wavefront owns an env: no atomics, no second launch, the result does not depend on scheduling; rows are accessed 16 bytes at a
 * time over their 16-byte aligned middle, whatever their width and start.  The kernel trusts the descriptors; rejected with
 * DTC_ERR_ARG before any launch: null `items`, n_items outside 1..cap, N outside 1..2^31, a null or not 4-byte aligned base,
 * width < 1, outer < 1, env_stride_elems < width, outer > 1 with outer_stride_elems < width, a mode other than 0 / 1, and a call
 * with both outputs NULL and no mode-1 item (nothing to do); also what would overflow the 64-bit element offsets: outer > 2^20,
 * env_stride_elems > 2^31, outer_stride_elems > 2^40 (where outer > 1). */
int dtc_act_contain_cap(void);
int dtc_act_contain(const DtcActItem* items, int n_items, int64_t N, uint8_t* act_valid_row, uint8_t* env_bad, void* stream);
/* sizeof() of DtcActItem, in a table of its own (dtc_abi_sizes keeps its 18 entries, dtc_contain_envs_abi_sizes its one): compared by
 * the binding at load time. */
int dtc_act_contain_abi_sizes(int64_t* out, int cap);

/* ---- mini-batch gather: rollout_storage.py:195-209 (`tensor[batch_idx]`) ------------------ */
int dtc_gather_rows(const void* src, const int64_t* idx, void* dst, int64_t rows, int64_t row_bytes,
                    void* stream);
/* inverse map, dst[idx[r]] = src[r] (fp32 rows): the backward of `unpad_trajectories`
 * (rsl_rl/rsl_rl/utils/utils.py:67-70) -- gradients of the valid steps go back into the padded layout. */
int dtc_scatter_rows(const float* src, const int64_t* idx, float* dst, int64_t rows, int64_t row_floats,
                     void* stream);

/* ---- dense layers (nn.Linear + ReLU/ELU and their autograd; actor_critic_decoder.py:98-188,
 *      323-349).  A "segmented matrix" is the virtual concatenation torch.cat([...], dim=1) of
 *      up to 4 column blocks, each optionally row-gathered by the mini-batch index
 *      (ppo.py:201, actor_critic_decoder.py:431,550; rollout_storage.py:195-209) -- the cat and
 *      the gather are never materialised. ------------------------------------------------- */
typedef struct DtcSeg {
    float* ptr;          /* base of the source matrix (NULL = segment absent for outputs)       */
    int64_t ld;          /* leading dimension of the source matrix                              */
    int32_t col0;        /* first column inside the source matrix                               */
    int32_t width;       /* number of columns of this block                                     */
    int32_t gather;      /* 1: row m of the virtual matrix is row idx[m] of the source          */
    int32_t accumulate;  /* outputs only: 1 = add into the destination instead of overwriting   */
    int64_t rows;        /* inputs: number of rows of the source matrix (rows*ld floats behind ptr are readable: the
                          * loaders read 16 bytes at a time and bound their buffer descriptor with it -- reads past
                          * the last row return 0); outputs: unused.  rows * ld must stay below 2^29 floats (2 GiB) for
                          * every entry point but dtc_h2i_pack, whose wide-source kernel addresses larger sources with
                          * 64-bit lane addresses (as does the target of dtc_linear_fwd_mse_h2i)                          */
    uint32_t* amax;      /* two-term fp16 path (dtc_*_h2) only, device pointer.  Inputs: slot that holds the bit pattern of the
                          * largest |x| of the source tensor (or of any superset of the block: an upper bound costs precision only
                          * when it is more than ~2^10 too large), written by dtc_amax or by the kernel that produced the tensor.
                          * Outputs: slot that receives max(slot, largest |value| this call writes to the block), or NULL    */
} DtcSeg;

typedef struct DtcSegMat {
    int32_t nseg;        /* 1..4                                                                */
    int32_t cols;        /* sum of widths                                                       */
    const int64_t* idx;  /* mini-batch row indices for gathered segments (may be NULL)          */
    DtcSeg seg[4];
} DtcSegMat;

/* dst[rows, X->cols] (row stride ld_dst) = the segments of X side by side, row-gathered where a segment asks for it: packs
 * the narrow leading blocks of a layer input into one dense operand (see csrc/gae.hip: dtc_pack_cols). */
int dtc_pack_cols(const DtcSegMat* X, float* dst, int64_t ld_dst, int64_t rows, uint32_t* dst_amax /* amax slot of dst (two-term fp16 GEMM
                  path, see DtcSeg.amax) or NULL */, void* stream);

/* Y[M,N] = act(X[M,K] W[N,K]^T + b).  X is segmented (host struct). */
int dtc_linear_fwd(const DtcSegMat* X, const float* W, const float* b, float* Y, int64_t ldy,
                   int M, int N, int K, int act, void* stream);
/* Same layer with the ReLU activation, additionally writing the SIGN RECORD of its output: one bit per element
 * (y > 0), dtc_relu_mask_elems(M, N) 16-bit words -- word [(row / 32) * 2 + half][col] holds the 16 rows
 * 4 * half + (r & 3) + 8 * (r >> 2), r = bit index, of its 32-row block (the accumulator layout of the kernels).
 * dtc_linear_dgrad_mask reads it instead of the saved activation: 1/32 of the bytes, the same bits as
 * `y > 0 ? g : 0` (torch's ReLU backward, rsl_rl/modules/actor_critic_decoder.py:98-131 encoder / decoder stacks under
 * ppo.py:252, 333).  Requires M % 128 == 0 and N a multiple of the launch's tile width (N % 128 == 0, or N == 64). */
int64_t dtc_relu_mask_elems(int M, int N);
int dtc_linear_fwd_mask(const DtcSegMat* X, const float* W, const float* b, float* Y, int64_t ldy, uint16_t* relu_mask,
                        int M, int N, int K, void* stream);
/* dX[M,K] = (dZ[M,N] W[N,K]) * (relu_mask bit), single-segment destination; M % 128 == 0, K as N above. */
int dtc_linear_dgrad_mask(const float* dZ, int64_t lddz, const float* W, const DtcSegMat* dX, const uint16_t* relu_mask,
                          int M, int N, int K, void* stream);
/* dtc_linear_fwd / dtc_linear_fwd_mask (relu_mask may be NULL) that also adds the largest |Y| it writes to the amax record y_amax of
 * the two-term fp16 GEMM path (DtcSeg.amax below) -- for the narrow layers whose result a split-path kernel consumes.  dtc_linear_dgrad /
 * dtc_linear_dgrad_mask do the same for a SINGLE destination block that brings a record in dX->seg[0].amax. */
int dtc_linear_fwd_amax(const DtcSegMat* X, const float* W, const float* b, float* Y, int64_t ldy, uint16_t* relu_mask,
                        uint32_t* y_amax, int M, int N, int K, int act, void* stream);
/* ---- split-precision path (csrc/gemm_s3.hip): the same products on the bf16 matrix pipe, every fp32 operand split into
 * three bf16 terms (a = a1 + a2 + a3 exactly to 2^-24 |a|) and the six leading cross products accumulated in fp32 -- fp32-level
 * accuracy (tests/test_hip_split.py measures it against fp64 next to the single-pass kernels) at up to 2.67x the fp32 MFMA
 * rate; results are NOT bit-identical to the fmaf chain of dtc_linear_fwd.  Same argument meaning as dtc_linear_fwd /
 * dtc_linear_fwd_mask (relu_mask may be NULL) and dtc_linear_dgrad / dtc_linear_dgrad_mask. */
/* Library-side switch for the entry points that have no `_s3` twin of their own: with it on, dtc_linear_wgrad (and through it
 * the W_hh / W_ih weight gradients inside dtc_gru_bwd / dtc_lstm_bwd) runs as a one-layer dtc_wgrad_group_s3, and
 * dtc_linear_wgrad_workspace / dtc_gru_workspace / dtc_lstm_workspace return sizes that fit either path.  Off by default;
 * dtc_amd/ops.py sets it from DTC_GEMM_SPLIT. */
void dtc_set_gemm_split(int on);
int dtc_get_gemm_split(void);
/* The two-term fp16 calls scale an operand that brings no amax record by the largest |x| of the tensor, computed by the call.  Off
 * (default): over every element -- one NaN or inf in the operand makes the exponent, and with it every row of the product, useless.  On:
 * over the FINITE elements only, so that a non-finite element stays in its row of the product (it converts to fp16 inf / NaN there); on
 * finite operands both settings give the same bits.  Set around the rollout step by the trainers under contain_nonfinite_act.
 * It is ONE host variable of the process, read when a call launches its amax kernel: not per thread, not per stream -- a second thread
 * that launches two-term calls while it is on gets the finite-only amax too -- and a graph captured while it is on keeps the value it
 * was captured with at every replay, whatever the switch says then. */
void dtc_set_amax_finite_only(int on);
int dtc_get_amax_finite_only(void);
/* Weight image: the W operand of a split-path call as the kernel's LDS planes -- for every 128-column tile and 16-k stage one
 * 12 KiB chunk [plane 3][row 128][16 k bf16], copied into LDS by LDS-DMA (no conversion work for W inside the K loop).  Built by
 * the call itself into `wplanes` (wimage_ready = 0; scratch of dtc_s3_planes_bytes(N, K) bytes -- for the data gradient
 * (K, N) --, 16-byte aligned, private to the call until it has completed on its stream), or beforehand for many calls at once
 * by dtc_s3_wimage_group (wimage_ready = 1: `wplanes` is the image of exactly this call: same W, shape and operand segments). */
int64_t dtc_s3_planes_bytes(int N, int K);
typedef struct DtcWimgJob {
    const float* W;              /* [N, K] as stored                                                                        */
    void* img;                   /* dtc_s3_planes_bytes(N, K) (trans: (K, N)) bytes                                         */
    const DtcSegMat* seg;        /* trans == 0: the X operand of the forward call; trans == 1: the dX destination          */
    int32_t N, K, trans;
} DtcWimgJob;
int dtc_s3_wimage_group(const DtcWimgJob* jobs, int count, void* stream);
int dtc_linear_fwd_s3(const DtcSegMat* X, const float* W, const float* b, float* Y, int64_t ldy, uint16_t* relu_mask,
                      void* wplanes, int wimage_ready, int M, int N, int K, int act, void* stream);
int dtc_linear_dgrad_s3(const float* dZ, int64_t lddz, const float* W, const DtcSegMat* dX, const float* Xsaved,
                        int64_t ldxs, const uint16_t* relu_mask, void* wplanes, int wimage_ready, int M, int N, int K, int act,
                        void* stream);
/* dtc_linear_fwd_mse / dtc_linear_fwd_mse_parts on the split-precision path */
/* ---- block-scaled two-term fp16 operand images (round 5; csrc/h2i_core.hpp, gemm_h2i.hip, wgrad_h2i.hip): THE representation of the
 * wide layers' operands -- the fp32 products of actor_critic_decoder.py:98-188, 323-349 (under ppo.py:197-218, 252, 265, 289, 333) with
 * every operand held in HBM as the (hi, lo) fp16 planes the K loops read by LDS-DMA, 4 bytes per element, scaled by a power of two chosen
 * PER ROW and block of 128 columns (weights alike: per row of the weight image, i.e. per feature) from the block's own largest finite element:
 *   image(M, K) = ceil(M / 128) x ceil(K / 16) chunks of 8 KiB [plane 2][slot 256][16 bytes] + int32 exps[row tile][k block][128];
 *   dtc_h2i_bytes(M, K) bytes, 16-byte aligned, < 2 GiB.  Rows >= M and columns >= K are zero.
 * Every element is exact to 2^-22 of its row block's largest element whatever the rest of the tensor holds (no tensor-wide amax, no
 * records, nothing to keep in step on the host), and a non-finite element poisons only the outputs that depend on it -- its row in the
 * forward / data-gradient products, its column of dW in the weight gradient -- as in the fp32 reference.
 * Producers: dtc_h2i_pack (fp32 segmented / row-gathered operand -> image: the rollout storage, narrow hand-over tensors), the epilogues
 * of dtc_linear_fwd_h2i / _mse_h2i / dtc_linear_dgrad_h2i (results as fp32, as an image, or both), dtc_h2i_wimage_group (weights).
 * dtc_h2i_unpack decodes an image (tests). */
int64_t dtc_h2i_bytes(int M, int K);
/* tuning: forward / data-gradient launches with at most max_tiles 128 x 128 result tiles run on 64-row tiles (twice the workgroups; default
 * 256 = one tile per CU; 0: never; -1: back to DTC_H2I_ROWS64_MAX / the default).  Results are bit-identical either way. */
void dtc_h2i_rows64_max(int max_tiles);
/* MFMA passes per product of the image-operand GEMM family: 3 (default) = lo hi' + hi lo' + hi hi', the arithmetic every accuracy
 * statement of this header is made for; 1 (OPT-IN) = hi hi' alone: a third of the matrix instructions, half of the LDS-DMA pieces and
 * fragment reads of the K loops, operands of 11 bits relative to their row block's largest element
 * (|C - C_exact| <= (2^-10 + 2^-22) (|A| |B|^T) + fp32 accumulation), fp32 accumulation, the same images, exponents and epilogues.
 * Read by dtc_linear_fwd_h2i, dtc_linear_fwd_chain_h2i, dtc_linear_dgrad_chain_h2i, dtc_linear_fwd_mse_h2i, dtc_linear_dgrad_h2i and
 * dtc_wgrad_group_h2i at each call and by no other entry point.  Any other value is refused (dtc_last_error) and changes nothing.
 * One pass has no form for a loss target of 2 GiB or more: dtc_linear_fwd_mse_h2i fails there instead of running three passes. */
void dtc_set_h2i_passes(int passes);
int dtc_get_h2i_passes(void);
void dtc_h2i_trace(void* buf);   /* debug: per-workgroup {start, K loop done, end (100 MHz ticks), HW_ID} records of the launches that follow (NULL: off) */
int dtc_h2i_pack(const DtcSegMat* X, int M, void* img, void* stream);
int dtc_h2i_unpack(const void* img, int M, int K, float* out, int64_t ld, void* stream);
/* A weight image.  Rows: up to 2 ranges (r0, nr) of the operand's rows, one after the other, each padded to whole 128-row tiles (all but the
 * last must be multiples of 128 long).  Reduction: up to 4 column ranges (c0, cw) side by side, each padded to whole 16-column stages --
 * the walk of the row operand's images.  trans = 0: element (row, c) = W[row * ld + c] (forward: rows (0, N), ranges = the column blocks of
 * W that meet the row operand's images, in that order); trans = 1: W[c * ld + row] (data gradient: rows = windows of W's columns, one
 * reduction range (0, N)).  img: dtc_h2i_wimage_bytes(job) bytes: the chunks, then int32 exps[row tile][k block][128] (one exponent per
 * image row and 128-column block of each range, as in an activation image; a row within 2^8 of its 128 x 128 block's largest element
 * takes the block's exponent). */
typedef struct DtcH2iWJob {
    const float* W;
    int64_t ld;
    void* img;
    int32_t trans, nrows, nseg;
    int32_t r0[2], nr[2];
    int32_t c0[4], cw[4];
} DtcH2iWJob;
int64_t dtc_h2i_wimage_bytes(const DtcH2iWJob* job);
int dtc_h2i_wimage_group(const DtcH2iWJob* jobs, int count, void* stream);
/* the row operand of a product: up to 4 images over the same M rows, side by side along the reduction (at most 2048 columns in all) */
typedef struct DtcH2iOperand {
    int32_t nseg;
    int32_t width[4];
    const void* img[4];
} DtcH2iOperand;
/* Y = act(X W^T + b) (actor_critic_decoder.py:98-131, 323-349); results: fp32 Y [M, >= N] (may be NULL) and / or Yimg = image(M, N) */
int dtc_linear_fwd_h2i(const DtcH2iOperand* X, const void* wimg, const float* b, float* Y, int64_t ldy, void* Yimg, uint16_t* relu_mask,
                       int M, int N, int act, void* stream);
/* Chains of narrow layers in ONE launch (csrc/gemm_h2i.hip: chain_h2i_kernel): up to three layers of at most 512 result columns each (round 6; a layer wider than
 * 128 columns = several column tiles, run one after the other by the row tile's workgroup: the actor's / critic's tails 512 -> 256 -> 128,
 * actor_critic_decoder.py:323-349, forward and backward),
 * layer i + 1 reading the image layer i wrote (the workgroup that owns a row tile runs the layers one after the other on it).  Same
 * arguments, same results bit for bit as the per-layer calls: the CE-net encoder 265 -> 128 -> 64 -> 35 / decoder 531 -> 64 -> 128 -> 53
 * (actor_critic_decoder.py:98-142) forward, and the data-gradient chains back through them. */
typedef struct DtcH2iFwdLayer {
    DtcH2iOperand X;             /* layer 0: up to 4 images; layers > 0: exactly the previous layer's Yimg                    */
    const void* wimg;
    const float* b;
    float* Y;                    /* fp32 result (may be NULL)                                                                   */
    int64_t ldy;
    void* Yimg;                  /* image result (NULL only for the last layer)                                                 */
    uint16_t* relu_mask;
    int32_t N, act;
} DtcH2iFwdLayer;
int dtc_linear_fwd_chain_h2i(const DtcH2iFwdLayer* layers, int count, int M, void* stream);
typedef struct DtcH2iDgradLayer {
    const void* dZimg;           /* layer 0: image(M, N); layers > 0: the previous layer's dXimg                                */
    const void* wimgT;
    const DtcSegMat* dX;         /* fp32 destination blocks (may be NULL)                                                       */
    void* dXimg;                 /* image result (NULL only for the last layer)                                                 */
    const float* add;
    int64_t ld_add;
    const float* Xsaved;
    int64_t ldxs;
    const uint16_t* relu_mask;
    int32_t N, Kwin, img_cols, act;
} DtcH2iDgradLayer;
int dtc_linear_dgrad_chain_h2i(const DtcH2iDgradLayer* layers, int count, int M, void* stream);
/* the terrain decoder's output layer fused with its MSE (ppo.py:223): dL/dY as fp32 (may be NULL) and / or image(M, N) */
int64_t dtc_linear_fwd_mse_h2i_parts(int M, int N);
int dtc_linear_fwd_mse_h2i(const DtcH2iOperand* X, const void* wimg, const float* b, const float* target, int64_t ldt, int64_t target_rows,
                           int tcol0, const int64_t* tidx, float scale, float* dY, int64_t lddy, void* dYimg, double* sq_part, int M, int N,
                           void* stream);
/* dX[:, window] = ((dZ W[:, window]) + add) * act'(.): dZimg = image(M, N), wimgT = image of W^T for the window (Kwin columns: the job's
 * row ranges one after the other); results over the window: fp32 destination blocks dX (may be NULL) and / or dXimg = image(M, img_cols)
 * of the window's first img_cols columns (0: all Kwin); add: fp32 [M, ld_add] or NULL */
int dtc_linear_dgrad_h2i(const void* dZimg, int N, const void* wimgT, int Kwin, const DtcSegMat* dX, void* dXimg, int img_cols,
                         const float* add, int64_t ld_add, const float* Xsaved, int64_t ldxs, const uint16_t* relu_mask, int M, int act,
                         void* stream);
/* dW_j = dZ_j^T X_j, db_j = colsum(dZ_j) for `count` <= 12 layers in ONE launch, both operands images over the same M batch rows
 * (M a multiple of 128 per batch slice: the per-row exponents of the two operands are folded into one operand's fragments per batch
 * row, csrc/wgrad_h2i.hip).  workspace >= dtc_wgrad_group_h2i_workspace() bytes, 16-byte aligned. */
typedef struct DtcWgradH2iJob {
    const void* dZimg;   /* image(M, N) */
    const void* Ximg;    /* image(M, K) */
    float* dW;           /* [N, ldw >= K]: columns [wcol0, wcol0 + K) of the layer's weight gradient */
    float* db;           /* [N] or NULL   */
    int64_t ldw;
    int32_t N, K, wcol0;
} DtcWgradH2iJob;
int64_t dtc_wgrad_group_h2i_workspace(const DtcWgradH2iJob* jobs, int count, int M);
int dtc_wgrad_group_h2i(const DtcWgradH2iJob* jobs, int count, int M, void* workspace, void* stream);
/* ---- two-term fp16 path (round 4, csrc/s3_core.hpp): the same products with every fp32 operand x scaled by a power of two chosen from
 * its tensor's amax (largest |x|: scaled into [2^14, 2^15)) and written as hi + lo, hi = fp16(x 2^e), lo = fp16(x 2^e - hi): 22 significant
 * bits (elements more than 2^18 below amax: absolute error 2^-40 amax), THREE fp16 MFMA passes per product (lo hi', hi lo', hi hi'; exact
 * in the fp32 accumulator) instead of six bf16 ones, the sums scaled back exactly.  Error level of the fp32 MFMA chain
 * (tests/test_hip_split.py); half the matrix-pipe work and energy of the bf16 x 3 path.  An operand brings its amax in a device
 * SLOT -- a record of dtc_amax_record_bytes() bytes (16 words on 16 cache lines: the waves of a producer spread their atomic maxima over
 * them, readers take the largest; each word the BIT PATTERN of a float; unsigned order = float order, NaN above everything) --:
 * DtcSeg.amax for segmented operands, dz_amax for dZ; NULL = the operand has none and the call computes it (one memset + one launch in
 * front of the GEMM for all such operands of the call).  A producer adds its result to a slot: ZERO it before the first kernel that writes the tensor (a stale
 * larger value is harmless up to ~2^10; a smaller one overflows fp16 and the result turns NaN -- never silently wrong).  Weight
 * images: same jobs and buffers as the bf16 ones, built by dtc_h2_wimage_group or by the call (wimage_ready = 0); the weight's own
 * amax lives inside the image buffer. */
int64_t dtc_amax_record_bytes(void);                                        /* size of one slot (see below)                   */
int dtc_amax(const DtcSegMat* X, int M, uint32_t* slot, void* stream);      /* slot = amax over rows < M of all segments of X */
int dtc_h2_wimage_group(const DtcWimgJob* jobs, int count, void* stream);
int dtc_linear_fwd_h2(const DtcSegMat* X, const float* W, const float* b, float* Y, int64_t ldy, uint16_t* relu_mask,
                      void* wplanes, int wimage_ready, uint32_t* y_amax, int M, int N, int K, int act, void* stream);
int dtc_linear_dgrad_h2(const float* dZ, int64_t lddz, const uint32_t* dz_amax, const float* W, const DtcSegMat* dX, const float* Xsaved,
                        int64_t ldxs, const uint16_t* relu_mask, void* wplanes, int wimage_ready, int M, int N, int K, int act,
                        void* stream);
int dtc_linear_fwd_mse_h2(const DtcSegMat* X, const float* W, const float* b, const float* target, int64_t ldt,
                          int64_t target_rows, int tcol0, const int64_t* tidx, float scale, float* dY, int64_t lddy,
                          double* sq_part, void* wplanes, int wimage_ready, uint32_t* dy_amax, int M, int N, int K, void* stream);
/* dtc_wgrad_group_s3 on the fp16 path: every job brings dz_amax and X.seg[i].amax (same workspace size) */
int dtc_wgrad_group_h2(const struct DtcWgradJob* jobs, int count, int M, void* workspace, void* stream);
int64_t dtc_linear_fwd_mse_s3_parts(int M, int N);
int dtc_linear_fwd_mse_s3(const DtcSegMat* X, const float* W, const float* b, const float* target, int64_t ldt,
                          int64_t target_rows, int tcol0, const int64_t* tidx, float scale, float* dY, int64_t lddy,
                          double* sq_part, void* wplanes, int wimage_ready, int M, int N, int K, void* stream);
/* GRU recurrence on the split-precision path (csrc/gru_s3.hip; H a multiple of 128): the per-time-step products with W_hh as an
 * LDS image built once per pass (dtc_gru_s3_image: backward = 0 for the forward steps, 1 for the data-gradient chunks), row
 * operands loaded two stages ahead -- kernels for the ~1500-row, one-workgroup-per-CU launches of one time step.  dtc_gru_fwd /
 * dtc_gru_bwd use them for T >= 4 when dtc_get_gemm_split() is on (DTC_GRU_S3=0: single-pass kernels). */
int64_t dtc_gru_s3_image_bytes(int H);
int dtc_gru_s3_image(const float* W_hh, void* img, int H, int backward, void* stream);
int dtc_gru_step_fwd_s3(const float* hprev, const void* img, const float* b_hh, const float* gi_t, float* hout, float* gates_t,
                        float* hn_t, int R, int H, void* stream);
/* chunk c of dgh_t [R, 3H] W_hh [3H, H] -> part + c * part_stride ([R, H]); (3H / nparts) a multiple of 32 */
int dtc_gru_dgrad_parts_s3(const float* dgh_t, const void* img, float* part, int64_t part_stride, int R, int H, int nparts,
                           void* stream);
/* dtc_wgrad_group on the split-precision path (same jobs, same outputs; its own workspace size). */
int64_t dtc_wgrad_group_s3_workspace(const struct DtcWgradJob* jobs, int count, int M);
int dtc_wgrad_group_s3(const struct DtcWgradJob* jobs, int count, int M, void* workspace, void* stream);
/* A chain of forward layers in ONE call (same kernels, same results as `count` dtc_linear_fwd calls issued in order on
 * `stream`): the rollout side of PPO.act / evaluate (ppo.py:137-155) is launch-bound -- ~16 small layers per env step at
 * M = num_envs rows -- and the host cost of marshalling each layer through the FFI is paid once per chain instead of
 * once per layer.  The caller may keep the array and patch input pointers between steps. */
typedef struct DtcFwdLayer {
    DtcSegMat X;         /* [M, K] segmented input                                              */
    const float* W;      /* [N, K]                                                               */
    const float* b;      /* [N] or NULL                                                          */
    float* Y;            /* [M, >= N]                                                            */
    int64_t ldy;
    int32_t N, K, act;
} DtcFwdLayer;
int dtc_linear_fwd_list(const DtcFwdLayer* layers, int count, int M, void* stream);

/* dX[M,K] = (dZ[M,N] W[N,K]) * act'(Xsaved), written through the segmented destination dX
 * (segments with ptr == NULL are skipped).  Xsaved (post-activation output of the previous
 * layer, leading dimension ldxs) may be NULL when act == DTC_ACT_NONE. */
int dtc_linear_dgrad(const float* dZ, int64_t lddz, const float* W, const DtcSegMat* dX,
                     const float* Xsaved, int64_t ldxs, int M, int N, int K, int act, void* stream);
/* Data gradient with the reduction index split into `nsplit` equal chunks that run side by side in ONE launch
 * (for GEMMs with few rows, e.g. one GRU time step: M ~ 1500, N = 3H): chunk g computes
 * dX + g*split_stride [M,K] (row stride lddx) = dZ[:, g*N/nsplit : (g+1)*N/nsplit] W[g*N/nsplit : (g+1)*N/nsplit, :];
 * no activation, no accumulation -- the caller adds the chunks in a fixed order (deterministic). */
int dtc_linear_dgrad_split(const float* dZ, int64_t lddz, const float* W, float* dX, int64_t lddx, int64_t split_stride,
                           int M, int N, int K, int nsplit, void* stream);

/* Host hint: non-zero while the caller launches weight gradients on a second stream next to the stream of the data
 * gradients (the overlapped schedule of PPO.update).  The data-gradient kernel then leaves one of its six workgroup slots
 * per CU to them.  Process-wide, not thread-safe against concurrent launches; results never depend on it. */
void dtc_set_concurrency_hint(int side_stream_active);

/* dW[N,K] = dZ^T X, db[N] = column sums of dZ.  workspace: >= dtc_linear_wgrad_workspace() bytes. */
int64_t dtc_linear_wgrad_workspace(int M, int N, int K);
int dtc_linear_wgrad(const float* dZ, int64_t lddz, const DtcSegMat* X, float* dW, float* db,
                     void* workspace, int M, int N, int K, void* stream);

/* The weight gradients of ALL layers of one gradient bucket (ppo.py:252 / 333: the parameters one `loss.backward()`
 * reaches; the decoders or the encoders of the VAE step, the actor + critic bodies or the encoders of the PPO step)
 * in ONE partial-product launch + ONE reduce launch.  Every job shares the row count M (the mini-batch) and runs
 * exactly as dtc_linear_wgrad would (same segmented / gathered X, same outputs); count <= 12.
 * workspace >= dtc_wgrad_group_workspace() bytes, 16-byte aligned, private to the call until it has completed. */
typedef struct DtcWgradJob {
    const float* dZ;     /* [M, N], row stride lddz                                              */
    int64_t lddz;
    DtcSegMat X;         /* [M, K] segmented input of the layer                                  */
    float* dW;           /* [N, K]                                                               */
    float* db;           /* [N] or NULL                                                          */
    int32_t N, K;
    int64_t dz_rows;     /* 0: row m of the product is dZ[m].  > 0 (split path only): dZ has dz_rows rows and row m of the
                          * product is dZ[X.idx[m]] -- the SAME row map as X's gathered segments (the recurrent trainers' valid
                          * rows of the padded trajectory layout: the padding rows carry zero gradient and are skipped)      */
    const uint32_t* dz_amax;   /* dtc_wgrad_group_h2 only: amax slot of dZ (see DtcSeg.amax)                                   */
} DtcWgradJob;
int64_t dtc_wgrad_group_workspace(const DtcWgradJob* jobs, int count, int M);
/* dtc_linear_wgrad over the rows idx[0 .. M) of BOTH operands (dZ [dz_rows, N] and the single-segment X [x_rows, K] share the row
 * map; split-precision path only: returns DTC_ERR_ARG when it is switched off -- the caller then runs the padded product). */
int dtc_linear_wgrad_rows(const float* dZ, int64_t lddz, int64_t dz_rows, const float* X, int64_t ldx, int64_t x_rows,
                          const int64_t* idx, float* dW, float* db, void* workspace, int M, int N, int K, void* stream);
int dtc_wgrad_group(const DtcWgradJob* jobs, int count, int M, void* workspace, void* stream);

/* ---- CE-net latent: actor_critic_decoder.py:274-302 ---------------------------------------- */
/* mulv [B,35] = [latent_mu(19) | latent_var(16)].  In place: outlier -> lower median of the
 * non-outliers (2-sigma rule on the batch statistics), then z = eps*exp(0.5*lv) + mu[:,3:].
 * mask [B,16] uint8 receives the outlier mask, info (int32[4]) {n_outliers, median_flat_index,
 * median bits, 0}.  workspace >= dtc_cenet_workspace() bytes. */
int64_t dtc_cenet_workspace(int B);
int dtc_cenet_latent_fwd(float* mulv, const float* eps, float* z, uint8_t* mask, int32_t* info,
                         void* workspace, int B, uint32_t* z_amax /* amax record of z (two-term fp16 GEMM path, DtcSeg.amax) or NULL */,
                         void* stream);
/* ... and zmu_img (may be NULL): the operand image (dtc_h2i_bytes(B, 19)) of [z | mu[:, :3]] -- the narrow input block of the CE-net
 * decoder's and the actor's first layer (actor_critic_decoder.py:431, 300) -- written by the same launch instead of a pack launch. */
int dtc_cenet_latent_fwd_img(float* mulv, const float* eps, float* z, uint8_t* mask, int32_t* info, void* workspace, int B,
                             uint32_t* z_amax, void* zmu_img, void* stream);
/* backward of the above: dmulv [B,35] holds the direct gradients w.r.t. (mu, lv_fixed) on entry
 * and the gradients w.r.t. the raw head outputs on exit. */
int dtc_cenet_latent_bwd(float* dmulv, const float* dz, const float* eps, const float* mulv,
                         const uint8_t* mask, const int32_t* info, void* workspace, int B,
                         uint32_t* dmulv_amax /* amax record of the whole [B,35] gradient on exit, or NULL */, void* stream);

/* ---- losses (fused forward + gradient) ------------------------------------------------------ */
/* VAE losses of ppo.py:205-247.  Gathered operands are read as src[idx[b]].  Outputs:
 * d_recons [B,53], d_hrecon [B,693], dmulv [B,35] (vel + 4*kld parts) and
 * losses[0..3] = {recons, vel, kld, height} (float, device). */
int dtc_vae_loss(const float* recons, const float* hrecon, const float* mulv, const float* next_obs,
                 const float* priv, const float* base_vel, const int64_t* idx, float* d_recons,
                 float* d_hrecon, float* dmulv, float* losses, void* workspace, int B,
                 uint32_t* drec_amax /* amax record of d_recons or NULL */, void* stream);

/* The terrain-decoder output layer fused with its loss (ppo.py:216-218: height_recon = terrain_decoder(l_t),
 * height_loss = mse(height_recon, priv[..., 696:])): e = (X W^T + b) - target[tidx[m], tcol0 + n]; writes
 * dY[m,n] = e * scale (scale = 2/(M*N): dL/d height_recon) and one double per workgroup, sum(e^2), into sq_part
 * (dtc_linear_fwd_mse_parts(M, N) slots).  height_recon itself never reaches HBM.  dtc_vae_loss_fused is dtc_vae_loss
 * without the height term; it adds the partials (in index order) into losses[3]. */
int64_t dtc_linear_fwd_mse_parts(int M, int N);
int dtc_linear_fwd_mse(const DtcSegMat* X, const float* W, const float* b, const float* target /*[target_rows, ldt]*/,
                       int64_t ldt, int64_t target_rows, int tcol0, const int64_t* tidx /*[M]*/, float scale, float* dY,
                       int64_t lddy, double* sq_part, int M, int N, int K, void* stream);
int dtc_vae_loss_fused(const float* recons, const float* mulv, const float* next_obs, const float* base_vel,
                       const int64_t* idx, float* d_recons, float* dmulv, const double* height_sq_part, int n_height_part,
                       float* losses, void* workspace, int B, uint32_t* drec_amax /* as dtc_vae_loss */, void* stream);
/* ... and drec_img (may be NULL): the operand image (dtc_h2i_bytes(B, 53)) of d_recons, written by the same launch. */
int dtc_vae_loss_fused_img(const float* recons, const float* mulv, const float* next_obs, const float* base_vel,
                           const int64_t* idx, float* d_recons, float* dmulv, const double* height_sq_part, int n_height_part,
                           float* losses, void* workspace, int B, uint32_t* drec_amax, void* drec_img, void* stream);
int64_t dtc_loss_workspace(int B);

typedef struct DtcPpoCfg {
    float clip_param, value_loss_coef, entropy_coef, desired_kl;
    int32_t use_clipped_value_loss, adaptive_schedule;
    float* kl_mirror;      /* NULL, or a device address that ALSO receives kl_mean from the finalize launch (data parallel: slot 0 of the
                              gradient header the first bucket's all-reduce carries -- no copy of its own between the loss and the backward pass) */
} DtcPpoCfg;
/* PPO losses + KL-adaptive learning rate of ppo.py:288-327.  mean [B,12], std [12], value [B].
 * Outputs: dmean [B,12], dvalue [B], dstd [12], losses[0..3] = {surrogate, value, entropy, kl_mean},
 * lr (double, device; read-modify-write exactly as ppo.py:301-307). */
int dtc_ppo_loss(const float* mean, const float* std, const float* value, const float* actions,
                 const float* old_logp, const float* old_mu, const float* old_sigma, const float* advantages,
                 const float* returns, const float* old_values, const int64_t* idx, const DtcPpoCfg* cfg,
                 float* dmean, float* dvalue, float* dstd, float* losses, double* lr, void* workspace,
                 int B, int num_actions, void* stream);
/* The actor's and the critic's output layers (mean = Ha Wa^T + ba, value = Hc Wc^T + bc over the last hidden activations
 * Ha, Hc [B,H], H in {64, 128, 256}), dtc_ppo_loss on them, and the data gradients of the two layers
 * (dHa = (dmean Wa) * act'(Ha), dHc = (dvalue Wc) * act'(Hc), act' through the saved post-activation values as in
 * dtc_linear_dgrad) in ONE launch + the finalize launch: replaces two dtc_linear_fwd, dtc_ppo_loss and two
 * dtc_linear_dgrad calls on the critical path of every policy step (ppo.py:288-327 with actor_critic_decoder.py:
 * 330-345).  Also writes mean [B,A], value [B], dmean, dvalue (the weight gradients of the two layers need them). */
int dtc_ppo_heads_loss(const float* Ha, int64_t ldha, const float* Hc, int64_t ldhc, int H, const float* Wa /*[A,H]*/,
                       const float* ba, const float* Wc /*[1,H]*/, const float* bc, int act_prev, const float* std,
                       const float* actions, const float* old_logp, const float* old_mu, const float* old_sigma,
                       const float* advantages, const float* returns, const float* old_values, const int64_t* idx,
                       const DtcPpoCfg* cfg, float* mean, float* value, float* dmean, float* dvalue, float* dHa,
                       int64_t lddha, float* dHc, int64_t lddhc, float* dstd, float* losses, double* lr, void* workspace,
                       int B, int num_actions, uint32_t* dha_amax, uint32_t* dhc_amax, uint32_t* dmean_amax,
                       uint32_t* dval_amax /* amax records of dHa / dHc / dmean / dvalue (two-term fp16 GEMM path, see DtcSeg.amax), each
                       may be NULL */, void* stream);
/* ... and the operand images (dtc_h2i_bytes(B, H), (B, H), (B, A), (B, 1); each may be NULL; the first two need H <= 128) of dHa, dHc, dmean,
 * dvalue, written by the same launch: the trainer's image-operand data / weight gradients read them without a pack launch.  Where an
 * image of dHa / dHc is given, its fp32 destination may be NULL (the image is then the only copy: 25 MB less to write per call). */
int dtc_ppo_heads_loss_img(const float* Ha, int64_t ldha, const float* Hc, int64_t ldhc, int H, const float* Wa, const float* ba,
                           const float* Wc, const float* bc, int act_prev, const float* std, const float* actions,
                           const float* old_logp, const float* old_mu, const float* old_sigma, const float* advantages,
                           const float* returns, const float* old_values, const int64_t* idx, const DtcPpoCfg* cfg, float* mean,
                           float* value, float* dmean, float* dvalue, float* dHa, int64_t lddha, float* dHc, int64_t lddhc,
                           float* dstd, float* losses, double* lr, void* workspace, int B, int num_actions, uint32_t* dha_amax,
                           uint32_t* dhc_amax, uint32_t* dmean_amax, uint32_t* dval_amax, void* dHa_img, void* dHc_img,
                           void* dmean_img, void* dval_img, void* stream);
/* The learning-rate rule of ppo.py:301-307 alone (data-parallel callers run dtc_ppo_loss with
 * adaptive_schedule = 0, all-reduce the KL mean, then call this so every rank takes the same branch).
 * The slot is CONSUMED: it is overwritten with a NaN of a payload of its own (0x7fc0dead), and finding exactly that pattern (a caller that
 * exchanged the gradient header without depositing this step's KL first) poisons *lr with NaN instead of silently re-using a stale value.
 * A KL that is NaN itself (any other payload) leaves *lr unchanged, as both comparisons of the reference do. */
int dtc_lr_adapt(float* kl_mean, double* lr, float desired_kl, float* kl_out /* NULL, or where the (averaged) KL is kept: the step's statistics row */, void* stream);
/* log-prob / sampling side of PPO.act (ppo.py:137-150): actions = mean + std*noise,
 * logp = sum_j log N(a; mean, std). */
int dtc_gaussian_act(const float* mean, const float* std, const float* noise, float* actions,
                     float* logp, float* mu_out, float* sigma_out, int B, int num_actions, void* stream);

/* ActorCriticDecoder.adapt_bootstrap_probability (actor_critic_decoder.py:404-407): out[0] = 1 - tanh(std(rewards) / mean(rewards)),
 * unbiased std as torch.std; rewards: n contiguous floats on the device, out: one device float. */
int dtc_bootstrap_probability(const float* rewards, int64_t n, float* out, void* stream);

/* ---- clip_grad_norm_ + Adam over one flat parameter range (ppo.py:253-254, 334-335) --------- */
/* gnorm_out (float, device) receives the pre-clip global L2 norm.  lr is a device double;
 * step is the 1-based Adam step count of this range. */
int dtc_clip_adam(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float max_grad_norm, const double* lr, double beta1, double beta2, double eps, int64_t step,
                  float* gnorm_out, void* workspace, void* stream);
int64_t dtc_adam_workspace(int64_t n);

/* ---- device random draws of PPO.update (counter-based: deterministic in (seed, offset / n), no host synchronisation) ----
 * dtc_randn: n standard-normal floats (Philox4x32-10 + Box-Muller; element 4g..4g+3 from counter g + offset) -- the
 * `torch.randn_like` of the CE-net reparameterisation (actor_critic_decoder.py:283).
 * dtc_randperm: a pseudo-random permutation of [0, n) as int64 (keyed Feistel bijection of [0, 2^k) with cycle walking; no
 * sort) -- the `torch.randperm` of the mini-batch generator (rollout_storage.py:165). */
int dtc_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
int dtc_randperm(int64_t* out, int64_t n, uint64_t seed, void* stream);

/* ---- GRU (torch.nn.GRU, 1 layer, gate order r,z,n; actor_critic_recurrent.py:92-116 `Memory`) ---- */
/* One fused GRU time step (forward), the building block of dtc_gru_fwd: the recurrent GEMM
 * gh = hprev W_hh^T + b_hh and the gate math of torch.nn.GRU in its epilogue (gh never reaches HBM):
 * hout [R,H], gates_t [R,3H] = (r | z | n), hn_t [R,H] = gh_n; gi_t [R,3H] = x_t W_ih^T + b_ih.  H % 32 == 0. */
int dtc_gru_step_fwd(const float* hprev /*[R,H]*/, const float* W_hh /*[3H,H]*/, const float* b_hh, const float* gi_t,
                     float* hout, float* gates_t, float* hn_t, int R, int H, void* stream);

/* gi [T,R,3H] = x W_ih^T + b_ih is computed by dtc_linear_fwd over all T*R rows; this runs the recurrence
 *     r = sig(gi_r + gh_r), z = sig(gi_z + gh_z), n = tanh(gi_n + r*gh_n), h_t = (1-z)*n + z*h_{t-1},
 *     gh = h_{t-1} W_hh^T + b_hh
 * for t < T over R sequences (R = padded trajectories of utils.py:33-64, or envs during the rollout).
 * hs_all is [T+1,R,H]: slot 0 receives h0, slot t+1 = h_t (so hs_all[1:] is nn.GRU's output and hs_all[:T]
 * the h_{t-1} operand of the backward pass).  gates [T,R,3H] receives (r, z, n), hn [T,R,H] = gh_n.
 * workspace >= dtc_gru_workspace() bytes. */
int64_t dtc_gru_workspace(int T, int R, int H);
int dtc_gru_fwd(const float* gi, const float* h0, const float* W_hh, const float* b_hh, float* hs_all,
                float* gates, float* hn, void* workspace, int T, int R, int H, void* stream);
/* BPTT.  dhs [T,R,H] = gradient w.r.t. the outputs h_1..h_T.  Produces dgi [T,R,3H] (gradient w.r.t. gi:
 * feed it to dtc_linear_wgrad with x for W_ih / b_ih), dW_hh [3H,H], db_hh [3H] and dh0 [R,H].
 * valid_rows (optional, n_valid entries of t * R + r): the (t, r) slots that belong to a trajectory -- the padding slots of the
 * padded layout carry zero gradient, and on the split-precision path the W_hh weight gradient then skips them.
 * dW_hh == db_hh == NULL: the W_hh weight gradient is left to the caller, who finds dgh_all [T,R,3H] (gradient w.r.t. the recurrent
 * pre-activations gh_t) at workspace + dtc_gru_dgh_offset(T, R, H) once the call has run -- dW_hh = dgh_all^T hs_all[:T], db_hh =
 * colsum(dgh_all); the operand-image trainers pack both into images and add the product to their grouped weight-gradient launch. */
int64_t dtc_gru_dgh_offset(int T, int R, int H);
int dtc_gru_bwd(const float* dhs, const float* hs_all, const float* gates, const float* hn, const float* W_hh,
                float* dgi, float* dW_hh, float* db_hh, float* dh0, void* workspace, const int64_t* valid_rows, int n_valid,
                int T, int R, int H, void* stream);

/* The recurrence as ONE persistent launch over all T time steps (csrc/gru_seq.hip; H = 512, R <= 2048, T >= 2): a workgroup owns a row
 * block x 16 hidden units, keeps its slice of W_hh in LDS as two-term fp16 for all steps and meets the other workgroups of its row block at
 * a counter barrier once per step.  OPT-IN (DTC_GRU_SEQ=1 or dtc_set_gru_seq(1); -1 = back to the environment's choice): dtc_gru_fwd / dtc_gru_fwd_multi then use it
 * on the split-precision path whenever dtc_gru_seq_supported(); results within fp32 rounding of the per-step kernels (another, equally
 * accurate, split of the operands).  Default: the per-step launches (measured no slower in the trainers).  A launch whose workgroups cannot meet (more than two such launches sharing the device) gives up after 2 s and raises the
 * flag dtc_gru_seq_status() returns (1; it synchronises with the device; reset != 0 clears it) -- its outputs are then incomplete.
 * seq_ws: dtc_gru_seq_workspace(R, H) bytes, 16-byte aligned (dtc_gru_workspace() includes them). */
void dtc_set_gru_seq(int on);
int dtc_get_gru_seq(void);
void dtc_gru_seq_trace(void* buf);   /* debugging: (workgroups x T x 4) 8-byte time stamps (100 MHz) per step of thread 0: met / K loop done / gates done / arrived */
int dtc_gru_seq_supported(int T, int R, int H, int exclusive /* 0: a launch that leaves half the CUs to a second one (dtc_gru_fwd); 1: dtc_gru_fwd_multi's */);
int dtc_gru_seq_status(int reset);
int64_t dtc_gru_seq_workspace(int R, int H);
int dtc_gru_seq_fwd(const float* gi, const float* h0, const float* W_hh, const float* b_hh, float* hs_all, float* gates, float* hn,
                    void* seq_ws, int T, int R, int H, void* stream);
int dtc_gru_seq_fwd_pair(const float* const* gi, const float* const* h0, const float* const* W_hh, const float* const* b_hh,
                         float* const* hs_all, float* const* gates, float* const* hn, void* const* seq_ws, int T, int R, int H, void* stream);

/* The recurrence on block-scaled two-term fp16 operand images (csrc/gru_h2i.hip; H a multiple of 128, at most 2048; any R, T >= 1): the
 * GRU of `Memory` (actor_critic_recurrent.py:92-116) over the padded trajectories of utils/utils.py:33-70, every per-step product from two
 * images by LDS-DMA (three fp16 MFMA passes, nothing converted in a K loop), and the results the rest of the policy step consumes written
 * as image rows by the kernels that produce them.  OPT-IN: DTC_GRU_H2I=1 or dtc_set_gru_h2i(1) (0 = off, -1 = back to the environment's
 * choice, default off); the switch is read by the recurrent trainers (dtc_amd/algorithms/recurrent_heads.py), dtc_gru_fwd / dtc_gru_bwd
 * never take this path by themselves. */
void dtc_set_gru_h2i(int on);
int dtc_get_gru_h2i(void);
/* Workspace of dtc_gru_fwd_h2i / dtc_gru_bwd_h2i (actor_critic_recurrent.py:92-116, utils/utils.py:33-70), 256-byte aligned; its own
 * size -- dtc_gru_workspace() does not include it.  dgh_all [T,R,3H] (fp32, the gradient w.r.t. the recurrent pre-activations) sits at
 * workspace + dtc_gru_h2i_dgh_offset() once the backward call has run, as dtc_gru_dgh_offset() for dtc_gru_bwd. */
int64_t dtc_gru_h2i_workspace(int T, int R, int H);
int64_t dtc_gru_h2i_dgh_offset(int T, int R, int H);
/* Forward pass of the GRU (actor_critic_recurrent.py:92-116) over padded trajectories (utils/utils.py:33-70), operands and outputs as
 * dtc_gru_fwd.  Row r of h_t carries ONE exponent for the whole call, e_r = min(14, 14 - floor(log2 max|finite h0[r, :]|)): |h_t| <=
 * max(1, max|h0 row|) for a GRU, so nothing overflows fp16 and no block maximum is needed.  slot_row (int32 [T * R], may be NULL): the
 * valid row of padded slot (t, r), or -1 -- the inverse of the trainers' unpad_idx.  With it, h_t is also written as row slot_row[t, r]
 * of hx_img = image(M_valid, H) of hs_all[1:] un-padded, and h_{t-1} (h0 at t = 0) as row slot_row[t, r] of hp_img = image(M_valid, H) of
 * hs_all[:T] un-padded; either image may be NULL.  Rows no slot names keep what the caller put there (HImage: "nothing here"). */
int dtc_gru_fwd_h2i(const float* gi, const float* h0, const float* W_hh, const float* b_hh, float* hs_all, float* gates, float* hn,
                    void* workspace, const int32_t* slot_row, int M_valid, void* hx_img, void* hp_img, int T, int R, int H, void* stream);
/* BPTT of the same recurrence (actor_critic_recurrent.py:92-116 under the padded layout of utils/utils.py:33-70) without the W_hh weight
 * gradient: dgi [T,R,3H], dh0 [R,H] and dgh_all in the workspace as dtc_gru_bwd with dW_hh == NULL; same gate arithmetic and summation
 * order.  With slot_row, the rows of the head's weight-gradient operands are written as images too, true exponents per row and block of 128
 * columns, each pointer may be NULL: drz_img = image(M_valid, 2H) of dgh[:, :2H] (= dgi[:, :2H]), dnh_img / dni_img = image(M_valid, H) of
 * dgh[:, 2H:] / dgi[:, 2H:], dgh_img / dgi_img = image(M_valid, 3H) of dgh / dgi. */
int dtc_gru_bwd_h2i(const float* dhs, const float* hs_all, const float* gates, const float* hn, const float* W_hh, float* dgi, float* dh0,
                    void* workspace, const int32_t* slot_row, int M_valid, void* drz_img, void* dnh_img, void* dni_img, void* dgh_img,
                    void* dgi_img, int T, int R, int H, void* stream);
/* The single steps of the two calls above (actor_critic_recurrent.py:92-116, utils/utils.py:33-70), as dtc_gru_s3_image /
 * dtc_gru_step_fwd_s3 / dtc_gru_dgrad_parts_s3.  dtc_gru_h2i_image: W_hh -> image with one exponent per image row and block of 128
 * reduction columns (backward = 0: tiles of 32 units x (r | z | n); 1: W_hh^T, tiles of 128 columns of dh), dtc_gru_h2i_image_bytes() bytes.
 * dtc_gru_step_fwd_h2i: one time step from hprev_img = image(R, H) of h_{t-1} (any exponents) and hprev (fp32, the z * h_{t-1} term);
 * hout_img / hx_img / hp_img (each may be NULL) receive h_t with the exponent row_exp[r] -- hout_img's exponent table is the caller's.
 * dtc_gru_dgrad_parts_h2i: chunk c of dgh_t W_hh from dgh_img = image(R, 3H) -> part + c * part_stride; (3H / nparts) a multiple of 16. */
int64_t dtc_gru_h2i_image_bytes(int H, int backward);
int dtc_gru_h2i_image(const float* W_hh, void* img, int H, int backward, void* stream);
int dtc_gru_step_fwd_h2i(const void* hprev_img, const float* hprev, const void* wimg, const float* b_hh, const float* gi_t, float* hout,
                         float* gates_t, float* hn_t, void* hout_img, const int32_t* row_exp, const int32_t* slot_x, const int32_t* slot_p,
                         int M_valid, void* hx_img, void* hp_img, int R, int H, void* stream);
int dtc_gru_dgrad_parts_h2i(const void* dgh_img, const void* wimg, float* part, int64_t part_stride, int R, int H, int nparts, void* stream);

/* Several recurrences of ONE shape (T, R, H) advanced together -- the actor's and the critic's `Memory` of ActorCriticRecurrent
 * (actor_critic_recurrent.py:45-46: memory_a, memory_c; both are evaluated on the same mini-batch of padded trajectories,
 * ppo.py:265-272): with count == 2 every time step is ONE launch for both (a time step of one recurrence is a latency-bound launch of
 * ~200-300 workgroups; two of them on two streams overlap by only ~20 %).  Results are bit-identical to dtc_gru_fwd / dtc_gru_bwd on
 * each item.  Settings or shapes without the split-path step kernels, and count == 1: the single calls, one after the other.
 * dtc_gru_bwd_multi never forms the W_hh weight gradients: dgh_all of item i sits at its workspace + dtc_gru_dgh_offset(T, R, H),
 * as after dtc_gru_bwd with dW_hh == NULL.  Each item brings its own workspace (>= dtc_gru_workspace bytes). */
#define DTC_GRU_MULTI_MAX 2
typedef struct DtcGruFwdItem {
    const float* gi;     /* [T,R,3H] */
    const float* h0;     /* [R,H]    */
    const float* W_hh;   /* [3H,H]   */
    const float* b_hh;   /* [3H]     */
    float* hs_all;       /* [T+1,R,H] */
    float* gates;        /* [T,R,3H] */
    float* hn;           /* [T,R,H]  */
    void* workspace;
} DtcGruFwdItem;
typedef struct DtcGruBwdItem {
    const float* dhs;    /* [T,R,H]  */
    const float* hs_all;
    const float* gates;
    const float* hn;
    const float* W_hh;
    float* dgi;          /* [T,R,3H] */
    float* dh0;          /* [R,H]    */
    void* workspace;
} DtcGruBwdItem;
int dtc_gru_fwd_multi(const DtcGruFwdItem* items, int count, int T, int R, int H, void* stream);
int dtc_gru_bwd_multi(const DtcGruBwdItem* items, int count, int T, int R, int H, void* stream);

/* ---- LSTM (torch.nn.LSTM, gate order i,f,g,o; the default `rnn_type` of actor_critic_recurrent.py:93-97) ----
 * gi [T,R,4H] = x W_ih^T + b_ih is computed by dtc_linear_fwd over all T*R rows; this runs
 *     a = gi_t + h_{t-1} W_hh^T + b_hh;  i,f,o = sig(a_i, a_f, a_o), g = tanh(a_g);  c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)
 * hs_all / cs_all are [T+1,R,H]: slot 0 receives h0 / c0, slot t+1 = h_t / c_t (hs_all[1:] is nn.LSTM's output);
 * gates [T,R,4H] receives the activated (i, f, g, o).  workspace >= dtc_lstm_workspace() bytes. */
int64_t dtc_lstm_workspace(int T, int R, int H);
int dtc_lstm_fwd(const float* gi, const float* h0, const float* c0, const float* W_hh /*[4H,H]*/, const float* b_hh,
                 float* hs_all, float* cs_all, float* gates, void* workspace, int T, int R, int H, void* stream);
/* One fused LSTM time step (forward), replacing one time step of torch.nn.LSTM inside `Memory` (actor_critic_recurrent.py:92-116,
 * `rnn_type = 'gru'#lstm` / `rnn_num_layers = 2` of AC_Args, actor_critic_decoder.py:85-88): the recurrent GEMM a = gi_t + hprev
 * W_hh^T + b_hh with the gate math above in its epilogue (a never reaches HBM).  A workgroup's column tile holds all four gate
 * blocks of 32 hidden units (rows j, H+j, 2H+j, 3H+j of W_hh, read in place).  hout / cout [R,H], gates_t [R,4H] = (i | f | g | o),
 * as one time step of dtc_lstm_fwd writes them.  H % 32 == 0; hout / cout must not alias hprev / cprev. */
int dtc_lstm_step_fwd(const float* hprev /*[R,H]*/, const float* cprev /*[R,H]*/, const float* W_hh /*[4H,H]*/, const float* b_hh,
                      const float* gi_t /*[R,4H]*/, float* hout, float* cout, float* gates_t, int R, int H, void* stream);
/* dtc_lstm_fwd with ONE dtc_lstm_step_fwd launch per time step (same arguments and outputs; results within fp32 rounding of
 * dtc_lstm_fwd's: another summation order of the same products).  H % 32 != 0: dtc_lstm_fwd's GEMM + gate-kernel pair. */
int dtc_lstm_fwd_fused(const float* gi, const float* h0, const float* c0, const float* W_hh /*[4H,H]*/, const float* b_hh,
                       float* hs_all, float* cs_all, float* gates, void* workspace, int T, int R, int H, void* stream);
/* BPTT.  dhs [T,R,H] = gradient w.r.t. the outputs h_1..h_T (the final states carry no gradient).  Produces dgi [T,R,4H]
 * (gradient w.r.t. the gate pre-activations: feed it to dtc_linear_wgrad with x for W_ih / b_ih and to dtc_linear_dgrad
 * for the layer below), dW_hh [4H,H], db_hh [4H], dh0 and dc0 [R,H]. */
int dtc_lstm_bwd(const float* dhs, const float* hs_all, const float* cs_all, const float* gates, const float* W_hh,
                 float* dgi, float* dW_hh, float* db_hh, float* dh0, float* dc0, void* workspace, int T, int R, int H,
                 void* stream);

/* ---- per-kernel timing (HIP events on `stream`) used by bench.py's roofline object ---------- */
void dtc_prof_enable(int on);
/* Fills up to `cap` records; returns the number of distinct kernel classes seen. */
/* work = algorithmic work of the launches in the unit of the kernel's roofline (FLOP for the MFMA-bound GEMMs, bytes for
 * HBM-bound kernels); bytes = algorithmic HBM bytes of the GEMM launches (every operand read once, every output
 * written once; 0 where not tracked) -- the denominator of bench.py's traffic ratio. */
typedef struct DtcProfRec { char name[48]; double ms_total; double work; int64_t launches; double bytes; } DtcProfRec;
int dtc_prof_report(DtcProfRec* out, int cap);
void dtc_prof_reset(void);

/* Measurement aid: one launch of the split kernels' bare MFMA stream (24 v_mfma_f32_32x32x16_bf16 per wave and stage, three waves per
 * SIMD, register operands taken from the 64 KiB at `operands`) -- blocks * 4 * iters * 24 * 32768 bf16 FLOP.  bench.py times it on
 * zero and on random operand bits: the rate the chip SUSTAINS (it clocks to its power budget) next to the data-sheet peak. */
int dtc_probe_mfma_stream(const void* operands, int blocks, int iters, float* sink, void* stream);
int dtc_probe_mfma_stream_h2(const void* operands, int blocks, int iters, float* sink, void* stream);   /* 12 fp16 MFMAs per stage (two-term path) */
/* Debugging aid (tools/flake_probe.py, tests): `blocks` workgroups that leave `pattern` in all of their 64 KiB of LDS and in ~240 VGPRs per
 * lane, so that a following kernel's reads of LDS words / registers it never wrote depend on `pattern` (uninitialised-read detector). */
int dtc_probe_poison(uint32_t pattern, int blocks, float* sink, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DTC_HIP_H */
