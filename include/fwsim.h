/*
 * fwsim.h -- C ABI of the MI355X-native vectorised fixed-wing env step.
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json:north_star:
 * N independent fixed-wing aircraft advanced in lockstep for one *agent step*
 * (= 4 Aviary steps = 8 physics ticks @240 Hz, with observation, reward,
 * termination/truncation and SB3-style auto-reset fused in).
 *
 * The reference (WdBlink/pyflyt-drone) has no FFI: its boundary is Python
 * duck typing (Gymnasium Env aggregated by SB3's VecEnv).  Each entry point
 * below names the reference interface it replaces (paths relative to the
 * reference repo root):
 *
 *   fw_create   <- gym.make(...)/FixedwingBaseEnv.__init__ x N inside SubprocVecEnv
 *                  envs/fixedwing_envs/fixedwing_base_env.py:21-106,
 *                  train/train_Fixedwing_Waypoints_v3.py:82-121,251
 *   fw_reset    <- Env.reset(): begin_reset/end_reset
 *                  envs/fixedwing_envs/fixedwing_base_env.py:193-257,
 *                  envs/fixedwing_objlock_env.py:177-251
 *   fw_step     <- Env.step(action) + the VecEnv worker's auto-reset
 *                  envs/fixedwing_envs/fixedwing_base_env.py:314-348
 *   fw_seed     <- VecEnv.seed(seed) / env.reset(seed=seed+rank)
 *                  train/train_Fixedwing_Waypoints_v3.py:119
 *   fw_get_state/fw_set_state <- (no reference twin) parity tests + checkpoints
 *   fw_get_counters <- (no reference twin) diagnostics of the auto-reset hand-off
 *   fw_render   <- Camera.capture_image() as consumed at envs/fixedwing_objlock_env.py:603-622 and replaced by a
 *                  network's mask at envs/fixedwing_envs/objlock_yolo_env.py:646-716
 *   fw_destroy  <- Env.close()  envs/fixedwing_envs/fixedwing_base_env.py:187-191
 *
 * Conventions
 *   - All I/O buffers of fw_reset/fw_step are DEVICE pointers owned by the
 *     caller (e.g. torch tensor .data_ptr()); nothing is retained past the call.
 *   - fw_get_state/fw_set_state take HOST pointers (double, canonical record).
 *   - Calls are asynchronous w.r.t. the host and ordered on `hip_stream`
 *     (a hipStream_t passed as void*; NULL = the legacy default stream).
 *   - A handle is not re-entrant.  Different handles are independent.
 *   - Return value: 0 = FW_OK, <0 = error enum; message via fw_last_error().
 *     Nothing throws across the ABI.
 *   - Element type T of action/obs/reward buffers is fw_config.dtype
 *     (FW_F64: double, the reference's arithmetic; FW_F32: float).
 */
#ifndef FWSIM_H
#define FWSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FW_ABI_VERSION 7

#define FW_NUM_SURFACES 5         /* left aileron, right aileron, h-tail, v-tail, main wing */
#define FW_NUM_ACTUATORS 6        /* 5 surfaces + throttle (aux_state order) */
#define FW_MAX_TARGETS 8
#define FW_MAX_COLLISION_PTS 8
#define FW_MAX_OBSTACLES 20
#define FW_VISION_FEATS 9         /* envs/fixedwing_objlock_env.py:745-761 */
#define FW_VISION_HIST 3          /* duck_vision_history_len default :69 */

/* error codes */
enum {
  FW_OK = 0,
  FW_EINVAL = -1,      /* bad argument / bad config (maps to ValueError) */
  FW_EHIP = -2,        /* HIP runtime error (no device, launch failure ...) */
  FW_ENOMEM = -3,
  FW_EVERSION = -4,    /* abi_version mismatch */
  FW_EUNSUPPORTED = -5
};

/* fw_config.task */
enum {
  FW_TASK_WAYPOINTS = 0,        /* PyFlyt/Fixedwing-Waypoints-v3 (train/train_Fixedwing_Waypoints_v3.py:100-110) */
  FW_TASK_OBJLOCK = 1,          /* envs/fixedwing_objlock_env.py */
  FW_TASK_WAYPOINT_OBJLOCK = 2, /* envs/fixedwing_waypoint_objlock_env.py */
  FW_TASK_LOWLEVEL = 3,         /* envs/fixedwing_envs/fixedwing_lowlevel_env.py: six actuator commands, heading / height / speed tracking */
  /* (4 is not a task: a config that carries it is rejected as "unknown task", as it was before the next id existed) */
  FW_TASK_WAYPOINTS_DIRECT = 5  /* the waypoints task flown in PyFlyt's mode -1: six actuator commands instead of the four mode-0 actions; the
                                 * base env of train/train_highlevel_cmd.py's HighLevelCmdEnv */
};

/* fw_config.lowlevel_variant (FW_TASK_LOWLEVEL only; DESIGN.md section 2d "SAC script's variant").  Both variants share the 21
 * observation columns, the six actions and the FW_SL_* state tail; they differ in start, reward, episode ends and in which
 * action obs[12:18] shows. */
enum {
  FW_LL_VARIANT_TRACKING = 0,   /* envs/fixedwing_envs/fixedwing_lowlevel_env.py (train/train_lowlevel_cmd.py) */
  FW_LL_VARIANT_SAC_DEMO = 1    /* the FixedwingLowLevelEnv examples/lowlevel.py defines for its SAC run */
};

/* fw_config.dtype */
enum { FW_F64 = 0, FW_F32 = 1 };

/* fw_config.wind_mode  (envs/fixedwing_envs/fixedwing_base_env.py:113-115) */
enum { FW_WIND_OFF = 0, FW_WIND_CONSTANT = 1, FW_WIND_GUST_SINE = 2 };

/* fw_config.wind_coupling: how the registered wind vector enters the dynamics.
 * Not in the reference (lives in un-vendored PyFlyt) -> explicit, build-owned. */
enum {
  FW_WIND_COUPLE_NONE = 0,
  FW_WIND_COUPLE_FORCE = 1,     /* world-frame force = wind_force_coef * w(t) on the base */
  FW_WIND_COUPLE_AIRSPEED = 2   /* w(t) subtracted from every surface's air velocity */
};

/* One lifting surface.  First 11 fields are my_models/fixedwing/fixewing.yaml:8-71
 * verbatim (angles in degrees); the geometry (units, link origin) is build-owned
 * because the URDF is not in the reference. */
typedef struct fw_surface_params {
  double Cl_alpha_2D;
  double chord;
  double span;
  double flap_to_chord;
  double eta;
  double alpha_0_base_deg;
  double alpha_stall_P_base_deg;
  double alpha_stall_N_base_deg;
  double Cd_0;
  double deflection_limit_deg;
  double tau;
  double lift_unit[3];     /* body frame */
  double forward_unit[3];  /* body frame */
  double pos[3];           /* link origin relative to the composite COM, body frame [m] */
} fw_surface_params;

/* my_models/fixedwing/fixewing.yaml:1-6 + geometry */
typedef struct fw_motor_params {
  double total_thrust;
  double thrust_coef;
  double torque_coef;
  double noise_ratio;
  double tau;
  double thrust_unit[3];
  double pos[3];
} fw_motor_params;

typedef struct fw_config {
  /* ---- integers ---- */
  int32_t abi_version;          /* must be FW_ABI_VERSION */
  int32_t task;                 /* FW_TASK_* */
  int32_t dtype;                /* FW_F64 | FW_F32 */
  int32_t angle_representation; /* 0 euler (attitude 12), 1 quaternion (13)  fixedwing_base_env.py:65-72 */
  int32_t agent_hz;             /* must divide 120              fixedwing_base_env.py:48-53 */
  int32_t physics_hz;           /* 240 */
  int32_t control_hz;           /* 120  => 2 ticks per Aviary step */
  int32_t warmup_aviary_steps;  /* 10                          fixedwing_base_env.py:254-255 */
  int32_t auto_reset;           /* 1: SB3 VecEnv worker semantics; 0: bare Gymnasium env */
  int32_t sparse_reward;
  int32_t num_targets;          /* <= FW_MAX_TARGETS */
  int32_t context_length;       /* flatten_waypoint_env.py:16 */
  int32_t wind_mode;            /* FW_WIND_* */
  int32_t wind_randomize_on_reset;
  int32_t wind_randomize_phase;
  int32_t wind_coupling;        /* FW_WIND_COUPLE_* */
  int32_t gyroscopic;           /* include  -w x (I w)  in the angular acceleration */
  int32_t n_collision_pts;      /* <= FW_MAX_COLLISION_PTS */
  int32_t num_obstacles;        /* <= FW_MAX_OBSTACLES (objlock tasks) */
  int32_t duck_camera_capture_interval_steps;
  int32_t duck_lock_hold_steps;
  int32_t duck_lock_decay_steps;
  int32_t duck_switch_min_consecutive_seen;
  int32_t camera_resolution;    /* square, pixels (analytic camera model) */
  int32_t duck_vision_no_deltas; /* ObjLock: 1 = duck_vision_use_deltas=False of the reference (envs/fixedwing_objlock_env.py:69-70, 440-441):
                                  * the observation ends with the 27 history values, without the 4 frame-to-frame deltas (52 wide, not 56).
                                  * (Round 5; one of the former reserved words, which callers zero: same layout, same ABI version.) */
  int32_t lowlevel_max_episode_steps; /* FW_TASK_LOWLEVEL: truncation at this many agent steps (2000, fixedwing_lowlevel_env.py:137).
                                  * (A former reserved word, which callers zero: same layout, same ABI version.) */
  int32_t lowlevel_variant;     /* FW_TASK_LOWLEVEL: FW_LL_VARIANT_* -- which of the reference's two low-level envs.  0 (what every caller
                                  * before it sends) is fixedwing_lowlevel_env.py; 1 is the env examples/lowlevel.py defines for its SAC run.
                                  * (This word and the next: former reserved words, which callers zero: same layout, same ABI version.) */
  int32_t lowlevel_fixed_heading; /* FW_LL_VARIANT_SAC_DEMO: 1 = target_heading_random=False (examples/lowlevel.py:109): psi_ref = 0.
                                  * Must be 0 or 1 there; the first variant neither reads nor checks it. */
  int32_t reserved_i[4];

  /* ---- env / task scalars ---- */
  double flight_dome_size;
  double max_duration_seconds;
  double goal_reach_distance;
  double waypoint_min_height;       /* 0.5  fixedwing_waypoint_objlock_env.py:103 */
  double waypoint_spawn_size;       /* dome used by the target sampler */
  double start_pos[3];
  double start_orn[3];              /* euler */
  double start_vel[3];              /* world frame, PyFlyt starting_velocity */

  /* ---- wind (fixedwing_base_env.py:108-173) ---- */
  double wind_enu_mps[3];
  double wind_enu_mps_range[3][2];
  double gust_amp_enu_mps[3];
  double gust_amp_enu_mps_range[3][2];
  double gust_freq_hz;
  double gust_phase_rad;
  double wind_force_coef;           /* N per (m/s) for FW_WIND_COUPLE_FORCE */

  /* ---- vehicle (build-owned: URDF is not in the reference) ---- */
  double mass;
  double inertia[6];                /* ixx iyy izz ixy ixz iyz, body frame about the COM */
  double gravity;                   /* 9.81, acts along -z world */
  double air_density;               /* 1.225 */
  double collision_pts[FW_MAX_COLLISION_PTS][3]; /* body-frame points; contact <=> world z <= 0 */
  double mixer[FW_NUM_ACTUATORS][4];/* mode-0: cmd = mixer * [roll,pitch,yaw,thrust01] */
  fw_surface_params surfaces[FW_NUM_SURFACES];
  fw_motor_params motor;

  /* ---- objlock tasks (envs/fixedwing_objlock_env.py:54-80) ---- */
  double duck_strike_distance_m;
  double duck_strike_reward;
  double duck_lock_step_reward;
  double duck_approach_reward_scale;
  double duck_global_scaling;
  double duck_distance_reward_scale;
  double duck_lock_center_radius;
  double duck_centering_reward_scale;
  double duck_visible_step_reward;
  double duck_area_reward_scale;
  double duck_lock_lost_penalty;
  double duck_approach_reward_clip_m;
  double duck_switch_min_area;
  double duck_radius_per_scale;     /* analytic duck = sphere of radius scale*this */
  double obstacle_radius;
  double obstacle_height_range[2];
  double obstacle_safe_distance_m;
  double obstacle_avoid_reward_scale;
  double obstacle_avoid_max_penalty;
  double camera_offset[3];          /* cockpit_fpv [0.8,0,0.12]  fixedwing_objlock_env.py:185 */
  double camera_angle_deg;          /* -5 */
  double camera_fov_deg;            /* 90 */
  double camera_near;               /* 0.1   fixedwing_objlock_env.py:692 */
  double camera_far;                /* 255.0 */
  /* ---- low-level task (envs/fixedwing_envs/fixedwing_lowlevel_env.py:32-33, 86-91); former reserved words, zero elsewhere ---- */
  double lowlevel_speed_range[2];   /* V_ref ~ U(lo, hi), (10, 20) */
  double lowlevel_height_range[2];  /* h_ref ~ U(lo, hi), (5, 20) */
  double lowlevel_min_speed;        /* FW_LL_VARIANT_SAC_DEMO: the stall-penalty threshold min_speed_mps, 8.0 (examples/lowlevel.py:41, 183);
                                     * finite and >= 0 there; the first variant neither reads nor checks it.  (A former reserved word, zero elsewhere.) */
  double reserved_d[3];
} fw_config;

/* ---- canonical per-env state record (doubles; used by fw_get_state/fw_set_state) ---- */
enum {
  FW_S_POS = 0,        /* 3  world position */
  FW_S_QUAT = 3,       /* 4  x y z w, body->world */
  FW_S_VEL = 7,        /* 3  world-frame linear velocity */
  FW_S_OMEGA = 10,     /* 3  world-frame angular velocity */
  FW_S_ACT = 13,       /* 6  surface actuations (5) + throttle */
  FW_S_ACTION = 19,    /* 4  raw action as shown in the current observation (obs[12:16]) */
  FW_S_STEP_COUNT = 23,
  FW_S_TICK_COUNT = 24,/* physics ticks since reset (elapsed_time * physics_hz) */
  FW_S_EPISODE = 25,   /* episode index (RNG counter word) */
  FW_S_FLAGS = 26,     /* bit0 termination, bit1 truncation, bit2 collision, bit3 oob, bit4 env_complete,
                          bits 8-11: waypoint index seen by the last compute_state() (the returned obs) */
  FW_S_NUM_REACHED = 27,
  FW_S_NEW_DIST = 28,  /* WaypointHandler.new_distance */
  FW_S_WIND = 29,      /* 7  base[3], gust amp[3], phase */
  FW_S_EP_RETURN = 36,
  FW_S_TARGETS = 37,   /* FW_MAX_TARGETS x 3 (world) */
  FW_S_TASK = 61,      /* task-specific tail, see FW_ST_* */
  FW_STATE_DIM = 176
};

/* objlock tail (offsets from FW_S_TASK); mirrors the private fields of
 * envs/fixedwing_objlock_env.py:143-156 plus the latest analytic camera frame */
enum {
  FW_ST_DUCK_POS = 0,      /* 3 */
  FW_ST_LOCK_STEPS = 3,
  FW_ST_PREV_EST = 4,      /* _prev_est_dist_m, <0 encodes None */
  FW_ST_LAST_CX = 5,
  FW_ST_LAST_CY = 6,
  FW_ST_LAST_AREA = 7,
  FW_ST_LAST_DEPTH = 8,
  FW_ST_SINCE_SEEN = 9,
  FW_ST_HIST_FILLED = 10,
  FW_ST_FRAME_HAS = 11,    /* 1 once the camera has captured a frame this episode */
  FW_ST_FRAME = 12,        /* 8: visible, cx, cy, area, depth_m, d_left, d_center, d_right of the latest frame */
  FW_ST_HIST = 20,         /* FW_VISION_HIST x FW_VISION_FEATS = 27, newest first */
  FW_ST_DUCK_PHASE = 47,   /* combined env: bit0 duck_phase, bit1 post_waypoints */
  FW_ST_SEEN_CONSEC = 48,
  FW_ST_NUM_OBST = 49,
  FW_ST_OBST = 50,         /* FW_MAX_OBSTACLES x 3 (x, y, height) -> 110 of the 115 tail slots */
  FW_ST_DIM = 110
};

/* low-level tail (offsets from FW_S_TASK): the episode's target and the action its observation shows.  The episode's step
 * count is FW_S_STEP_COUNT, as for every task.  FW_TASK_WAYPOINTS_DIRECT uses the same two slots: FW_SL_TARGET holds the last
 * conditioned command of fw_command_hl, FW_SL_PREV_ACTION the six actuator commands its observation shows (obs[12:18] / [13:19]);
 * FW_S_ACTION stays zero for it.  With lowlevel_variant = FW_LL_VARIANT_SAC_DEMO, FW_SL_PREV_ACTION is the last action taken, clipped to
 * [-1, 1]: the row of the step that took it shows the one before (examples/lowlevel.py:127-133), fw_observe and the next step's row show it. */
enum {
  FW_SL_TARGET = 0,        /* 3: psi_ref, h_ref, V_ref            fixedwing_lowlevel_env.py:86-91 */
  FW_SL_PREV_ACTION = 3,   /* 6: the last action (obs[12:18])     :99 */
  FW_SL_DIM = 9
};

/* info_i32 columns written by fw_step (info of the step that just ran, i.e. of
 * the finished episode when the env was auto-reset). */
enum {
  FW_INFO_NUM_TARGETS_REACHED = 0,
  FW_INFO_COLLISION = 1,
  FW_INFO_OUT_OF_BOUNDS = 2,
  FW_INFO_ENV_COMPLETE = 3,
  FW_INFO_DUCK_STRIKE = 4,
  FW_INFO_IS_SUCCESS = 5,
  FW_INFO_EP_LEN = 6,     /* agent steps of the finished episode (valid when done) */
  FW_INFO_RESERVED = 7,
  FW_INFO_DIM = 8
};

/* fw_get_counters columns: how the auto-resets of fw_step were served so far (diagnostics; they let a test assert that
 * the background hand-off -- and not only its in-kernel fallback -- was exercised, e.g. under hipGraph replay). */
enum {
  FW_CTR_LAUNCHES = 0,       /* fw_step launches so far (the device-side launch index the hand-off protocol uses) */
  FW_CTR_RESETS = 1,         /* auto-resets performed inside fw_step */
  FW_CTR_SHADOW_HITS = 2,    /* ... served by a pre-simulated ("shadow") episode start: wind / camera tasks */
  FW_CTR_SCENARIO_HITS = 3,  /* ... served by pre-sampled waypoints: wind-free waypoints task */
  FW_CTR_FALLBACKS = 4,      /* ... served by the in-kernel sampler / warm-up */
  FW_CTR_HELPER_TIMEOUTS = 5,/* camera tasks, 8-lane mapping: waits of a step wave for its capture wave that gave up (a protocol error; 0 always) */
  FW_CTR_DIM = 8
};

typedef struct fw_env* fw_handle;

/* Size of fw_config as compiled into the library (binding self-check). */
int32_t fw_sizeof_config(void);
int32_t fw_abi_version(void);
int32_t fw_state_dim(void);      /* FW_STATE_DIM of the canonical state record */

/* Observation width D for a config (22/23 attitude + task part; 21 for FW_TASK_LOWLEVEL; 24/25 + 3 context_length for
 * FW_TASK_WAYPOINTS_DIRECT, whose action block is six wide); <0 on error. */
int32_t fw_obs_dim(const fw_config* cfg);
/* Action width A for a config: 6 for FW_TASK_LOWLEVEL and FW_TASK_WAYPOINTS_DIRECT (the actuator commands), 4 otherwise
 * ([roll, pitch, yaw, thrust]); <0 on error. */
int32_t fw_act_dim(const fw_config* cfg);

/* Validate a config exactly like the reference constructors do.  On error
 * returns FW_EINVAL and writes a message (same wording class as the
 * reference's ValueError) into msg[msg_len]. */
int32_t fw_validate_config(const fw_config* cfg, char* msg, int32_t msg_len);

/* Create N envs on HIP device `device`.  global_env_offset is added to the
 * local env index to form the RNG key, so that a sharded job (rank r owns
 * [r*N, (r+1)*N)) draws the same scenarios as a single-device job. */
int32_t fw_create(const fw_config* cfg, int32_t num_envs, int32_t device,
                  uint64_t seed, int64_t global_env_offset, fw_handle* out);

/* Scenario of the episode a fw_reset starts, supplied by the caller instead of drawn by the env -- e.g. the targets /
 * duck / obstacles / wind a PyFlyt run sampled, so that reference traces can be replayed without
 * forging whole state records.  HOST arrays indexed by the handle's local env; any pointer may be NULL = keep the
 * env's own draw for that item.  Only the episode started by this call is affected (later auto-resets draw again). */
typedef struct fw_scenario {
  const double* targets;        /* [N][FW_MAX_TARGETS][3] world waypoints (rows >= num_targets ignored)     WaypointHandler.reset */
  const double* duck_pos;       /* [N][3] duck base position                         envs/fixedwing_objlock_env.py:472-491 */
  const double* obstacles;      /* [N][FW_MAX_OBSTACLES][3]  x, y, height            envs/fixedwing_objlock_env.py:528-565 */
  const int32_t* num_obstacles; /* [N]  cylinders actually placed (required with `obstacles`; clipped to fw_config.num_obstacles) */
  const double* wind_base;      /* [N][3]  wind_enu_mps                              envs/fixedwing_envs/fixedwing_base_env.py:135-143 */
  const double* gust_amp;       /* [N][3]  gust_amp_enu_mps                          :155-159 */
  const double* gust_phase;     /* [N]     gust_phase_rad                            :162-165 */
} fw_scenario;

/* Reset envs.  mask: device u8[N] (non-zero = reset) or NULL = all.
 * scenario: NULL, or the caller-supplied scenario of the new episodes (see fw_scenario; applied to the reset envs only).
 * obs_out: device T[N,D] or NULL.  Rows of non-reset envs are rewritten with
 * their current observation. */
int32_t fw_reset(fw_handle h, const uint8_t* mask, const fw_scenario* scenario, void* obs_out, void* hip_stream);

/* One agent step for all N envs.
 *   actions       T[N,A]  in [-1,1] (caller clips, as SB3 does); A = fw_act_dim(cfg)
 *   obs           T[N,D]  next observation (first obs of the new episode if auto-reset fired)
 *   reward        T[N]
 *   terminated    u8[N]
 *   truncated     u8[N]
 *   terminal_obs  T[N,D]  rows written only where terminated|truncated (may be NULL)
 *   info_i32      i32[N,FW_INFO_DIM] (may be NULL) */
int32_t fw_step(fw_handle h, const void* actions, void* obs, void* reward,
                uint8_t* terminated, uint8_t* truncated, void* terminal_obs,
                int32_t* info_i32, void* hip_stream);

/* Re-key the RNG: subsequent resets use (seed, global env id, episode=0...). */
int32_t fw_seed(fw_handle h, uint64_t seed);

/* Canonical state records, HOST memory, double[N, FW_STATE_DIM]. Synchronous. */
int32_t fw_get_state(fw_handle h, double* state_out);
int32_t fw_set_state(fw_handle h, const double* state_in);

/* Diagnostic counters, HOST uint64[FW_CTR_DIM] (see FW_CTR_*).  Synchronous. */
int32_t fw_get_counters(fw_handle h, uint64_t* out);

/* Recompute the observation from the current state (no dynamics), device T[N,D]. */
int32_t fw_observe(fw_handle h, void* obs_out, void* hip_stream);

/* FPV image of every env's CURRENT pose, for a network front end (the reference's camera hands the env segImg / depthImg,
 * envs/fixedwing_objlock_env.py:603-622; its CNN path replaces segImg by a detector's mask,
 * envs/fixedwing_envs/objlock_yolo_env.py:646-716).  The scene is the analytic one the vision features of the objlock tasks are
 * functionals of: out = device float32 [N][2][res][res], channel 0 = duck mask (0 / 1), channel 1 =
 * depth-buffer value in [0, 1] of the nearest fragment (sky 1.0); same camera (offset, tilt, FOV), focal length scaled to `res`.
 * FW_EUNSUPPORTED for the waypoints task (no camera). */
int32_t fw_render(fw_handle h, int32_t res, float* out, void* hip_stream);

/* ---- rollout-collector helpers (the caller side of the path: SB3's OnPolicyAlgorithm /
 * RolloutBuffer / VecNormalize as driven by train/train_Fixedwing_Waypoints_v3.py:260,293-337).
 * Stateless, float32 device buffers laid out [T, N] (time-major, env contiguous). ---- */

/* Generalised advantage estimation, SB3 RolloutBuffer.compute_returns_and_advantage:
 *   delta_t = r_t + gamma * V_{t+1} * (1 - start_{t+1}) - V_t
 *   A_t     = delta_t + gamma * lambda * (1 - start_{t+1}) * A_{t+1},   returns = A + V
 * with V_T = last_values, start_T = last_dones.  episode_starts[t,n] = 1 iff step t is the
 * first of an episode.  One lane per env, T sequential steps, coalesced across envs. */
int32_t fw_gae(const float* rewards, const float* values, const float* episode_starts,
               const float* last_values, const float* last_dones, float* advantages, float* returns,
               int32_t T, int32_t N, float gamma, float gae_lambda, void* hip_stream);

/* Episode bookkeeping of an evaluation loop (SB3 evaluate_policy; evaluate.ReplayedEvaluation): after a vec-step, add `reward` [N]
 * (env dtype) to cur_rew and 1 to cur_len; where terminated | truncated and counts[i] < targets[i], record the episode (reward, length,
 * the vec-step index, the info row) in slot counts[i] of env i ([N, E] buffers; info may be NULL) and count it; clear the accumulators of
 * finished episodes; advance step_ctr[0].  One launch, all buffers on the device. */
int32_t fw_eval_track(const void* reward, int32_t reward_is_f64, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                      int32_t info_dim, const int64_t* targets, int64_t* counts, double* cur_rew, int64_t* cur_len, int64_t* step_ctr,
                      double* fin_rew, int64_t* fin_len, int64_t* fin_step, int32_t* fin_info, int32_t N, int32_t E, void* hip_stream);
/* Episode statistics of a training run (monitor.EpisodeMonitor; SB3's Monitor + ep_info_buffer, DESIGN.md section 4b "Episode
 * statistics").  The state block is the caller's: fw_episode_state_bytes(N, W) bytes of device memory, zeroed once (FW_EINVAL for
 * N <= 0 or W <= 0), in 8-byte words:
 *   [0]  episodes finished (int64; the ring's cursor is this mod W)      [1]  vec-steps folded       [2]  truncated episodes
 *   [3]  sum of lengths     [4..9]  sums of the info columns FW_INFO_NUM_TARGETS_REACHED .. FW_INFO_IS_SUCCESS (all int64, exact)
 *   [10] sum of returns     [11] sum of squared returns (double)         [12..15] reserved, zero
 *   then the ring, W words each: return (double), length, vec-step index (1-based), env index, truncated flag (int64), and 4 W
 *   words of info rows (int32 [W][FW_INFO_DIM]);  then per env, N words each: cur_ret (double), cur_len (int64).
 * fw_episode_fold folds one vec-step: cur_ret[i] += reward[i] (env dtype, added in double), cur_len[i] += 1; where terminated |
 * truncated the episode (cur_ret, cur_len, the step's index, i, truncated[i] != 0, the first min(info_dim, FW_INFO_DIM) columns of
 * its info row -- zeros when info is NULL) is pushed and the accumulators are cleared.  Pushes are ordered by vec-step and inside one
 * by ascending env index; the slot is the push rank mod W: the ring holds what collections.deque(maxlen=W) holds after extend() in
 * env order, also when more than W episodes end in one step (only the last W of them are written).  The double sums are reduced in
 * a fixed order (the same bits in every run).  One launch, one workgroup, graph-capturable: no host reads, fixed addresses.
 * FW_EINVAL for a NULL reward / terminated / truncated / state, N <= 0, W <= 0, or info with info_dim <= 0. */
int64_t fw_episode_state_bytes(int32_t N, int32_t W);
int32_t fw_episode_fold(const void* reward, int32_t reward_is_f64, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                        int32_t info_dim, void* state, int32_t N, int32_t W, void* hip_stream);
/* The same fold over many workgroups, for env counts at which one workgroup walking all N envs costs more than the step itself
 * (DESIGN.md section 4b "Episode statistics").  Same semantics, same state block (layout and fw_episode_state_bytes above): the two
 * forms may be mixed on one block from one vec-step to the next.  Every word of the block comes out the same bits as from
 * fw_episode_fold except the two double totals [10] and [11], whose summation order differs (fixed too: the same bits in every run).
 * fw_episode_fold_span() is the number of envs a workgroup owns, a build constant (a multiple of 64); B = ceil(N / span) workgroups.
 * The workspace is the caller's: fw_episode_fold_workspace_bytes(N) bytes of device memory (FW_EINVAL for N <= 0), no
 * initialisation needed -- every call writes every word it later reads.  Three launches on the caller's stream (count the dones per
 * workgroup; fold, each workgroup ranking its dones behind those of the workgroups below it; one workgroup adds the partial sums to
 * the header), kernel boundaries the only synchronisation between workgroups: no atomics, no in-grid waits, no host reads, fixed
 * addresses, graph-capturable.  No upper limit on N other than int32.  FW_EINVAL as for fw_episode_fold, and for a NULL workspace. */
int32_t fw_episode_fold_span(void);
int64_t fw_episode_fold_workspace_bytes(int32_t N);
int32_t fw_episode_fold_wide(const void* reward, int32_t reward_is_f64, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                             int32_t info_dim, void* state, void* workspace, int32_t N, int32_t W, void* hip_stream);
/* fw_eval_track for FW_TASK_LOWLEVEL, plus its tracking figures.  Everything fw_eval_track does, and from the
 * post-step observation row o of env i -- terminal_obs[i] where terminated | truncated, else obs[i]; [N, 21], obs_is_f64 the env
 * dtype -- with e_psi = wrap(o[18] - o[5]) (to [-pi, pi)), e_h = o[19] - o[11], e_V = o[20] - |o[6:9]|, w = |o[0:3]| it adds
 * (|e_psi|, e_psi^2, |e_h|, e_h^2, |e_V|, e_V^2, w) in double to cur_track [N, 7]; a recorded episode's seven sums and
 * survived = !terminated (1.0 / 0.0) go to fin_track [N, E, 8] at its slot, and the sums of finished episodes are cleared.
 * FW_EINVAL for NULL buffers, obs_dim != 21, N <= 0 or E <= 0.  One launch. */
int32_t fw_eval_track_ll(const void* reward, int32_t reward_is_f64, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                         int32_t info_dim, const void* obs, const void* terminal_obs, int32_t obs_is_f64, int32_t obs_dim,
                         const int64_t* targets, int64_t* counts, double* cur_rew, int64_t* cur_len, int64_t* step_ctr, double* cur_track,
                         double* fin_rew, int64_t* fin_len, int64_t* fin_step, int32_t* fin_info, double* fin_track, int32_t N, int32_t E,
                         void* hip_stream);
/* fw_eval_track for the high-level command task (HighLevelCmdVecEnv; DESIGN.md section 2e "Evaluation").  Everything fw_eval_track
 * does, and from the post-step observation row o of env i -- terminal_obs[i] where terminated | truncated, else obs[i]; [N, 30],
 * obs_is_f64 the env dtype -- the conditioned command c = command[i] ([N, 3], the env dtype: the triple in force during the step)
 * and p = prev_cmd[i] ([N, 3] double, owned by the caller), in double: e_psi = wrap(c0 - o[5]) (to [-pi, pi)), e_h = c1 - o[11],
 * e_V = c2 - |o[6:9]|, w = |o[0:3]|; d_psi = |wrap(c0 - p0)|, d_h = |c1 - p1|, d_V = |c2 - p2| where cur_len[i] was > 0 before the
 * step, else 0 (an episode's first step has no previous command); sat = 1 if c1 <= 0, c1 >= alt_high, c2 <= 0 or c2 >= speed_high,
 * else 0.  It adds (|e_psi|, e_psi^2, |e_h|, e_h^2, |e_V|, e_V^2, w, d_psi, d_h, d_V, sat) to cur_track [N, 11]; a recorded
 * episode's eleven sums go to fin_track [N, E, 11] at its slot, the sums of finished episodes are cleared, and prev_cmd[i] = c on
 * every step.  FW_EINVAL for NULL buffers, obs_dim != 30, N <= 0 or E <= 0.  One launch, one workgroup. */
int32_t fw_eval_track_hl(const void* reward, int32_t reward_is_f64, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                         int32_t info_dim, const void* obs, const void* terminal_obs, const void* command, int32_t obs_is_f64,
                         int32_t obs_dim, double alt_high, double speed_high, const int64_t* targets, int64_t* counts, double* cur_rew,
                         int64_t* cur_len, int64_t* step_ctr, double* cur_track, double* prev_cmd, double* fin_rew, int64_t* fin_len,
                         int64_t* fin_step, int32_t* fin_info, double* fin_track, int32_t N, int32_t E, void* hip_stream);

/* Commanding the low-level controller (FW_TASK_LOWLEVEL; DESIGN.md section 2d "Commanding the controller").
 * fw_command_ll: cmd is a device [T, N, 3] double schedule of (psi, h, V) commands; env i takes row min(*step_idx, T - 1) (row 0
 * when step_idx is NULL; step_idx is only read).  In double, as train/train_highlevel_cmd.py:164-166: psi wrapped to [-pi, pi)
 * (the reward's wrap), h clipped to [0, flight_dome_size], V clipped to [0, 100]; then converted to the handle's dtype and written
 * to the env's FW_SL_TARGET tail and, when obs is not NULL, to obs[i, 18:21] ([N, 21], the env dtype).  mask (optional, uint8 [N]):
 * rows with mask[i] == 0 are not touched.  A row with a non-finite component is left unchanged and counted into rejected[0]
 * (optional; the caller zeroes it).  The command holds until the env's episode ends: the auto-reset draws a new random target.
 * FW_EUNSUPPORTED for any other task; FW_EINVAL for a NULL cmd or T <= 0.  One thread per env, either lane mapping, f64 / f32. */
int32_t fw_command_ll(fw_handle h, const double* cmd, int32_t T, const int64_t* step_idx, const uint8_t* mask, void* obs,
                      int32_t* rejected, void* hip_stream);
/* The high-level command step (train/train_highlevel_cmd.py:93-101, 158-171), for a FW_TASK_WAYPOINTS_DIRECT
 * handle with the Euler attitude: `action` is the high-level policy's raw [N, 3] output (heading, altitude, airspeed; double when
 * action_is_f64, else float).  Per env, in double: clipped to the reference's action Box ([-pi, 0, 0], [pi, flight_dome_size, 30]),
 * then conditioned as :164-166 (heading wrapped to [-pi, pi), altitude clipped to [0, flight_dome_size], airspeed to [0, 100]),
 * converted to the handle's dtype and written to low_obs[i] = (obs[i, 0:18], command) ([N, 21], the env dtype: the low-level
 * controller's raw observation), to the env's FW_SL_TARGET tail and, when not NULL, to cmd_out[i] ([N, 3], the env dtype).  `obs` is
 * the env's observation buffer ([N, fw_obs_dim]), only read.  mask (optional, uint8 [N]): rows with mask[i] == 0 are not touched,
 * low_obs and cmd_out included.  A row with a non-finite component keeps the env's stored command (after a reset: 0, start height,
 * start speed) and is counted into rejected[0] (optional; the caller zeroes it).  FW_EUNSUPPORTED for any other task or the
 * quaternion attitude; FW_EINVAL for NULL action / obs / low_obs.  One thread per env, either lane mapping, f64 / f32. */
int32_t fw_command_hl(fw_handle h, const void* action, int32_t action_is_f64, const uint8_t* mask, const void* obs, void* low_obs,
                      void* cmd_out, int32_t* rejected, void* hip_stream);
/* fw_trace_ll: with k = *step_idx, and only when 0 <= k < T, the post-step row o of env i -- terminal_obs[i] where terminated |
 * truncated, else obs[i]; [N, 21], obs_is_f64 the env dtype -- goes to trace[k, i, :] ([T, N, 8] double) as
 * (o[18], o[5], o[19], o[11], o[20], |o[6:9]|, |o[0:3]|, flag), flag 0 = running, 1 = terminated, 2 = truncated; then *step_idx
 * advances by one.  terminated / truncated / terminal_obs may be NULL (no env is done).  One workgroup.
 * FW_EINVAL for NULL obs / trace / step_idx, N <= 0 or T <= 0. */
int32_t fw_trace_ll(const void* obs, const void* terminal_obs, const uint8_t* terminated, const uint8_t* truncated, int32_t obs_is_f64,
                    int32_t N, double* trace, int32_t T, int64_t* step_idx, void* hip_stream);
/* fw_trace_hl: fw_trace_ll for the high-level command task (same step_idx semantics).  With k = *step_idx, and only when
 * 0 <= k < T, the post-step row o of env i ([N, 30]) and the conditioned command c = command[i] ([N, 3], the env dtype) go to
 * trace[k, i, :] ([T, N, 11] double) as (c0, o[5], c1, o[11], c2, |o[6:9]|, |o[0:3]|, o[9], o[10],
 * info[i, FW_INFO_NUM_TARGETS_REACHED] as the step left it (0 when info is NULL; info_dim its row length), flag); then *step_idx
 * advances by one.  terminated / truncated / terminal_obs may be NULL.  One workgroup.
 * FW_EINVAL for NULL obs / command / trace / step_idx, N <= 0, T <= 0, or info with info_dim <= 0. */
int32_t fw_trace_hl(const void* obs, const void* terminal_obs, const uint8_t* terminated, const uint8_t* truncated, const void* command,
                    const int32_t* info, int32_t info_dim, int32_t obs_is_f64, int32_t N, double* trace, int32_t T, int64_t* step_idx,
                    void* hip_stream);

/* fw_trace_rows: the flight recorder of the waypoint and duck tasks (fw_trace_hl's step_idx semantics).  With
 * k = *step_idx, and only when 0 <= k < T, the post-step row o of env i -- terminal_obs[i] where terminated | truncated, else obs[i];
 * [N, obs_dim], obs_is_f64 the env dtype -- goes to trace[k, i, :] ([T, N, obs_dim + 2] double) as (o[0 : obs_dim] widened to double,
 * info[i, FW_INFO_NUM_TARGETS_REACHED] as the step left it (0 when info is NULL; info_dim its row length), flag), flag 0 = running,
 * 1 = terminated, 2 = truncated (terminated wins); then *step_idx advances by one.  terminated / truncated / terminal_obs / info may
 * be NULL.  The kernel copies: any observation layout.  One workgroup of 1024 threads, no atomics.
 * FW_EINVAL for NULL obs / trace / step_idx, N <= 0, T <= 0, obs_dim <= 0, or info with info_dim <= 0. */
int32_t fw_trace_rows(const void* obs, const void* terminal_obs, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                      int32_t info_dim, int32_t obs_is_f64, int32_t N, int32_t obs_dim, double* trace, int32_t T, int64_t* step_idx,
                      void* hip_stream);
/* fw_eval_track plus twelve per-episode path sums for the waypoint and duck tasks.  Everything fw_eval_track
 * does, and from the post-step row o of env i (terminal_obs[i] where terminated | truncated, else obs[i]; [N, obs_dim]) with
 * omega = o[0:3], v = o[att_dim-6 : att_dim-3], p = o[att_dim-3 : att_dim], a = o[att_dim : att_dim+act_dim],
 * throttle = o[att_dim+act_dim+5], delta = o[att_dim+act_dim+6 : +3] (present when obs_dim >= att_dim+act_dim+9), r = info[i, 0]
 * (0 when info is NULL), L = cur_len[i] + 1 and carry[i] = (p_prev[3], p_leg[3], a_prev[6], reached_prev) ([N, 13] double, owned by the
 * caller, seeded from the reset observation), all in double, cur_path [N, 12]:
 *   0 path_len += |p - p_prev|      1 speed_sum += |v|      2 alt_sum += p_z      3 alt_min = min(., p_z)      4 ang_vel_sum += |omega|
 *   5 act_delta_sum += sum_j |a_j - a_prev_j|      6 throttle_sum += throttle
 *   and where r > reached_prev:  7 first_reach_step = L if still 0,  8 last_reach_step = L,  9 chord_len += |p - p_leg|,
 *   10 path_at_last_reach = path_len (after this step),  11 miss_dist = +inf;  else 11 miss_dist = min(., |delta|) when delta is present.
 * On an episode's first step (cur_len[i] == 0) the sums start at 0, alt_min and miss_dist at +inf.  Where the episode goes on:
 * p_prev = p, a_prev = a, reached_prev = r, and p_leg = p on a reach step.  Where it ended: the twelve sums go to fin_path [N, E, 12] at
 * the episode's slot (fw_eval_track's recording rule), are cleared, and the carry is re-seeded from the live row obs[i]:
 * p_prev = p_leg = its p, a_prev = its action block, reached_prev = 0.
 * FW_EINVAL for NULL buffers, att_dim not 12 or 13, act_dim not 4 or 6, obs_dim < att_dim + act_dim + 6, N <= 0 or E <= 0.
 * One launch, one workgroup, no atomics. */
int32_t fw_eval_track_wp(const void* reward, int32_t reward_is_f64, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                         int32_t info_dim, const void* obs, const void* terminal_obs, int32_t obs_is_f64, int32_t obs_dim, int32_t att_dim,
                         int32_t act_dim, const int64_t* targets, int64_t* counts, double* cur_rew, int64_t* cur_len, int64_t* step_ctr,
                         double* cur_path, double* carry, double* fin_rew, int64_t* fin_len, int64_t* fin_step, int32_t* fin_info,
                         double* fin_path, int32_t N, int32_t E, void* hip_stream);

/* VecNormalize step (SB3 VecNormalize.step_wait + RunningMeanStd.update, Chan et al. merge),
 * fused: one pass over obs[N,D] (env dtype T_in = double|float per `in_is_f64`) that
 *   (a) if `update` != 0 merges the batch moments into (mean[D], var[D], count[1]) (double),
 *   (b) writes clip((obs - mean) / sqrt(var + eps), +-clip) as float32 to obs_out[N,D]
 *       using the UPDATED statistics, as SB3 does.
 * mean/var/count are device double buffers owned by the caller (checkpointable).
 * workspace: device buffer of fw_normalize_obs_workspace_bytes(D) bytes owned by the caller (needed when update != 0):
 * the per-block partial sums live there, so concurrent callers / streams share nothing and nothing is ever allocated
 * on the launch path (safe under hipGraph capture).
 * batch_acc (may be NULL): device double[2 D + 1]; when update != 0 the batch's column sums, sums of squares and row count
 * are ADDED to it.  A job sharded over GPUs all-reduces these accumulators once per rollout (RCCL) and re-derives the
 * statistics of all envs from them (collective 2) -- no collective sits between two env steps. */
int64_t fw_normalize_obs_workspace_bytes(int32_t D);
int32_t fw_normalize_obs(const void* obs, int32_t in_is_f64, int32_t N, int32_t D, double* mean, double* var,
                         double* count, int32_t update, float clip, float eps, float* obs_out, void* workspace,
                         double* batch_acc, void* hip_stream);

/* PPO minibatch updates (SB3 PPO.train() inner loop; train/train_Fixedwing_Waypoints_v3.py:293-310) for the
 * reference's MlpPolicy (separate 64-64 tanh nets for pi and V, 4-dim diagonal Gaussian, log_std parameter),
 * fused into ONE kernel that walks `n_minibatches` consecutive minibatches: forward, clipped-surrogate +
 * value + entropy loss, backward, global grad-norm clipping and Adam, weights resident in LDS.
 * Flat layout of params (float32, fw_ppo_param_count(obs_dim) elements):
 *   for net in (pi, vf): W1[Dp][64] b1[64] W2[64][64] b2[64] Wo[64][KO] bo[KO]   (KO = 4, 1; W = Linear.weight^T;
 *   Dp = obs_dim rounded up to even, the pad row is zero), then log_std[4].
 * Adam moments mom_m / mom_v (float32, fw_ppo_moment_count() elements each) are in the kernel's "slot" order, in
 * which every lane's elements are contiguous: fw_ppo_moment_map(obs_dim, out) gives the flat parameter index of
 * each slot (-1 for padding and for the unused second half of the buffers), which is all a caller needs to
 * move them to and from its optimiser.  The slot order belongs to a library build (round 3 moved Wo's moments): persist
 * moments in the optimiser's own order, never in slot order.
 * obs[S,obs_dim], act[S,4], old_logp[S], adv[S], ret[S]: the rollout buffer (float32, device);
 * perm[n_minibatches * batch_size]: sample indices of consecutive minibatches (int32, device).
 * batch_size must be a multiple of 16, obs_dim <= 64.  loss_acc[3] (may be NULL) accumulates the per-minibatch
 * mean policy loss, value loss and entropy loss.  The caller advances its Adam step count by n_minibatches.
 * workspace: caller-owned device buffer of >= fw_ppo_update_workspace_bytes(n_minibatches, batch_size, obs_dim) bytes: exchange
 * words, the gradient hand-off buffer and the PACKED ROWS of this call -- a parallel pre-pass (one workgroup per minibatch, all
 * CUs) writes every minibatch's rows in walking order, observation | action | old log-prob, normalised advantage, return,
 * (obs_dim rounded up to 4) + 8 floats each, so that the sequential kernel reads each 16- / 32- / 64-sample pass as one contiguous block
 * (144 B per sample and epoch for 28 observations: 189 MB for 20 epochs x 65 536 samples).  Two learners never share it.
 * The learner-side entry points run on the device their buffers live on, whatever the thread's current device.
 * The call runs on 2, 4, 8 or 16 workgroups: (policy, value) x 1, 2, 4 or 8 workgroups per network that share every minibatch (128
 * samples: 8 x 16, 64: 4 x 16) and exchange gradients (and, from four on, updated weights) once per minibatch; all of them end the call
 * with the same bits.
 * Failure inside the launch: the workgroups of a call wait for each other two or three times per minibatch, every wait
 * bounded.  A wait that runs out raises FW_PPO_ST_* in the workspace's status word and the workgroups leave.  `params`, `mom_m`
 * and `mom_v` are written back only behind a verdict every workgroup waits for at the end of the call (the last one to get through
 * its final minibatch reads the status word and says "write" or "do not"): a workgroup that gave up never arrives, so in that case
 * NOBODY writes and the three buffers are exactly as they were before the call.  The one exception is a verdict wait that itself
 * runs out (FW_PPO_ST_COMMIT): some workgroups may then have written their share.  The contract is therefore: status 0 = the
 * buffers hold the result; any other status = treat `params`, `mom_m`, `mom_v` as UNDEFINED and restore them from the caller's own
 * copies (rollout.FusedPpoUpdate reloads them from the module / optimiser, which it only overwrites after status 0).
 * fw_ppo_update_status reads
 * the word after the call (it synchronises `hip_stream`): 0 = the call ran to its end.  `paths` (may be NULL) receives which
 * exchanges went through an XCD's shared L2 rather than device-scope accesses: bit 2 b = workgroup b's gradient swap, bit
 * 2 b + 1 = its norm exchange, b = 2 * part + net (part = the workgroup's index inside its network).  Environment (read per call):
 * FWSIM_PPO_SPLIT=CHxN forces the cut (CH = 16 / 32 / 64 samples per pass, N = 1 / 2 / 4 / 8 workgroups per network); FWSIM_PPO_RS=0 makes
 * (up to four) workgroups swap whole gradients all-to-all instead of reduce-scatter + weight all-gather; FWSIM_PPO_NO_L2_SWAP=1 forces the
 * device-scope form of every exchange (same arithmetic: results must be bit-identical -- tests/test_protocols_gpu.py);
 * FWSIM_SPIN_LOG2=k shrinks every wait's budget to 2^k polls (tests provoke the timeout with it). */
#define FW_PPO_ST_IDS 1u    /* the workgroups never found each other at the start of the call */
#define FW_PPO_ST_SWAP 2u   /* gradient swap between the workgroups of a network */
#define FW_PPO_ST_NORM 4u   /* gradient-norm exchange between the policy and the value workgroup */
#define FW_PPO_ST_COMMIT 8u /* the closing verdict did not arrive: some workgroups may have written their results, others not */
typedef struct fw_ppo_hyper {
  float lr, clip_range, ent_coef, vf_coef, max_grad_norm, beta1, beta2, eps;
  float adv_mean, adv_std;      /* used when norm_adv == 2 */
  int32_t norm_adv;             /* 0: off, 1: per minibatch (SB3 default), 2: with the given statistics */
  int32_t step0;                /* Adam steps taken before this call */
} fw_ppo_hyper;
int32_t fw_ppo_param_count(int32_t obs_dim);
int32_t fw_ppo_moment_count(void);
int32_t fw_ppo_moment_map(int32_t obs_dim, int32_t* flat_index_of_slot /* host, [fw_ppo_moment_count()] */);
int64_t fw_ppo_update_workspace_bytes(int32_t n_minibatches, int32_t batch_size, int32_t obs_dim);
int32_t fw_ppo_update(float* params, float* mom_m, float* mom_v, const float* obs, const float* act,
                      const float* old_logp, const float* adv, const float* ret, const int32_t* perm,
                      int32_t n_minibatches, int32_t batch_size, int32_t obs_dim, const fw_ppo_hyper* hyper,
                      float* loss_acc, void* workspace, int64_t workspace_bytes, void* hip_stream);
int32_t fw_ppo_update_status(const void* workspace, int64_t workspace_bytes, uint32_t* status_out, uint32_t* paths_out, void* hip_stream);
/* The same learner for a policy head of act_dim actions: act_dim = 4 runs exactly what the entry points above run; act_dim = 6 (the
 * low-level control task's six actuator commands) runs a six-action instantiation of the same kernel, every cut and exchange form
 * included.  Any other act_dim: FW_EINVAL (fw_last_error says why).  With A = act_dim:
 *   flat layout   for net in (pi, vf): W1[Dp][64] b1[64] W2[64][64] b2[64] Wo[64][KO] bo[KO] (KO = A, 1), then log_std[A]
 *                 -- fw_ppo_param_count_a(obs_dim, act_dim) elements;
 *   moments       fw_ppo_moment_count_a(act_dim) slots each, mapped by fw_ppo_moment_map_a (A = 6 adds one slot row: the policy
 *                 head's 64 x 6 weights are two per-thread elements of 256 threads);
 *   act           [S, A]; the packed rows of the workspace are (obs_dim rounded up to 4) + 4 ceil(A / 4) + 4 floats wide, which
 *                 fw_ppo_update_workspace_bytes_a accounts for.
 * The size and layout functions return FW_EINVAL (negative) for bad arguments. */
int32_t fw_ppo_param_count_a(int32_t obs_dim, int32_t act_dim);
int32_t fw_ppo_moment_count_a(int32_t act_dim);
int32_t fw_ppo_moment_map_a(int32_t obs_dim, int32_t act_dim, int32_t* flat_index_of_slot /* host, [fw_ppo_moment_count_a(act_dim)] */);
int64_t fw_ppo_update_workspace_bytes_a(int32_t n_minibatches, int32_t batch_size, int32_t obs_dim, int32_t act_dim);
int32_t fw_ppo_update_a(float* params, float* mom_m, float* mom_v, const float* obs, const float* act,
                        const float* old_logp, const float* adv, const float* ret, const int32_t* perm,
                        int32_t n_minibatches, int32_t batch_size, int32_t obs_dim, int32_t act_dim, const fw_ppo_hyper* hyper,
                        float* loss_acc, void* workspace, int64_t workspace_bytes, void* hip_stream);
/* The same learner for a policy head of THREE actions (the high-level command task's heading / altitude / airspeed): the *_a family
 * with the width fixed -- the *_a entry points themselves keep refusing act_dim = 3.  A three-action instantiation of the same
 * kernel, every cut and exchange form included; the contracts (status word, results only behind the closing verdict, the FWSIM_PPO_* /
 * FWSIM_SPIN_LOG2 switches) are those above.  Flat layout as documented with A = 3: Wo[64][3], bo[3], log_std[3]
 * (fw_ppo_param_count_a3(obs_dim) elements); fw_ppo_moment_count_a3() = fw_ppo_moment_count() slots, mapped by fw_ppo_moment_map_a3 (the
 * places of a fourth component are padding); act is [S, 3]; the packed rows keep the four-action width, their fourth action float is
 * written as zero by the pre-pass and reaches no sum. */
int32_t fw_ppo_param_count_a3(int32_t obs_dim);
int32_t fw_ppo_moment_count_a3(void);
int32_t fw_ppo_moment_map_a3(int32_t obs_dim, int32_t* flat_index_of_slot /* host, [fw_ppo_moment_count_a3()] */);
int64_t fw_ppo_update_workspace_bytes_a3(int32_t n_minibatches, int32_t batch_size, int32_t obs_dim);
int32_t fw_ppo_update_a3(float* params, float* mom_m, float* mom_v, const float* obs, const float* act /* [S, 3] */,
                         const float* old_logp, const float* adv, const float* ret, const int32_t* perm,
                         int32_t n_minibatches, int32_t batch_size, int32_t obs_dim, const fw_ppo_hyper* hyper,
                         float* loss_acc, void* workspace, int64_t workspace_bytes, void* hip_stream);

/* The learner with TRAINING DIAGNOSTICS (SB3's train/approx_kl, train/clip_fraction, the per-minibatch losses): the arguments of
 * fw_ppo_update_a, then `diag` and its size in floats.  act_dim is 3, 4 or 6 (the workspace is sized by the width's own function:
 * fw_ppo_update_workspace_bytes / _a / _a3); anything else, a NULL `diag` or diag_floats < fw_ppo_diag_floats(n_minibatches): FW_EINVAL.
 * It runs the diagnostics instantiation of the kernel the plain entry point of that width would run (same cut, same exchanges, same
 * status word and closing verdict); `params`, `mom_m`, `mom_v` and `loss_acc` end bit-identical to the plain call on the same inputs.
 * diag: device float32, logically [n_minibatches][2 nets: policy, value][8 parts][4 waves][4] -- one row of four floats per WAVE of
 * every workgroup, written once per minibatch with a plain 16-byte store (no atomics, no wait):
 *   policy rows  { sum -min(l1, l2), sum (ratio - 1) - (logp - old_logp), count |ratio - 1| > clip_range, E } each over the samples the
 *                wave owns and times 1 / batch_size; E = the minibatch's entropy loss -sum_k (0.5 + 0.5 ln 2 pi + log_std_k), at the
 *                log_std its forward pass used, in the row of part 0 / wave 0 and zero in every other row;
 *   value rows   { sum (v - return)^2 / batch_size, 0, 0, 0 }.
 * Rows of parts the cut does not use are not written: the caller zeroes `diag` before the call and sums a minibatch's 32 rows per net
 * in index order (a fixed order: the same bits in every run).  On a non-zero status `diag` is undefined. */
int64_t fw_ppo_diag_floats(int32_t n_minibatches);
int32_t fw_ppo_update_diag(float* params, float* mom_m, float* mom_v, const float* obs, const float* act,
                           const float* old_logp, const float* adv, const float* ret, const int32_t* perm,
                           int32_t n_minibatches, int32_t batch_size, int32_t obs_dim, int32_t act_dim, const fw_ppo_hyper* hyper,
                           float* loss_acc, void* workspace, int64_t workspace_bytes, void* hip_stream,
                           float* diag, int64_t diag_floats);

/* The learner with SB3's `target_kl` EARLY STOPPING: the arguments of fw_ppo_update_diag, then the limit and where the number of
 * optimiser steps taken goes.  SB3's PPO.train() looks at approx_kl = mean((ratio - 1) - log ratio) of every minibatch after its
 * losses are computed and before its optimiser step, and ends the update at the first one above 1.5 * target_kl.  Here the decision is
 * taken inside the launch: every policy workgroup's KL sum rides on the gradient-norm exchange (one tagged word per workgroup, in the
 * per-call zeroed region of the workspace; no further wait round), every workgroup of both networks adds the words in part order,
 * scales by 1 / batch_size and compares in float32 with kl_stop = (float)(1.5 * (double)target_kl) -- the same bits, so the same
 * verdict, everywhere.  With the stop at minibatch m (0-based):
 *   params, mom_m, mom_v   the plain call's over minibatches 0 .. m - 1 (m Adam steps from hyper->step0), bit for bit; m = 0: untouched;
 *   loss_acc               += the plain call's sums over minibatches 0 .. m: the stopping minibatch's losses count (SB3 books them);
 *   *minibatches_stepped   m.  Without a stop: n_minibatches, and everything as the plain call leaves it.
 *   diag                   may be NULL here (then nothing is written; diag_floats is ignored).  Otherwise as fw_ppo_update_diag for
 *                          minibatches 0 .. m; the rows of later minibatches stay as the caller zeroed them.
 * minibatches_stepped is a DEVICE pointer to one int32, written once by the workgroup that writes the closing verdict; it is valid
 * after fw_ppo_update_status reported 0, like everything else: a non-zero status leaves all outputs undefined, as above.
 * target_kl <= 0 or not finite, a NULL minibatches_stepped, an act_dim other than 3, 4, 6: FW_EINVAL, nothing runs.  The workspace is
 * that of the width's own size function; the status word, the closing verdict and the FWSIM_PPO_* / FWSIM_SPIN_LOG2 switches are
 * those of the plain entry points, which themselves take and refuse exactly what they did. */
int32_t fw_ppo_update_kl(float* params, float* mom_m, float* mom_v, const float* obs, const float* act,
                         const float* old_logp, const float* adv, const float* ret, const int32_t* perm,
                         int32_t n_minibatches, int32_t batch_size, int32_t obs_dim, int32_t act_dim, const fw_ppo_hyper* hyper,
                         float* loss_acc, void* workspace, int64_t workspace_bytes, void* hip_stream,
                         float* diag /* may be NULL */, int64_t diag_floats, float target_kl,
                         int32_t* minibatches_stepped /* device, one int32 */);

/* Rollout collection between two env steps (SB3 OnPolicyAlgorithm.collect_rollouts + VecNormalize reward path,
 * train/train_Fixedwing_Waypoints_v3.py:260,293-310), for the same MlpPolicy / flat parameter image as fw_ppo_update.
 * fw_policy_act: obs[N,obs_dim] (normalised, float32) -> for `nets` bit 0 (policy): act_raw[N,4] = mean + sigma * z
 *   (z ~ N(0,1) from Philox(rng[0] = seed; rng[1] = draw counter, global env id = env_offset + row); mean if
 *   `deterministic`), logp[N], act_env[N,4] = clip(act_raw, +-1) in the env dtype (the fw_step input), and obs copied to
 *   obs_copy (rollout buffer, may be NULL); for bit 1 (value): value[N].
 * fw_rollout_post: VecNormalize.step_wait's reward path + the bootstrap of truncated episodes:
 *   returns = returns * gamma + reward; running variance of `returns` (if training && norm_reward);
 *   rew_out = clip(reward / sqrt(var + epsilon), +-clip_reward) (+ gamma * tvalue where truncated && !terminated);
 *   start_out = terminated | truncated; returns = 0 where done; rng[1] += 1 (rng may be NULL);
 *   ret_acc (may be NULL): device double[3], the tracker batch's (sum, sum of squares, count) are added to it (the
 *   reward-side twin of fw_normalize_obs's batch_acc). */
int32_t fw_policy_act(const float* params, const float* obs, int32_t N, int32_t obs_dim, int32_t nets, int32_t deterministic,
                      const uint64_t* rng, int64_t env_offset, float* obs_copy, float* act_raw, void* act_env,
                      int32_t act_is_f64, float* logp, float* value, void* hip_stream);
/* V(normalised terminal_observation) for the envs whose episode was truncated but not terminated (the only ones SB3
 * bootstraps): terminal_obs[N,obs_dim] is the env's raw buffer (fw_step's terminal_obs), normalised on load with
 * (mean, var, clip, eps) exactly like fw_normalize_obs; value[i] is written for every row of a 64-row block that
 * contains such an env and left untouched elsewhere. */
int32_t fw_policy_terminal_value(const float* params, const void* terminal_obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim,
                                 const double* mean, const double* var, float clip, float eps, const uint8_t* terminated,
                                 const uint8_t* truncated, float* value, void* hip_stream);
int32_t fw_rollout_post(const void* reward, int32_t rew_is_f64, const uint8_t* terminated, const uint8_t* truncated,
                        const float* tvalue, double* returns, double* ret_mean, double* ret_var, double* ret_count,
                        int32_t N, int32_t training, int32_t norm_reward, double gamma, float clip_reward, float epsilon,
                        float* rew_out, float* start_out, uint64_t* rng, double* ret_acc, void* hip_stream);

/* The same collection in THREE launches per vec-step (fw_collect_act -> fw_step -> fw_collect_stats) instead of seven:
 * fw_collect_act  = fw_policy_act reading the env's RAW observation buffer and normalising it on load with (obs_mean, obs_var,
 *   clip_obs, eps_obs) -- the normalised rows still go to obs_copy -- whose value block also FINALISES THE PREVIOUS STEP for its
 *   rows when prev_reward != NULL: rew_out = clip(prev_reward / sqrt(ret_var + eps_reward), +-clip_reward) (if norm_reward)
 *   + gamma * V(normalised prev_terminal_obs) where prev_truncated && !prev_terminated (a second pass through the value network in
 *   the blocks that hold such a row), start_out = prev_terminated | prev_truncated.  It runs BEFORE the next fw_step, while the
 *   env's reward / flag / terminal-observation buffers still hold the previous step.
 * fw_collect_stats = VecNormalize.step_wait's statistics after an env step, one launch: observation moments -> (obs_mean, obs_var,
 *   obs_count) if update_obs; returns = returns * gamma + reward, their moments -> (ret_mean, ret_var, ret_count) if update_ret,
 *   returns = 0 where the episode ended; rng[1] += 1 (rng may be NULL); obs_acc / ret_acc as batch_acc / ret_acc above.
 *   workspace: caller-owned, fw_collect_stats_workspace_bytes(D) bytes, zero-initialised once. */
int32_t fw_collect_act(const float* params, const void* raw_obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim, const double* obs_mean,
                       const double* obs_var, float clip_obs, float eps_obs, int32_t nets, int32_t deterministic, const uint64_t* rng,
                       int64_t env_offset, float* obs_copy, float* act_raw, void* act_env, int32_t act_is_f64, float* logp, float* value,
                       const void* prev_reward, const uint8_t* prev_terminated, const uint8_t* prev_truncated, const void* prev_terminal_obs,
                       const double* ret_var, int32_t norm_reward, float clip_reward, float eps_reward, float gamma, float* rew_out,
                       float* start_out, void* hip_stream);
/* fw_policy_act_a / fw_collect_act_a: the same for a flat image of the act_dim layout above (act_dim 4: exactly fw_policy_act /
 * fw_collect_act; 6: act_raw and act_env are [N, 6]).  Sampling with six actions: components 0-3 are the four-action draw bit for bit,
 * components 4, 5 come from a second Philox4x32-10 block of the same key (seed) and counter except bit 31 of counter word 3, through
 * the same Box-Muller map.  fw_collect_step / fw_collect_close stay four-action: they refuse the low-level task's handle. */
int32_t fw_policy_act_a(const float* params, const float* obs, int32_t N, int32_t obs_dim, int32_t act_dim, int32_t nets, int32_t deterministic,
                        const uint64_t* rng, int64_t env_offset, float* obs_copy, float* act_raw, void* act_env,
                        int32_t act_is_f64, float* logp, float* value, void* hip_stream);
int32_t fw_collect_act_a(const float* params, const void* raw_obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim, int32_t act_dim,
                         const double* obs_mean, const double* obs_var, float clip_obs, float eps_obs, int32_t nets, int32_t deterministic,
                         const uint64_t* rng, int64_t env_offset, float* obs_copy, float* act_raw, void* act_env, int32_t act_is_f64, float* logp,
                         float* value, const void* prev_reward, const uint8_t* prev_terminated, const uint8_t* prev_truncated,
                         const void* prev_terminal_obs, const double* ret_var, int32_t norm_reward, float clip_reward, float eps_reward,
                         float gamma, float* rew_out, float* start_out, void* hip_stream);
/* The act side of a collected vec-step of the HIGH-LEVEL COMMAND task in one launch (instead of fw_collect_act for the commander,
 * fw_command_hl, fw_collect_act_a for the controller); a collected vec-step is fw_collect_act_hl -> fw_step -> fw_collect_stats.
 * `h`: a FW_TASK_WAYPOINTS_DIRECT handle with the euler attitude (fw_command_hl's rule: FW_EUNSUPPORTED otherwise), either dtype,
 * either lane mapping; N = fw_num_envs(h), the env dtype T = the handle's.  Grid (ceil(N / 64), 2):
 *   value block  (nets bit 1): what fw_collect_act's value block does with the three-action flat image `params`
 *     (fw_ppo_param_count_a3(30) floats): value[N] = V(normalised obs), and -- when prev_reward != NULL -- the finalisation of the
 *     previous step (rew_out, start_out; see fw_collect_act);
 *   policy block (nets bit 0): obs (the env's raw buffer, T[N, 30]) normalised on load with (obs_mean, obs_var, clip_obs, eps_obs) ->
 *     obs_copy (may be NULL); the commander 30 -> 64 -> 64 -> 3; act_raw[N, 3] = mean + exp(log_std) z with z = components 0-2 of the
 *     four-action draw for (rng[0] = seed, rng[1] = draw counter, env_offset + row) (mean if `deterministic`), logp[N]; then
 *     fw_command_hl's arithmetic on the float32 act_raw row: the conditioned command -> the env's FW_SL_TARGET tail, cmd_out T[N, 3]
 *     and low_obs T[N, 21] = (obs[:, 0:18], command), a non-finite row keeping the stored command and counted into `rejected`
 *     (may be NULL); low_obs normalised with the controller's frozen (low_mean, low_var, low_clip, low_eps); the controller
 *     21 -> 64 -> 64 -> 6 of `low_params` (six-action flat image, fw_ppo_param_count_a(21, 6) floats), deterministic, clipped to
 *     [-1, 1] -> act_env T[N, 6], the fw_step input.
 * Given the same act_raw, cmd_out / low_obs / act_env / the tail / rejected are those of fw_command_hl + fw_collect_act_a bit for
 * bit, and obs_copy is fw_normalize_obs's.  nets = 2 is the closing call of a rollout (value and finalisation only).  No in-grid
 * wait, no host synchronisation: capturable.  A missing required pointer: FW_EINVAL. */
typedef struct fw_collect_hl_args {
  const float *params, *low_params;        /* the commander's and the controller's flat parameter images */
  const void* obs;                         /* T[N, 30]: the env's raw observation buffer */
  const double *obs_mean, *obs_var;        /* [30] VecNormalize statistics of the commander's observation */
  const double *low_mean, *low_var;        /* [21] the controller's frozen statistics */
  const uint64_t* rng;                     /* [2] seed, draw counter (only read; fw_collect_stats advances it) */
  int64_t env_offset;                      /* global env id of row 0 */
  float *obs_copy, *act_raw, *logp, *value;/* rollout-buffer rows of the step being acted */
  void *low_obs, *cmd_out, *act_env;       /* T[N, 21], T[N, 3], T[N, 6] */
  int32_t* rejected;                       /* [1] += rows with a non-finite action (may be NULL) */
  const void* prev_reward;                 /* the previous-step block of fw_collect_act (all NULL / 0: nothing to finalise) */
  const uint8_t *prev_terminated, *prev_truncated;
  const void* prev_terminal_obs;
  const double* ret_var;
  float *rew_out, *start_out;
  float clip_obs, eps_obs, low_clip, low_eps, clip_reward, eps_reward, gamma;
  int32_t nets, deterministic, norm_reward;
} fw_collect_hl_args;
int32_t fw_sizeof_collect_hl_args(void);   /* for bindings: the size of the structure this build was compiled with */
int32_t fw_collect_act_hl(fw_handle h, const fw_collect_hl_args* a, void* hip_stream);

/* The high-level command task with the frozen controller at the control rate (controller_hz = control_hz): ONE agent step of a
 * FW_TASK_WAYPOINTS_DIRECT handle with the euler attitude (anything else: FW_EUNSUPPORTED, fw_command_hl's rule) in which the
 * controller runs in front of every Aviary step of the agent step, inside the step kernel, instead of once per agent step in front
 * of fw_step.  There is no action input: the command in force is the env's FW_SL_TARGET tail, written by fw_command_hl /
 * fw_collect_act_hl (after an auto-reset: level flight at the start height and speed).  Per Aviary step the controller's raw row is
 * (columns 0:12 of the observation of the current rigid state, the six actuator commands last issued -- the tail's on the first
 * Aviary step, zeros after a reset -- and the command), normalised as fw_collect_act_a normalises (low_mean / low_var / low_clip /
 * low_eps, frozen); the policy net of the six-action flat image low_params (fw_ppo_param_count_a(21, 6) floats) gives the mean
 * action, clipped to [-1, 1]: fw_controller_forward's arithmetic, bit for bit.  Warm-up steps of an in-kernel reset and envs that
 * are done at entry run no controller.  The output buffers are fw_step's; low_action (T[N, 6], may be NULL) receives the
 * controller's output that was in force when the step ended.  The observation and the tail show the same six values (zeros after
 * an auto-reset).  No in-grid wait, no host synchronisation: capturable.  A missing required pointer: FW_EINVAL. */
typedef struct fw_step_hl_args {
  const float* low_params;                 /* the controller's flat parameter image */
  const double *low_mean, *low_var;        /* [21] its frozen observation statistics */
  void *obs, *reward;                      /* the output buffers of fw_step */
  uint8_t *terminated, *truncated;
  void* terminal_obs;                      /* may be NULL */
  int32_t* info_i32;                       /* may be NULL */
  void* low_action;                        /* T[N, 6], may be NULL */
  float low_clip, low_eps;
} fw_step_hl_args;
int32_t fw_sizeof_step_hl_args(void);      /* for bindings: the size of the structure this build was compiled with */
int32_t fw_step_hl(fw_handle h, const fw_step_hl_args* a, void* hip_stream);
/* The controller as fw_step_hl's kernel computes it, on raw rows [N, 21] (float64 or float32), one thread per env:
 * act_out[i] (float64 or float32 [N, 6]) = clip(policy_net(clip((raw_obs[i] - mean) / sqrt(var + eps), +-clip)), +-1). */
int32_t fw_controller_forward(const float* params, const void* raw_obs, int32_t obs_is_f64, int32_t N, const double* mean, const double* var,
                              float clip, float eps, void* act_out, int32_t act_is_f64, void* hip_stream);
int64_t fw_collect_stats_workspace_bytes(int32_t D);
int32_t fw_collect_stats(const void* obs, int32_t obs_is_f64, int32_t N, int32_t D, double* obs_mean, double* obs_var, double* obs_count,
                         int32_t update_obs, const void* reward, int32_t rew_is_f64, const uint8_t* terminated, const uint8_t* truncated,
                         double* returns, double* ret_mean, double* ret_var, double* ret_count, int32_t update_ret, double gamma,
                         uint64_t* rng, void* workspace, double* obs_acc, double* ret_acc, void* hip_stream);

/* The same collection in ONE launch per vec-step: the policy / value forward of step t (fw_collect_act's work, by "act waves" at
 * the front of the grid), the env step (fw_step's waves, which wait for their actions inside the launch) and the statistics
 * of VecNormalize.step_wait.  Semantics and arithmetic are those of fw_collect_act -> fw_step -> fw_collect_stats called with the
 * same buffers (statistics to ~1e-12: another summation order; normalised observations within an ulp of double before the
 * float32 rounding): `obs`, `reward`, `terminated`, `truncated`, `terminal_obs` hold the PREVIOUS step on entry (obs = the
 * observation to act on) and this step on return; rew_out / start_out (both or neither) receive the finalisation of the
 * previous step.  The batch sums of a step are folded by "fold waves" at the end of its own launch and merged into the
 * statistics buffers by the NEXT fw_collect_step (which needs them first) -- or by fw_collect_finish: call it after the last
 * step of a rollout, before anything else reads (obs_mean, obs_var, obs_count) / the return statistics.  Serves handles on the 8-lanes-per-env mapping, either build (FW_EUNSUPPORTED
 * otherwise -- one lane per env, i.e. beyond 24 576 waypoint envs per GPU: use the three calls).  workspace: caller-owned, fw_collect_step_workspace_bytes(h) bytes, one per handle, prepared ONCE with
 * fw_collect_workspace_init (stream-ordered; not inside a graph that is replayed).
 * Failure inside a launch: the waves of the grid wait for waves in front of them (step waves for their actions, fold waves for
 * the partial sums, the merge wave for the act waves), every wait bounded.  A wait that runs out does not stop the launch --
 * the wave goes on with what it has (zero actions, partial sums, an early commit) -- but raises FW_COLLECT_ST_* in the
 * workspace's status word, the uint32 at (fw_collect_step_workspace_bytes(h) - 64 + 12); the word is sticky until
 * fw_collect_workspace_init.  Non-zero means: everything collected since the last zero reading is void.  Read it at least once
 * per rollout -- fw_collect_status (synchronises `hip_stream`) or a copy of that word; rollout.PPO raises RuntimeError.
 * FWSIM_SPIN_LOG2=k (environment, read per call) shrinks the budgets to 2^k polls: tests provoke the timeouts with it. */
#define FW_COLLECT_ST_ACTIONS 1u  /* a step wave gave up waiting for its actions (it stepped with zeros) */
#define FW_COLLECT_ST_FOLD 2u     /* a fold wave summed without every partial, or never saw the merge wave finish */
#define FW_COLLECT_ST_MERGE 4u    /* the merge wave committed the statistics before every act wave had read the old ones */
#define FW_COLLECT_ST_NOINIT 8u   /* the workspace was never passed to fw_collect_workspace_init */
#define FW_COLLECT_ST_EPOCH 16u   /* the merge wave never saw the launch's index published */
#define FW_COLLECT_ST_NANACT 32u  /* the policy produced a NaN action (diverged weights or statistics): the env stepped with -1 in its place */
typedef struct fw_collect_args {
  const float* params;                     /* flat parameter image (fw_ppo_update layout) */
  double *obs_mean, *obs_var, *obs_count;  /* VecNormalize observation statistics (in/out) */
  double *returns;                         /* [N] discounted-return tracker (in/out) */
  double *ret_mean, *ret_var, *ret_count;  /* its running statistics (in/out) */
  double *obs_acc, *ret_acc;               /* sharded jobs: batch-sum accumulators (may be NULL) */
  uint64_t* rng;                           /* [2] seed, draw counter (advanced by one) */
  float *obs_copy, *act_raw, *logp, *value;/* rollout-buffer rows of the step being acted (obs_copy may be NULL) */
  void* act_env;                           /* T[N,4] the clipped actions the envs step with (scratch owned by the caller, one per handle;
                                            * between launches every word is NaN = "not there yet": the library fills a new buffer itself) */
  float *rew_out, *start_out;              /* finalisation of the previous step: both or neither */
  void *obs, *reward;                      /* env buffers, as fw_step (in: previous step, out: this step) */
  uint8_t *terminated, *truncated;
  void* terminal_obs;
  int32_t* info_i32;                       /* may be NULL */
  void* workspace; int64_t workspace_bytes;
  void* trace;                             /* NULL, or device int64[(grid size) * 8]: per-workgroup wall-clock stamps (diagnostic, tools/trace_collect.py) */
  double gamma;
  float clip_obs, eps_obs, clip_reward, eps_reward;
  int32_t update_obs, update_ret, norm_reward, deterministic;
} fw_collect_args;
int64_t fw_collect_step_workspace_bytes(fw_handle h);
int32_t fw_collect_workspace_init(fw_handle h, void* workspace, int64_t workspace_bytes, void* hip_stream);
int32_t fw_collect_step(fw_handle h, const fw_collect_args* a, void* hip_stream);
int32_t fw_collect_finish(fw_handle h, const fw_collect_args* a, void* hip_stream);   /* statistics buffers, flags and workspace of `a` only */
int32_t fw_collect_status(fw_handle h, const void* workspace, int64_t workspace_bytes, uint32_t* status_out, void* hip_stream);
/* The end of a rollout of T fw_collect_step launches in ONE more launch instead of fw_collect_finish + a value forward + a
 * normalisation + fw_gae: merges the last step's statistics; V(final observation) -> a->value [N] (SB3's last values); the
 * normalised final observation -> a->obs_copy (may be NULL); finalises step T - 1 (a->rew_out = row T - 1 of `rewards`,
 * a->start_out = the episode starts after the last step: fw_gae's last_dones); then SB3's
 * RolloutBuffer.compute_returns_and_advantage over the [T, N] float32 buffers (fw_gae's arithmetic, each value wave for its
 * own rows).  `a` as for fw_collect_step (obs / reward / terminated / truncated / terminal_obs = the outputs of the last
 * step; the policy-side buffers are not used). */
typedef struct fw_collect_close_args {
  const float *rewards, *values, *episode_starts;   /* [T, N] rollout buffers */
  float *adv, *ret;                                  /* [T, N] out */
  int32_t T;
  float gae_gamma, gae_lambda;
} fw_collect_close_args;
int32_t fw_collect_close(fw_handle h, const fw_collect_args* a, const fw_collect_close_args* c, void* hip_stream);

int32_t fw_num_envs(fw_handle h);
/* Lane mapping of this handle's step kernels: 8 = eight lanes of a wavefront share one env (latency mapping, one wave per SIMD),
 * 16 = the same mapping built for two waves per SIMD (256 registers), 1 = one lane per env (throughput mapping); chosen by
 * fw_create from the env count.  Diagnostic; results do not depend on it. */
int32_t fw_lanes_per_env(fw_handle h);
/* 1 when this handle's fw_step workgroups carry a capture wave (camera tasks on the 8-lane mapping, opt-in: environment variable
 * FWSIM_CAPTURE_WAVE=1 at fw_create; csrc/fwsim_objlock.hpp "The capture wave"), else 0.  Diagnostic; results agree with the
 * one-wave kernel to rounding. */
int32_t fw_capture_wave(fw_handle h);
/* 1 when this handle's fw_step runs the axis-aligned variant of the physics tick (f64 wind-free waypoints on the one-wave 8-lane
 * build, every surface with forward = e_x and lift = e_y or e_z, diagonal inertia), else 0.  Diagnostic; results are bit-identical
 * to the general tick. */
int32_t fw_axis_aligned(fw_handle h);
/* 1 when this handle's fw_step workgroups carry a noise wave (the axis-aligned kernel with motor noise on and step_ratio <= 8, up to
 * 4096 envs: a second wave per workgroup draws the launch's motor noise while the step wave is in its prologue; environment variable
 * FWSIM_AUX_WAVE=0|1 at fw_create overrides where that kernel applies), else 0.  Diagnostic; results are bit-identical to the
 * one-wave kernel. */
int32_t fw_aux_wave(fw_handle h);
/* 1 when this handle's fw_step runs the noise-wave kernel compiled for the shape of the headline training config (30 Hz agent steps
 * of four 2-tick control steps, 2 of 8 waypoints in a 28-word euler observation, sparse reward, motor noise, gyroscopic term: those
 * integers are constants of the kernel instead of loads; environment variable FWSIM_STEP_SHAPE=0 at fw_create turns it off, no value
 * turns it on for another config), else 0.  Diagnostic; results are bit-identical to the noise-wave kernel. */
int32_t fw_step_shape(fw_handle h);
/* 1 when this handle's fw_step runs the fixed-shape kernel whose second wave stays to the end of the launch (behind the noise draw it
 * pre-samples the next episodes' waypoints for its own tile -- the grid has no worker workgroups -- and then writes the observation
 * rows, the terminal observations among them, while the step wave stores state and counters; up to 4096 envs; environment variable
 * FWSIM_OBS_WAVE=0|1 at fw_create overrides where fw_step_shape is 1; default on), else 0.  Diagnostic; results are bit-identical. */
int32_t fw_obs_wave(fw_handle h);
/* TEST HOOK, not used by the product: evaluates ONE device building block (a __device__ function of csrc/fwsim_device.hpp, called,
 * not copied) on n rows.  `in` [n, in_cols] and `out` [n, out_cols] are DEVICE buffers of doubles; the constants (Params / TickC /
 * SurfC as fw_create folded them) and the dtype are the handle's: a row is converted to the handle's dtype inside the kernel and
 * the results are widened back.  Rows map to lanes one to one, or (8-lane forms, marked "group") to groups of 8 consecutive lanes
 * that all get the row's inputs.  Stream-ordered, no host synchronisation.  An unknown op / variant, a NULL pointer, n <= 0 or
 * n > 2^24, or column counts other than the table's: FW_EINVAL; a variant this handle has no kernel for: FW_EUNSUPPORTED.
 *
 *   op          variant              in columns                                    out columns
 *   MATH1       0                    x                                             rcp, sqrt, sin, sincos.s, sincos.c, asin, log
 *   MATH2       0                    a, b                                          div(a, b), atan2(a, b)
 *   ROT         0                    q[4], d                                       rot_from_quat[9], rot_from_unit_quat[9], normalize_quat[4], two_over_norm2(d)
 *   EULER       LANE | LANES8(group) q[4]                                          euler[3], gimbal guard taken (0 | 1); LANES8: per lane, [8][4]
 *               INVERSE              euler[3]                                      quat_from_euler[4]
 *   QUAT_STEP   0                    w[3], q[4]                                    quat_integrate: q[4] after one physics tick
 *   SURFACE     SCALAR | REGS(group) surface, actuation, v_b[3], w_b[3], wind_b[3] force[3], torque about the COM[3]
 *               | LDS(group) | AX(group: float64 and an axis-aligned airframe only)
 *   GROUP       0 (group)            v[8], b[8]: one of each per lane              per lane [10]: group_sum v, group_min v, group_or (uint32) b,
 *                                                                                  group_any (b odd), lane_pick5 of v[0..4], act[0..4] after
 *                                                                                  lane_act_scatter, + 1000 * lane, lane_act_gather
 *   RNG         PHILOX               counter[4], key[2]  (uint32 values)           philox4x32_10[4]
 *               UNIFORM              env, episode, j, lo, hi                       rng_uniform (the handle's seed, scenario stream)
 *               NORMAL2              a.hi, a.lo, b.hi, b.lo  (uint32 values)       the two normals of the Box-Muller half of rng_normal2
 *   WIND        0                    base[3], amp[3], phase, tick, k (0..64)       gust_init(tick) + k x gust_advance + wind_from_phase [3], wind_at(tick + k) [3]
 */
enum {
  FW_PROBE_MATH1 = 0, FW_PROBE_MATH2 = 1, FW_PROBE_ROT = 2, FW_PROBE_EULER = 3, FW_PROBE_QUAT_STEP = 4, FW_PROBE_SURFACE = 5,
  FW_PROBE_GROUP = 6, FW_PROBE_RNG = 7, FW_PROBE_WIND = 8
};
enum { FW_PROBE_EULER_LANE = 0, FW_PROBE_EULER_LANES8 = 1, FW_PROBE_EULER_INVERSE = 2 };
enum { FW_PROBE_SURFACE_SCALAR = 0, FW_PROBE_SURFACE_REGS = 1, FW_PROBE_SURFACE_LDS = 2, FW_PROBE_SURFACE_AX = 3 };
enum { FW_PROBE_RNG_PHILOX = 0, FW_PROBE_RNG_UNIFORM = 1, FW_PROBE_RNG_NORMAL2 = 2 };
int32_t fw_probe(fw_handle h, int32_t op, int32_t variant, const double* in, int32_t in_cols, double* out, int32_t out_cols,
                 int32_t n, void* hip_stream);
/* ---- Soft actor-critic for the low-level task (csrc/fwsim_sac.hpp; SB3 `SAC("MlpPolicy")`, one gradient step of `SAC.train()`) ----
 * ReLU MLPs in fp32: the actor obs_dim -> hidden -> hidden -> 2 act_dim (mean | log_std, clamped to [-20, 2]), two critics and their two
 * targets (obs_dim + act_dim) -> hidden -> hidden -> 1.  Built for obs_dim <= 64, act_dim <= 8, hidden 64 or 256 and batches that are
 * multiples of 16 in [16, 512] or multiples of 64 in (512, 8192] (the wide form of the gradient step, below): anything else
 * FW_EUNSUPPORTED; NULL pointers and non-positive sizes FW_EINVAL.  No handle: every
 * buffer is a device buffer of the caller, everything is stream-ordered, nothing allocates, synchronises or reads device state on the
 * host, so all five entry points can be captured into a graph.
 *
 * Flat image (floats, fw_sac_param_count of them), W[in][out] = torch Linear.weight^T:
 *   actor | q1 | q2 | log_ent_coef | q1 target | q2 target | exp_avg[T] | exp_avg_sq[T] | tail[4]
 *   one network: W1[in][hidden] b1 W2[hidden][hidden] b2 W3[hidden][out] b3;  T = actor + 2 critics + 1;  tail[0] = Adam step count (int32).
 * Device counters (int64[4]): [0] ring cursor (rows), [1] rows filled, [2] vec-steps stored, [3] gradient steps.
 * Ring / batch rows (floats): obs[obs_dim] | action[act_dim] | reward | next_obs[obs_dim] | done. */
typedef struct fw_sac_hyper {
  float lr, gamma, tau, beta1, beta2, eps, target_entropy, ent_coef;   /* ent_coef: the fixed coefficient when auto_ent == 0 */
  int32_t auto_ent, target_update_interval;   /* Polyak when the Adam step count after the step is a multiple of the interval */
  uint64_t seed;                              /* of the step's noise (fw_sac_noise's) */
} fw_sac_hyper;
int32_t fw_sizeof_sac_hyper(void);
int32_t fw_sac_param_count(int32_t obs_dim, int32_t act_dim, int32_t hidden);
int64_t fw_sac_update_workspace_bytes(int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t batch);
/* One launch per vec-step: the actor on obs [N, obs_dim] (the env's dtype, read as fp32), eps from Philox keyed by (seed, env_offset +
 * row, counters[2]), action = tanh(mean + exp(log_std) eps) (mode 0), tanh(mean) (mode 1) or uniform in [-1, 1) without a forward
 * (mode 2, SB3's learning_starts).  Writes the action as fp32 (act_f32) and in the env's dtype (act_env, fw_step's input), the fp32
 * copy of obs (obs_stage: the step overwrites the env's buffer) and, where non-NULL, logp [N] and eps [N, act_dim]. */
int32_t fw_sac_act(const float* image, const void* obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t mode,
                   uint64_t seed, int64_t env_offset, const int64_t* counters, float* act_f32, void* act_env, float* obs_stage, float* logp,
                   float* eps, void* hip_stream);
/* After fw_step: appends N rows at counters[0] of the ring (capacity rows, a multiple of N): next_obs is terminal_obs where the episode
 * ended and the new obs otherwise, done is `terminated` alone (a pure time-limit end bootstraps).  A closing one-lane launch advances
 * cursor, fill and step counter. */
int32_t fw_replay_store(float* ring, int64_t capacity, int64_t* counters, const float* obs_stage, const float* act_f32, const void* reward,
                        const void* next_obs, const void* terminal_obs, const uint8_t* terminated, const uint8_t* truncated, int32_t env_is_f64,
                        int32_t N, int32_t obs_dim, int32_t act_dim, void* hip_stream);
/* `batch` uniform row indices in [0, counters[1]) from Philox keyed by (seed, counters[3]); gathers the rows into out [batch, row_floats]
 * and writes the indices to idx_out (optional).  Any positive batch: the batch rule above is fw_sac_update's and its workspace's. */
int32_t fw_replay_sample(const float* ring, int64_t capacity, const int64_t* counters, uint64_t seed, int32_t row_floats, int32_t batch,
                         float* out, int32_t* idx_out, void* hip_stream);
/* n-step returns.  ends: a caller-owned uint8[capacity] side ring, bit 0 = terminated, bit 1 = truncated of the row's step (the row's own
 * done column is `terminated` alone).  fw_replay_mark_ends writes ends[cursor + i], i < N, for the rows the NEXT fw_replay_store will
 * write: launch it in front of that call on the same stream.  It reads counters[0] (normalised as the store does) and writes no counter. */
int32_t fw_replay_mark_ends(uint8_t* ends, int64_t capacity, const int64_t* counters, const uint8_t* terminated, const uint8_t* truncated, int32_t N,
                            void* hip_stream);
/* fw_replay_sample with an n-step target.  The start index i of batch row b is fw_replay_sample's draw (equal counters: equal idx_out).
 * Env e's steps are N rows apart: row_j = (i + j N) mod capacity, j = 0, 1, ...; row_j is used, and the walk stops behind it when
 * j + 1 == n_steps, or ends[row_j] != 0, or row_j lies in the newest vec-step stored (the next row would be the oldest data or an
 * unfilled row).  With k rows used and g_0 = 1, g_j = g_(j-1) gamma (fp32) the output row, in fw_replay_sample's layout, is
 *   obs | action from row_0,  reward = r_0 + g_1 r_1 + ... + g_(k-1) r_(k-1) (fp32, ascending j, one fma per term),  next_obs from
 *   row_(k-1),  last column = 1 - (1 - done_(k-1)) g_(k-1):
 * fw_sac_update's (1 - last) gamma is then (1 - done) gamma^k, and for k = 1 the row is fw_replay_sample's bit for bit.  k_out
 * (optional) [batch] receives k.  obs_dim locates the reward column (row_floats = 2 obs_dim + act_dim + 2).  n_steps in [1, 16]
 * (FW_EUNSUPPORTED otherwise).  Reads counters only; every row index is taken mod capacity, so an empty ring is not read out of bounds
 * (its result is unspecified, as fw_replay_sample's). */
int32_t fw_replay_sample_nstep(const float* ring, int64_t capacity, const int64_t* counters, uint64_t seed, int32_t row_floats, int32_t batch,
                               float* out, int32_t* idx_out, const uint8_t* ends, int32_t obs_dim, int32_t N, int32_t n_steps, float gamma,
                               int32_t* k_out, void* hip_stream);
/* Hindsight goal relabelling (SB3's HerReplayBuffer, "future" strategy) for the low-level task, whose goal (psi_ref, h_ref, V_ref) is
 * obs[18:21] and whose reward is a closed function of the post-step observation and that goal.  Built for obs_dim 21 and row_floats 50
 * (Euler attitude): anything else FW_EUNSUPPORTED. */
typedef struct fw_her_task {      /* the low-level task's reward, the part the relabelled goal changes */
  int32_t variant;                /* 0: fixedwing_lowlevel_env.py   1: FW_LL_VARIANT_SAC_DEMO */
  float dome, min_speed;          /* variant 1 only: flight_dome_size, lowlevel_min_speed */
} fw_her_task;
int32_t fw_sizeof_her_task(void);
/* fw_replay_sample with relabelled goals.  The start index i of batch row b is fw_replay_sample's draw (equal counters: equal idx_out).
 * A second Philox block, counter words (b, 0, gs, gs >> 32 ^ 0x5AC0E000) under the same key, gives o[0] and o[1].  The row is relabelled
 * iff (uint64)o[0] < (uint64)((double)relabel_prob 2^32): 0 never, 1 always.  A row that is not relabelled is the ring row, bit for bit.
 * Candidates: row_j = (i + j N) mod capacity, j < horizon; row_j is used, and the walk stops behind it when j + 1 == horizon, or
 * ends[row_j] != 0, or row_j lies in the newest vec-step stored -- fw_replay_sample_nstep's rule.  With k rows used, j* = umulhi(o[1], k)
 * in [0, k - 1] (0: the goal this very transition achieved) and the achieved goal g' = (next_obs[5], next_obs[11], |next_obs[6:9]|) of
 * row_j*, the norm in double from the fp32 values, rounded to fp32.  Output row, in fw_replay_sample's layout: obs[0:18], action,
 * next_obs[0:18] and the last column of row_0 bit for bit; obs[18:21] = next_obs[18:21] = g'; reward = the task's reward for
 * (next_obs[0:18] of row_0, g', done of row_0), in double, rounded once to fp32; the airspeed it reads is the achieved one as above
 * (rounded to fp32), so with j* = 0 the tracking errors are exactly 0.  done stays what it was.  j_out (optional) [batch]: -1 where the row
 * was not relabelled, else j*.  horizon in [1, 64] (FW_EUNSUPPORTED otherwise); relabel_prob outside [0, 1] or a variant other than
 * 0 / 1: FW_EINVAL.  Reads counters only, no atomics; every row index is taken mod capacity. */
int32_t fw_replay_sample_her(const float* ring, int64_t capacity, const int64_t* counters, uint64_t seed, int32_t row_floats, int32_t batch,
                             float* out, int32_t* idx_out, const uint8_t* ends, int32_t obs_dim, int32_t N, int32_t horizon, float relabel_prob,
                             const fw_her_task* task, int32_t* j_out, void* hip_stream);
/* The same reward on caller-given goals [batch, 3]: reward_out[b] for (next_obs[0:18] of rows[b], goals[b], done of rows[b]). */
int32_t fw_her_reward(const float* rows, int32_t row_floats, int32_t batch, int32_t obs_dim, const float* goals, const fw_her_task* task,
                      float* reward_out, void* hip_stream);
/* eps and eps' [2][batch][act_dim] of gradient step counters[3]: the values fw_sac_update draws inside.  A row's noise does not
 * depend on the batch size.  Any positive batch, as fw_replay_sample. */
int32_t fw_sac_noise(uint64_t seed, const int64_t* counters, int32_t batch, int32_t act_dim, float* out, void* hip_stream);
/* One gradient step on the image from batch_rows [batch, 2 obs_dim + act_dim + 2]: a fixed sequence of 24 launches, kernel boundaries
 * the only synchronisation between workgroups, every weight gradient summed over the batch by one workgroup in a fixed order (two runs
 * give the same bits).  out (optional) [5]: critic loss, actor loss, ent-coef loss, alpha (before the step), mean logp.  Increments
 * tail[0] and counters[3].
 * batch > 512 takes the wide form, 29 launches: the stages that sum over the batch run one workgroup per 256 rows and a one-lane fold
 * adds their partial sums in ascending order; a weight gradient is split into chunks of 512 batch rows (one workgroup per tile and
 * chunk) and a second launch adds the chunks in ascending order and applies Adam.  The split depends on batch alone: two runs still
 * give the same bits.  fw_sac_update_workspace_bytes grows by the partial sums for these sizes only. */
int32_t fw_sac_update(float* image, const float* batch_rows, int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t batch, const fw_sac_hyper* hyper,
                      int64_t* counters, float* out, void* workspace, int64_t workspace_bytes, void* hip_stream);
/* ---- Prioritized experience replay on the ring (csrc/fwsim_per.hpp; Schaul et al. 2016, the proportional variant) ----
 * Caller-owned device state, all float32: prio [capacity], one leaf (|td| + eps)^alpha per ring row, 0 for a row never written;
 * sum1 / min1 [ceil(capacity / 256)], the sum and the smallest positive entry of 256 consecutive leaves; sum2 / min2
 * [ceil(len(sum1) / 256)], the same over sum1 / min1 (a min is +inf where nothing below it is positive); per_state [4]: [0] the
 * running max leaf (the caller initialises it, 1.0), [1] the total, [2] the smallest positive leaf, [3] spare.  capacity above 2^22
 * rows (more than 64 level-2 entries; beyond it an fp32 sum stops resolving one leaf): FW_EUNSUPPORTED.  NULL pointers and
 * non-positive sizes FW_EINVAL.  Nothing allocates, synchronises or reads device state on the host: all five entry points can be
 * captured into a graph.
 * The order of a group of 256 entries x_0 .. x_255 (missing entries are 0), in fp32: p(4l) = x_(4l), p(4l + j) = p(4l + j - 1) +
 * x_(4l + j) for j = 1, 2, 3 (64 chains of four); E_0 = 0, E_(l+1) = E_l + p(4l + 3) (one chain of 64).  The running sum up to and
 * including entry 4l + j is S(4l + j) = E_l + p(4l + j), the group's sum is E_64, and the running sum in front of an entry is S of
 * the entry before it (0 in front of entry 0).  Both the rebuild and the draw use it, so two runs give the same bits.
 *
 * fw_replay_per_mark_new writes per_state[0] into the N leaves of the rows the NEXT fw_replay_store will write: launch it in front of
 * that call on the same stream.  It reads counters[0] (normalised as fw_replay_mark_ends does) and writes no counter. */
int32_t fw_replay_per_mark_new(float* prio, int64_t capacity, const int64_t* counters, const float* per_state, int32_t N, void* hip_stream);
/* Recomputes sum1 / min1, sum2 / min2, per_state[1] (the group sum of sum2) and per_state[2] from the leaves -- always from the leaves,
 * never incrementally, so nothing drifts.  Two launches, no in-grid wait, no atomics. */
int32_t fw_replay_per_rebuild(const float* prio, int64_t capacity, float* sum1, float* min1, float* sum2, float* min2, float* per_state,
                              void* hip_stream);
/* fw_replay_sample with a proportional draw.  Row b takes fw_replay_sample's Philox block (same counter words, same tag): u = (o[0] +
 * 0.5) 2^-32 in double, t = (float)(u (double)per_state[1]).  Descent through sum2, the chosen group of sum1, the chosen group of
 * prio: at each level the FIRST positive entry whose running sum S exceeds t; if rounding leaves none, the LAST positive entry of the
 * group; t becomes t - (the running sum in front of the entry).  With sums a rebuild wrote, the chosen row has a positive leaf and lies
 * below counters[1].  (A group with no positive entry -- sums that no rebuild followed, or an empty ring -- gives its entry 0: no index
 * leaves the ring and nothing is read out of bounds; the result is unspecified, as fw_replay_sample's on an empty ring.)  The row is
 * gathered as fw_replay_sample gathers it; idx_out [batch] (optional) receives it; w_out [batch] (optional) receives the importance
 * weight (per_state[2] / prio[row])^beta, which is (n P(row))^-beta divided by its maximum over the ring, as exp(beta log x) in fp32.
 * beta = beta_steps > 0 ? min(1, beta0 + (1 - beta0) counters[3] / beta_steps) : beta0, in fp32 on the device: the annealing lives
 * inside a captured graph.  beta0 outside [0, 1] or beta_steps < 0: FW_EINVAL.  One wave per batch row; reads counters only. */
int32_t fw_replay_sample_per(const float* ring, int64_t capacity, const int64_t* counters, uint64_t seed, int32_t row_floats, int32_t batch,
                             float* out, int32_t* idx_out, float* w_out, const float* prio, const float* sum1, const float* sum2,
                             const float* per_state, float beta0, int64_t beta_steps, void* hip_stream);
/* prio[idx[b]] = (|td[b]| + eps)^alpha (exp(alpha log x) in fp32) for the batch's rows; a row that occurs more than once receives the
 * LARGEST of its leaves, and per_state[0] becomes the max of itself and the batch's leaves.  Two launches: the touched leaves are
 * zeroed, then an integer max on the float bits goes through the vector memory path -- the result does not depend on execution order.
 * An idx outside [0, capacity) is skipped, and so is a td that is not finite (its leaf stays 0: the row is not drawn again).  alpha
 * outside [0, 1] or eps not positive: FW_EINVAL.  The sums are stale behind it: follow it with fw_replay_per_rebuild. */
int32_t fw_replay_per_update(float* prio, int64_t capacity, const int32_t* idx, const float* td, int32_t batch, float alpha, float eps,
                             float* per_state, void* hip_stream);
/* fw_sac_update with importance weights on the critic loss: the same launch sequence with ONE launch inserted behind the target stage
 * (25 launches up to 512 rows, 30 in the wide form).  It writes td_out[b] = (|Q1 - y| + |Q2 - y|) / 2 (optional; recovered from the
 * target stage's dL/dQ_i as |dL/dQ_i| batch) and scales dL/dQ_1 and dL/dQ_2 of row b by weights[b] [batch]: the critics train on
 * mean(w (Q_i - y)^2) / 2.  The actor and entropy losses are not weighted, and out[0] stays the unweighted critic loss.  With all
 * weights 1.0 the image holds fw_sac_update's bits.  Workspace and every other argument as fw_sac_update. */
int32_t fw_sac_update_weighted(float* image, const float* batch_rows, int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t batch,
                               const fw_sac_hyper* hyper, int64_t* counters, float* out, void* workspace, int64_t workspace_bytes,
                               const float* weights, float* td_out, void* hip_stream);
/* ---- Running observation / reward normalisation for the off-policy learner (SB3's VecNormalize with a replay buffer) ----
 * The ring keeps RAW rows; the statistics (fw_collect_stats writes them, behind the env step) are applied where a value is read.
 *
 * fw_sac_act_norm is fw_sac_act on clip((float)(((double)x - obs_mean[k]) / sqrt(obs_var[k] + (double)eps_obs)), +-clip_obs) -- the
 * arithmetic of fw_normalize_obs(update = 0), so its actions, logp and eps are those of fw_sac_act on that call's fp32 output, bit for
 * bit.  The observation is normalised as it is loaded in front of the forward pass (the obs_dim means and standard deviations are formed
 * once per workgroup); obs_stage still receives the RAW fp32 observation.  Mode 2 runs no forward pass and reads no statistics
 * (obs_mean / obs_var may be NULL there; in modes 0 and 1 a NULL one is FW_EINVAL). */
int32_t fw_sac_act_norm(const float* image, const void* obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim, int32_t act_dim, int32_t hidden,
                        int32_t mode, uint64_t seed, int64_t env_offset, const int64_t* counters, float* act_f32, void* act_env, float* obs_stage,
                        float* logp, float* eps, const double* obs_mean, const double* obs_var, float clip_obs, float eps_obs, void* hip_stream);
/* One launch, in place on a gathered batch [batch, 2 obs_dim + act_dim + 2] (behind any of the four samplers; hindsight rewards and
 * n-step sums are formed on raw values before it, so an n-step row's summed reward is scaled and clipped as one number).  With obs_mean
 * / obs_var [obs_dim]: the columns [0, obs_dim) and [obs_dim + act_dim + 1, 2 obs_dim + act_dim + 1) become the expression above.
 * With ret_var [1]: column obs_dim + act_dim becomes clip((float)((double)r / sqrt(ret_var[0] + (double)eps_reward)), +-clip_reward).
 * The action and done columns are not written.  obs_mean == NULL leaves the observations alone, ret_var == NULL the reward; both NULL,
 * or obs_mean without obs_var: FW_EINVAL.  Any positive batch; obs_dim <= 64 and act_dim <= 8 (FW_EUNSUPPORTED otherwise).  Every
 * element is written by one thread from its own old value: no atomics, no in-grid wait. */
int32_t fw_replay_normalize(float* batch_rows, int32_t batch, int32_t obs_dim, int32_t act_dim, const double* obs_mean, const double* obs_var,
                            float clip_obs, float eps_obs, const double* ret_var, float clip_reward, float eps_reward, void* hip_stream);
/* ---- TD3 for the low-level task (csrc/fwsim_td3.hpp; SB3 `TD3("MlpPolicy")`, one gradient step of `TD3.train()`) ----
 * ReLU MLPs in fp32: the actor obs_dim -> hidden -> hidden -> act_dim (tanh on its output), two critics (obs_dim + act_dim) -> hidden ->
 * hidden -> 1, and a target of each of the three.  Built for obs_dim <= 64, act_dim <= 8, hidden 64 or 256 and batches that are multiples
 * of 16 in [16, 512]: anything else FW_EUNSUPPORTED; NULL pointers and non-positive sizes FW_EINVAL.  No handle, caller-owned device
 * buffers, stream-ordered, nothing allocates, synchronises or reads device state on the host: both entry points can be captured into a
 * graph.  The replay ring, its counters, its rows and every sampler are the ones above.
 *
 * Flat image (floats, fw_td3_param_count of them), W[in][out] = torch Linear.weight^T, one network as in the SAC image:
 *   actor | q1 | q2 | actor target | q1 target | q2 target | exp_avg[T] | exp_avg_sq[T] | tail[4]
 *   T = actor + 2 critics (the moments cover the trained range actor | q1 | q2);  tail[0] = gradient steps taken, tail[1] = actor steps
 *   taken (int32): the critics' Adam bias correction counts the first, the actor's the second. */
typedef struct fw_td3_hyper {
  float lr, gamma, tau, beta1, beta2, eps;
  float policy_noise, noise_clip;             /* target policy smoothing: clamp(policy_noise eps, +-noise_clip) */
  uint64_t seed;                              /* of the smoothing noise (fw_sac_noise's first block) */
} fw_td3_hyper;
int32_t fw_sizeof_td3_hyper(void);
int32_t fw_td3_param_count(int32_t obs_dim, int32_t act_dim, int32_t hidden);
int64_t fw_td3_update_workspace_bytes(int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t batch);
/* fw_sac_act's launch for the deterministic actor, with its modes: 0 exploring, clamp(tanh(mean) + sigma eps, -1, 1) with eps keyed as
 * fw_sac_act keys it (seed, env_offset + row, counters[2]); 1 deterministic, tanh(mean); 2 uniform in [-1, 1) without a forward.  Writes
 * act_f32, act_env (the env's dtype), obs_stage (the fp32 copy of obs) and, where non-NULL, eps [N, act_dim] (the draw, also in mode 1;
 * zeros in mode 2).  sigma must be non-negative. */
int32_t fw_td3_act(const float* image, const void* obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t mode,
                   uint64_t seed, int64_t env_offset, const int64_t* counters, float* act_f32, void* act_env, float* obs_stage, float sigma,
                   float* eps, void* hip_stream);
/* One gradient step on the image from batch_rows [batch, 2 obs_dim + act_dim + 2]: a fixed launch sequence over the SAC product kernel.
 * The critics train on mse(Q1, y) + mse(Q2, y), y = r + (1 - last) gamma min(Q1t, Q2t)(s', a'), a' = clamp(tanh(actor_target(s')) +
 * clamp(policy_noise eps, +-noise_clip), -1, 1), eps = fw_sac_noise's first block at counters[3].  with_actor != 0 (the caller passes it on
 * every policy_delay-th step) adds the actor's step on -mean Q1(s, tanh(actor(s))) with the stepped critics and the Polyak step of all
 * three targets: 28 launches.  with_actor == 0: 13 launches; the actor, its moments, all three targets and tail[1] are not written.
 * out (optional) [2]: critic loss, actor loss (written with the actor part only).  Increments tail[0] and counters[3].  Every sum over
 * the batch runs in a fixed order: two runs give the same bits. */
int32_t fw_td3_update(float* image, const float* batch_rows, int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t batch, const fw_td3_hyper* hyper,
                      int32_t with_actor, int64_t* counters, float* out, void* workspace, int64_t workspace_bytes, void* hip_stream);
const char* fw_last_error(fw_handle h); /* h may be NULL: last create/validate error */
int32_t fw_destroy(fw_handle h);

#ifdef __cplusplus
}
#endif
#endif /* FWSIM_H */
