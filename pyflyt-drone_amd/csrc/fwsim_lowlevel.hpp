// ------------------------------------------------------------------------------------------
// FW_TASK_LOWLEVEL: the six actions are the actuator commands (mode -1, no mixer), one Aviary step (2 physics
// ticks) per agent step, a target (psi_ref, h_ref, V_ref) per episode.  There is no sub-step loop, no warm-up and no hand-off, so none
// of step_body's machinery applies: the task has a step and a reset kernel of its own, on the same inlined Aviary step.  The reset is
// inline (no warm-up, three draws): a wave that contains one runs ~50 more instructions per lane.
//
// One frame, two variants (config.lowlevel_variant, the template parameter V of both kernels):
//   FW_LL_VARIANT_TRACKING  envs/fixedwing_envs/fixedwing_lowlevel_env.py, the version train/train_lowlevel_cmd.py imports: tracking
//                           reward, termination on height, truncation on the step count.  Line numbers in its pieces are that file's.
//   FW_LL_VARIANT_SAC_DEMO  the FixedwingLowLevelEnv that the reference's examples/lowlevel.py defines for its SAC run ("SAC script's
//                           variant").  Line numbers in its pieces are examples/lowlevel.py's.
// The frame is written once: the lane roles, the state / tail / wind loads, the done-at-entry rule, the six actuator commands
// (surfaces a[0..4] as given, throttle 0.5 a[5] + 0.5), the one inlined Aviary step with the motor-noise keying of every task, the
// 21 observation columns (ll_write_obs), the target draw (ll_target on STREAM_LL_TARGET), the FW_SL_* state tail (ll_load_tail /
// ll_store_tail), the info words, the auto-reset, the final stores and the tile flush.  What the SAC script's variant does differently
// sits under `if constexpr (V == ...)` in the kernels, on the small pieces below:
//   * the action is clipped to [-1, 1] by the env (:121, lld_clip1);
//   * obs[12:18] and the reward's action term are the PREVIOUS step's clipped action -- the script assigns prev_action after it has
//     computed observation and reward (:127-133) -- zeros on an episode's first step;
//   * the reward (:157-185), termination on height or airspeed (:187-198), truncation on 1.2 x the dome radius or the clock (:200-208);
//   * psi_ref = 0 with lowlevel_fixed_heading (:109, lld_begin_episode), from the LldC block that only this variant reads.
// Start pose, speed and target ranges are config (config.lowlevel_demo_config).
//
// Included by fwsim.hip behind the generic step / reset kernels.
// ------------------------------------------------------------------------------------------
#pragma once

// (ll_wrap_pi, the heading wrap, is in fwsim_device.hpp: the evaluation's tracking sums use it too)
// the episode's target, drawn on a stream of its own keyed on (seed, global env, episode): :86-91
template <typename T> __device__ __forceinline__ void ll_target(const Params<T>& P, uint32_t genv, uint32_t ep, T tgt[3]) {
  const double k = 1.0 / 9007199254740992.0;
  const double u0 = (double)(rng_u64(P, genv, ep, STREAM_LL_TARGET, 0) >> 11) * k;
  const double u1 = (double)(rng_u64(P, genv, ep, STREAM_LL_TARGET, 1) >> 11) * k;
  const double u2 = (double)(rng_u64(P, genv, ep, STREAM_LL_TARGET, 2) >> 11) * k;
  tgt[0] = (T)(-kPi + (2.0 * kPi) * u0);
  tgt[1] = (T)(P.ll_height[0] + (P.ll_height[1] - P.ll_height[0]) * u1);
  tgt[2] = (T)(P.ll_speed[0] + (P.ll_speed[1] - P.ll_speed[0]) * u2);
}
// Aviary.reset() + reset() (:73-95): start pose and velocity, zero actuators, no warm-up; the wind of the episode; the target
template <typename T, int G>
__device__ __forceinline__ void ll_begin_episode(const Params<T>& P, const DevState<T>& D, int env, int32_t episode, Rigid<T>& S,
                                                 int32_t& tick, T tgt[3], T wb[3], T wa[3], T& wph) {
  Scenario<T> sc;
  sample_scenario_inl<T, G>(&P, D.r, (size_t)D.npad, env, (uint32_t)episode, &sc);      // wind rows (num_targets = 0: no waypoints)
#pragma unroll
  for (int k = 0; k < 3; ++k) { wb[k] = sc.wb[k]; wa[k] = sc.wa[k]; }
  wph = sc.wph;
#pragma unroll
  for (int k = 0; k < 3; ++k) { S.p[k] = P.start_pos[k]; S.v[k] = P.start_vel[k]; S.w[k] = (T)0; }
#pragma unroll
  for (int k = 0; k < 4; ++k) S.q[k] = P.start_quat[k];
#pragma unroll
  for (int k = 0; k < FW_NUM_ACTUATORS; ++k) S.act[k] = (T)0;
  tick = 0;
  ll_target<T>(P, (uint32_t)(P.env_offset + env), (uint32_t)episode, tgt);
}
// _compute_obs() (:144-156): [ang_vel, ang_pos (Euler), lin_vel, lin_pos] -- the first 12 values of the Euler attitude block --
// then the previous action (6) and the target (3).  Also hands back psi, z and |v| for the reward.
template <typename T, typename W>
__device__ __forceinline__ void ll_write_obs(const Rigid<T>& S, const T act[6], const T tgt[3], T& psi, T& speed, W&& put) {
  T R[9], ang_vel[3], lin_vel[3], eul[3];
  rot_from_quat(S.q, R);
  mtv(R, S.w, ang_vel);
  mtv(R, S.v, lin_vel);
  (void)euler_from_quat(S.q, eul);
  int o = 0;
  put(o++, ang_vel[0]); put(o++, ang_vel[1]); put(o++, ang_vel[2]);
  put(o++, eul[0]); put(o++, eul[1]); put(o++, eul[2]);
  put(o++, lin_vel[0]); put(o++, lin_vel[1]); put(o++, lin_vel[2]);
  put(o++, S.p[0]); put(o++, S.p[1]); put(o++, S.p[2]);
#pragma unroll
  for (int k = 0; k < 6; ++k) put(o++, act[k]);
  put(o++, tgt[0]); put(o++, tgt[1]); put(o++, tgt[2]);
  psi = eul[2];
  speed = M<T>::sqrt_(lin_vel[0] * lin_vel[0] + lin_vel[1] * lin_vel[1] + lin_vel[2] * lin_vel[2]);
}
// the env's target (component k) in the state tail: the step and reset kernels and fw_command_ll read / write it here
template <typename T>
__device__ __forceinline__ T& ll_target_slot(const DevState<T>& D, int env, int k) {
  return D.r[(size_t)(RF_TASK + FW_SL_TARGET + k) * D.npad + env];
}
template <typename T>
__device__ __forceinline__ void ll_load_tail(const DevState<T>& D, int env, T tgt[3], T act[6]) {
  const size_t n = D.npad;
#pragma unroll
  for (int k = 0; k < 3; ++k) tgt[k] = ll_target_slot<T>(D, env, k);
#pragma unroll
  for (int k = 0; k < 6; ++k) act[k] = D.r[(size_t)(RF_TASK + FW_SL_PREV_ACTION + k) * n + env];
}
template <typename T>
__device__ __forceinline__ void ll_store_tail(const DevState<T>& D, int env, const T tgt[3], const T act[6]) {
  const size_t n = D.npad;
#pragma unroll
  for (int k = 0; k < 3; ++k) ll_target_slot<T>(D, env, k) = tgt[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) D.r[(size_t)(RF_TASK + FW_SL_PREV_ACTION + k) * n + env] = act[k];
}

// ---- what only the SAC script's variant has ----
// Its two constants live in a block of their own behind the handle's Params and step image, not in Params: sizeof(Params)
// is an operand of every 8-lane kernel (load_tick_constants: Pp + opaque_zero()), so a field added to it -- even at its end --
// changes the device code of kernels that have nothing to do with this task.  Written where Params is (fw_create / fw_seed).
template <typename T> struct LldC {
  T min_speed;                // lowlevel_min_speed: the stall-penalty threshold (:183)
  int32_t fixed_heading;      // lowlevel_fixed_heading: psi_ref = 0 instead of the draw (:109)
};
template <typename T> __host__ __device__ inline size_t lld_consts_offset() { return (step_image_offset<T>() + sizeof(StepImage<T>) + 127) & ~(size_t)127; }
template <typename T> __device__ __forceinline__ const LldC<T>& lld_consts_of(const Params<T>* Pp) {
  return *reinterpret_cast<const LldC<T>*>(reinterpret_cast<const unsigned char*>(Pp) + lld_consts_offset<T>());
}

// np.clip(a, -1, 1) as numpy computes it (a NaN stays a NaN)
template <typename T> __device__ __forceinline__ T lld_clip1(T a) { return a < (T)-1 ? (T)-1 : (a > (T)1 ? (T)1 : a); }

// reset() (:100-116): ll_begin_episode's start state, wind and target draws; the heading draw (index 0 of the stream) is dropped for
// a fixed heading, the other two keep their indices
template <typename T, int G>
__device__ __forceinline__ void lld_begin_episode(const Params<T>& P, const LldC<T>& LC, const DevState<T>& D, int env, int32_t episode,
                                                  Rigid<T>& S, int32_t& tick, T tgt[3], T wb[3], T wa[3], T& wph) {
  ll_begin_episode<T, G>(P, D, env, episode, S, tick, tgt, wb, wa, wph);
  if (LC.fixed_heading) tgt[0] = (T)0;
}

// _compute_obs() (:146-155) into `put`, and what the reward and the episode ends read from the same row: roll, pitch, psi, |v|
template <typename T, typename W>
__device__ __forceinline__ void lld_write_obs(const Rigid<T>& S, const T a_prev[6], const T tgt[3], T& roll, T& pitch, T& psi, T& speed, W&& put) {
  T r = (T)0, p = (T)0;
  ll_write_obs<T>(S, a_prev, tgt, psi, speed, [&](int k, T v) { if (k == 3) r = v; if (k == 4) p = v; put(k, v); });
  roll = r; pitch = p;
}

// K1 (low-level task): one agent step.  G lanes per env as in step_body (G = 8: lane j evaluates lifting surface j); WIND = the
// config has wind (per-env wind registers and gust clock); V = the variant.  The lanes of an env's group compute the same scalars;
// lane 0 stores.
template <typename T, int G, bool WIND, int V>
__global__ __launch_bounds__(kWave) void fw_step_kernel_ll(const Params<T>* __restrict__ Pp, const ObjC<T>* __restrict__ OCp, DevState<T> Dg,
                                                           const T* __restrict__ actions, T* __restrict__ obs, T* __restrict__ reward,
                                                           uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
                                                           T* __restrict__ terminal_obs, int32_t* __restrict__ info) {
  constexpr bool DEMO = V == FW_LL_VARIANT_SAC_DEMO;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const Params<T>& P = *Pp;
  const LldC<T>& LC = lld_consts_of<T>(Pp);           // (read by the SAC script's variant only)
  constexpr int EPW = kWave / G, Dobs = 21, ld = Dobs + 1;
  Dg.epoch = launch_index(Dg.lctr);
  const DevState<T> D = tile_view<T, EPW>(Dg, (int)blockIdx.x);
  const int lane = threadIdx.x, sub = (G == 1) ? 0 : (lane & (G - 1)), row = lane / G;
  const bool leader = sub == 0;
  const int env0 = (int)blockIdx.x * EPW, env = env0 + row;
  const bool active = env < D.n;
  const int envc = active ? env : D.n - 1;           // inactive lanes shadow the last env and never store
  const size_t n = D.npad;

  int32_t step_count = D.i[IF_STEP * n + envc];
  int32_t tick = D.i[IF_TICK * n + envc];
  int32_t episode = D.i[IF_EPISODE * n + envc];
  int32_t flags = D.i[IF_FLAGS * n + envc];
  Rigid<T> S;
  load_rigid<T>(D, envc, S);
  T ep_return = D.r[RF_EP_RETURN * n + envc];
  // the tail: the episode's target and the last action.  `act` is what the env acts on and what goes back to the tail; `shown` is
  // what the observation and the reward's action term see: this step's action -- the tail's in an env that does not step -- or
  // (SAC script's variant) the previous step's, a_prev.
  T tgt[3], act[6], a_prev[6];
  const T (&shown)[6] = DEMO ? a_prev : act;
  ll_load_tail<T>(D, envc, tgt, DEMO ? a_prev : act);
  T wb[3] = {(T)0, (T)0, (T)0}, wa[3] = {(T)0, (T)0, (T)0}, wphase = (T)0;
  if (WIND) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { wb[k] = D.r[(RF_WIND + k) * n + envc]; wa[k] = D.r[(RF_WIND + 3 + k) * n + envc]; }
    wphase = D.r[(RF_WIND + 6) * n + envc];
  }
  TickC<T> C; SurfC<T> mine; T wmask;
  load_tick_constants<T, G>(Pp, C, mine, wmask);
  normalize_quat<T>(S.q);
  T R[9];
  rot_from_unit_quat<T>(S.q, R);
  T gust[2] = {(T)0, (T)1};
  if (WIND) gust_init<T>(P, wphase, tick, gust);

  // An env that is already done (an un-reset env, or a finished one without auto-reset) is inert: it keeps its state, tail
  // included, and returns its observation with reward 0 and its flags.
  const bool done_at_entry = (flags & (FL_TERM | FL_TRUNC)) != 0;
  const bool stepping = !done_at_entry;
  if constexpr (DEMO) {                              // :120-122: this step's action, clipped; the next step's previous action
#pragma unroll
    for (int k = 0; k < 6; ++k) act[k] = stepping ? lld_clip1<T>(actions[(size_t)envc * 6 + k]) : a_prev[k];
  } else if (stepping) {                             // :97-103: prev_action = action
#pragma unroll
    for (int k = 0; k < 6; ++k) act[k] = actions[(size_t)envc * 6 + k];
  }
  // set_setpoint in mode -1: the surfaces take a[0..4] as given, the throttle command is 0.5 a[5] + 0.5 (build-owned)
  const T cmd[FW_NUM_ACTUATORS] = { act[0], act[1], act[2], act[3], act[4], act[5] * (T)0.5 + (T)0.5 };
  LaneAct<T> LA; LA.a = (T)0; LA.cmd = (T)0;
  if (G == 8) { lane_act_scatter<T>(S, LA); LA.cmd = lane_pick5<T>(cmd[0], cmd[1], cmd[2], cmd[3], cmd[4]); }
  // one Aviary step; the motor-noise normals are those of every task: Aviary step tick / ticks_per_aviary of the episode
  const uint32_t genv = (uint32_t)(P.env_offset + envc);
  T z0 = (T)0, z1 = (T)0;
  if (P.has_noise && stepping) rng_normal2<T>(P, genv, (uint32_t)episode, (uint32_t)(tick / P.ticks_per_aviary), z0, z1);
  ObjState<T> O;                                     // (no task objects: aviary_step<..., OBJ = false> never touches it)
  if (stepping) (void)aviary_step<T, WIND, G, false>(P, C, *OCp, D, envc, O, S, R, cmd, tick, z0, z1, wb, wa, gust, mine, wmask, LA);
  if (G == 8) lane_act_gather<T>(S, LA);

  // observation, reward, termination, truncation, all on the post-step state (tracking :105-142; SAC script :127-130)
  T* trow = tile + row * ld;
  T roll, pitch, psi, speed;
  if constexpr (DEMO) lld_write_obs<T>(S, shown, tgt, roll, pitch, psi, speed, [&](int k, T v) { if (leader) trow[k] = v; });
  else ll_write_obs<T>(S, shown, tgt, psi, speed, [&](int k, T v) { if (leader) trow[k] = v; });
  T rew = (T)0;
  if (stepping) {
    step_count += 1;
    const T z = S.p[2];
    if constexpr (DEMO) {
      const T rho = M<T>::sqrt_(S.p[0] * S.p[0] + S.p[1] * S.p[1]);
      const T a_norm = M<T>::sqrt_(shown[0] * shown[0] + shown[1] * shown[1] + shown[2] * shown[2] + shown[3] * shown[3] +
                                   shown[4] * shown[4] + shown[5] * shown[5]);
      const T psi_err = M<T>::fabs_(ll_wrap_pi<T>(tgt[0] - psi)), h_err = M<T>::fabs_(tgt[1] - z), v_err = M<T>::fabs_(tgt[2] - speed);
      rew = -((T)1.5 * psi_err + (T)1.2 * h_err + (T)0.8 * v_err);                                            // :174
      rew -= (T)0.3 * M<T>::fmax_(M<T>::fabs_(roll) - (T)(35.0 * kPi / 180.0), (T)0);                         // :178
      rew -= (T)0.3 * M<T>::fmax_(M<T>::fabs_(pitch) - (T)(20.0 * kPi / 180.0), (T)0);
      rew -= (T)0.05 * a_norm;                                                                                // :180
      rew -= M<T>::fmax_(rho - P.dome, (T)0);                                                                 // :182
      if (speed < LC.min_speed) rew -= (T)2;                                                                  // :183
      flags = 0;
      if (z < (T)1 || speed < (T)5) flags |= FL_TERM;                                                         // :194-197
      if (rho > P.dome * (T)1.2 || step_count >= P.ll_max_steps) flags |= FL_TRUNC;                           // :204-207
    } else {
      const T psi_err = M<T>::fabs_(ll_wrap_pi<T>(tgt[0] - psi)), h_err = M<T>::fabs_(tgt[1] - z), v_err = M<T>::fabs_(tgt[2] - speed);
      rew = -((T)1 * psi_err + (T)1 * h_err + (T)0.5 * v_err);
      rew += (T)0.1;
      flags = 0;
      if (z < (T)1 || z > (T)100) { flags |= FL_TERM; rew -= (T)100; }      // :132-134
      if (step_count >= P.ll_max_steps) flags |= FL_TRUNC;                  // :137-138
    }
    ep_return += rew;
  }
  if (active && leader) {
    reward[env] = rew;
    terminated[env] = (uint8_t)((flags & FL_TERM) ? 1 : 0);
    truncated[env] = (uint8_t)((flags & FL_TRUNC) ? 1 : 0);
    if (info) {
      int4* ip = reinterpret_cast<int4*>(info + (size_t)env * FW_INFO_DIM);
      ip[0] = make_int4(0, 0, 0, 0);
      ip[1] = make_int4(0, 0, step_count, 0);
    }
  }
  // SB3 worker auto-reset: the row just written is the terminal observation; the new episode's first observation replaces it
  if ((flags & (FL_TERM | FL_TRUNC)) && P.auto_reset) {
    if (active && leader && terminal_obs) {
      T* out = terminal_obs + (size_t)env * Dobs;
      for (int k = 0; k < Dobs; ++k) out[k] = trow[k];
    }
    episode += 1;
    if constexpr (DEMO) lld_begin_episode<T, G>(P, LC, D, envc, episode, S, tick, tgt, wb, wa, wphase);
    else ll_begin_episode<T, G>(P, D, envc, episode, S, tick, tgt, wb, wa, wphase);
#pragma unroll
    for (int k = 0; k < 6; ++k) act[k] = (T)0;
    step_count = 0; flags = 0; ep_return = (T)0;
    if constexpr (DEMO) lld_write_obs<T>(S, act, tgt, roll, pitch, psi, speed, [&](int k, T v) { if (leader) trow[k] = v; });
    else ll_write_obs<T>(S, act, tgt, psi, speed, [&](int k, T v) { if (leader) trow[k] = v; });
    if (active && leader) { stat_add(D.stats, FW_CTR_RESETS); stat_add(D.stats, FW_CTR_FALLBACKS); }
  }
  if (active && leader) {
    store_rigid<T>(D, env, S);
    ll_store_tail<T>(D, env, tgt, act);
    D.r[RF_EP_RETURN * n + env] = ep_return;
    D.i[IF_STEP * n + env] = step_count;
    D.i[IF_TICK * n + env] = tick;
    D.i[IF_EPISODE * n + env] = episode;
    D.i[IF_FLAGS * n + env] = flags;
  }
  __syncthreads();
  flush_obs_tile<T>(tile, ld, obs, env0, EPW, D.n, Dobs);
  launch_done(Dg.lctr, Dg.epoch);
}

// K2 (low-level task): reset (masked) + observation, fw_reset / fw_observe.  A caller-supplied scenario's wind replaces the draw.
// The observation shows the tail's action: zeros after a reset; in fw_observe the last action taken.
template <typename T, int G, int V>
__global__ __launch_bounds__(kWave) void fw_reset_kernel_ll(const Params<T>* __restrict__ Pp, DevState<T> Dg, const uint8_t* __restrict__ mask,
                                                            T* __restrict__ obs, int do_reset, ScenOv ov) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const Params<T>& P = *Pp;
  const LldC<T>& LC = lld_consts_of<T>(Pp);           // (read by the SAC script's variant only)
  constexpr int EPW = kWave / G, Dobs = 21, ld = Dobs + 1;
  const DevState<T> D = tile_view<T, EPW>(Dg, (int)blockIdx.x);
  const int lane = threadIdx.x, sub = (G == 1) ? 0 : (lane & (G - 1)), row = lane / G;
  const bool leader = sub == 0;
  const int env0 = (int)blockIdx.x * EPW, env = env0 + row;
  const bool active = env < D.n;
  const int envc = active ? env : D.n - 1;
  const size_t n = D.npad;
  Rigid<T> S;
  load_rigid<T>(D, envc, S);
  T tgt[3], act[6];
  ll_load_tail<T>(D, envc, tgt, act);
  const bool resetting = active && do_reset && (!mask || mask[envc]);
  if (resetting) {
    int32_t episode = D.i[IF_EPISODE * n + env] + 1, tick = 0;
    T wb[3], wa[3], wph;
    if constexpr (V == FW_LL_VARIANT_SAC_DEMO) lld_begin_episode<T, G>(P, LC, D, env, episode, S, tick, tgt, wb, wa, wph);
    else ll_begin_episode<T, G>(P, D, env, episode, S, tick, tgt, wb, wa, wph);
#pragma unroll
    for (int k = 0; k < 6; ++k) act[k] = (T)0;
    if (leader) {
      if (P.wind_mode != FW_WIND_OFF) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (ov.wind_base) D.r[(RF_WIND + k) * n + env] = (T)ov.wind_base[3 * (size_t)env + k];
          if (ov.gust_amp) D.r[(RF_WIND + 3 + k) * n + env] = (T)ov.gust_amp[3 * (size_t)env + k];
        }
        if (ov.gust_phase) D.r[(RF_WIND + 6) * n + env] = (T)ov.gust_phase[env];
      }
      store_rigid<T>(D, env, S);
      ll_store_tail<T>(D, env, tgt, act);
      D.r[RF_EP_RETURN * n + env] = (T)0;
      D.i[IF_STEP * n + env] = 0;
      D.i[IF_TICK * n + env] = tick;
      D.i[IF_EPISODE * n + env] = episode;
      D.i[IF_FLAGS * n + env] = 0;
      D.i[IF_NUM_REACHED * n + env] = 0;
    }
  }
  if (obs) {
    T psi, speed;
    if (active && leader) ll_write_obs<T>(S, act, tgt, psi, speed, [&](int k, T v) { tile[row * ld + k] = v; });
    __syncthreads();
    flush_obs_tile<T>(tile, ld, obs, env0, EPW, D.n, Dobs);
  }
}
