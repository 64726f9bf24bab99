// FW_TASK_LOWLEVEL, lowlevel_variant = FW_LL_VARIANT_SAC_DEMO (DESIGN.md section 2d "SAC script's variant"): the FixedwingLowLevelEnv
// that the reference's examples/lowlevel.py defines for its SAC run -- not the env of the same name that train/train_lowlevel_cmd.py
// imports (fw_step_kernel_ll above).  Line numbers below are examples/lowlevel.py's.
//
// What the two share is shared in code: the six actuator commands (surfaces a[0..4] as given, throttle 0.5 a[5] + 0.5), one inlined
// Aviary step per agent step with the motor-noise keying of every task, the 21 observation columns (ll_write_obs), the target draw
// (ll_target on STREAM_LL_TARGET, through ll_begin_episode), the FW_SL_* state tail (ll_load_tail / ll_store_tail), the heading wrap
// (ll_wrap_pi), the tile, launch-counter and auto-reset conventions.  What differs is here:
//   * the action is clipped to [-1, 1] by the env (:121);
//   * obs[12:18] and the reward's action term are the PREVIOUS step's clipped action -- the script assigns prev_action after it has
//     computed observation and reward (:127-133) -- zeros on an episode's first step;
//   * the reward (:157-185), termination on height or airspeed (:187-198), truncation on 1.2 x the dome radius or the clock (:200-208);
//   * psi_ref = 0 with lowlevel_fixed_heading (:109).
// Start pose, speed and target ranges are config (config.lowlevel_demo_config).
//
// Kernels of their own rather than a flag of fw_step_kernel_ll / fw_reset_kernel_ll: those stay exactly as they were.
// Included by fwsim.hip behind the low-level task's kernels.
#pragma once

// The variant's two constants live in a block of their own behind the handle's Params and step image, not in Params: sizeof(Params)
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

// K1 (low-level task, SAC script's variant): one agent step.  G, WIND and the lane roles as in fw_step_kernel_ll.
template <typename T, int G, bool WIND>
__global__ __launch_bounds__(kWave) void fw_step_kernel_lld(const Params<T>* __restrict__ Pp, const ObjC<T>* __restrict__ OCp, DevState<T> Dg,
                                                            const T* __restrict__ actions, T* __restrict__ obs, T* __restrict__ reward,
                                                            uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
                                                            T* __restrict__ terminal_obs, int32_t* __restrict__ info) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const Params<T>& P = *Pp;
  const LldC<T>& LC = lld_consts_of<T>(Pp);
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
  T tgt[3], a_prev[6];                                // the tail: the episode's target, the previous step's clipped action
  ll_load_tail<T>(D, envc, tgt, a_prev);
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
  T act[6];                                           // :120-122: this step's action, clipped; the next step's a_prev
#pragma unroll
  for (int k = 0; k < 6; ++k) act[k] = stepping ? lld_clip1<T>(actions[(size_t)envc * 6 + k]) : a_prev[k];
  // set_setpoint in mode -1: the surfaces take a[0..4] as given, the throttle command is 0.5 a[5] + 0.5 (build-owned)
  const T cmd[FW_NUM_ACTUATORS] = { act[0], act[1], act[2], act[3], act[4], act[5] * (T)0.5 + (T)0.5 };
  LaneAct<T> LA; LA.a = (T)0; LA.cmd = (T)0;
  if (G == 8) { lane_act_scatter<T>(S, LA); LA.cmd = lane_pick5<T>(cmd[0], cmd[1], cmd[2], cmd[3], cmd[4]); }
  // one Aviary step (:123); the motor-noise normals are those of every task: Aviary step tick / ticks_per_aviary of the episode
  const uint32_t genv = (uint32_t)(P.env_offset + envc);
  T z0 = (T)0, z1 = (T)0;
  if (P.has_noise && stepping) rng_normal2<T>(P, genv, (uint32_t)episode, (uint32_t)(tick / P.ticks_per_aviary), z0, z1);
  ObjState<T> O;                                     // (no task objects: aviary_step<..., OBJ = false> never touches it)
  if (stepping) (void)aviary_step<T, WIND, G, false>(P, C, *OCp, D, envc, O, S, R, cmd, tick, z0, z1, wb, wa, gust, mine, wmask, LA);
  if (G == 8) lane_act_gather<T>(S, LA);

  // observation, reward, termination, truncation (:127-130), all on the post-step state and the previous action
  T* trow = tile + row * ld;
  T roll, pitch, psi, speed;
  lld_write_obs<T>(S, a_prev, tgt, roll, pitch, psi, speed, [&](int k, T v) { if (leader) trow[k] = v; });
  T rew = (T)0;
  if (stepping) {
    step_count += 1;
    const T z = S.p[2];
    const T rho = M<T>::sqrt_(S.p[0] * S.p[0] + S.p[1] * S.p[1]);
    const T a_norm = M<T>::sqrt_(a_prev[0] * a_prev[0] + a_prev[1] * a_prev[1] + a_prev[2] * a_prev[2] + a_prev[3] * a_prev[3] +
                                 a_prev[4] * a_prev[4] + a_prev[5] * a_prev[5]);
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
    lld_begin_episode<T, G>(P, LC, D, envc, episode, S, tick, tgt, wb, wa, wphase);
#pragma unroll
    for (int k = 0; k < 6; ++k) act[k] = (T)0;
    step_count = 0; flags = 0; ep_return = (T)0;
    lld_write_obs<T>(S, act, tgt, roll, pitch, psi, speed, [&](int k, T v) { if (leader) trow[k] = v; });
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

// K2 (low-level task, SAC script's variant): reset (masked) + observation, fw_reset / fw_observe.  A caller-supplied scenario's wind
// replaces the draw.  The observation shows the tail's action: zeros after a reset, the previous step's in fw_observe.
template <typename T, int G>
__global__ __launch_bounds__(kWave) void fw_reset_kernel_lld(const Params<T>* __restrict__ Pp, DevState<T> Dg, const uint8_t* __restrict__ mask,
                                                             T* __restrict__ obs, int do_reset, ScenOv ov) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const Params<T>& P = *Pp;
  const LldC<T>& LC = lld_consts_of<T>(Pp);
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
    lld_begin_episode<T, G>(P, LC, D, env, episode, S, tick, tgt, wb, wa, wph);
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
