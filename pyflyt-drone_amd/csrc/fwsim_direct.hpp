// FW_TASK_WAYPOINTS_DIRECT: the waypoints task flown in PyFlyt's mode -1 -- the base env under the
// reference's high-level command env (train/train_highlevel_cmd.py:35-181) -- and the command step in front of it.
//
// The six actions are the actuator commands, exactly as FW_TASK_LOWLEVEL takes them (surfaces a[0..4] as given, throttle
// 0.5 a[5] + 0.5; no mixer).  Everything else is the waypoints task: start pose and velocity, the warm-up Aviary steps under an
// all-zero setpoint, step_ratio Aviary steps per agent step with the early break, waypoint rewards, contact / dome termination,
// truncation, target draws, wind.  The observation is the flattened waypoint observation with the action block six wide
// (attitude 12 / 13, last actuator command 6, aux 6, 3 context_length target deltas), so that in Euler mode columns 0:18 are
// columns 0:18 of the low-level task's observation (ll_write_obs).
//
// One step frame (fw_step_kernel_wd) and one reset kernel (fw_reset_kernel_wd), beside step_body / fw_reset_kernel of the
// four-action tasks.  The step frame serves fw_step and fw_step_hl alike: where the six commands come from is its template
// parameter SRC (WdSource below); the phase machine, the end-of-step block with the auto-reset, the motor noise and the Aviary
// step, the waypoint reward / termination block, the warm-up branch and the epilogue are written once.  What the other kernels
// are built from is shared: the inlined Aviary step, begin_reset / end_reset and the scenario sampler, the attitude block of the
// observation.  Auto-resets run in the kernel (sampler, and the warm-up when wind acts on the
// dynamics; wind-free the cached warm state is copied): FW_CTR_FALLBACKS.  The shadow / scenario hand-off of step_body is not
// wired to this task.
//
// The six-wide last command lives in the task tail (FW_SL_PREV_ACTION, through ll_load_tail / ll_store_tail); FW_SL_TARGET holds
// the last conditioned command of fw_command_hl.  RF_ACTION is not touched.
//
// Included by fwsim.hip behind the low-level task's kernels and the controller (fwsim_hl_step.hpp).
#pragma once

// the flattened waypoint observation with a six-wide action block: the shared attitude writer's columns, with its four action
// columns dropped and what follows them moved two to the right
template <typename T, typename W>
__device__ __forceinline__ void wd_write_obs(const Params<T>& P, const DevState<T>& D, int env, const Rigid<T>& S, const T act[6],
                                             int tgt_idx, W&& put) {
  T R[9];
  const int pre = P.att_dim - 12;                    // 12 (euler) / 13 (quaternion): where the action block starts
  const T a4[4] = {(T)0, (T)0, (T)0, (T)0};
  (void)write_obs_attitude<T, false>(P, S, a4, R, [&](int k, T v) { if (k < pre) put(k, v); else if (k >= pre + 4) put(k + 2, v); });
#pragma unroll
  for (int k = 0; k < 6; ++k) put(pre + k, act[k]);
  int o = P.att_dim;
  for (int i = 0; i < P.ctx; ++i) {
    const int t = tgt_idx + i;
    T d[3] = {(T)0, (T)0, (T)0}, b[3] = {(T)0, (T)0, (T)0};
    if (t < P.num_targets) {
      const T* tp = D.r + (size_t)(RF_TARGETS + 3 * t) * D.npad + env;
      d[0] = tp[0] - S.p[0]; d[1] = tp[D.npad] - S.p[1]; d[2] = tp[2 * (size_t)D.npad] - S.p[2];
      mtv(R, d, b);
    }
    put(o++, b[0]); put(o++, b[1]); put(o++, b[2]);
  }
}

// the command an env holds before fw_command_hl has written one (only a rejected row ever shows it): level flight at the start
// height and speed
template <typename T> __device__ __forceinline__ void wd_default_command(const Params<T>& P, T tgt[3]) {
  tgt[0] = (T)0;
  tgt[1] = P.start_pos[2];
  tgt[2] = M<T>::sqrt_(P.start_vel[0] * P.start_vel[0] + P.start_vel[1] * P.start_vel[1] + P.start_vel[2] * P.start_vel[2]);
}

// Where the six actuator commands of an agent step come from -- the template parameter SRC of fw_step_kernel_wd, which also decides
// the type of the kernel's fourth parameter:
//   WD_HELD  fw_step: `const T* actions` [N, 6], read once in front of the loop and held for every Aviary step of the agent step;
//   WD_CTL   fw_step_hl: fwsim_ctl::CtlArgs, the frozen low-level controller (fwsim_hl_step.hpp), evaluated in front of every stepping
//            Aviary step on the command in force -- the env's FW_SL_TARGET tail, which fw_command_hl / fw_collect_act_hl wrote.  Its
//            statistics and (G = 8) weights are staged in LDS behind the observation tile; the output in force when the step ends goes
//            to CtlArgs::low_action.  Warm-up steps keep the all-zero setpoint and run no controller; an env that is done at entry
//            runs nothing.
enum WdSource { WD_HELD = 0, WD_CTL = 1 };
template <typename T, int SRC> struct WdSourceArg { typedef const T* __restrict__ type; };
template <typename T> struct WdSourceArg<T, WD_CTL> { typedef fwsim_ctl::CtlArgs type; };

// K1 (waypoints, direct actuator commands): one agent step.  G lanes per env as in step_body (G = 8: lane j evaluates lifting
// surface j and samples waypoint j of a reset); WIND = the config has wind; SRC as above.  One tick site: the step's Aviary steps and
// the warm-up of an in-kernel reset share the loop, as in step_body.  Outputs are latched in registers and stored once at the end.
template <typename T, int G, bool WIND, int SRC>
__global__ __launch_bounds__(kWave) void fw_step_kernel_wd(const Params<T>* __restrict__ Pp, const ObjC<T>* __restrict__ OCp, DevState<T> Dg,
                                                           typename WdSourceArg<T, SRC>::type input, T* __restrict__ obs, T* __restrict__ reward,
                                                           uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
                                                           T* __restrict__ terminal_obs, int32_t* __restrict__ info) {
  constexpr bool CTL = SRC == WD_CTL;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const Params<T>& P = *Pp;
  constexpr int EPW = kWave / G;
  Dg.epoch = launch_index(Dg.lctr);
  const DevState<T> D = tile_view<T, EPW>(Dg, (int)blockIdx.x);
  const int lane = threadIdx.x, sub = (G == 1) ? 0 : (lane & (G - 1)), row = lane / G;
  const bool leader = sub == 0;
  const int env0 = (int)blockIdx.x * EPW, env = env0 + row;
  const bool active = env < D.n;
  const int envc = active ? env : D.n - 1;           // inactive lanes shadow the last env and never store
  const size_t n = D.npad;
  const int Dobs = P.obs_dim, ld = Dobs + 1;

  // ---- WD_CTL: the controller's LDS behind the tile: statistics, (G = 8) the policy net, one activation row per env ----
  double *cstd = nullptr, *cmean = nullptr;
  float *wlds = nullptr, *rowp = nullptr;
  if constexpr (CTL) {
    using namespace fwsim_ctl;
    cstd = reinterpret_cast<double*>(smem_raw + Dg.stash_off);
    cmean = cstd + kStatDoubles / 2;
    wlds = reinterpret_cast<float*>(cstd + kStatDoubles);
    rowp = wlds + (G == 8 ? kNetFloatsPad : 0) + row * kRowLd;
    ctl_load_stats(input.mean, input.var, input.eps, cstd, cmean);
    if (G == 8) {
      int i0 = 0;
      if ((reinterpret_cast<uintptr_t>(input.params) & 15) == 0) {       // (an allocation of its own is; a view into a larger buffer may not be)
        const float4* __restrict__ src = reinterpret_cast<const float4*>(input.params);
        float4* dst = reinterpret_cast<float4*>(wlds);
        for (int i = lane; i < kNetFloats / 4; i += kWave) dst[i] = src[i];
        i0 = kNetFloats & ~3;
      }
      for (int i = i0 + lane; i < kNetFloats; i += kWave) wlds[i] = input.params[i];
    }
    __syncthreads();                                 // (uniform: before anything diverges)
  }

  int32_t step_count = D.i[IF_STEP * n + envc];
  int32_t tick = D.i[IF_TICK * n + envc];
  int32_t episode = D.i[IF_EPISODE * n + envc];
  int32_t flags = D.i[IF_FLAGS * n + envc];
  int32_t num_reached = D.i[IF_NUM_REACHED * n + envc];
  Rigid<T> S;
  load_rigid<T>(D, envc, S);
  T new_dist = D.r[RF_NEW_DIST * n + envc];
  T ep_return = D.r[RF_EP_RETURN * n + envc];
  T hl_cmd[3], act[6];                               // the tail: fw_command_hl's last command, the actuator commands last issued (the observation shows them)
  ll_load_tail<T>(D, envc, hl_cmd, act);
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

  // An env that is already done (bare-Gymnasium mode) runs no sub-step: it returns its stale view, previous command included.
  const bool done_at_entry = (flags & (FL_TERM | FL_TRUNC)) != 0;
  int tgt_obs = (flags >> FL_TGT_SHIFT) & 15;        // target index the last compute_state() saw
  flags &= FL_MASK;
  // mode -1: the surfaces take a[0..4] as given, the throttle command is 0.5 a[5] + 0.5 (as FW_TASK_LOWLEVEL)
  T cmd[FW_NUM_ACTUATORS], cmd_mine = (T)0;          // (WD_HELD only: the step's commands, and this lane's surface's)
  if constexpr (!CTL) {
    if (!done_at_entry) {
#pragma unroll
      for (int k = 0; k < 6; ++k) act[k] = input[(size_t)envc * 6 + k];
    }
#pragma unroll
    for (int k = 0; k < FW_NUM_SURFACES; ++k) cmd[k] = act[k];
    cmd[FW_NUM_SURFACES] = act[5] * (T)0.5 + (T)0.5;
  }
  LaneAct<T> LA; LA.a = (T)0; LA.cmd = (T)0;
  if (G == 8) {
    lane_act_scatter<T>(S, LA);
    if constexpr (!CTL) { cmd_mine = lane_pick5<T>(cmd[0], cmd[1], cmd[2], cmd[3], cmd[4]); LA.cmd = cmd_mine; }
  }

  // current and next waypoint stay in registers
  T tcur[3], tnext[3];
  {
    const int i0 = min(num_reached, FW_MAX_TARGETS - 1), i1 = min(num_reached + 1, FW_MAX_TARGETS - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      tcur[k] = D.r[(size_t)(RF_TARGETS + 3 * i0 + k) * n + envc];
      tnext[k] = D.r[(size_t)(RF_TARGETS + 3 * i1 + k) * n + envc];
    }
  }
  const uint32_t genv = (uint32_t)(P.env_offset + envc);
  T rew = (T)-0.1;                                   // fixedwing_base_env.py:325-331
  T o_rew = (T)0;                                    // the step's outputs, latched when it ends
  int32_t o_flags = 0, o_reached = 0, o_steps = 0;
  int phase = active ? PH_STEP : PH_DONE;
  int it = 0, warm_left = 0;
  bool step_over = active && done_at_entry;          // nothing to simulate: finalise immediately
  ObjState<T> O;                                     // (no task objects: aviary_step<..., OBJ = false> never touches it)
  T* trow = tile + row * ld;

#pragma unroll 1
  for (;;) {
    if (phase == PH_STEP && step_over) {
      // ---- end of env.step(): outputs, SB3 worker auto-reset ----
      step_count += 1;
      ep_return += rew;
      phase = PH_DONE;
      o_rew = rew; o_flags = flags; o_reached = num_reached; o_steps = step_count;
      if constexpr (CTL) {
        if (input.low_action && leader) {               // the controller's output in force when the step ended (a reset below zeroes act)
          T* la = reinterpret_cast<T*>(input.low_action) + (size_t)env * 6;
#pragma unroll
          for (int k = 0; k < 6; ++k) la[k] = act[k];
        }
      }
      if ((flags & (FL_TERM | FL_TRUNC)) && P.auto_reset) {
        if (G == 8) lane_act_gather<T>(S, LA);        // the terminal observation shows all six actuators
        if (terminal_obs && leader) {
          T* out = terminal_obs + (size_t)env * Dobs;
          wd_write_obs<T>(P, D, env, S, act, tgt_obs, [&](int k, T v) { out[k] = v; });
        }
        T t_mine[3] = {(T)0, (T)0, (T)0};
        warm_left = begin_reset<T, G>(P, D, env, S, tick, episode, num_reached, wb, wa, wphase, t_mine);
        if (G > 1) {                                  // the group's lane 0 sampled waypoint 0
          const int src = lane & ~(G - 1);
#pragma unroll
          for (int k = 0; k < 3; ++k) t_mine[k] = __shfl(t_mine[k], src, kWave);
        }
        if (WIND) gust_init<T>(P, wphase, tick, gust);
        if (G == 8) lane_act_scatter<T>(S, LA);
        step_count = 0; flags = 0; ep_return = (T)0; tgt_obs = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) act[k] = (T)0;
        wd_default_command<T>(P, hl_cmd);
        if (leader) { stat_add(D.stats, FW_CTR_RESETS); stat_add(D.stats, FW_CTR_FALLBACKS); }
        rot_from_unit_quat<T>(S.q, R);
        if (warm_left > 0) phase = PH_WARM;
        else new_dist = end_reset<T, G>(P, D, env, episode, S, t_mine);
      }
    }
    if (__ballot(phase != PH_DONE) == 0ull) break;   // wave-uniform exit
    const bool stepped = phase != PH_DONE;
    const bool stepping = phase == PH_STEP;
    if (stepped) {
      if constexpr (CTL) {
        if (stepping) {
          // ---- the controller, at the rate it was trained at: (attitude block, last actuator commands, command) -> six commands ----
          using namespace fwsim_ctl;
          T xa[12];
          ctl_attitude_row<T>(S, xa);
          if (leader) {
#pragma unroll
            for (int d = 0; d < 12; ++d) rowp[d] = ctl_normalise((double)xa[d], cmean[d], cstd[d], input.clip);
#pragma unroll
            for (int d = 0; d < 6; ++d) rowp[12 + d] = ctl_normalise((double)act[d], cmean[12 + d], cstd[12 + d], input.clip);
#pragma unroll
            for (int d = 0; d < 3; ++d) rowp[18 + d] = ctl_normalise((double)hl_cmd[d], cmean[18 + d], cstd[18 + d], input.clip);
          }
          float a[kA];
          if constexpr (G == 8) ctl_forward<G>(wlds, rowp, sub, a);
          else ctl_forward<G>((ctl_const_ptr)input.params, rowp, sub, a);
#pragma unroll
          for (int k = 0; k < 6; ++k) act[k] = (T)a[k];
        }
      }
      // motor noise of this Aviary step; the warm-up runs under a zero setpoint without noise
      T z0 = (T)0, z1 = (T)0;
      if (P.has_noise && stepping) rng_normal2<T>(P, genv, (uint32_t)episode, (uint32_t)(tick / P.ticks_per_aviary), z0, z1);
      T c_eff[FW_NUM_ACTUATORS];
      if constexpr (CTL) {
#pragma unroll
        for (int c = 0; c < FW_NUM_SURFACES; ++c) c_eff[c] = stepping ? act[c] : (T)0;
        c_eff[FW_NUM_SURFACES] = stepping ? act[5] * (T)0.5 + (T)0.5 : (T)0;
        if (G == 8) LA.cmd = lane_pick5<T>(c_eff[0], c_eff[1], c_eff[2], c_eff[3], c_eff[4]);
      } else {
#pragma unroll
        for (int c = 0; c < FW_NUM_ACTUATORS; ++c) c_eff[c] = stepping ? cmd[c] : (T)0;
        LA.cmd = stepping ? cmd_mine : (T)0;
      }
      const bool contact = aviary_step<T, WIND, G, false>(P, C, *OCp, D, envc, O, S, R, c_eff, tick, z0, z1, wb, wa, gust, mine, wmask, LA);
      if (stepping) {
        // compute_state(): WaypointHandler.distance_to_targets side effects
        const int nleft = P.num_targets - num_reached;
        const T old_dist = new_dist;
        if (nleft > 0) {
          T dx = tcur[0] - S.p[0], dy = tcur[1] - S.p[1], dz = tcur[2] - S.p[2];
          new_dist = M<T>::sqrt_(dx * dx + dy * dy + dz * dz);
        }
        tgt_obs = num_reached;
        // compute_base_term_trunc_reward(): fixedwing_base_env.py:296-312
        if (step_count > P.max_steps) flags |= FL_TRUNC;
        if (contact) { rew = (T)-100; flags |= FL_COLLISION | FL_TERM; }
        if (S.p[0] * S.p[0] + S.p[1] * S.p[1] + S.p[2] * S.p[2] > P.dome * P.dome) { rew = (T)-100; flags |= FL_OOB | FL_TERM; }
        // waypoint reward (upstream FixedwingWaypointsEnv)
        if (nleft > 0) {
          if (!P.sparse) {
            T progress = (old_dist != (T)0) ? (old_dist - new_dist) : (T)0;
            rew += M<T>::fmax_((T)3 * progress, (T)0);
            rew += M<T>::rcp_(new_dist);
          }
          if (new_dist < P.reach) {
            rew = (T)100;
            num_reached += 1;
            if (num_reached == P.num_targets) flags |= FL_TRUNC | FL_COMPLETE;
            const int i1 = min(num_reached + 1, FW_MAX_TARGETS - 1);     // advance_targets(): shift the register window
#pragma unroll
            for (int k = 0; k < 3; ++k) { tcur[k] = tnext[k]; tnext[k] = D.r[(size_t)(RF_TARGETS + 3 * i1 + k) * n + envc]; }
          }
        }
        step_over = (it + 1 >= P.step_ratio) || (flags & (FL_TERM | FL_TRUNC));     // :334-337
      } else {
        warm_left -= 1;
        if (warm_left == 0) { new_dist = end_reset<T, G>(P, D, env, episode, S); phase = PH_DONE; }
      }
    }
    it += 1;
  }
  // G = 8: waypoints sampled by sibling lanes during an in-launch reset are read back by the observation pass
  if (G > 1) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  if (G == 8) lane_act_gather<T>(S, LA);
  if (active && leader) {
    wd_write_obs<T>(P, D, env, S, act, tgt_obs, [&](int k, T v) { trow[k] = v; });
    store_rigid<T>(D, env, S);
    ll_store_tail<T>(D, env, hl_cmd, act);
    D.r[RF_NEW_DIST * n + env] = new_dist;
    D.r[RF_EP_RETURN * n + env] = ep_return;
    D.i[IF_STEP * n + env] = step_count;
    D.i[IF_TICK * n + env] = tick;
    D.i[IF_EPISODE * n + env] = episode;
    D.i[IF_FLAGS * n + env] = flags | (tgt_obs << FL_TGT_SHIFT);
    D.i[IF_NUM_REACHED * n + env] = num_reached;
    reward[env] = o_rew;
    terminated[env] = (uint8_t)((o_flags & FL_TERM) ? 1 : 0);
    truncated[env] = (uint8_t)((o_flags & FL_TRUNC) ? 1 : 0);
    if (info) {
      int4* ip = reinterpret_cast<int4*>(info + (size_t)env * FW_INFO_DIM);
      ip[0] = make_int4(o_reached, (o_flags & FL_COLLISION) ? 1 : 0, (o_flags & FL_OOB) ? 1 : 0, (o_flags & FL_COMPLETE) ? 1 : 0);
      ip[1] = make_int4(0, 0, o_steps, 0);
    }
  }
  __syncthreads();
  flush_obs_tile<T>(tile, ld, obs, env0, EPW, D.n, Dobs);
  launch_done(Dg.lctr, Dg.epoch);
}

// K2 (waypoints, direct actuator commands): reset (masked) + observation, fw_reset / fw_observe.  A caller-supplied scenario's
// waypoints and wind replace the draw, as in fw_reset_kernel.
template <typename T, int G>
__global__ __launch_bounds__(kWave) void fw_reset_kernel_wd(const Params<T>* __restrict__ Pp, const ObjC<T>* __restrict__ OCp, DevState<T> Dg,
                                                            const uint8_t* __restrict__ mask, T* __restrict__ obs, int do_reset, ScenOv ov) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const Params<T>& P = *Pp;
  constexpr int EPW = kWave / G;
  const DevState<T> D = tile_view<T, EPW>(Dg, (int)blockIdx.x);
  const int lane = threadIdx.x, sub = (G == 1) ? 0 : (lane & (G - 1)), row = lane / G;
  const bool leader = sub == 0;
  const int env0 = (int)blockIdx.x * EPW, env = env0 + row;
  const bool active = env < D.n;
  const int envc = active ? env : D.n - 1;
  const size_t n = D.npad;
  const int Dobs = P.obs_dim, ld = Dobs + 1;
  TickC<T> C; SurfC<T> mine; T wmask;
  load_tick_constants<T, G, false>(Pp, C, mine, wmask);
  Rigid<T> S;
  load_rigid<T>(D, envc, S);
  T hl_cmd[3], act[6];
  ll_load_tail<T>(D, envc, hl_cmd, act);
  int32_t num_reached = D.i[IF_NUM_REACHED * n + envc];
  int tgt_obs = (D.i[IF_FLAGS * n + envc] >> FL_TGT_SHIFT) & 15;
  const bool resetting = active && do_reset && (!mask || mask[envc]);
  int32_t tick = 0, episode = D.i[IF_EPISODE * n + envc];
  T new_dist = (T)0, wb[3] = {(T)0, (T)0, (T)0}, wa[3] = {(T)0, (T)0, (T)0}, wphase = (T)0;
  int warm_left = 0;
  T t_first[3] = {(T)0, (T)0, (T)0};                 // waypoint 0 of the new episode, for end_reset
  if (resetting) {
    warm_left = begin_reset<T, G>(P, D, env, S, tick, episode, num_reached, wb, wa, wphase, t_first);
    if (G > 1) {                                      // the group's lane 0 sampled waypoint 0
      const int src = lane & ~(G - 1);
#pragma unroll
      for (int k = 0; k < 3; ++k) t_first[k] = __shfl(t_first[k], src, kWave);
    }
    // ---- caller-supplied scenario: replaces what begin_reset drew, before anything depends on it ----
    if (P.wind_mode != FW_WIND_OFF && (ov.wind_base || ov.gust_amp || ov.gust_phase)) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (ov.wind_base) wb[k] = (T)ov.wind_base[3 * (size_t)env + k];
        if (ov.gust_amp) wa[k] = (T)ov.gust_amp[3 * (size_t)env + k];
      }
      if (ov.gust_phase) wphase = (T)ov.gust_phase[env];
      if (leader) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { D.r[(RF_WIND + k) * n + env] = wb[k]; D.r[(RF_WIND + 3 + k) * n + env] = wa[k]; }
        D.r[(RF_WIND + 6) * n + env] = wphase;
      }
    }
    if (ov.targets && P.num_targets > 0) {
      if (leader)
        for (int t = 0; t < P.num_targets; ++t)
#pragma unroll
          for (int k = 0; k < 3; ++k) D.r[(size_t)(RF_TARGETS + 3 * t + k) * n + env] = (T)ov.targets[((size_t)env * FW_MAX_TARGETS + t) * 3 + k];
#pragma unroll
      for (int k = 0; k < 3; ++k) t_first[k] = (T)ov.targets[(size_t)env * FW_MAX_TARGETS * 3 + k];
    }
    if (warm_left == 0) new_dist = end_reset<T, G>(P, D, env, episode, S, t_first);
  }
  const T cmd0[FW_NUM_ACTUATORS] = {(T)0, (T)0, (T)0, (T)0, (T)0, (T)0};
  T R[9];
  normalize_quat<T>(S.q);
  rot_from_unit_quat<T>(S.q, R);
  T gust[2];
  gust_init<T>(P, wphase, tick, gust);
  LaneAct<T> LA; LA.cmd = (T)0; LA.a = (T)0;
  if (G == 8) lane_act_scatter<T>(S, LA);
  ObjState<T> O;
#pragma unroll 1
  while (__ballot(warm_left > 0) != 0ull) {
    if (warm_left > 0) {
      (void)aviary_step<T, true, G, false>(P, C, *OCp, D, envc, O, S, R, cmd0, tick, (T)0, (T)0, wb, wa, gust, mine, wmask, LA);
      warm_left -= 1;
      if (warm_left == 0) new_dist = end_reset<T, G>(P, D, env, episode, S, t_first);
    }
  }
  if (G > 1) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  if (G == 8) lane_act_gather<T>(S, LA);
  if (resetting) {
#pragma unroll
    for (int k = 0; k < 6; ++k) act[k] = (T)0;
    wd_default_command<T>(P, hl_cmd);
    tgt_obs = 0;
    if (leader) {
      store_rigid<T>(D, env, S);
      ll_store_tail<T>(D, env, hl_cmd, act);
      D.r[RF_NEW_DIST * n + env] = new_dist;
      D.r[RF_EP_RETURN * n + env] = (T)0;
      D.i[IF_STEP * n + env] = 0;
      D.i[IF_TICK * n + env] = tick;
      D.i[IF_EPISODE * n + env] = episode;
      D.i[IF_FLAGS * n + env] = 0;
      D.i[IF_NUM_REACHED * n + env] = num_reached;
    }
  }
  if (obs) {
    if (active && leader) wd_write_obs<T>(P, D, env, S, act, tgt_obs, [&](int k, T v) { tile[row * ld + k] = v; });
    __syncthreads();
    flush_obs_tile<T>(tile, ld, obs, env0, EPW, D.n, Dobs);
  }
}

// fw_command_hl_kernel: one thread per env (train/train_highlevel_cmd.py:97-101, 164-166).  The raw high-level action is clipped to
// the reference's Box and conditioned in double, converted once to the handle's dtype and written, behind columns 0:18 of the env's
// observation, into the low-level controller's raw observation row, into the FW_SL_TARGET tail and (optionally) cmd_out.  A row with
// a non-finite component takes the command the tail already holds instead and is counted.
// The command of one env from its raw action (a0, a1, a2), for fw_command_hl_kernel and fw_collect_act_hl_kernel alike: c = the
// conditioned triple in the handle's dtype, written to the env's FW_SL_TARGET tail -- or, for a non-finite action, the triple the
// tail already holds, the row counted into `rejected`.  D: the env's state tile.
template <typename T>
__device__ __forceinline__ void hl_command(const DevState<T>& D, int env, double a0, double a1, double a2, double dome,
                                           int32_t* __restrict__ rejected, T (&c)[3]) {
  if (::isfinite(a0) && ::isfinite(a1) && ::isfinite(a2)) {
    // np.clip(x, lo, hi) as numpy computes it for finite x (a -0.0 stays -0.0): the Box first, then :164-166
    auto clip = [](double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); };
    const double psi = clip(a0, -kPi, kPi), alt = clip(a1, 0.0, dome), spd = clip(a2, 0.0, 30.0);
    c[0] = (T)ll_wrap_pi<double>(psi); c[1] = (T)clip(alt, 0.0, dome); c[2] = (T)clip(spd, 0.0, 100.0);
#pragma unroll
    for (int k = 0; k < 3; ++k) ll_target_slot<T>(D, env, k) = c[k];
  } else {
    if (rejected) (void)atomicAdd(rejected, 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = ll_target_slot<T>(D, env, k);
  }
}

template <typename T, int G, typename TA>
__global__ __launch_bounds__(256) void fw_command_hl_kernel(DevState<T> Dg, const TA* __restrict__ action, const uint8_t* __restrict__ mask,
                                                            const T* __restrict__ obs, int32_t obs_dim, T* __restrict__ low_obs,
                                                            T* __restrict__ cmd_out, int32_t* __restrict__ rejected, double dome) {
  constexpr int EPW = kWave / G;                     // envs per state tile of this lane mapping (fwsim_device.hpp: tile_index)
  const int env = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (env >= Dg.n) return;
  if (mask && mask[env] == 0) return;
  const DevState<T> D = tile_view<T, EPW>(Dg, env / EPW);
  const double a0 = (double)action[(size_t)env * 3], a1 = (double)action[(size_t)env * 3 + 1], a2 = (double)action[(size_t)env * 3 + 2];
  T c[3];
  hl_command<T>(D, env, a0, a1, a2, dome, rejected, c);
  const T* o = obs + (size_t)env * obs_dim;
  T* lo = low_obs + (size_t)env * fwsim_cmd::kLLObs;
#pragma unroll
  for (int k = 0; k < 18; ++k) lo[k] = o[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) { lo[18 + k] = c[k]; if (cmd_out) cmd_out[(size_t)env * 3 + k] = c[k]; }
}
