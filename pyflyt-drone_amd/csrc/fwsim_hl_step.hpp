// The high-level command task with the frozen controller at the control rate (controller_hz): the controller
// runs inside fw_step_hl's kernel, once in front of every Aviary step of the agent step, instead of once per agent step in a launch
// of its own.  fw_step_kernel_wdc is fw_step_kernel_wd (fwsim_direct.hpp, untouched) with two differences: it takes no actions --
// the command in force is the env's FW_SL_TARGET tail, which fw_command_hl / fw_collect_act_hl wrote -- and in front of every
// stepping Aviary step the env's lanes build the controller's raw row (attitude block of the current rigid state, the six actuator
// commands last issued, the command), normalise it with the frozen statistics and evaluate the policy net.
//
// ctl_forward is the controller, one function for the step kernel on either lane mapping and for fw_controller_forward_kernel (one
// thread per env): every unit of every layer is one chain of fused multiply-adds in a fixed order, evaluated by exactly one lane, so
// how the units are spread over lanes does not change a bit of the result.
//   h1[j] = ppo_tanh(fma(x[20], W1[20][j], ... fma(x[0], W1[0][j], b1[j])))      j = 0 .. 63   (d ascending)
//   h2[j] = ppo_tanh(fma(h1[63], W2[63][j], ... fma(h1[0], W2[0][j], b2[j])))                  (k ascending)
//   a[o]  = fma(h2[63], Wo[63][o], ... fma(h2[0], Wo[0][o], bo[o]))              o = 0 .. 5    (k ascending)
// NL lanes share an env: lane `sub` takes the eight hidden units 8 sub .. 8 sub + 7 (NL = 8) or all of them, eight at a time
// (NL = 1); the outputs go one to a lane (NL = 8: lanes 0-5) or all six to the one lane.  x, h1 and h2 pass through the env's LDS row
// (2 x 64 floats: [x | h2][h1 | a]); the exchange is ordered by wave-level fences -- the callers run it in divergent code, where a
// workgroup barrier has no place.  The weights are the policy net of the six-action flat image (fw_ppo_param_count_a(21, 6) floats,
// what fw_collect_act_hl reads as low_params), read in place: from LDS where the caller staged them (the 8-lane step kernel), else
// from global memory through the constant address space (ctl_const_ptr) -- every lane wants the same weight at the same time, so the
// addresses are wave-uniform and the loads scalar; through a plain pointer they would be vector loads, each with its own round trip.
//
// Included by fwsim.hip behind fwsim_direct.hpp.
#pragma once

namespace fwsim_ctl {
constexpr int kD = fwsim_cmd::kLLObs, kDp = (kD + 1) & ~1, kH = fwsim::kPH, kA = 6;
// the policy net at the front of the flat image (fwsim_ppo.hpp: ppo_net_params)
constexpr int oW1 = 0, ob1 = oW1 + kDp * kH, oW2 = ob1 + kH, ob2 = oW2 + kH * kH, oWo = ob2 + kH, obo = oWo + kH * kA;
constexpr int kNetFloats = obo + kA, kNetFloatsPad = (kNetFloats + 3) & ~3;
constexpr int kRowLd = 2 * kH + 1;                  // an env's activation row (odd stride: the envs of a wave sit on different banks)
constexpr int kStatDoubles = 2 * 24;                // sqrt(var + eps) and mean of the 21 columns

typedef const float __attribute__((address_space(4)))* ctl_const_ptr;      // read-only for the whole launch

struct CtlArgs {
  const float* params;               // the controller's flat image
  const double *mean, *var;          // its frozen observation statistics [21]
  float clip, eps;
  void* low_action;                  // T[N, 6]: the output in force at the end of the step (may be null)
};

// LDS of fw_step_kernel_wdc behind the observation tile, and of fw_controller_forward_kernel
inline size_t ctl_lds_bytes(int envs, bool weights) {
  return sizeof(double) * kStatDoubles + sizeof(float) * ((weights ? (size_t)kNetFloatsPad : 0) + (size_t)envs * kRowLd);
}

// cstd / cmean of the normalisation, once per workgroup (the caller's barrier follows)
__device__ __forceinline__ void ctl_load_stats(const double* __restrict__ mean, const double* __restrict__ var, float eps, double* cstd, double* cmean) {
  const int t = threadIdx.x;
  if (t < kD) { cstd[t] = sqrt(var[t] + (double)eps); cmean[t] = mean[t]; }
}
// one element of the raw row, normalised as fw_collect_act_a normalises on load
__device__ __forceinline__ float ctl_normalise(double raw, double cmean, double cstd, float clip) {
  return fminf(fmaxf((float)((raw - cmean) / cstd), -clip), clip);
}

template <int NL, typename WP>
__device__ __forceinline__ void ctl_forward(WP W, float* __restrict__ rowp, int sub, float (&out)[kA]) {
  constexpr int U = 8;
  float* A = rowp;                                   // x, then h2
  float* B = rowp + kH;                              // h1, then the six outputs
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // x is in the row
#pragma unroll 1
  for (int c = sub; c < kH / U; c += NL) {
    const int j0 = c * U;
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = W[ob1 + j0 + u];
#pragma unroll 3
    for (int d = 0; d < kD; ++d) {
      const float xd = A[d];
#pragma unroll
      for (int u = 0; u < U; ++u) acc[u] = fmaf(xd, W[oW1 + d * kH + j0 + u], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) B[j0 + u] = fwsim::ppo_tanh(acc[u]);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // h1 is complete; x is dead
#pragma unroll 1
  for (int c = sub; c < kH / U; c += NL) {
    const int j0 = c * U;
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = W[ob2 + j0 + u];
#pragma unroll 4
    for (int k = 0; k < kH; ++k) {
      const float hk = B[k];
#pragma unroll
      for (int u = 0; u < U; ++u) acc[u] = fmaf(hk, W[oW2 + k * kH + j0 + u], acc[u]);
    }
    // (NL = 1: the lane's later chunks still read h1 -- h2 goes to the other half of the row)
#pragma unroll
    for (int u = 0; u < U; ++u) A[j0 + u] = fwsim::ppo_tanh(acc[u]);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // h2 is complete; h1 is dead
  if (NL == 1) {
#pragma unroll
    for (int o = 0; o < kA; ++o) out[o] = W[obo + o];
#pragma unroll 4
    for (int k = 0; k < kH; ++k) {
      const float hk = A[k];
#pragma unroll
      for (int o = 0; o < kA; ++o) out[o] = fmaf(hk, W[oWo + k * kA + o], out[o]);
    }
  } else {
    if (sub < kA) {
      float acc = W[obo + sub];
#pragma unroll 8
      for (int k = 0; k < kH; ++k) acc = fmaf(A[k], W[oWo + k * kA + sub], acc);
      B[sub] = acc;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int o = 0; o < kA; ++o) out[o] = B[o];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");    // the row is free for the next x
  }
  // the mean action, clipped to the actuator range (a NaN becomes -1, as in fw_collect_act_a)
#pragma unroll
  for (int o = 0; o < kA; ++o) out[o] = fminf(fmaxf(out[o], -1.0f), 1.0f);
}
}  // namespace fwsim_ctl

// fw_controller_forward: the controller on raw rows [N, 21], one thread per env -- act_out[i] = clip(ctl_forward(normalise(raw[i])), +-1)
template <typename T, typename TO>
__global__ __launch_bounds__(kWave) void fw_controller_forward_kernel(const float* __restrict__ params, const T* __restrict__ raw, int N,
                                                                      const double* __restrict__ mean, const double* __restrict__ var,
                                                                      float clip, float eps, TO* __restrict__ act_out) {
  using namespace fwsim_ctl;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* cstd = reinterpret_cast<double*>(smem_raw);
  double* cmean = cstd + kStatDoubles / 2;
  float* rows = reinterpret_cast<float*>(cstd + kStatDoubles);
  ctl_load_stats(mean, var, eps, cstd, cmean);
  __syncthreads();
  const int env = (int)(blockIdx.x * kWave + threadIdx.x);
  if (env >= N) return;
  float* rowp = rows + threadIdx.x * kRowLd;
  const T* r = raw + (size_t)env * kD;
#pragma unroll
  for (int d = 0; d < kD; ++d) rowp[d] = ctl_normalise((double)r[d], cmean[d], cstd[d], clip);
  float a[kA];
  ctl_forward<1>((ctl_const_ptr)params, rowp, 0, a);
#pragma unroll
  for (int k = 0; k < kA; ++k) act_out[(size_t)env * kA + k] = (TO)a[k];
}

// The controller's raw row of the current rigid state: the first twelve columns of the Euler observation, by the arithmetic of
// write_obs_attitude (angular velocity and linear velocity in the body frame of S.q, Euler angles, position).
template <typename T>
__device__ __forceinline__ void ctl_attitude_row(const Rigid<T>& S, T (&x)[12]) {
  T Rq[9], av[3], lv[3], eul[3];
  rot_from_quat(S.q, Rq);
  mtv(Rq, S.w, av);
  mtv(Rq, S.v, lv);
  (void)euler_from_quat(S.q, eul);
#pragma unroll
  for (int k = 0; k < 3; ++k) { x[k] = av[k]; x[3 + k] = eul[k]; x[6 + k] = lv[k]; x[9 + k] = S.p[k]; }
}

// K1 (waypoints, direct actuator commands, the controller in the loop): one agent step.  The frame is fw_step_kernel_wd's -- one
// wave per workgroup, G lanes per env, one tick site shared by the step's Aviary steps and the warm-up of an in-kernel reset,
// outputs latched in registers and stored once at the end.  Warm-up steps keep the all-zero setpoint and run no controller; an
// env that is done at entry runs nothing.
template <typename T, int G, bool WIND>
__global__ __launch_bounds__(kWave) void fw_step_kernel_wdc(const Params<T>* __restrict__ Pp, const ObjC<T>* __restrict__ OCp, DevState<T> Dg,
                                                            fwsim_ctl::CtlArgs CA, T* __restrict__ obs, T* __restrict__ reward,
                                                            uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
                                                            T* __restrict__ terminal_obs, int32_t* __restrict__ info) {
  using namespace fwsim_ctl;
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

  // ---- the controller's LDS behind the tile: statistics, (G = 8) the policy net, one activation row per env ----
  double* cstd = reinterpret_cast<double*>(smem_raw + Dg.stash_off);
  double* cmean = cstd + kStatDoubles / 2;
  float* wlds = reinterpret_cast<float*>(cstd + kStatDoubles);
  float* rowp = wlds + (G == 8 ? kNetFloatsPad : 0) + row * kRowLd;
  ctl_load_stats(CA.mean, CA.var, CA.eps, cstd, cmean);
  if (G == 8) {
    int i0 = 0;
    if ((reinterpret_cast<uintptr_t>(CA.params) & 15) == 0) {       // (an allocation of its own is; a view into a larger buffer may not be)
      const float4* __restrict__ src = reinterpret_cast<const float4*>(CA.params);
      float4* dst = reinterpret_cast<float4*>(wlds);
      for (int i = lane; i < kNetFloats / 4; i += kWave) dst[i] = src[i];
      i0 = kNetFloats & ~3;
    }
    for (int i = i0 + lane; i < kNetFloats; i += kWave) wlds[i] = CA.params[i];
  }
  __syncthreads();                                   // (uniform: before anything diverges)

  int32_t step_count = D.i[IF_STEP * n + envc];
  int32_t tick = D.i[IF_TICK * n + envc];
  int32_t episode = D.i[IF_EPISODE * n + envc];
  int32_t flags = D.i[IF_FLAGS * n + envc];
  int32_t num_reached = D.i[IF_NUM_REACHED * n + envc];
  Rigid<T> S;
  load_rigid<T>(D, envc, S);
  T new_dist = D.r[RF_NEW_DIST * n + envc];
  T ep_return = D.r[RF_EP_RETURN * n + envc];
  T hl_cmd[3], act[6];                               // the tail: the command in force, the actuator commands last issued
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
  LaneAct<T> LA; LA.a = (T)0; LA.cmd = (T)0;
  if (G == 8) lane_act_scatter<T>(S, LA);

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
      if (CA.low_action && leader) {                  // the controller's output in force when the step ended (a reset below zeroes act)
        T* la = reinterpret_cast<T*>(CA.low_action) + (size_t)env * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) la[k] = act[k];
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
      if (stepping) {
        // ---- the controller, at the rate it was trained at: (attitude block, last actuator commands, command) -> six commands ----
        T xa[12];
        ctl_attitude_row<T>(S, xa);
        if (leader) {
#pragma unroll
          for (int d = 0; d < 12; ++d) rowp[d] = ctl_normalise((double)xa[d], cmean[d], cstd[d], CA.clip);
#pragma unroll
          for (int d = 0; d < 6; ++d) rowp[12 + d] = ctl_normalise((double)act[d], cmean[12 + d], cstd[12 + d], CA.clip);
#pragma unroll
          for (int d = 0; d < 3; ++d) rowp[18 + d] = ctl_normalise((double)hl_cmd[d], cmean[18 + d], cstd[18 + d], CA.clip);
        }
        float a[kA];
        if constexpr (G == 8) ctl_forward<G>(wlds, rowp, sub, a);
        else ctl_forward<G>((ctl_const_ptr)CA.params, rowp, sub, a);
#pragma unroll
        for (int k = 0; k < 6; ++k) act[k] = (T)a[k];
      }
      // motor noise of this Aviary step; the warm-up runs under a zero setpoint without noise
      T z0 = (T)0, z1 = (T)0;
      if (P.has_noise && stepping) rng_normal2<T>(P, genv, (uint32_t)episode, (uint32_t)(tick / P.ticks_per_aviary), z0, z1);
      // mode -1: the surfaces take a[0..4] as given, the throttle command is 0.5 a[5] + 0.5 (as FW_TASK_LOWLEVEL)
      T c_eff[FW_NUM_ACTUATORS];
#pragma unroll
      for (int c = 0; c < FW_NUM_SURFACES; ++c) c_eff[c] = stepping ? act[c] : (T)0;
      c_eff[FW_NUM_SURFACES] = stepping ? act[5] * (T)0.5 + (T)0.5 : (T)0;
      if (G == 8) LA.cmd = lane_pick5<T>(c_eff[0], c_eff[1], c_eff[2], c_eff[3], c_eff[4]);
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
