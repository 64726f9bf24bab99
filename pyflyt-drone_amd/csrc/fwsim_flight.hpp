// Flight records and path figures of the waypoint and duck tasks: what fw_trace_hl / fw_eval_track_hl are to
// the high-level command task, for FW_TASK_WAYPOINTS, FW_TASK_OBJLOCK, FW_TASK_WAYPOINT_OBJLOCK and FW_TASK_WAYPOINTS_DIRECT.
//
// fw_trace_rows_kernel: one workgroup of 1024 threads striding over N (as fw_trace_hl_kernel): the post-step row of every env --
// terminal_obs where terminated | truncated -- widened to double, then info[i, num_targets_reached] as the step left it and the
// done flag, into trace[k, i, 0 : obs_dim + 2] for k = *step_idx < T; then k + 1 into *step_idx behind a barrier (no other workgroup
// reads the counter).  The kernel only copies: which column is what is the host's business (flight.RowLayout), so one kernel serves
// every observation layout.
//
// fw_eval_track_wp_kernel: fw_eval_track_kernel's bookkeeping (same arithmetic, same order) plus twelve per-episode path sums, from
// the post-step row o and a caller-owned carry (p_prev[3], p_leg[3], a_prev[6], reached_prev) per env.  Row layout (flatten_obs):
// omega = o[0:3], v = o[att-6 : att-3], p = o[att-3 : att], a = o[att : att+act], throttle = o[att+act+5], first target row
// delta = o[att+act+6 : +3] when the row is that long.  The chord of a leg is measured between the aircraft's positions at
// consecutive reaches and the closest approach skips the reach step itself: on a reach in the last sub-step the row's delta still
// points at the target just reached while info already counts it, and neither rule reads it then.
//
// Included by fwsim.hip behind fwsim_command.hpp.
#pragma once

namespace fwsim {

constexpr int kPathSums = 12;
constexpr int kPathCarry = 13;
enum PathSum { PS_PATH_LEN = 0, PS_SPEED = 1, PS_ALT = 2, PS_ALT_MIN = 3, PS_ANG_VEL = 4, PS_ACT_DELTA = 5, PS_THROTTLE = 6,
               PS_FIRST_REACH = 7, PS_LAST_REACH = 8, PS_CHORD = 9, PS_PATH_AT_REACH = 10, PS_MISS = 11 };
enum PathCarry { PC_P_PREV = 0, PC_P_LEG = 3, PC_A_PREV = 6, PC_REACHED = 12 };
struct EvalTrackWPArgs {
  const void *obs, *terminal_obs; int32_t obs_is_f64;     // [N, obs_dim], env dtype
  int32_t obs_dim, att_dim, act_dim;
  double* cur_path;                                        // [N, 12]
  double* carry;                                           // [N, 13]
  double* fin_path;                                        // [N, E, 12]
};

__device__ __forceinline__ double wp_norm3(double x, double y, double z) {
#pragma clang fp contract(off)
  return ::sqrt(x * x + y * y + z * z);
}

__global__ __launch_bounds__(256) void fw_eval_track_wp_kernel(EvalTrackArgs A, EvalTrackWPArgs W) {
#pragma clang fp contract(off)
  // (no fused multiply-adds: the norms are the plain sums of squares the torch statement computes)
  const long long step = A.step_ctr[0] + 1;
  const double inf = __builtin_huge_val();
  const int att = W.att_dim, act = W.act_dim, D = W.obs_dim;
  const bool has_delta = D >= att + act + 9;
  for (int i = threadIdx.x; i < A.N; i += (int)blockDim.x) {
    const double rw = A.reward_is_f64 ? reinterpret_cast<const double*>(A.reward)[i] : (double)reinterpret_cast<const float*>(A.reward)[i];
    const double cr = A.cur_rew[i] + rw;
    const long long len0 = A.cur_len[i];
    const long long cl = len0 + 1;
    const bool done = (A.terminated[i] | A.truncated[i]) != 0;
    const long long c = A.counts[i];
    const void* src = done ? W.terminal_obs : W.obs;
    auto rd = [&](const void* b, int k) -> double {
      const size_t j = (size_t)i * D + k;
      return W.obs_is_f64 ? reinterpret_cast<const double*>(b)[j] : (double)reinterpret_cast<const float*>(b)[j];
    };
    auto o = [&](int k) -> double { return rd(src, k); };
    double* cy = W.carry + (size_t)i * kPathCarry;
    double* cp = W.cur_path + (size_t)i * kPathSums;
    double s[kPathSums];
#pragma unroll
    for (int k = 0; k < kPathSums; ++k) s[k] = len0 == 0 ? ((k == PS_ALT_MIN || k == PS_MISS) ? inf : 0.0) : cp[k];
    const double p0 = o(att - 3), p1 = o(att - 2), p2 = o(att - 1);
    const double r = A.info ? (double)A.info[(size_t)i * A.info_dim] : 0.0;
    const bool reach = r > cy[PC_REACHED];
    s[PS_PATH_LEN] += wp_norm3(p0 - cy[PC_P_PREV], p1 - cy[PC_P_PREV + 1], p2 - cy[PC_P_PREV + 2]);
    s[PS_SPEED] += wp_norm3(o(att - 6), o(att - 5), o(att - 4));
    s[PS_ALT] += p2;
    s[PS_ALT_MIN] = p2 < s[PS_ALT_MIN] ? p2 : s[PS_ALT_MIN];
    s[PS_ANG_VEL] += wp_norm3(o(0), o(1), o(2));
    double da = 0.0;
    for (int j = 0; j < act; ++j) da += ::fabs(o(att + j) - cy[PC_A_PREV + j]);
    s[PS_ACT_DELTA] += da;
    s[PS_THROTTLE] += o(att + act + 5);
    if (reach) {
      if (s[PS_FIRST_REACH] == 0.0) s[PS_FIRST_REACH] = (double)cl;
      s[PS_LAST_REACH] = (double)cl;
      s[PS_CHORD] += wp_norm3(p0 - cy[PC_P_LEG], p1 - cy[PC_P_LEG + 1], p2 - cy[PC_P_LEG + 2]);
      s[PS_PATH_AT_REACH] = s[PS_PATH_LEN];
      s[PS_MISS] = inf;
    } else if (has_delta) {
      const double d = wp_norm3(o(att + act + 6), o(att + act + 7), o(att + act + 8));
      s[PS_MISS] = d < s[PS_MISS] ? d : s[PS_MISS];
    }
    if (done && c < A.targets[i]) {
      const size_t e = (size_t)i * A.E + (size_t)(c < A.E ? c : A.E - 1);
      A.fin_rew[e] = cr; A.fin_len[e] = cl; A.fin_step[e] = step;
      if (A.info) for (int k = 0; k < A.info_dim; ++k) A.fin_info[e * A.info_dim + k] = A.info[(size_t)i * A.info_dim + k];
#pragma unroll
      for (int k = 0; k < kPathSums; ++k) W.fin_path[e * kPathSums + k] = s[k];
      A.counts[i] = c + 1;
    }
    A.cur_rew[i] = done ? 0.0 : cr;
    A.cur_len[i] = done ? 0 : cl;
#pragma unroll
    for (int k = 0; k < kPathSums; ++k) cp[k] = done ? ((k == PS_ALT_MIN || k == PS_MISS) ? inf : 0.0) : s[k];
    if (done) {                                          // the new episode's first observation seeds the carry
      for (int k = 0; k < 3; ++k) { const double q = rd(W.obs, att - 3 + k); cy[PC_P_PREV + k] = q; cy[PC_P_LEG + k] = q; }
      for (int j = 0; j < 6; ++j) cy[PC_A_PREV + j] = j < act ? rd(W.obs, att + j) : 0.0;
      cy[PC_REACHED] = 0.0;
    } else {
      cy[PC_P_PREV] = p0; cy[PC_P_PREV + 1] = p1; cy[PC_P_PREV + 2] = p2;
      if (reach) { cy[PC_P_LEG] = p0; cy[PC_P_LEG + 1] = p1; cy[PC_P_LEG + 2] = p2; }
      for (int j = 0; j < act; ++j) cy[PC_A_PREV + j] = o(att + j);
      cy[PC_REACHED] = r;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) A.step_ctr[0] = step;
}

__global__ __launch_bounds__(1024) void fw_trace_rows_kernel(const void* __restrict__ obs, const void* __restrict__ terminal_obs,
                                                            const uint8_t* __restrict__ terminated, const uint8_t* __restrict__ truncated,
                                                            const int32_t* __restrict__ info, int32_t info_dim, int32_t info_col,
                                                            int32_t obs_is_f64, int32_t N, int32_t D, double* __restrict__ trace,
                                                            int32_t Tn, int64_t* __restrict__ step_idx) {
  const long long k = step_idx[0];
  if (k >= 0 && k < (long long)Tn) {
    for (int i = threadIdx.x; i < N; i += (int)blockDim.x) {
      const bool te = terminated && terminated[i] != 0, tr = truncated && truncated[i] != 0;
      const void* src = ((te || tr) && terminal_obs) ? terminal_obs : obs;
      double* out = trace + ((size_t)k * (size_t)N + (size_t)i) * (size_t)(D + 2);
      const size_t q = (size_t)i * D;
      if (obs_is_f64) for (int j = 0; j < D; ++j) out[j] = reinterpret_cast<const double*>(src)[q + j];
      else            for (int j = 0; j < D; ++j) out[j] = (double)reinterpret_cast<const float*>(src)[q + j];
      out[D] = info ? (double)info[(size_t)i * info_dim + info_col] : 0.0;
      out[D + 1] = te ? 1.0 : (tr ? 2.0 : 0.0);
    }
  }
  __syncthreads();                                   // every thread has read the counter before it moves
  if (threadIdx.x == 0) step_idx[0] = k + 1;
}

}  // namespace fwsim
