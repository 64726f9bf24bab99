// Commanding the low-level controller (FW_TASK_LOWLEVEL, DESIGN.md section 2d "Commanding the controller"): the command input a
// layer above the controller drives, and a per-step trace of how the controller follows it.
//
// fw_command_ll_kernel: one thread per env.  Env i takes row min(*step_idx, T - 1) of a caller-owned [T, N, 3] schedule of
// (psi, h, V) commands (row 0 without step_idx), conditions it in double as train/train_highlevel_cmd.py:164-166 does -- psi
// wrapped to [-pi, pi) by ll_wrap_pi, h clipped to [0, flight_dome_size], V clipped to [0, 100] -- and writes the result, in the
// handle's dtype, into the env's FW_SL_TARGET tail (the target the next fw_step's reward reads) and, optionally, into obs[i, 18:21]
// (what the next policy forward sees).  A row with a non-finite component is left as it is and counted.  The step index is only
// read, so the kernel can sit in a captured hipGraph in front of the act / fw_step pair and pick its row on the device.
//
// fw_trace_ll_kernel: one workgroup of 1024 threads striding over N (as fw_eval_track_ll): the post-step row of every env --
// terminal_obs where terminated | truncated -- as 8 doubles (o[18], o[5], o[19], o[11], o[20], |o[6:9]|, |o[0:3]|, flag) into
// trace[k, i, :] for k = *step_idx < T, then k + 1 into *step_idx behind a barrier (no other workgroup reads the counter).
//
// fw_trace_hl_kernel: the same for the high-level command task (DESIGN.md section 2e "Evaluation"): the post-step row [30] and the
// conditioned command c [3] in force during the step, as 11 doubles (c0, o[5], c1, o[11], c2, |o[6:9]|, |o[0:3]|, o[9], o[10],
// info[i, num_targets_reached] as the step left it, flag) into trace[k, i, :].
//
// Included by fwsim.hip behind the low-level task's kernels: the target is written through their accessor ll_target_slot.
#pragma once

namespace fwsim_cmd {
constexpr int kTraceCols = 8;
constexpr int kLLObs = 21;
constexpr int kTraceColsHL = 11;
constexpr int kHLObs = 30;
}

template <typename T, int G>
__global__ __launch_bounds__(256) void fw_command_ll_kernel(DevState<T> Dg, const double* __restrict__ cmd, int32_t Tn,
                                                            const int64_t* __restrict__ step_idx, const uint8_t* __restrict__ mask,
                                                            T* __restrict__ obs, int32_t* __restrict__ rejected, double dome) {
  constexpr int EPW = kWave / G;                     // envs per state tile of this lane mapping (fwsim_device.hpp: tile_index)
  const int env = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (env >= Dg.n) return;
  if (mask && mask[env] == 0) return;
  long long row = 0;
  if (step_idx) {
    row = step_idx[0];
    row = row < (long long)Tn - 1 ? row : (long long)Tn - 1;
    row = row > 0 ? row : 0;
  }
  const double* c = cmd + ((size_t)row * (size_t)Dg.n + (size_t)env) * 3;
  const double psi = c[0], h = c[1], v = c[2];
  if (!(::isfinite(psi) && ::isfinite(h) && ::isfinite(v))) {
    if (rejected) (void)atomicAdd(rejected, 1);
    return;
  }
  // np.clip(x, lo, hi) as numpy computes it for finite x (a -0.0 stays -0.0)
  const double tc[3] = { ll_wrap_pi<double>(psi), h < 0.0 ? 0.0 : (h > dome ? dome : h), v < 0.0 ? 0.0 : (v > 100.0 ? 100.0 : v) };
  const DevState<T> D = tile_view<T, EPW>(Dg, env / EPW);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const T t = (T)tc[k];
    ll_target_slot<T>(D, env, k) = t;
    if (obs) obs[(size_t)env * fwsim_cmd::kLLObs + 18 + k] = t;
  }
}

__global__ __launch_bounds__(1024) void fw_trace_ll_kernel(const void* __restrict__ obs, const void* __restrict__ terminal_obs,
                                                          const uint8_t* __restrict__ terminated, const uint8_t* __restrict__ truncated,
                                                          int32_t obs_is_f64, int32_t N, double* __restrict__ trace, int32_t Tn,
                                                          int64_t* __restrict__ step_idx) {
#pragma clang fp contract(off)
  // (no fused multiply-adds: the norms are the plain sums of squares a torch / numpy restatement computes)
  const long long k = step_idx[0];
  if (k >= 0 && k < (long long)Tn) {
    for (int i = threadIdx.x; i < N; i += (int)blockDim.x) {
      const bool te = terminated && terminated[i] != 0, tr = truncated && truncated[i] != 0;
      const void* src = ((te || tr) && terminal_obs) ? terminal_obs : obs;
      auto o = [&](int j) -> double {
        const size_t q = (size_t)i * fwsim_cmd::kLLObs + j;
        return obs_is_f64 ? reinterpret_cast<const double*>(src)[q] : (double)reinterpret_cast<const float*>(src)[q];
      };
      const double v0 = o(6), v1 = o(7), v2 = o(8), w0 = o(0), w1 = o(1), w2 = o(2);
      const double row[fwsim_cmd::kTraceCols] = { o(18), o(5), o(19), o(11), o(20), ::sqrt(v0 * v0 + v1 * v1 + v2 * v2),
                                                  ::sqrt(w0 * w0 + w1 * w1 + w2 * w2), te ? 1.0 : (tr ? 2.0 : 0.0) };
      double* out = trace + ((size_t)k * (size_t)N + (size_t)i) * fwsim_cmd::kTraceCols;
#pragma unroll
      for (int j = 0; j < fwsim_cmd::kTraceCols; ++j) out[j] = row[j];
    }
  }
  __syncthreads();                                   // every thread has read the counter before it moves
  if (threadIdx.x == 0) step_idx[0] = k + 1;
}

__global__ __launch_bounds__(1024) void fw_trace_hl_kernel(const void* __restrict__ obs, const void* __restrict__ terminal_obs,
                                                          const uint8_t* __restrict__ terminated, const uint8_t* __restrict__ truncated,
                                                          const void* __restrict__ command, const int32_t* __restrict__ info,
                                                          int32_t info_dim, int32_t info_col, int32_t obs_is_f64, int32_t N,
                                                          double* __restrict__ trace, int32_t Tn, int64_t* __restrict__ step_idx) {
#pragma clang fp contract(off)
  const long long k = step_idx[0];
  if (k >= 0 && k < (long long)Tn) {
    for (int i = threadIdx.x; i < N; i += (int)blockDim.x) {
      const bool te = terminated && terminated[i] != 0, tr = truncated && truncated[i] != 0;
      const void* src = ((te || tr) && terminal_obs) ? terminal_obs : obs;
      auto o = [&](int j) -> double {
        const size_t q = (size_t)i * fwsim_cmd::kHLObs + j;
        return obs_is_f64 ? reinterpret_cast<const double*>(src)[q] : (double)reinterpret_cast<const float*>(src)[q];
      };
      auto c = [&](int j) -> double {
        const size_t q = (size_t)i * 3 + j;
        return obs_is_f64 ? reinterpret_cast<const double*>(command)[q] : (double)reinterpret_cast<const float*>(command)[q];
      };
      const double v0 = o(6), v1 = o(7), v2 = o(8), w0 = o(0), w1 = o(1), w2 = o(2);
      const double reached = info ? (double)info[(size_t)i * info_dim + info_col] : 0.0;
      const double row[fwsim_cmd::kTraceColsHL] = { c(0), o(5), c(1), o(11), c(2), ::sqrt(v0 * v0 + v1 * v1 + v2 * v2),
                                                    ::sqrt(w0 * w0 + w1 * w1 + w2 * w2), o(9), o(10), reached,
                                                    te ? 1.0 : (tr ? 2.0 : 0.0) };
      double* out = trace + ((size_t)k * (size_t)N + (size_t)i) * fwsim_cmd::kTraceColsHL;
#pragma unroll
      for (int j = 0; j < fwsim_cmd::kTraceColsHL; ++j) out[j] = row[j];
    }
  }
  __syncthreads();                                   // every thread has read the counter before it moves
  if (threadIdx.x == 0) step_idx[0] = k + 1;
}
