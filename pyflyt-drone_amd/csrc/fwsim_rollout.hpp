// fwsim_rollout.hpp -- device kernels of the rollout collector (caller side of the env
// step): GAE scan and the fused VecNormalize observation pass.  HBM-bound, coalesced.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fwsim {

// K3: GAE.  One lane per env; the time loop runs backwards in registers; every access at
// step t is a coalesced row of the [T, N] buffers.  (SB3 RolloutBuffer.compute_returns_and_advantage.)
__global__ __launch_bounds__(256) void fw_gae_kernel(const float* __restrict__ rewards, const float* __restrict__ values,
                                                     const float* __restrict__ episode_starts,
                                                     const float* __restrict__ last_values,
                                                     const float* __restrict__ last_dones, float* __restrict__ adv,
                                                     float* __restrict__ ret, int T, int N, float gamma, float lam) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float next_value = last_values[n];
  float next_non_terminal = 1.0f - last_dones[n];
  float last_gae = 0.0f;
  for (int t = T - 1; t >= 0; --t) {
    const size_t i = (size_t)t * N + n;
    const float v = values[i];
    const float delta = rewards[i] + gamma * next_value * next_non_terminal - v;
    last_gae = delta + gamma * lam * next_non_terminal * last_gae;
    adv[i] = last_gae;
    ret[i] = last_gae + v;
    next_value = v;
    next_non_terminal = 1.0f - episode_starts[i];
  }
}

// Episode bookkeeping of an evaluation (evaluate.ReplayedEvaluation, SB3's evaluate_policy loop): one vec-step's rewards and dones into
// the running accumulators, a finished episode into the next slot of its env -- what the harness did with ~20 framework ops.
// One workgroup: the step counter is read by everybody and advanced once, behind the barrier.
struct EvalTrackArgs {
  const void* reward; int32_t reward_is_f64;
  const uint8_t *terminated, *truncated;
  const int32_t* info; int32_t info_dim;     // may be NULL
  const int64_t* targets;                    // [N] episodes wanted of each env
  int64_t* counts;                           // [N] episodes taken so far
  double* cur_rew; int64_t* cur_len;         // [N] accumulators of the running episodes
  int64_t* step_ctr;                         // [1] vec-steps so far
  double* fin_rew; int64_t *fin_len, *fin_step; int32_t* fin_info;      // [N, E] (fin_info [N, E, info_dim])
  int32_t N, E;
};
// FW_TASK_LOWLEVEL's tracking sums (fw_eval_track_ll): from the post-step observation row o -- the terminal
// observation on the step that ends an episode -- e_psi = wrap(o[18] - o[5]), e_h = o[19] - o[11], e_V = o[20] - |o[6:9]|,
// w = |o[0:3]|; per env the running sums |e_psi|, e_psi^2, |e_h|, e_h^2, |e_V|, e_V^2, w, and for a finished episode those seven
// plus survived = !terminated.  All in double, whatever the env dtype.
constexpr int kTrackSums = 7;
struct EvalTrackLLArgs {
  const void *obs, *terminal_obs; int32_t obs_is_f64;     // [N, 21], env dtype
  double* cur_track;                                       // [N, 7]
  double* fin_track;                                       // [N, E, 8]
};
// The high-level command task's sums (fw_eval_track_hl, DESIGN.md section 2e "Evaluation"): o is the post-step row [30] (columns 0:18
// are the low-level observation's), c the conditioned command in force during the step, p the command of the step before.
// e_psi = wrap(c0 - o[5]), e_h = c1 - o[11], e_V = c2 - |o[6:9]|, w = |o[0:3]|; d = (|wrap(c0 - p0)|, |c1 - p1|, |c2 - p2|), 0 on an
// episode's first step; sat = c1 or c2 on a bound of the action Box.  Eleven running sums per env, in double; X carries obs /
// terminal_obs / cur_track [N, 11] / fin_track [N, E, 11] (no survived column).  prev_cmd takes c on every step.
constexpr int kTrackSumsHL = 11;
constexpr int kHLObs = 30;
struct EvalTrackHLArgs {
  const void* command;                                     // [N, 3], env dtype (X.obs_is_f64)
  double* prev_cmd;                                        // [N, 3]
  double alt_high, speed_high;
};
template <bool TRACK, bool HL = false>
__device__ __forceinline__ void eval_track_body(EvalTrackArgs A, EvalTrackLLArgs X, EvalTrackHLArgs H = EvalTrackHLArgs{}) {
  const long long step = A.step_ctr[0] + 1;
  for (int i = threadIdx.x; i < A.N; i += (int)blockDim.x) {
    const double r = A.reward_is_f64 ? reinterpret_cast<const double*>(A.reward)[i] : (double)reinterpret_cast<const float*>(A.reward)[i];
    const double cr = A.cur_rew[i] + r;
    const long long cl = A.cur_len[i] + 1;
    const bool done = (A.terminated[i] | A.truncated[i]) != 0;
    const long long c = A.counts[i];
    double ts[kTrackSums];
    if (TRACK) {
      const void* src = done ? X.terminal_obs : X.obs;
      auto o = [&](int k) -> double {
        const size_t j = (size_t)i * 21 + k;
        return X.obs_is_f64 ? reinterpret_cast<const double*>(src)[j] : (double)reinterpret_cast<const float*>(src)[j];
      };
      const double e_psi = ll_wrap_pi<double>(o(18) - o(5)), e_h = o(19) - o(11);
      const double e_v = o(20) - ::sqrt(o(6) * o(6) + o(7) * o(7) + o(8) * o(8));
      const double w = ::sqrt(o(0) * o(0) + o(1) * o(1) + o(2) * o(2));
      const double add[kTrackSums] = { ::fabs(e_psi), e_psi * e_psi, ::fabs(e_h), e_h * e_h, ::fabs(e_v), e_v * e_v, w };
#pragma unroll
      for (int k = 0; k < kTrackSums; ++k) ts[k] = X.cur_track[(size_t)i * kTrackSums + k] + add[k];
    }
    double th[kTrackSumsHL];
    if (HL) {
#pragma clang fp contract(off)
      // (no fused multiply-adds: the norms are the plain sums of squares the torch statement computes)
      const void* src = done ? X.terminal_obs : X.obs;
      auto o = [&](int k) -> double {
        const size_t j = (size_t)i * kHLObs + k;
        return X.obs_is_f64 ? reinterpret_cast<const double*>(src)[j] : (double)reinterpret_cast<const float*>(src)[j];
      };
      double cm[3], pc[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const size_t j = (size_t)i * 3 + k;
        cm[k] = X.obs_is_f64 ? reinterpret_cast<const double*>(H.command)[j] : (double)reinterpret_cast<const float*>(H.command)[j];
        pc[k] = H.prev_cmd[j];
        H.prev_cmd[j] = cm[k];
      }
      const bool first = cl == 1;                         // cur_len was 0: the episode has no previous command
      const double v0 = o(6), v1 = o(7), v2 = o(8), w0 = o(0), w1 = o(1), w2 = o(2);
      const double e_psi = ll_wrap_pi<double>(cm[0] - o(5)), e_h = cm[1] - o(11);
      const double e_v = cm[2] - ::sqrt(v0 * v0 + v1 * v1 + v2 * v2);
      const double w = ::sqrt(w0 * w0 + w1 * w1 + w2 * w2);
      const double sat = (cm[1] <= 0.0 || cm[1] >= H.alt_high || cm[2] <= 0.0 || cm[2] >= H.speed_high) ? 1.0 : 0.0;
      const double add[kTrackSumsHL] = { ::fabs(e_psi), e_psi * e_psi, ::fabs(e_h), e_h * e_h, ::fabs(e_v), e_v * e_v, w,
                                         first ? 0.0 : ::fabs(ll_wrap_pi<double>(cm[0] - pc[0])), first ? 0.0 : ::fabs(cm[1] - pc[1]),
                                         first ? 0.0 : ::fabs(cm[2] - pc[2]), sat };
#pragma unroll
      for (int k = 0; k < kTrackSumsHL; ++k) th[k] = X.cur_track[(size_t)i * kTrackSumsHL + k] + add[k];
    }
    if (done && c < A.targets[i]) {
      const size_t s = (size_t)i * A.E + (size_t)(c < A.E ? c : A.E - 1);
      A.fin_rew[s] = cr; A.fin_len[s] = cl; A.fin_step[s] = step;
      if (A.info) for (int k = 0; k < A.info_dim; ++k) A.fin_info[s * A.info_dim + k] = A.info[(size_t)i * A.info_dim + k];
      if (TRACK) {
#pragma unroll
        for (int k = 0; k < kTrackSums; ++k) X.fin_track[s * (kTrackSums + 1) + k] = ts[k];
        X.fin_track[s * (kTrackSums + 1) + kTrackSums] = A.terminated[i] ? 0.0 : 1.0;
      }
      if (HL) {
#pragma unroll
        for (int k = 0; k < kTrackSumsHL; ++k) X.fin_track[s * kTrackSumsHL + k] = th[k];
      }
      A.counts[i] = c + 1;
    }
    A.cur_rew[i] = done ? 0.0 : cr;
    A.cur_len[i] = done ? 0 : cl;
    if (TRACK) {
#pragma unroll
      for (int k = 0; k < kTrackSums; ++k) X.cur_track[(size_t)i * kTrackSums + k] = done ? 0.0 : ts[k];
    }
    if (HL) {
#pragma unroll
      for (int k = 0; k < kTrackSumsHL; ++k) X.cur_track[(size_t)i * kTrackSumsHL + k] = done ? 0.0 : th[k];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) A.step_ctr[0] = step;
}
__global__ __launch_bounds__(256) void fw_eval_track_kernel(EvalTrackArgs A) { eval_track_body<false>(A, EvalTrackLLArgs{}); }
__global__ __launch_bounds__(256) void fw_eval_track_ll_kernel(EvalTrackArgs A, EvalTrackLLArgs X) { eval_track_body<true>(A, X); }
__global__ __launch_bounds__(256) void fw_eval_track_hl_kernel(EvalTrackArgs A, EvalTrackLLArgs X, EvalTrackHLArgs H) {
  eval_track_body<false, true>(A, X, H);
}

// Episode statistics of a training run (monitor.EpisodeMonitor; SB3's Monitor / ep_info_buffer): one vec-step's rewards and dones into
// the per-env accumulators, the finished episodes into a ring of W slots in SB3's order (by vec-step, inside one by ascending env
// index; slot = push rank mod W: what collections.deque(maxlen=W) holds after extend() in env order), and the running totals.
// The state block, caller-owned and zeroed once, in 8-byte words (fw_episode_state_bytes; the layout of include/fwsim.h):
//   [0, 16)   header (EpisodeHeader below)
//   then W words each: ring_ret (double), ring_len, ring_step, ring_env, ring_trunc (int64), 4 W words ring_info (int32 [W][8])
//   then N words each: cur_ret (double), cur_len (int64)
// One workgroup, no atomics, no in-grid waits.  More than W episodes may end in one step (all envs meet the time limit together), so
// the step's dones are counted first (pass 1) and only the last W of them are written (pass 2): consecutive ranks, distinct slots.
// A done's rank: wave ballot + prefix inside the wave, an LDS scan across the waves, a running base across the passes over N.
constexpr int kEpThreads = 1024;
constexpr int kEpWaves = kEpThreads / 64;
constexpr int kEpInfo = 8;                  // info columns kept per ring entry (FW_INFO_DIM)
constexpr int kEpInfoSums = 6;              // ... of which the flags and counts are totalled (FW_INFO_NUM_TARGETS_REACHED .. FW_INFO_IS_SUCCESS)
enum EpisodeHeader { EP_EPISODES = 0, EP_STEPS = 1, EP_TRUNCATED = 2, EP_SUM_LEN = 3, EP_SUM_INFO = 4 /* .. 9 */, EP_SUM_RET = 10,
                     EP_SUM_RET2 = 11, EP_HEADER_WORDS = 16 };
struct EpisodeFoldArgs {
  const void* reward; int32_t reward_is_f64;
  const uint8_t *terminated, *truncated;
  const int32_t* info; int32_t info_dim;     // may be NULL: the ring entries then carry a zero info row
  int64_t* state;
  int32_t N, W;
};
__device__ __forceinline__ long long ep_wave_sum(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double ep_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);       // a fixed tree: the same bits in every lane, in every run
  return v;
}
__global__ __launch_bounds__(kEpThreads) void fw_episode_fold_kernel(EpisodeFoldArgs A) {
  __shared__ long long s_cnt[2][kEpWaves];
  __shared__ long long s_int[kEpWaves][2 + kEpInfoSums];
  __shared__ double s_dbl[kEpWaves][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = A.N, W = A.W;
  long long* hdr = reinterpret_cast<long long*>(A.state);
  double* ring_ret = reinterpret_cast<double*>(hdr + EP_HEADER_WORDS);
  long long* ring_len = hdr + EP_HEADER_WORDS + (size_t)W;
  long long* ring_step = ring_len + W;
  long long* ring_env = ring_step + W;
  long long* ring_trunc = ring_env + W;
  int32_t* ring_info = reinterpret_cast<int32_t*>(ring_trunc + W);
  double* cur_ret = reinterpret_cast<double*>(ring_trunc + W + (size_t)W * (kEpInfo / 2));
  long long* cur_len = reinterpret_cast<long long*>(cur_ret) + N;
  const long long pushed0 = hdr[EP_EPISODES], step = hdr[EP_STEPS] + 1;
  const int passes = (N + kEpThreads - 1) / kEpThreads;

  // pass 1: how many episodes end in this step
  long long mine = 0;
  for (int p = 0; p < passes; ++p) {
    const long long i = (long long)p * kEpThreads + tid;
    if (i < N) mine += (A.terminated[i] | A.truncated[i]) != 0;
  }
  mine = ep_wave_sum(mine);
  if (lane == 0) s_cnt[0][wave] = mine;
  __syncthreads();
  long long D = 0;
#pragma unroll
  for (int w = 0; w < kEpWaves; ++w) D += s_cnt[0][w];
  const long long first_kept = D - W;          // ranks below it would be pushed out of the ring by this very step
  __syncthreads();

  // pass 2: accumulate, rank the dones, write the last W of them, clear
  long long base = 0, n_trunc = 0, sum_len = 0, sum_info[kEpInfoSums] = {0, 0, 0, 0, 0, 0};
  double sum_ret = 0.0, sum_ret2 = 0.0;
  const int ncol = A.info ? (A.info_dim < kEpInfo ? A.info_dim : kEpInfo) : 0;
  for (int p = 0; p < passes; ++p) {
    const long long i = (long long)p * kEpThreads + tid;
    const bool on = i < N;
    bool done = false, trunc = false;
    double cr = 0.0;
    long long cl = 0;
    if (on) {
      const double r = A.reward_is_f64 ? reinterpret_cast<const double*>(A.reward)[i] : (double)reinterpret_cast<const float*>(A.reward)[i];
      cr = cur_ret[i] + r;
      cl = cur_len[i] + 1;
      trunc = A.truncated[i] != 0;
      done = trunc || A.terminated[i] != 0;
      cur_ret[i] = done ? 0.0 : cr;
      cur_len[i] = done ? 0 : cl;
    }
    const unsigned long long ballot = __ballot(done);
    if (lane == 0) s_cnt[p & 1][wave] = __popcll(ballot);
    __syncthreads();                           // (two buffers: a wave already in pass p + 1 writes the other one)
    long long before = 0, chunk = 0;
#pragma unroll
    for (int w = 0; w < kEpWaves; ++w) { const long long c = s_cnt[p & 1][w]; chunk += c; before += w < wave ? c : 0; }
    if (done) {
      const long long rank = base + before + __popcll(ballot & ((1ull << lane) - 1ull));
      int32_t row[kEpInfo];
#pragma unroll
      for (int k = 0; k < kEpInfo; ++k) row[k] = k < ncol ? A.info[(size_t)i * A.info_dim + k] : 0;
      sum_ret += cr; sum_ret2 += cr * cr; sum_len += cl; n_trunc += trunc;
#pragma unroll
      for (int k = 0; k < kEpInfoSums; ++k) sum_info[k] += row[k];
      if (rank >= first_kept) {
        const size_t s = (size_t)((pushed0 + rank) % W);
        ring_ret[s] = cr; ring_len[s] = cl; ring_step[s] = step; ring_env[s] = i; ring_trunc[s] = trunc;
#pragma unroll
        for (int k = 0; k < kEpInfo; ++k) ring_info[s * kEpInfo + k] = row[k];
      }
    }
    base += chunk;
  }

  // the step's sums: lane tree, then the waves in order -- a fixed order for the doubles
  sum_ret = ep_wave_sum(sum_ret); sum_ret2 = ep_wave_sum(sum_ret2);
  sum_len = ep_wave_sum(sum_len); n_trunc = ep_wave_sum(n_trunc);
#pragma unroll
  for (int k = 0; k < kEpInfoSums; ++k) sum_info[k] = ep_wave_sum(sum_info[k]);
  if (lane == 0) {
    s_dbl[wave][0] = sum_ret; s_dbl[wave][1] = sum_ret2;
    s_int[wave][0] = sum_len; s_int[wave][1] = n_trunc;
#pragma unroll
    for (int k = 0; k < kEpInfoSums; ++k) s_int[wave][2 + k] = sum_info[k];
  }
  __syncthreads();
  if (tid < 2 + kEpInfoSums) {
    long long v = 0;
    for (int w = 0; w < kEpWaves; ++w) v += s_int[w][tid];
    const int at = tid == 0 ? EP_SUM_LEN : tid == 1 ? EP_TRUNCATED : EP_SUM_INFO + (tid - 2);
    hdr[at] += v;
  } else if (tid < 4 + kEpInfoSums) {
    const int c = tid - (2 + kEpInfoSums);
    double v = 0.0;
    for (int w = 0; w < kEpWaves; ++w) v += s_dbl[w][c];
    double* tot = reinterpret_cast<double*>(hdr) + (c == 0 ? EP_SUM_RET : EP_SUM_RET2);
    tot[0] += v;
  } else if (tid == 4 + kEpInfoSums) {
    hdr[EP_EPISODES] = pushed0 + D;            // (every thread read both words in front of the first barrier)
    hdr[EP_STEPS] = step;
  }
}

// The same fold over many workgroups (fw_episode_fold_wide): the same state block, three launches on one stream, workgroup b owning
// envs [b * kEpSpan, min(N, (b + 1) * kEpSpan)), one env per thread.  Kernel boundaries are the only synchronisation between
// workgroups: no atomics, no in-grid waits, and a kernel that reads a header word does not write it (the idiom of fw_replay_store /
// fw_sac_update) -- only the one-workgroup finish moves the header.  The caller-owned workspace, in 8-byte words, B = ceil(N / kEpSpan):
//   [0]            D, the step's dones (written by workgroup 0 of the fold, read by the finish)
//   [1, 1 + 10 B)  part[c][b]: workgroup b's sums -- c = 0 length, 1 truncated, 2..7 the info sums (int64), 8 return, 9 squared return (double)
//   then B int32   count[b]: workgroup b's dones (written by the count kernel, read by every workgroup of the fold)
// Every word is written by the call that reads it.  The ring order comes out of a scan: a done's rank is the sum of the counts of the
// workgroups below its own, the dones of the waves below its own (LDS) and of the lanes below its own (ballot); the ranks kept by one
// step are consecutive and at most W, so no two workgroups write one slot.
#ifndef FW_EP_SPAN
#define FW_EP_SPAN 256
#endif
constexpr int kEpSpan = FW_EP_SPAN;         // envs (= threads) per workgroup of the wide form
constexpr int kEpSpanWaves = kEpSpan / 64;
constexpr int kEpParts = 4 + kEpInfoSums;   // words of part[] per workgroup
constexpr int kEpFinishThreads = 1024;
static_assert(kEpSpan % 64 == 0 && kEpSpan >= 64 && kEpSpan <= 1024, "the wide fold runs one env per thread, whole waves");
struct EpisodeWideArgs {
  EpisodeFoldArgs F;
  int64_t* ws;
  int32_t B;
};
__device__ __forceinline__ int32_t* ep_ws_count(int64_t* ws, int B) { return reinterpret_cast<int32_t*>(ws + 1 + (size_t)kEpParts * B); }

__global__ __launch_bounds__(kEpSpan) void fw_episode_count_kernel(EpisodeWideArgs X) {
  __shared__ int s_cnt[kEpSpanWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i = (long long)blockIdx.x * kEpSpan + tid;
  const bool done = i < X.F.N && (X.F.terminated[i] | X.F.truncated[i]) != 0;
  const unsigned long long ballot = __ballot(done);
  if (lane == 0) s_cnt[wave] = __popcll(ballot);
  __syncthreads();
  if (tid == 0) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kEpSpanWaves; ++w) c += s_cnt[w];
    ep_ws_count(X.ws, X.B)[blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(kEpSpan) void fw_episode_fold_wide_kernel(EpisodeWideArgs X) {
  __shared__ long long s_cnt[kEpSpanWaves][3];         // dones of the workgroups below this one, of all of them, of this wave
  __shared__ long long s_int[kEpSpanWaves][2 + kEpInfoSums];
  __shared__ double s_dbl[kEpSpanWaves][2];
  const EpisodeFoldArgs& A = X.F;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, B = X.B;
  const int N = A.N, W = A.W;
  const long long* hdr = reinterpret_cast<const long long*>(A.state);          // read only: the finish kernel writes the header
  long long* ring = reinterpret_cast<long long*>(A.state) + EP_HEADER_WORDS;
  double* ring_ret = reinterpret_cast<double*>(ring);
  long long* ring_len = ring + (size_t)W;
  long long* ring_step = ring_len + W;
  long long* ring_env = ring_step + W;
  long long* ring_trunc = ring_env + W;
  int32_t* ring_info = reinterpret_cast<int32_t*>(ring_trunc + W);
  double* cur_ret = reinterpret_cast<double*>(ring_trunc + W + (size_t)W * (kEpInfo / 2));
  long long* cur_len = reinterpret_cast<long long*>(cur_ret) + N;
  const long long pushed0 = hdr[EP_EPISODES], step = hdr[EP_STEPS] + 1;

  // the scan over workgroups: every workgroup reduces the count array itself (integers: any order)
  const int32_t* count = ep_ws_count(X.ws, B);
  long long below = 0, all = 0;
  for (int k = tid; k < B; k += kEpSpan) { const long long c = count[k]; all += c; below += k < b ? c : 0; }
  below = ep_wave_sum(below); all = ep_wave_sum(all);

  const long long i = (long long)b * kEpSpan + tid;
  bool done = false, trunc = false;
  double cr = 0.0;
  long long cl = 0;
  if (i < N) {
    const double r = A.reward_is_f64 ? reinterpret_cast<const double*>(A.reward)[i] : (double)reinterpret_cast<const float*>(A.reward)[i];
    cr = cur_ret[i] + r;
    cl = cur_len[i] + 1;
    trunc = A.truncated[i] != 0;
    done = trunc || A.terminated[i] != 0;
    cur_ret[i] = done ? 0.0 : cr;
    cur_len[i] = done ? 0 : cl;
  }
  const unsigned long long ballot = __ballot(done);
  if (lane == 0) { s_cnt[wave][0] = below; s_cnt[wave][1] = all; s_cnt[wave][2] = __popcll(ballot); }
  __syncthreads();
  long long base = 0, D = 0;
#pragma unroll
  for (int w = 0; w < kEpSpanWaves; ++w) { base += s_cnt[w][0] + (w < wave ? s_cnt[w][2] : 0); D += s_cnt[w][1]; }
  const long long first_kept = D - W;          // ranks below it would be pushed out of the ring by this very step

  long long n_trunc = 0, sum_len = 0, sum_info[kEpInfoSums] = {0, 0, 0, 0, 0, 0};
  double sum_ret = 0.0, sum_ret2 = 0.0;
  const int ncol = A.info ? (A.info_dim < kEpInfo ? A.info_dim : kEpInfo) : 0;
  if (done) {
    const long long rank = base + __popcll(ballot & ((1ull << lane) - 1ull));
    int32_t row[kEpInfo];
#pragma unroll
    for (int k = 0; k < kEpInfo; ++k) row[k] = k < ncol ? A.info[(size_t)i * A.info_dim + k] : 0;
    sum_ret = cr; sum_ret2 = cr * cr; sum_len = cl; n_trunc = trunc;
#pragma unroll
    for (int k = 0; k < kEpInfoSums; ++k) sum_info[k] = row[k];
    if (rank >= first_kept) {
      const size_t s = (size_t)((pushed0 + rank) % W);
      ring_ret[s] = cr; ring_len[s] = cl; ring_step[s] = step; ring_env[s] = i; ring_trunc[s] = trunc;
#pragma unroll
      for (int k = 0; k < kEpInfo; ++k) ring_info[s * kEpInfo + k] = row[k];
    }
  }

  // the workgroup's sums: lane tree, then the waves in order -- a fixed order for the doubles
  sum_ret = ep_wave_sum(sum_ret); sum_ret2 = ep_wave_sum(sum_ret2);
  sum_len = ep_wave_sum(sum_len); n_trunc = ep_wave_sum(n_trunc);
#pragma unroll
  for (int k = 0; k < kEpInfoSums; ++k) sum_info[k] = ep_wave_sum(sum_info[k]);
  if (lane == 0) {
    s_dbl[wave][0] = sum_ret; s_dbl[wave][1] = sum_ret2;
    s_int[wave][0] = sum_len; s_int[wave][1] = n_trunc;
#pragma unroll
    for (int k = 0; k < kEpInfoSums; ++k) s_int[wave][2 + k] = sum_info[k];
  }
  __syncthreads();
  long long* part = reinterpret_cast<long long*>(X.ws) + 1;
  if (tid < 2 + kEpInfoSums) {
    long long v = 0;
#pragma unroll
    for (int w = 0; w < kEpSpanWaves; ++w) v += s_int[w][tid];
    part[(size_t)tid * B + b] = v;
  } else if (tid < kEpParts) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < kEpSpanWaves; ++w) v += s_dbl[w][tid - (2 + kEpInfoSums)];
    reinterpret_cast<double*>(part)[(size_t)tid * B + b] = v;
  } else if (tid == kEpParts && b == 0) {
    X.ws[0] = D;
  }
}

// One workgroup: the workgroups' sums in ascending workgroup order per thread (thread t takes b = t, t + 1024, ...), lane tree, waves
// in order -- a fixed tree for the two doubles, the same bits in every run -- then the header.
__global__ __launch_bounds__(kEpFinishThreads) void fw_episode_finish_kernel(EpisodeWideArgs X) {
  constexpr int kWaves = kEpFinishThreads / 64;
  __shared__ long long s_int[kWaves][2 + kEpInfoSums];
  __shared__ double s_dbl[kWaves][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, B = X.B;
  long long* hdr = reinterpret_cast<long long*>(X.F.state);
  const long long* part = reinterpret_cast<const long long*>(X.ws) + 1;
  const double* partd = reinterpret_cast<const double*>(part);
  long long vi[2 + kEpInfoSums] = {0, 0, 0, 0, 0, 0, 0, 0};
  double vd[2] = {0.0, 0.0};
  for (int k = tid; k < B; k += kEpFinishThreads) {
#pragma unroll
    for (int c = 0; c < 2 + kEpInfoSums; ++c) vi[c] += part[(size_t)c * B + k];
    vd[0] += partd[(size_t)(2 + kEpInfoSums) * B + k]; vd[1] += partd[(size_t)(3 + kEpInfoSums) * B + k];
  }
#pragma unroll
  for (int c = 0; c < 2 + kEpInfoSums; ++c) vi[c] = ep_wave_sum(vi[c]);
  vd[0] = ep_wave_sum(vd[0]); vd[1] = ep_wave_sum(vd[1]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 2 + kEpInfoSums; ++c) s_int[wave][c] = vi[c];
    s_dbl[wave][0] = vd[0]; s_dbl[wave][1] = vd[1];
  }
  __syncthreads();
  if (tid < 2 + kEpInfoSums) {
    long long v = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) v += s_int[w][tid];
    const int at = tid == 0 ? EP_SUM_LEN : tid == 1 ? EP_TRUNCATED : EP_SUM_INFO + (tid - 2);
    hdr[at] += v;
  } else if (tid < kEpParts) {
    const int c = tid - (2 + kEpInfoSums);
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) v += s_dbl[w][c];
    double* tot = reinterpret_cast<double*>(hdr) + (c == 0 ? EP_SUM_RET : EP_SUM_RET2);
    tot[0] += v;
  } else if (tid == kEpParts) {
    hdr[EP_EPISODES] += X.ws[0];
    hdr[EP_STEPS] += 1;
  }
}

// K4a: per-column batch moments of obs[N,D] (two-pass-free: shifted sums in double), one
// workgroup per column chunk; K4b merges them into the running statistics (Chan et al.) and
// K4c normalises.  N*D is small (4096 x 28), so the three launches are latency-trivial and
// can all be captured in the rollout hipGraph.
template <typename TIN>
__global__ __launch_bounds__(256) void fw_obs_moments_kernel(const TIN* __restrict__ obs, int N, int D,
                                                             double* __restrict__ part /*[gridDim.x][2][D]*/) {
  // Block b reduces rows [r0, r1).  Thread t handles column t % D of rows r0 + t / D + k * (256 / D): consecutive
  // threads read consecutive addresses; one LDS reduction over the 256 / D row slots at the end.  (D <= 256)
  __shared__ double sm1[256], sm2[256];
  const int t = threadIdx.x;
  const int rows_per_block = (N + gridDim.x - 1) / gridDim.x;
  const int r0 = blockIdx.x * rows_per_block, r1 = min(N, r0 + rows_per_block);
  const int rpi = 256 / D;
  const bool on = t < rpi * D;
  const int col = on ? t % D : 0, rr = on ? t / D : 0;
  double a0 = 0.0, b0 = 0.0, a1 = 0.0, b1 = 0.0;          // two chains: the loads are independent, the adds are not
  if (on) {
    int r = r0 + rr;
    for (; r + rpi < r1; r += 2 * rpi) {
      const double x0 = (double)obs[(size_t)r * D + col], x1 = (double)obs[(size_t)(r + rpi) * D + col];
      a0 += x0; b0 += x0 * x0; a1 += x1; b1 += x1 * x1;
    }
    if (r < r1) { const double x0 = (double)obs[(size_t)r * D + col]; a0 += x0; b0 += x0 * x0; }
  }
  sm1[t] = a0 + a1; sm2[t] = b0 + b1;
  __syncthreads();
  if (t < D) {
    double s = 0.0, s2 = 0.0;
    for (int k = 0; k < rpi; ++k) { s += sm1[k * D + t]; s2 += sm2[k * D + t]; }
    part[((size_t)blockIdx.x * 2 + 0) * D + t] = s;
    part[((size_t)blockIdx.x * 2 + 1) * D + t] = s2;
  }
}

// RunningMeanStd.update_from_moments (SB3 common/running_mean_std.py); one block of 256 threads:
// thread (q, d) sums a quarter of the per-block partials of column d (fixed order => reproducible), D <= 64 per pass
// `acc` (may be null): double[2 D + 1] accumulators of the batch sums (sum, sum of squares per column, rows) -- what a
// sharded job all-reduces once per rollout to bring every rank's statistics to the statistics of ALL envs.
__global__ __launch_bounds__(256) void fw_obs_merge_kernel(const double* __restrict__ part, int nblocks, int N, int D,
                                                           double* __restrict__ mean, double* __restrict__ var,
                                                           double* __restrict__ count, double* __restrict__ acc) {
  __shared__ double sm1[256], sm2[256];
  const int t = threadIdx.x, q = t >> 6, dl = t & 63;
  const double cnt = count[0];
  for (int d0 = 0; d0 < D; d0 += 64) {
    const int d = d0 + dl;
    double s = 0, s2 = 0;
    if (d < D)
      for (int b = q; b < nblocks; b += 4) { s += part[((size_t)b * 2 + 0) * D + d]; s2 += part[((size_t)b * 2 + 1) * D + d]; }
    sm1[t] = s; sm2[t] = s2;
    __syncthreads();
    if (q == 0 && d < D) {
      s = sm1[dl] + sm1[64 + dl] + sm1[128 + dl] + sm1[192 + dl];
      s2 = sm2[dl] + sm2[64 + dl] + sm2[128 + dl] + sm2[192 + dl];
      const double bm = s / N;
      double bv = s2 / N - bm * bm;                // population variance, as np.var
      bv = bv < 0 ? 0 : bv;
      const double delta = bm - mean[d];
      const double tot = cnt + N;
      const double new_mean = mean[d] + delta * N / tot;
      const double m2 = var[d] * cnt + bv * N + delta * delta * cnt * N / tot;
      mean[d] = new_mean;
      var[d] = m2 / tot;
      if (acc) { acc[d] += s; acc[D + d] += s2; }
    }
    __syncthreads();
  }
  if (t == 0) { count[0] = cnt + N; if (acc) acc[2 * D] += (double)N; }
}

template <typename TIN>
__global__ __launch_bounds__(256) void fw_obs_normalize_kernel(const TIN* __restrict__ obs, int total, int D,
                                                               const double* __restrict__ mean,
                                                               const double* __restrict__ var, float clip, float eps,
                                                               float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int d = i % D;
  double z = ((double)obs[i] - mean[d]) / sqrt(var[d] + (double)eps);
  float zf = (float)z;
  out[i] = fminf(fmaxf(zf, -clip), clip);
}

}  // namespace fwsim
