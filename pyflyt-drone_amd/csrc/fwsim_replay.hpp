// The SAC replay ring: fp32 rows [obs d | action A | reward | next_obs d | done] at a device-resident cursor, and every gather from it --
// the uniform sample, n-step returns, hindsight goal relabelling -- plus the in-place normalisation of a gathered batch.  (Prioritized
// replay, csrc/fwsim_per.hpp, draws its own index; it uses this header's cursor, draw word and row copy.)  What the kernels share is
// written once, as force-inlined functions of plain values: replay_cursor / _newest, replay_philox, replay_draw_word / _uniform,
// replay_walk, replay_copy_row.  The device counters (int64[4]) are fwsim_sac.hpp's: no kernel writes one it reads in the same launch.
// Ballots and lane reads are the compiler builtins, not hip's __ballot / __shfl / __ffsll: with the wrappers in the n-step gather sixteen
// camera kernels of this translation unit came out with two operands of one v_or3_b32 swapped and their schedule moved behind it.
// ds_bpermute takes the source lane as a byte address, lane << 2.
#pragma once
#include "fwsim_sac.hpp"

namespace fwsim {

// the ring cursor: a value the store could not use (negative, or a vec-step of N rows would not fit behind it) reads as 0
__device__ __forceinline__ int64_t replay_cursor(const int64_t* ctr, int64_t capacity, int N) {
  int64_t cursor = ctr[0];
  if (cursor < 0 || cursor + N > capacity) cursor = 0;
  return cursor;
}
// first row of the newest vec-step stored: the N rows in front of the (normalised) cursor
__device__ __forceinline__ uint32_t replay_newest(int64_t cursor, int64_t capacity, int N) { return (uint32_t)(cursor == 0 ? capacity - N : cursor - N); }
// batch row b's Philox block of gradient step gs under `tag`
__device__ __forceinline__ void replay_philox(int b, uint64_t gs, uint32_t tag, uint64_t seed, uint32_t o[4]) {
  philox4x32_10((uint32_t)b, 0u, (uint32_t)gs, (uint32_t)(gs >> 32) ^ tag, (uint32_t)seed, (uint32_t)(seed >> 32), o);
}
// the word batch row b draws its ring row from, whatever the sampler: the first of its block under the sample tag
__device__ __forceinline__ uint32_t replay_draw_word(int b, uint64_t gs, uint64_t seed) {
  uint32_t o[4];
  replay_philox(b, gs, kSacTagSample, seed, o);
  return o[0];
}
// the uniform index: floor(u * size), u that word, size = the rows filled (ctr[1]) held to [1, capacity]
__device__ __forceinline__ uint32_t replay_draw_uniform(int b, uint64_t gs, int64_t size, int64_t capacity, uint64_t seed) {
  size = size < 1 ? 1 : (size > capacity ? capacity : size);
  return __umulhi(replay_draw_word(b, gs, seed), (uint32_t)size);
}
// The walk from row idx along its env's later steps, one lane per step.  Lane j < limit looks at row_j = (idx + j N) mod cap (row_out;
// idx in the other lanes) and has to stop if it is the last one allowed, if its ends byte is set, or if it lies in the newest vec-step
// (the row behind it would be the oldest data, or unfilled).  `also(row_j)` is the caller's own load from row_j: all of these loads are
// independent, so the walk costs one memory round trip whatever the limit is.  Returns the first lane that stops, k - 1 (a ballot; the
// caller adds the 1, so that the compiler folds its (k - 1) as it did): lane limit - 1 always stops, 1 <= k <= limit.
template <typename Also>
__device__ __forceinline__ int replay_walk(uint32_t idx, int lane, int limit, const uint8_t* __restrict__ ends, int N, uint32_t cap,
                                           uint32_t newest, uint32_t& row_out, Also&& also) {
  row_out = idx;
  bool stop = false;
  if (lane < limit) {
    row_out = (uint32_t)(((uint64_t)idx + (uint64_t)lane * (uint32_t)N) % cap);
    also(row_out);
    stop = lane + 1 == limit || ends[row_out] != 0 || row_out - row_out % (uint32_t)N == newest;
  }
  return __builtin_ctzll(__builtin_amdgcn_ballot_w64(stop));
}
// one wave copies row `from` of src[.][R] to row `to` of dst[.][R]
__device__ __forceinline__ void replay_copy_row(float* __restrict__ dst, int to, const float* __restrict__ src, uint32_t from, int R, int lane) {
  for (int c = lane; c < R; c += 64) dst[(size_t)to * R + c] = src[(size_t)from * R + c];
}

struct SacStoreArgs {
  float* ring; int64_t capacity; int64_t* ctr;
  const float *obs_stage, *act; const void *reward, *next_obs, *terminal_obs; const uint8_t *terminated, *truncated;
  int32_t N, d, A;
};
template <typename T>
__global__ __launch_bounds__(256) void fw_replay_store_kernel(SacStoreArgs s) {
  const int R = 2 * s.d + s.A + 2;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)s.N * R) return;
  const int i = (int)(e / R), c = (int)(e % R), d = s.d, A = s.A;
  const int64_t cursor = replay_cursor(s.ctr, s.capacity, s.N);
  const bool ended = (s.terminated[i] | s.truncated[i]) != 0;
  float v;
  if (c < d) v = s.obs_stage[(size_t)i * d + c];
  else if (c < d + A) v = s.act[(size_t)i * A + (c - d)];
  else if (c == d + A) v = (float)((const T*)s.reward)[i];
  else if (c < 2 * d + A + 1) v = (float)((const T*)(ended ? s.terminal_obs : s.next_obs))[(size_t)i * d + (c - d - A - 1)];
  else v = s.terminated[i] ? 1.0f : 0.0f;          // a pure time-limit end bootstraps
  s.ring[(size_t)(cursor + i) * R + c] = v;
}
__global__ __launch_bounds__(64) void fw_replay_advance_kernel(int64_t* ctr, int64_t capacity, int32_t N) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t next = replay_cursor(ctr, capacity, N) + N;          // behind the rows just stored
  int64_t size = ctr[1];
  ctr[0] = next + N > capacity ? 0 : next;
  size += N;
  ctr[1] = size > capacity ? capacity : size;
  ctr[2] = ctr[2] + 1;
}
// the uniform sample: one wave per batch row
__global__ __launch_bounds__(256) void fw_replay_sample_kernel(const float* __restrict__ ring, int64_t capacity, const int64_t* __restrict__ ctr,
                                                               uint64_t seed, int R, int B, float* __restrict__ batch, int32_t* __restrict__ idx_out) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  const uint32_t idx = replay_draw_uniform(b, (uint64_t)ctr[3], ctr[1], capacity, seed);
  replay_copy_row(batch, b, ring, idx, R, lane);
  if (lane == 0 && idx_out) idx_out[b] = (int32_t)idx;
}

// ---- n-step returns from the ring ----
// Env e's consecutive steps sit exactly N rows apart, so the k-step transition that starts at row i is rows i, i + N, ... (mod capacity).
// A side ring `ends` (uint8[capacity]: bit 0 terminated, bit 1 truncated) says where an episode stopped -- the row's own done column is
// `terminated` alone, so a time-limit end is in no other place.  fw_replay_mark_ends writes the N bytes of the rows the NEXT fw_replay_store
// will write (same cursor, reads the counter, writes none).
__global__ __launch_bounds__(256) void fw_replay_mark_ends_kernel(uint8_t* __restrict__ ends, int64_t capacity, const int64_t* __restrict__ ctr,
                                                                  const uint8_t* __restrict__ terminated, const uint8_t* __restrict__ truncated, int32_t N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int64_t cursor = replay_cursor(ctr, capacity, N);
  ends[cursor + i] = (uint8_t)((terminated[i] ? 1 : 0) | (truncated[i] ? 2 : 0));
}
constexpr int kSacMaxNStep = 16;
// One wave per batch row, the uniform sampler's start index, replay_walk with n_steps as the limit; lane j also loads row_j's reward.
// Every lane then adds the k discounted rewards in ascending j with one fma each (not a tree: two runs give the same bits), and the
// row copy takes obs | action from row_0 and next_obs | done from row_(k-1).  The last column leaves as 1 - (1 - done) g_(k-1), g_j =
// gamma^j by repeated fp32 products: the consumer's (1 - last) gamma is then (1 - done) gamma^k, and for k = 1 it is `done` itself.
__global__ __launch_bounds__(256) void fw_replay_sample_nstep_kernel(const float* __restrict__ ring, int64_t capacity, const int64_t* __restrict__ ctr,
                                                                     uint64_t seed, int R, int B, float* __restrict__ batch, int32_t* __restrict__ idx_out,
                                                                     const uint8_t* __restrict__ ends, int d, int N, int n_steps, float gamma,
                                                                     int32_t* __restrict__ k_out) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  const uint32_t idx = replay_draw_uniform(b, (uint64_t)ctr[3], ctr[1], capacity, seed);
  const uint32_t newest = replay_newest(replay_cursor(ctr, capacity, N), capacity, N);
  const int rcol = R - d - 2;                      // the reward column (d + A)
  uint32_t row; float r = 0.f;
  const int k = replay_walk(idx, lane, n_steps, ends, N, (uint32_t)capacity, newest, row, [&](uint32_t at) { r = ring[(size_t)at * R + rcol]; }) + 1;
  const uint32_t last = (uint32_t)__builtin_amdgcn_ds_bpermute((k - 1) << 2, (int)row);
  float ret = __int_as_float(__builtin_amdgcn_ds_bpermute(0, __float_as_int(r))), g = 1.0f;
  for (int j = 1; j < k; ++j) {
    g *= gamma;
    ret = __builtin_fmaf(g, __int_as_float(__builtin_amdgcn_ds_bpermute(j << 2, __float_as_int(r))), ret);
  }
  for (int c = lane; c < R; c += 64) {
    float v;
    if (c < rcol) v = ring[(size_t)idx * R + c];
    else if (c == rcol) v = ret;
    else {
      v = ring[(size_t)last * R + c];
      if (c == R - 1) v = 1.0f - (1.0f - v) * g;
    }
    batch[(size_t)b * R + c] = v;
  }
  if (lane == 0) {
    if (idx_out) idx_out[b] = (int32_t)idx;
    if (k_out) k_out[b] = k;
  }
}

// ---- hindsight goal relabelling from the ring ----
// The low-level task is goal-conditioned: the episode's target (psi_ref, h_ref, V_ref) is obs[18:21], and the reward is a closed function
// of the post-step observation and that target.  SB3's HerReplayBuffer ("future" strategy) gives some sampled transitions a goal the
// same episode achieved at or after them and recomputes the reward.  The rows of an episode are N apart and `ends` marks where it stopped:
// replay_walk with the horizon as its limit, and one more row read.
constexpr int kSacMaxHerHorizon = 64, kHerObsDim = 21, kHerRowFloats = 50;
constexpr uint32_t kSacTagHer = 0x5AC0E000u;
struct HerTask { int32_t variant; float dome, min_speed; };          // mirrors fw_her_task (include/fwsim.h)
// the goal a post-step observation achieved: (psi, z, |v|), the norm in double from the fp32 components, rounded to fp32
__device__ __forceinline__ float her_speed(const float* no) {
  const double vx = no[6], vy = no[7], vz = no[8];
  return (float)::sqrt(vx * vx + vy * vy + vz * vz);
}
// The task's reward (fwsim_lowlevel.hpp, the block behind "observation, reward, termination" of fw_step_kernel_ll) restated on a stored
// row: `no` is next_obs[0:18], g the goal, done the row's `terminated`.  In double, rounded once.  The airspeed it reads is the achieved
// goal's, her_speed(): a goal the transition itself achieved then has tracking errors of exactly 0.
__device__ __forceinline__ float her_reward(const HerTask& t, const float* no, const float g[3], bool done) {
  const double roll = no[3], pitch = no[4], psi = no[5], z = no[11], speed = (double)her_speed(no);
  const double psi_err = ::fabs(ll_wrap_pi<double>((double)g[0] - psi)), h_err = ::fabs((double)g[1] - z), v_err = ::fabs((double)g[2] - speed);
  double rew;
  if (t.variant == FW_LL_VARIANT_SAC_DEMO) {
    const double x = no[9], y = no[10], rho = ::sqrt(x * x + y * y);
    double aa = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) aa += (double)no[12 + k] * (double)no[12 + k];
    rew = -(1.5 * psi_err + 1.2 * h_err + 0.8 * v_err);
    rew -= 0.3 * ::fmax(::fabs(roll) - 35.0 * kPi / 180.0, 0.0);
    rew -= 0.3 * ::fmax(::fabs(pitch) - 20.0 * kPi / 180.0, 0.0);
    rew -= 0.05 * ::sqrt(aa);
    rew -= ::fmax(rho - (double)t.dome, 0.0);
    if (speed < (double)t.min_speed) rew -= 2.0;
  } else {
    rew = -(psi_err + h_err + 0.5 * v_err);
    rew += 0.1;
    if (done) rew -= 100.0;
  }
  return (float)rew;
}
// fw_her_reward: her_reward() on caller-given goals, one thread per row (the tests hold the restatement to the env with it)
__global__ __launch_bounds__(256) void fw_her_reward_kernel(const float* __restrict__ rows, int R, int B, int d, const float* __restrict__ goals,
                                                            HerTask task, float* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float* row = rows + (size_t)b * R;
  const float g[3] = { goals[(size_t)b * 3], goals[(size_t)b * 3 + 1], goals[(size_t)b * 3 + 2] };
  out[b] = her_reward(task, row + (R - d - 1), g, row[R - 1] != 0.0f);
}
// One wave per batch row, the uniform sampler's start index; a second Philox block under kSacTagHer decides whether the row is
// relabelled (o[0] against `thresh` = relabel_prob 2^32, formed on the host) and which of the k candidate rows gives the goal
// (__umulhi(o[1], k)).  A row that is not relabelled is the 1-step gather.  Otherwise replay_walk gives k; the goal row's index follows
// from j* by arithmetic, so no lane read is needed.  Every lane forms the goal and the reward (uniform addresses), and the copy replaces
// seven columns of row_0 (two goals and the reward).  d = 21 and R = 50 (the entry point insists): one column per lane.
__global__ __launch_bounds__(256) void fw_replay_sample_her_kernel(const float* __restrict__ ring, int64_t capacity, const int64_t* __restrict__ ctr,
                                                                   uint64_t seed, int B, float* __restrict__ batch, int32_t* __restrict__ idx_out,
                                                                   const uint8_t* __restrict__ ends, int N, int horizon, uint64_t thresh,
                                                                   HerTask task, int32_t* __restrict__ j_out) {
  constexpr int R = kHerRowFloats, d = kHerObsDim, rcol = R - d - 2, nobs = rcol + 1;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  const uint64_t gs = (uint64_t)ctr[3];
  const uint32_t idx = replay_draw_uniform(b, gs, ctr[1], capacity, seed);
  uint32_t h[4];
  replay_philox(b, gs, kSacTagHer, seed, h);
  const float* row0 = ring + (size_t)idx * R;
  float v = lane < R ? row0[lane] : 0.0f;
  int jstar = -1;
  if ((uint64_t)h[0] < thresh) {                    // (the same in every lane of the wave)
    const uint32_t cap = (uint32_t)capacity, newest = replay_newest(replay_cursor(ctr, capacity, N), capacity, N);
    uint32_t row;
    const int k = replay_walk(idx, lane, horizon, ends, N, cap, newest, row, [](uint32_t) {}) + 1;
    jstar = (int)__umulhi(h[1], (uint32_t)k);                                      // in [0, k - 1]
    const uint32_t fut = (uint32_t)(((uint64_t)idx + (uint64_t)jstar * (uint32_t)N) % cap);
    const float* fno = ring + (size_t)fut * R + nobs;
    const float g[3] = { fno[5], fno[11], her_speed(fno) };
    const float rew = her_reward(task, row0 + nobs, g, row0[R - 1] != 0.0f);
    if (lane == rcol) v = rew;
#pragma unroll
    for (int c = 0; c < 3; ++c)                     // obs[18:21] and next_obs[18:21]
      if (lane == d - 3 + c || lane == nobs + d - 3 + c) v = g[c];
  }
  if (lane < R) batch[(size_t)b * R + lane] = v;
  if (lane == 0) {
    if (idx_out) idx_out[b] = (int32_t)idx;
    if (j_out) j_out[b] = jstar;
  }
}

// ---- fw_replay_normalize: VecNormalize's statistics applied to a gathered batch, in place (SB3's ReplayBuffer._normalize_obs /
// _normalize_reward: the ring keeps raw rows, a batch is normalised with the statistics of the moment it is sampled) ----
// One launch behind whichever sampler gathered the batch.  A workgroup takes 64 rows, a wave 16 of them, a lane the columns lane,
// lane + 64, ... of the 2 d (+ 1) columns that change: both observation blocks by fw_obs_normalize_kernel's arithmetic (double, one
// division per element; the d means and standard deviations are formed once per workgroup) and the reward column as
// clip((float)((double)r / sqrt(ret_var + eps)), +-clip).  The action and done columns are never written, every element is written by
// the one lane that read it, and nothing waits on another workgroup.
struct SacBatchNormArgs {
  float* batch; int32_t B, d, A;
  const double *mean, *var, *ret_var;              // mean / var NULL: the observations stay; ret_var NULL: the reward stays
  float clip_obs, eps_obs, clip_rew, eps_rew;
};
constexpr int kSacNormRows = 64;
__global__ __launch_bounds__(256) void fw_replay_normalize_kernel(SacBatchNormArgs n) {
  __shared__ double cmean[kSacMaxD], cstd[kSacMaxD], rstd;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, d = n.d, A = n.A;
  if (n.mean && t < d) { cmean[t] = n.mean[t]; cstd[t] = sqrt(n.var[t] + (double)n.eps_obs); }
  if (n.ret_var && t == 64) rstd = sqrt(n.ret_var[0] + (double)n.eps_rew);
  __syncthreads();
  const int R = 2 * d + A + 2, nobs = n.mean ? 2 * d : 0, W = nobs + (n.ret_var ? 1 : 0);
  const long long first = (long long)blockIdx.x * kSacNormRows + w * (kSacNormRows / 4);
  for (int i = 0; i < kSacNormRows / 4; ++i) {
    const long long b = first + i;
    if (b >= n.B) break;
    float* row = n.batch + (size_t)b * R;
    for (int j = lane; j < W; j += 64) {
      if (j < nobs) {
        const int k = j < d ? j : j - d, c = j < d ? j : j + A + 1;          // obs column k, or next_obs column k behind action and reward
        row[c] = fminf(fmaxf((float)(((double)row[c] - cmean[k]) / cstd[k]), -n.clip_obs), n.clip_obs);
      } else {
        row[d + A] = fminf(fmaxf((float)((double)row[d + A] / rstd), -n.clip_rew), n.clip_rew);
      }
    }
  }
}

}  // namespace fwsim
