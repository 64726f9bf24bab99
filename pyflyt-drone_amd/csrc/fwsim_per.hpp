// Prioritized experience replay on the device replay ring (Schaul et al. 2016, the proportional variant): a three-level sum structure
// over one priority leaf per ring row, the proportional draw, the importance weights, the priority write-back and the one launch
// fw_sac_update_weighted inserts into the gradient step.  sac.py restates every contract in numpy (per_sums_reference,
// per_draw_reference, per_update_reference).
//
// Levels.  prio[capacity] are the leaves, (|td| + eps)^alpha, 0 for a row never written.  sum1 / min1 [ceil(capacity / 256)] hold the
// sum and the smallest positive entry of 256 consecutive leaves, sum2 / min2 [ceil(len(sum1) / 256)] the same over sum1 / min1; the
// capacity limit of 2^22 rows keeps level 2 at no more than 64 entries, so the top of the structure is one more group of 256.  A min is
// +inf where nothing below it is positive.  per_state[4]: running max leaf | total | smallest positive leaf | spare.
//
// THE order of a group.  One wave works on one group of 256 entries (missing entries read as 0): lane l owns entries 4l .. 4l + 3,
//   p_0 = x_0, p_j = p_(j-1) + x_j        (its own three adds),
//   E_0 = 0,   E_(l+1) = E_l + p_3 of lane l   (a chain over the 64 lanes, every lane runs it on values read across the wave),
// and the running sum up to and including entry 4l + j is E_l + p_j; the group's sum is E_64.  The running sum in front of entry
// 4l + j is E_l for j = 0 and E_l + p_(j-1) otherwise -- the running sum of the entry before it, so the sequence never decreases.
// The rebuild and the draw share this code: the sums are recomputed from the leaves every time, never adjusted, and two runs give the
// same bits.  No atomics but the integer max of fw_replay_per_update, no in-grid wait.
// (Lane reads and ballots are the compiler builtins: see csrc/fwsim_replay.hpp.)
#pragma once
#include "fwsim_replay.hpp"

namespace fwsim {

constexpr int kPerGroup = 256;
constexpr int64_t kPerMaxCapacity = (int64_t)1 << 22;          // 64 level-2 entries; above it fp32 sums stop resolving one leaf
enum { PER_S_MAX = 0, PER_S_TOTAL = 1, PER_S_MIN = 2 };
inline int per_groups(int64_t n) { return (int)((n + kPerGroup - 1) / kPerGroup); }

__device__ __forceinline__ float per_lane_read(float x, int lane) {          // x of lane `lane` (each lane may name another one)
  return __int_as_float(__builtin_amdgcn_ds_bpermute(lane << 2, __float_as_int(x)));
}
// lane l's four entries of base[0, n), n <= 256; `pad` where there is none
__device__ __forceinline__ void per_load4(const float* __restrict__ base, int n, int lane, float pad, float x[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = 4 * lane + j < n ? base[4 * lane + j] : pad;
}
// the group's running sums in THE order: p (this lane's), E (in front of this lane); returns the group's sum
__device__ __forceinline__ float per_scan(const float x[4], int lane, float p[4], float& E) {
  p[0] = x[0]; p[1] = p[0] + x[1]; p[2] = p[1] + x[2]; p[3] = p[2] + x[3];
  float run = 0.f;
  E = 0.f;
#pragma unroll
  for (int l = 0; l < 64; ++l) {
    if (lane == l) E = run;
    run += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p[3]), l));
  }
  return run;
}
__device__ __forceinline__ float per_wave_min(float m) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) m = fminf(m, per_lane_read(m, (int)(threadIdx.x & 63) ^ s));
  return m;
}
// sum (THE order) and smallest positive entry of one group: sums from `vals`, mins from `mins` (null: the positive entries of vals)
__device__ __forceinline__ void per_group_reduce(const float* __restrict__ vals, const float* __restrict__ mins, int n, int lane, float& sum,
                                                 float& mn) {
  float x[4], p[4], E, m[4];
  per_load4(vals, n, lane, 0.f, x);
  sum = per_scan(x, lane, p, E);
  if (mins) per_load4(mins, n, lane, __builtin_inff(), m);
  float lo = __builtin_inff();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float c = mins ? m[j] : x[j];
    if (c > 0.f) lo = fminf(lo, c);
  }
  mn = per_wave_min(lo);
}

// ---- fw_replay_per_rebuild: level 1 from the leaves (one wave per group), then level 2, the total and the minimum (one workgroup) ----
__global__ __launch_bounds__(256) void fw_replay_per_level1_kernel(const float* __restrict__ prio, int capacity, float* __restrict__ sum1,
                                                                   float* __restrict__ min1) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, n1 = (capacity + kPerGroup - 1) / kPerGroup;
  if (g >= n1) return;
  const int left = capacity - g * kPerGroup;
  float sum, mn;
  per_group_reduce(prio + (size_t)g * kPerGroup, nullptr, left < kPerGroup ? left : kPerGroup, lane, sum, mn);
  if (lane == 0) { sum1[g] = sum; min1[g] = mn; }
}
__global__ __launch_bounds__(256) void fw_replay_per_level2_kernel(const float* __restrict__ sum1, const float* __restrict__ min1, int n1,
                                                                   float* __restrict__ sum2, float* __restrict__ min2, float* __restrict__ per_state) {
  __shared__ float s2[64], m2[64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, n2 = (n1 + kPerGroup - 1) / kPerGroup;          // n2 <= 64 (the entry point insists)
  for (int g = w; g < n2; g += 4) {
    const int left = n1 - g * kPerGroup;
    float sum, mn;
    per_group_reduce(sum1 + (size_t)g * kPerGroup, min1 + (size_t)g * kPerGroup, left < kPerGroup ? left : kPerGroup, lane, sum, mn);
    if (lane == 0) { sum2[g] = sum; min2[g] = mn; s2[g] = sum; m2[g] = mn; }
  }
  __syncthreads();
  if (w != 0) return;
  float total, mn;
  per_group_reduce(s2, m2, n2, lane, total, mn);
  if (lane == 0) { per_state[PER_S_TOTAL] = total; per_state[PER_S_MIN] = mn; }
}

// ---- fw_replay_per_mark_new: the running max into the leaves of the rows the NEXT fw_replay_store writes (fw_replay_mark_ends' cursor) ----
__global__ __launch_bounds__(256) void fw_replay_per_mark_new_kernel(float* __restrict__ prio, int64_t capacity, const int64_t* __restrict__ ctr,
                                                                     const float* __restrict__ per_state, int32_t N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int64_t cursor = replay_cursor(ctr, capacity, N);
  prio[cursor + i] = per_state[PER_S_MAX];
}

// ---- the proportional draw ----
// One level of the descent on base[0, n): the first positive entry whose running sum exceeds t, or -- rounding left none -- the last
// positive entry; t becomes t - (the running sum in front of it).  A group with no positive entry (sums that no rebuild followed)
// gives entry 0 and t = 0, so the index stays inside [0, n).  Everything is the same in every lane of the wave.
__device__ __forceinline__ int per_pick(const float* __restrict__ base, int n, int lane, float& t) {
  float x[4], p[4], E;
  per_load4(base, n, lane, 0.f, x);
  per_scan(x, lane, p, E);
  int hit_j = 4, pos_j = -1;
  float hit_front = 0.f, pos_front = 0.f;
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    const float front = j == 0 ? E : E + p[j - 1];
    if (x[j] > 0.f && E + p[j] > t) { hit_j = j; hit_front = front; }          // descending j: the smallest j stays
    if (x[j] > 0.f && pos_j < 0) { pos_j = j; pos_front = front; }             // descending j: the largest j stays
  }
  unsigned long long m = __builtin_amdgcn_ballot_w64(hit_j < 4);
  int L, sel_j = hit_j;
  float sel_front = hit_front;
  if (m != 0ull) {
    L = __builtin_ctzll(m);
  } else {
    m = __builtin_amdgcn_ballot_w64(pos_j >= 0);
    if (m == 0ull) { t = 0.f; return 0; }
    L = 63 - __builtin_clzll(m);
    sel_j = pos_j; sel_front = pos_front;
  }
  const int j = __builtin_amdgcn_ds_bpermute(L << 2, sel_j);
  t = t - per_lane_read(sel_front, L);
  return 4 * L + j;
}
// One wave per batch row, the word every sampler draws from (replay_draw_word: o0); u = (o0 + 0.5) 2^-32 in double, t = (float)(u total),
// three levels of per_pick, then the uniform sampler's row copy.  w = (p_min / p_row)^beta as exp(beta log x) in fp32.
__global__ __launch_bounds__(256) void fw_replay_sample_per_kernel(const float* __restrict__ ring, int capacity, const int64_t* __restrict__ ctr,
                                                                   uint64_t seed, int R, int B, float* __restrict__ batch, int32_t* __restrict__ idx_out,
                                                                   float* __restrict__ w_out, const float* __restrict__ prio,
                                                                   const float* __restrict__ sum1, const float* __restrict__ sum2,
                                                                   const float* __restrict__ per_state, float beta0, int64_t beta_steps) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  const uint32_t o0 = replay_draw_word(b, (uint64_t)ctr[3], seed);
  const int n1 = (capacity + kPerGroup - 1) / kPerGroup, n2 = (n1 + kPerGroup - 1) / kPerGroup;
  const double u = ((double)o0 + 0.5) * (1.0 / 4294967296.0);
  float t = (float)(u * (double)per_state[PER_S_TOTAL]);
  const int k2 = per_pick(sum2, n2, lane, t);                                   // k2 < n2
  const int left1 = n1 - k2 * kPerGroup;
  const int g = k2 * kPerGroup + per_pick(sum1 + (size_t)k2 * kPerGroup, left1 < kPerGroup ? left1 : kPerGroup, lane, t);          // g < n1
  const int left0 = capacity - g * kPerGroup;
  uint32_t idx = (uint32_t)(g * kPerGroup + per_pick(prio + (size_t)g * kPerGroup, left0 < kPerGroup ? left0 : kPerGroup, lane, t));
  if (idx >= (uint32_t)capacity) idx = 0u;                                       // (cannot happen: every pick stays inside its group)
  replay_copy_row(batch, b, ring, idx, R, lane);
  if (lane == 0) {
    if (idx_out) idx_out[b] = (int32_t)idx;
    if (w_out) {
      float beta = beta0;
      if (beta_steps > 0) beta = fminf(1.0f, beta0 + (1.0f - beta0) * ((float)ctr[3] / (float)beta_steps));
      w_out[b] = expf(beta * logf(per_state[PER_S_MIN] / prio[idx]));
    }
  }
}

// ---- fw_replay_per_update: leaf = (td + eps)^alpha to the sampled rows, the largest one where a row was drawn more than once ----
// Two launches: the first zeroes the touched leaves, the second takes an integer max on the float bits (positive floats order as
// their bits do) with a vector-memory atomic, so the result does not depend on the order the lanes arrive in.  The batch's largest
// leaf goes into per_state[0] the same way, one atomic per wave.  An index outside the ring is skipped; so is a td that is not finite
// (its leaf stays 0: the row is not drawn again).
__global__ __launch_bounds__(256) void fw_replay_per_clear_kernel(float* __restrict__ prio, int capacity, const int32_t* __restrict__ idx, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const uint32_t i = (uint32_t)idx[b];
  if (i < (uint32_t)capacity) prio[i] = 0.f;
}
__global__ __launch_bounds__(256) void fw_replay_per_max_kernel(float* __restrict__ prio, int capacity, const int32_t* __restrict__ idx,
                                                                const float* __restrict__ td, int B, float alpha, float eps,
                                                                float* __restrict__ per_state) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  float leaf = 0.f;
  if (b < B) {
    const uint32_t i = (uint32_t)idx[b];
    const float v = expf(alpha * logf(fabsf(td[b]) + eps));
    if (i < (uint32_t)capacity && v > 0.f && v < __builtin_inff()) {
      leaf = v;
      __hip_atomic_fetch_max((unsigned int*)(prio + i), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) leaf = fmaxf(leaf, per_lane_read(leaf, (int)(threadIdx.x & 63) ^ s));
  if ((threadIdx.x & 63) == 0 && leaf > 0.f)
    __hip_atomic_fetch_max((unsigned int*)(per_state + PER_S_MAX), __float_as_uint(leaf), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- fw_sac_update_weighted: the launch behind the target stage ----
// The target stage left g3 = (Q_i - y) / B for both critics.  td_out[b] = (|e1| + |e2|) / 2 with |e_i| recovered as |g3_i| B, then
// both entries are scaled by the row's weight: the critics' backward pass and weight gradients read g3, nothing else of the step does,
// so only the critic loss is weighted.  A weight of 1.0 leaves the bits of g3 as they are.
__global__ __launch_bounds__(256) void fw_sac_per_weight_kernel(float* __restrict__ g3, int B, const float* __restrict__ weights,
                                                                float* __restrict__ td_out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float g1 = g3[b], g2 = g3[B + b], w = weights[b];
  if (td_out) td_out[b] = 0.5f * (fabsf(g1) + fabsf(g2)) * (float)B;
  g3[b] = g1 * w; g3[B + b] = g2 * w;
}

}  // namespace fwsim
