// The act side of a collected vec-step of the high-level command task in ONE launch instead of three
// (fw_collect_act for the commander, fw_command_hl, fw_collect_act_a for the frozen controller): at the reference's 16 envs every
// launch is pure latency.  The frame is fw_policy_act_kernel's: grid (ceil(N / 64), 2), 256 threads, weights and activations in LDS,
// act_forward on fp32 MFMA.
//   block (c, 1): what the value block of fw_collect_act does, on the three-action flat image (hl_value_block: fw_policy_act_kernel's
//                 value half in raw-observation mode, restated here so that kernel stays as it is): V(obs) and the finalisation of
//                 the previous step for rows 64 c ..;
//   block (c, 0): for the same rows -- the env's raw 30-value observation normalised on load (-> obs_copy), the commander
//                 30 -> 64 -> 64 -> 3, three sampled actions (components 0-2 of act_normal4's draw; -> act_raw, logp), the command
//                 (hl_command: fw_command_hl_kernel's arithmetic; -> FW_SL_TARGET tail, cmd_out, low_obs), low_obs normalised with the
//                 controller's frozen statistics, the controller 21 -> 64 -> 64 -> 6 from a second flat image, deterministic, its
//                 output clipped to [-1, 1] -> act_env, the fw_step input.
// Both networks' weights are fetched up front (they fit the LDS side by side: hl_act_lds_bytes), so the controller's arrive while
// the commander's forward runs.  Every output is what the three launches write, bit for bit, given the same act_raw: the
// normalisations, act_forward and the command arithmetic are the same code.  No in-grid wait, no host synchronisation.
//
// Included by fwsim.hip behind fwsim_direct.hpp (hl_command, the state tile accessors).
#pragma once

struct HlActArgs {
  fwsim::ActArgs A;                  // the commander: fw_collect_act's arguments (raw-observation mode; act_raw is [N, 3], act_env the
                                     // CONTROLLER's clipped output [N, 6])
  const float* low_params;           // the controller's flat image (six-action layout, 21 observations)
  const double *low_mean, *low_var;  // its frozen observation statistics [21]
  float low_clip, low_eps;
  void *low_obs, *cmd_out;           // [N, 21], [N, 3] in the env dtype
  int32_t* rejected;                 // rows with a non-finite action (may be null)
  double dome;
};

constexpr int kHlLowD = fwsim_cmd::kLLObs, kHlLowDp = (kHlLowD + 1) & ~1, kHlLowLdx = kHlLowDp + 1, kHlLowA = 6, kHlLowLdo = 8;
constexpr int kHlDoubles = 2 * 64 + 2 * 32 + 3 * fwsim::kPChunk;      // column statistics of both normalisations, the chunk's commands

inline size_t hl_act_lds_bytes(int D) {
  using namespace fwsim;
  const int Dp = (D + 1) & ~1, ldx = Dp + 1;
  const size_t pol = sizeof(double) * kHlDoubles
                   + sizeof(float) * ((size_t)Dp * kPH + kPH + kPH * kPLdh + kPH + kPH * 3 + 3 + 3 + (size_t)kPChunk * ldx + 2 * (size_t)kPChunk * kPLdh + kPChunk * 4
                                      + (size_t)kHlLowDp * kPH + kPH + kPH * kPLdh + kPH + kPH * kHlLowA + kHlLowA + kHlLowA + (size_t)kPChunk * kHlLowLdx + kPChunk * kHlLowLdo);
  const size_t val = sizeof(double) * 128 + sizeof(float) * ((size_t)Dp * kPH + kPH + kPH * kPLdh + kPH + kPH + 2 + (size_t)kPChunk * ldx + 2 * (size_t)kPChunk * kPLdh + kPChunk * 4);
  return std::max(pol, val);
}

// X[64][ldx] = the rows row0 .. row0 + 63 of a raw [N, D] buffer of the env dtype, normalised as fw_normalize_obs does (the division
// per element, sqrt(var + eps) once per column: cstd / cmean in LDS), rows past N and columns past D zero; the normalised rows also
// go to obs_copy when it is given.  The loads of a batch of elements leave together (one memory round trip per batch); the caller
// has issued the first batch already (hl_load_batch(.., threadIdx.x, rawv)) so that its round trip overlaps the weight loads.
constexpr int kHlXB = 8;
template <typename T>
__device__ __forceinline__ void hl_load_batch(const T* __restrict__ src, int N, int D, int ldx, int row0, int e0, double (&rawv)[kHlXB]) {
#pragma unroll
  for (int u = 0; u < kHlXB; ++u) {
    const int e = e0 + u * fwsim::kPThreads;
    const int s_ = e / ldx, d = e - s_ * ldx, row = row0 + s_;
    rawv[u] = 0.0;
    if (e < fwsim::kPChunk * ldx && d < D && row < N) rawv[u] = (double)src[(size_t)row * D + d];
  }
}
template <typename T>
__device__ __forceinline__ void hl_normalise_rows(const T* __restrict__ src, int N, int D, int ldx, int row0, const double* cmean, const double* cstd,
                                                  float clip, float* X, float* obs_copy, double (&rawv)[kHlXB]) {
  const int t = threadIdx.x;
  for (int e0 = t; e0 < fwsim::kPChunk * ldx; e0 += kHlXB * fwsim::kPThreads) {
    if (e0 != t) hl_load_batch<T>(src, N, D, ldx, row0, e0, rawv);
#pragma unroll
    for (int u = 0; u < kHlXB; ++u) {
      const int e = e0 + u * fwsim::kPThreads;
      if (e >= fwsim::kPChunk * ldx) continue;
      const int s_ = e / ldx, d = e - s_ * ldx, row = row0 + s_;
      float x = 0.f;
      if (d < D && row < N) {
        x = fminf(fmaxf((float)((rawv[u] - cmean[d]) / cstd[d]), -clip), clip);
        if (obs_copy) obs_copy[(size_t)row * D + d] = x;
      }
      X[e] = x;
    }
  }
}

// The value block: V(normalised obs) -> value, and the finalisation of the previous vec-step for its 64 rows when prev_reward is given
// (VecNormalize's reward path, the bootstrap through V(normalised terminal observation) where an episode was truncated but not
// terminated -- a second pass through the network, only in blocks that hold such a row -- and the episode starts): the arithmetic of
// fw_policy_act_kernel's value block in raw-observation mode, term for term.
template <typename T>
__device__ __forceinline__ void hl_value_block(const fwsim::ActArgs& A, float* lds) {
  using namespace fwsim;
  constexpr int LDO = 4;
  const int t = threadIdx.x;
  const int D = A.D, Dp = (D + 1) & ~1, ldx = Dp + 1;
  const int row0 = blockIdx.x * kPChunk;
  double* cstd = reinterpret_cast<double*>(lds);
  double* cmean = cstd + 64;
  float* p = reinterpret_cast<float*>(cmean + 64);
  PpoNetLds W;
  W.W1 = p; p += Dp * kPH; W.b1 = p; p += kPH; W.W2 = p; p += kPH * kPLdh; W.b2 = p; p += kPH; W.Wo = p; p += kPH; W.bo = p; p += 2;      // (bo follows Wo; one float of padding)
  float* X = p;  p += kPChunk * ldx;
  float* H1 = p; p += kPChunk * kPLdh;
  float* H2 = p; p += kPChunk * kPLdh;
  float* out = p; p += kPChunk * LDO;

  double c_var = 1.0, c_mean = 0.0;
  if (t < D) { c_var = A.var[t]; c_mean = A.mean[t]; }
  const int frow = row0 + (t & 63);
  const bool fmine = A.prev_reward && t < kPChunk && frow < A.N;
  uint8_t f_term = 0, f_trunc = 0; double f_rew = 0.0, f_var = 1.0;
  if (fmine) {
    f_term = A.prev_term[frow]; f_trunc = A.prev_trunc[frow]; f_var = A.ret_var[0];
    f_rew = (double)reinterpret_cast<const T*>(A.prev_reward)[frow];
  }
  double rawv[kHlXB];
  hl_load_batch<T>(reinterpret_cast<const T*>(A.raw), A.N, D, ldx, row0, t, rawv);
  {
    const float* __restrict__ params = A.params;
    const int oW1 = ppo_net_params(Dp, 3), ob1 = oW1 + Dp * kPH, oW2 = ob1 + kPH, ob2 = oW2 + kPH * kPH, oWo = ob2 + kPH;
    for (int i = t; i < Dp * kPH; i += kPThreads) W.W1[i] = params[oW1 + i];
    for (int i = t; i < kPH; i += kPThreads) { W.b1[i] = params[ob1 + i]; W.b2[i] = params[ob2 + i]; }
    for (int i = t; i < kPH * kPH; i += kPThreads) W.W2[(i >> 6) * kPLdh + (i & 63)] = params[oW2 + i];
    for (int i = t; i < kPH + 1; i += kPThreads) W.Wo[i] = params[oWo + i];
  }
  if (t < D) { cstd[t] = sqrt(c_var + (double)A.eps); cmean[t] = c_mean; }
  __syncthreads();
  hl_normalise_rows<T>(reinterpret_cast<const T*>(A.raw), A.N, D, ldx, row0, cmean, cstd, A.clip, X, nullptr, rawv);
  __syncthreads();
  act_forward(W, X, H1, H2, out, 1, Dp, ldx, LDO);
  if (t < kPChunk && row0 + t < A.N) A.value[row0 + t] = out[t * LDO];
  if (!A.prev_reward) return;
  const bool timeout = fmine && f_trunc && !f_term;
  if (__syncthreads_or(timeout ? 1 : 0)) {                      // block-uniform: some episode of my rows was truncated
    hl_load_batch<T>(reinterpret_cast<const T*>(A.prev_tobs), A.N, D, ldx, row0, t, rawv);
    hl_normalise_rows<T>(reinterpret_cast<const T*>(A.prev_tobs), A.N, D, ldx, row0, cmean, cstd, A.clip, X, nullptr, rawv);
    __syncthreads();
    act_forward(W, X, H1, H2, out, 1, Dp, ldx, LDO);
  }
  if (fmine) {
    double rn = f_rew;
    if (A.norm_reward) {
      rn *= 1.0 / sqrt(f_var + (double)A.rew_eps);
      rn = rn > A.clip_reward ? A.clip_reward : (rn < -A.clip_reward ? -A.clip_reward : rn);
    }
    float o = (float)rn;
    if (timeout) o += A.gamma * out[t * LDO];                    // SB3: bootstrap truncated episodes with V(terminal_observation)
    A.rew_out[frow] = o;
    A.start_out[frow] = (f_term || f_trunc) ? 1.0f : 0.0f;
  }
}

template <typename T, int G>
__global__ __launch_bounds__(fwsim::kPThreads) void fw_collect_act_hl_kernel(DevState<T> Dg, HlActArgs HA) {
  using namespace fwsim;
  extern __shared__ __align__(16) float lds[];
  const ActArgs& A = HA.A;
  if (blockIdx.y == 1) {
    if (A.nets & 2) hl_value_block<T>(A, lds);
    return;
  }
  if (!(A.nets & 1)) return;
  constexpr int EPW = kWave / G;
  constexpr int NA = 3, LDO = 4;
  const int t = threadIdx.x;
  const int D = A.D, Dp = (D + 1) & ~1, ldx = Dp + 1;
  const int row0 = blockIdx.x * kPChunk;
  const T* __restrict__ raw = reinterpret_cast<const T*>(A.raw);

  // ---- LDS carve-up: the doubles first (8-byte aligned), then the commander, the activations both forwards use, the controller ----
  double* cstd = reinterpret_cast<double*>(lds);      // [64] sqrt(var + eps) of the env's observation columns
  double* cmean = cstd + 64;                          // [64]
  double* lstd = cmean + 64;                          // [32] the same of the controller's 21 columns
  double* lmean = lstd + 32;                          // [32]
  double* cmdl = lmean + 32;                          // [64][3] the chunk's commands (the handle's dtype, widened)
  float* p = reinterpret_cast<float*>(cmdl + 3 * kPChunk);
  PpoNetLds W, LW;
  W.W1 = p; p += Dp * kPH; W.b1 = p; p += kPH; W.W2 = p; p += kPH * kPLdh; W.b2 = p; p += kPH; W.Wo = p; p += kPH * NA; W.bo = p; p += NA;
  float* log_std = p; p += NA;
  float* X = p;  p += kPChunk * ldx;
  float* H1 = p; p += kPChunk * kPLdh;
  float* H2 = p; p += kPChunk * kPLdh;
  float* out = p; p += kPChunk * LDO;
  LW.W1 = p; p += kHlLowDp * kPH; LW.b1 = p; p += kPH; LW.W2 = p; p += kPH * kPLdh; LW.b2 = p; p += kPH; LW.Wo = p; p += kPH * kHlLowA; LW.bo = p; p += kHlLowA;
  float* llog_std = p; p += kHlLowA;
  float* LX = p; p += kPChunk * kHlLowLdx;
  float* lout = p; p += kPChunk * kHlLowLdo;

  // small loads first (as fw_policy_act_kernel): the column statistics of both normalisations, the draw's key and counter
  double c_var = 1.0, c_mean = 0.0, l_var = 1.0, l_mean = 0.0;
  if (t < D) { c_var = A.var[t]; c_mean = A.mean[t]; }
  if (t < kHlLowD) { l_var = HA.low_var[t]; l_mean = HA.low_mean[t]; }
  uint64_t rng_key = 0, rng_ctr = 0;
  if (!A.deterministic && t < kPChunk) { rng_key = A.rng[0]; rng_ctr = A.rng[1]; }
  // ... and the first batch of observation elements: their round trip overlaps the weights'
  double rawv[kHlXB];
  hl_load_batch<T>(raw, A.N, D, ldx, row0, t, rawv);
  // both networks' weights: the policy net of each image (the commander's image has the three-action layout, the controller's the six-action one)
  {
    const float* __restrict__ params = A.params;
    const int ob1 = Dp * kPH, oW2 = ob1 + kPH, ob2 = oW2 + kPH * kPH, oWo = ob2 + kPH;
    const int oLs = ppo_net_params(Dp, NA) + ppo_net_params(Dp, 1);
    for (int i = t; i < Dp * kPH; i += kPThreads) W.W1[i] = params[i];
    for (int i = t; i < kPH; i += kPThreads) { W.b1[i] = params[ob1 + i]; W.b2[i] = params[ob2 + i]; }
    for (int i = t; i < kPH * kPH; i += kPThreads) W.W2[(i >> 6) * kPLdh + (i & 63)] = params[oW2 + i];
    for (int i = t; i < kPH * NA + NA; i += kPThreads) W.Wo[i] = params[oWo + i];
    if (t < NA) log_std[t] = params[oLs + t];
  }
  {
    const float* __restrict__ params = HA.low_params;
    constexpr int ob1 = kHlLowDp * kPH, oW2 = ob1 + kPH, ob2 = oW2 + kPH * kPH, oWo = ob2 + kPH;
    const int oLs = ppo_net_params(kHlLowDp, kHlLowA) + ppo_net_params(kHlLowDp, 1);
    for (int i = t; i < kHlLowDp * kPH; i += kPThreads) LW.W1[i] = params[i];
    for (int i = t; i < kPH; i += kPThreads) { LW.b1[i] = params[ob1 + i]; LW.b2[i] = params[ob2 + i]; }
    for (int i = t; i < kPH * kPH; i += kPThreads) LW.W2[(i >> 6) * kPLdh + (i & 63)] = params[oW2 + i];
    for (int i = t; i < kPH * kHlLowA + kHlLowA; i += kPThreads) LW.Wo[i] = params[oWo + i];
    if (t < kHlLowA) llog_std[t] = params[oLs + t];
  }
  if (t < D) { cstd[t] = sqrt(c_var + (double)A.eps); cmean[t] = c_mean; }
  if (t < kHlLowD) { lstd[t] = sqrt(l_var + (double)HA.low_eps); lmean[t] = l_mean; }
  __syncthreads();
  // the normalised observations of the chunk: X, and the rollout buffer on the way
  hl_normalise_rows<T>(raw, A.N, D, ldx, row0, cmean, cstd, A.clip, X, A.obs_copy, rawv);
  __syncthreads();

  act_forward(W, X, H1, H2, out, NA, Dp, ldx, LDO);
  // ---- sample, command: one thread per row ----
  if (t < kPChunk) {
    const int row = row0 + t;
    if (row < A.N) {
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if (!A.deterministic) act_normal4(rng_key, rng_ctr, (uint64_t)(A.env_offset + row), z);      // (the fourth component is not used)
      float lp = 0.f, a[NA];
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const float ls = log_std[k];
        a[k] = out[t * LDO + k] + z[k] * expf(ls);
        lp += -0.5f * z[k] * z[k] - ls - 0.9189385332046727f;
      }
      float* ar = A.act_raw + (size_t)row * NA;
#pragma unroll
      for (int k = 0; k < NA; ++k) ar[k] = a[k];
      A.logp[row] = lp;
      const DevState<T> Dt = tile_view<T, EPW>(Dg, row / EPW);
      T c[3];
      hl_command<T>(Dt, row, (double)a[0], (double)a[1], (double)a[2], HA.dome, HA.rejected, c);
      T* lo = reinterpret_cast<T*>(HA.low_obs) + (size_t)row * kHlLowD;
      T* co = reinterpret_cast<T*>(HA.cmd_out) + (size_t)row * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) { lo[18 + k] = c[k]; co[k] = c[k]; cmdl[t * 3 + k] = (double)c[k]; }
    }
  }
  __syncthreads();
  // ---- the controller's input: low_obs = (obs[:, 0:18], command), normalised with its own statistics ----
  for (int e = t; e < kPChunk * kHlLowLdx; e += kPThreads) {
    const int s_ = e / kHlLowLdx, d = e - s_ * kHlLowLdx, row = row0 + s_;
    float x = 0.f;
    if (d < kHlLowD && row < A.N) {
      double v;
      if (d < 18) {
        const T o = raw[(size_t)row * D + d];
        reinterpret_cast<T*>(HA.low_obs)[(size_t)row * kHlLowD + d] = o;
        v = (double)o;
      } else {
        v = cmdl[s_ * 3 + (d - 18)];
      }
      x = fminf(fmaxf((float)((v - lmean[d]) / lstd[d]), -HA.low_clip), HA.low_clip);
    }
    LX[e] = x;
  }
  __syncthreads();
  act_forward(LW, LX, H1, H2, lout, kHlLowA, kHlLowDp, kHlLowLdx, kHlLowLdo);
  if (t < kPChunk) {
    const int row = row0 + t;
    if (row < A.N) {
      float a[kHlLowA];
#pragma unroll
      for (int k = 0; k < kHlLowA; ++k) {
        a[k] = lout[t * kHlLowLdo + k] + 0.f * expf(llog_std[k]);      // (fw_policy_act_kernel's deterministic action, term for term)
        a[k] = fminf(fmaxf(a[k], -1.0f), 1.0f);
      }
      T* o = reinterpret_cast<T*>(A.act_env) + (size_t)row * kHlLowA;
#pragma unroll
      for (int k = 0; k < kHlLowA; ++k) o[k] = (T)a[k];
    }
  }
}
