// Soft actor-critic for the low-level task (SB3 `SAC("MlpPolicy")`, one gradient step of `SAC.train()`): the act side of a vec-step,
// the step's noise and the gradient step as a fixed sequence of launches.  (The device-resident replay ring: csrc/fwsim_replay.hpp.)
//   reference: examples/lowlevel.py (net_arch [256, 256], buffer 200 000, batch 256, gamma 0.99, tau 0.02, update-to-data 1).
//
// Networks are ReLU MLPs in -> H -> H -> out in fp32: the actor d -> H -> H -> 2A (mean | log_std), two critics and their two targets
// (d + A) -> H -> H -> 1 on cat(obs, action).  Flat parameter image (floats; sac.py packs it), W[in][out] = torch Linear.weight^T:
//   actor | q1 | q2 | log_ent_coef | q1 target | q2 target | exp_avg[T] | exp_avg_sq[T] | tail[4]
//   one network: W1[in][H] b1[H] W2[H][H] b2[H] W3[H][out] b3[out];  T = actor + 2 critics + 1 (the trained part is the front of the image,
//   so a parameter and its moments sit at the same offset of their blocks);  tail[0] = Adam step count (int32 bits).
//
// The gradient step (fw_sac_update) is 24 launches on the caller's stream.  Kernel boundaries are the only synchronisation between
// workgroups: no in-grid wait, no cooperative launch, no atomics.  Every product -- forward X W, back-propagation G W^T, weight gradient
// X^T G -- is ONE tiled kernel (fw_sac_gemm_kernel: 64 x 64 output tile per workgroup, operands staged through LDS from strided sources,
// v_mfma_f32_16x16x4_f32) that takes up to six independent products per launch (blockIdx.z), so the four critic passes, the two actor
// passes and the six / three weight gradients of a network family share a grid.  A weight element's gradient is the K loop of one
// workgroup over the batch in a fixed order, and Adam is applied to it in the epilogue: the launches that read a network's weights
// (forward, G W^T) all precede the one that updates them, so every gradient comes from the pre-step weights (the actor loss reads the
// critics AFTER their step, as SB3 does).
//
// Batches of 16 to 512 rows (multiples of 16) take that sequence.  Larger ones, up to 8192 rows in multiples of 64, take the WIDE form
// of the same stages, 29 launches: the three stages that sum over the batch run one workgroup per 256 rows, each storing its sum to a
// workspace slot that a one-lane fold launch adds in ascending order; a weight gradient is cut into chunks of 512 batch rows, one
// workgroup per (tile, chunk) storing raw partial sums, and a second launch adds the chunks of each element in ascending order and
// applies Adam.  The number of chunks depends on B alone, so two runs still give the same bits.
//
// Device counters (int64[4], caller-owned, shared with the replay ring): [0] ring cursor (rows), [1] rows filled, [2] vec-steps stored,
// [3] gradient steps.  The kernels that read a counter never write it in the same launch: fw_replay_store and fw_sac_update advance
// them from one lane of a closing launch, with plain vector stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fwsim_device.hpp"
#include "fwsim_ppo.hpp"

namespace fwsim {

constexpr int kSacMaxD = 64, kSacMaxA = 8, kSacMaxB = 512;
// the wide form of the gradient step (B > kSacMaxB): element-wise stages of kSacStageRows rows per workgroup, weight gradients split
// over the batch in chunks of kSacSplitRows rows
constexpr int kSacMaxBWide = 8192, kSacWideMultiple = 64, kSacStageRows = 256, kSacSplitRows = 512;
constexpr int kSacWideSlots = 2 * kSacMaxBWide / kSacStageRows;          // partial sums of one stage (the head stage has 2B rows)
constexpr uint32_t kSacTagAct = 0x5AC0A000u, kSacTagWarm = 0x5AC0B000u, kSacTagSample = 0x5AC0C000u, kSacTagNoise = 0x5AC0D000u;
constexpr float kSacLogStdMin = -20.0f, kSacLogStdMax = 2.0f, kSacHalfLog2Pi = 0.9189385332046727f, kSacTanhEps = 1e-6f;

struct SacHyper {          // mirrors fw_sac_hyper (include/fwsim.h)
  float lr, gamma, tau, beta1, beta2, eps, target_entropy, ent_coef;
  int32_t auto_ent, target_update_interval;
  uint64_t seed;
};

struct SacNet { int W1, b1, W2, b2, W3, b3, n; };
__host__ __device__ constexpr SacNet sac_net(int in, int H, int out) {
  SacNet s{};
  s.W1 = 0; s.b1 = in * H; s.W2 = s.b1 + H; s.b2 = s.W2 + H * H; s.W3 = s.b2 + H; s.b3 = s.W3 + H * out; s.n = s.b3 + out;
  return s;
}
struct SacLayout { int actor, q1, q2, lec, t1, t2, P, T, m, v, tail, total; };
__host__ __device__ constexpr SacLayout sac_layout(int d, int A, int H) {
  const int na = sac_net(d, H, 2 * A).n, nc = sac_net(d + A, H, 1).n;
  SacLayout L{};
  L.actor = 0; L.q1 = na; L.q2 = na + nc; L.lec = na + 2 * nc; L.t1 = L.lec + 1; L.t2 = L.t1 + nc; L.P = L.t2 + nc;
  L.T = L.lec + 1; L.m = L.P; L.v = L.P + L.T; L.tail = L.P + 2 * L.T; L.total = L.tail + 4;
  return L;
}
inline bool sac_shape_ok(int d, int A, int H) { return d >= 1 && d <= kSacMaxD && A >= 1 && A <= kSacMaxA && (H == 64 || H == 256); }
inline bool sac_batch_wide(int B) { return B > kSacMaxB && B <= kSacMaxBWide && B % kSacWideMultiple == 0; }
inline bool sac_batch_ok(int B) { return (B >= 16 && B <= kSacMaxB && B % 16 == 0) || sac_batch_wide(B); }
__host__ __device__ constexpr int sac_splits(int B) { return (B + kSacSplitRows - 1) / kSacSplitRows; }

// workspace of fw_sac_update (floats)
struct SacWs { int noise, h1a, h2a, outa, logp, xpi, xnext, ch1, ch2, q, g3, G2, G1, dx, gout, scal, total; };
__host__ __device__ constexpr SacWs sac_ws(int d, int A, int H, int B) {
  SacWs w{}; int o = 0;
  auto take = [&](int n) { const int at = o; o += (n + 3) & ~3; return at; };
  w.noise = take(2 * B * A); w.h1a = take(2 * B * H); w.h2a = take(2 * B * H); w.outa = take(2 * B * 2 * A); w.logp = take(2 * B);
  w.xpi = take(B * (d + A)); w.xnext = take(B * (d + A)); w.ch1 = take(4 * B * H); w.ch2 = take(4 * B * H); w.q = take(4 * B);
  w.g3 = take(2 * B); w.G2 = take(2 * B * H); w.G1 = take(2 * B * H); w.dx = take(2 * B * (d + A)); w.gout = take(B * 2 * A);
  w.scal = take(16); w.total = o;
  return w;
}
// what the wide form (B > kSacMaxB) adds behind it: the stages' partial sums (slots: head | target | actor-q, kSacWideSlots each) and
// the weight gradients' partial sums (part[split][T], indexed like the trained part of the image); up to kSacMaxB nothing is added
struct SacWsWide { int slots, part, total; };
__host__ __device__ constexpr SacWsWide sac_ws_wide(int d, int A, int H, int B) {
  SacWsWide w{};
  w.slots = w.part = w.total = sac_ws(d, A, H, B).total;
  if (B > kSacMaxB) {
    w.part = w.slots + 3 * kSacWideSlots;
    w.total = w.part + ((sac_splits(B) * sac_layout(d, A, H).T + 3) & ~3);
  }
  return w;
}
// The kernels index the workspace with int.  The layout grows with every argument, so the largest shape decides; constant evaluation
// rejects a signed overflow, so this line compiles only while every offset of that shape fits.
static_assert(sac_ws_wide(kSacMaxD, kSacMaxA, 256, kSacMaxBWide).total > 0, "fw_sac_update's workspace offsets must stay inside int");
// scal: the step's scalars, written by the head / target / actor kernels and read by later launches
enum { SAC_S_ALPHA = 0, SAC_S_STEP_SIZE = 1, SAC_S_INV_BC2 = 2, SAC_S_POLYAK = 3, SAC_S_MEAN_LOGP = 4, SAC_S_ENT_LOSS = 5,
       SAC_S_CRITIC_LOSS = 6, SAC_S_ACTOR_LOSS = 7 };

// ---- noise: Philox4x32-10 + Box-Muller (float32), four normals per block; counter (c0, c1, ctr) under a per-use tag ----
__device__ __forceinline__ void sac_normal4(uint64_t seed, uint32_t c0, uint32_t c1, uint64_t ctr, uint32_t tag, float z[4]) {
  uint32_t o[4];
  philox4x32_10(c0, c1, (uint32_t)ctr, (uint32_t)(ctr >> 32) ^ tag, (uint32_t)seed, (uint32_t)(seed >> 32), o);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = ((float)(o[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);          // (0, 1)
    const float u2 = ((float)(o[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * h] = rad * cs; z[2 * h + 1] = rad * sn;
  }
}
// eps[which][b][0..A) of gradient step gs: what fw_sac_noise writes and fw_sac_update draws inside
__device__ __forceinline__ void sac_update_noise4(uint64_t seed, uint64_t gs, int which, int b, int j, float z[4]) {
  sac_normal4(seed, (uint32_t)b, (uint32_t)(which * 2 + j), gs, kSacTagNoise, z);
}
__global__ __launch_bounds__(256) void fw_sac_noise_kernel(uint64_t seed, const int64_t* __restrict__ ctr, int B, int A, float* __restrict__ out) {
  const int nb = (A + 3) >> 2, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * B * nb) return;
  const int j = e % nb, b = (e / nb) % B, which = e / (nb * B);
  float z[4];
  sac_update_noise4(seed, (uint64_t)ctr[3], which, b, j, z);
  for (int c = 0; c < 4 && 4 * j + c < A; ++c) out[((size_t)which * B + b) * A + 4 * j + c] = z[c];
}

// one squashed-Gaussian row: (mean, raw log_std, eps) -> action and log-probability
__device__ __forceinline__ float sac_squash(const float* mu, const float* ls_raw, const float* eps, int A, bool deterministic, float* act) {
  float logp = 0.f;
  for (int j = 0; j < A; ++j) {
    const float ls = fminf(fmaxf(ls_raw[j], kSacLogStdMin), kSacLogStdMax);
    const float e = deterministic ? 0.f : eps[j];
    const float a = ppo_tanh(mu[j] + expf(ls) * e);
    act[j] = a;
    logp += -0.5f * e * e - ls - kSacHalfLog2Pi - logf(1.0f - a * a + kSacTanhEps);
  }
  return logp;
}

// ---- fw_sac_act: 16 envs per workgroup, activations in LDS, weights read from the image (L2) as the B operand ----
// out[16][ldo] = act(A[16][K4] W[Kreal][Nout] + bias); wave w takes the column tiles w, w + 4, ...
__device__ __forceinline__ void sac_layer16(const float* Als, int lda, int K4, int Kreal, const float* __restrict__ W, int ldw,
                                            const float* __restrict__ bias, int Nout, float* out, int ldo, bool relu) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  for (int nt = w; nt * 16 < Nout; nt += 4) {
    const int n = nt * 16 + i;
    const bool nok = n < Nout;
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K4; k0 += 4) {
      const int k = k0 + g;
      const float a = Als[i * lda + k];
      const float b = (nok && k < Kreal) ? W[(size_t)k * ldw + n] : 0.f;
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    if (nok) {
      const float bn = bias[n];
#pragma unroll
      for (int v = 0; v < 4; ++v) { const float y = c[v] + bn; out[(4 * g + v) * ldo + n] = relu ? fmaxf(y, 0.f) : y; }
    }
  }
}
struct SacActArgs {
  const float* image; const void* obs; int32_t N, d, A, mode;     // mode 0 stochastic, 1 deterministic, 2 warm-up (uniform, no forward)
  uint64_t seed; int64_t env_offset; const int64_t* ctr;
  float* act_f32; void* act_env; float* obs_stage; float* logp; float* eps;
};
// fw_sac_act_norm's argument block: fw_sac_act's and VecNormalize's statistics.  The observation enters the forward pass as
//   clip((float)(((double)x - mean[k]) / sqrt(var[k] + (double)eps)), +-clip)   -- fw_obs_normalize_kernel's arithmetic, bit for bit --
// while obs_stage keeps the raw fp32 value, because the ring stores raw rows
struct SacActNormArgs : SacActArgs { const double *obs_mean, *obs_var; float clip_obs, eps_obs; };
// NORM = false is fw_sac_act, NORM = true fw_sac_act_norm: every addition sits under `if constexpr (NORM)`, so the first instantiation's
// statements and argument block are the ones the kernel had before it gained the parameter.
template <typename T, int H, bool NORM = false>
__global__ __launch_bounds__(256) void fw_sac_act_kernel(std::conditional_t<NORM, SacActNormArgs, SacActArgs> a) {
  constexpr int LDX = 65, LDH = H + 1, LDO = 17;
  __shared__ float X[16 * LDX], H1[16 * LDH], H2[16 * LDH], O[16 * LDO];
  const int t = threadIdx.x, r0 = blockIdx.x * 16, d = a.d, A = a.A;
  const T* obs = (const T*)a.obs;
  if constexpr (NORM) {
    // the d <= 64 means and standard deviations once per workgroup: no square root per element (the division stays per element)
    __shared__ double cmean[kSacMaxD], cstd[kSacMaxD];
    const bool fwd = a.mode != 2;                  // warm-up runs no forward pass: X is not read and no statistics are needed
    if (fwd) {
      if (t < d) { cmean[t] = a.obs_mean[t]; cstd[t] = sqrt(a.obs_var[t] + (double)a.eps_obs); }
      __syncthreads();
    }
    for (int idx = t; idx < 16 * 64; idx += 256) {
      const int row = idx >> 6, k = idx & 63;
      float x = 0.f;
      if (r0 + row < a.N && k < d) {
        const T raw = obs[(size_t)(r0 + row) * d + k];
        a.obs_stage[(size_t)(r0 + row) * d + k] = (float)raw;
        if (fwd) x = fminf(fmaxf((float)(((double)raw - cmean[k]) / cstd[k]), -a.clip_obs), a.clip_obs);
      }
      X[row * LDX + k] = x;
    }
  } else {
    for (int idx = t; idx < 16 * 64; idx += 256) {
      const int row = idx >> 6, k = idx & 63;
      float x = 0.f;
      if (r0 + row < a.N && k < d) {
        x = (float)obs[(size_t)(r0 + row) * d + k];
        a.obs_stage[(size_t)(r0 + row) * d + k] = x;
      }
      X[row * LDX + k] = x;
    }
  }
  if (a.mode != 2) {
    const SacNet n = sac_net(d, H, 2 * A);
    const float* P = a.image;
    __syncthreads();
    sac_layer16(X, LDX, (d + 3) & ~3, d, P + n.W1, H, P + n.b1, H, H1, LDH, true);
    __syncthreads();
    sac_layer16(H1, LDH, H, H, P + n.W2, H, P + n.b2, H, H2, LDH, true);
    __syncthreads();
    sac_layer16(H2, LDH, H, H, P + n.W3, 2 * A, P + n.b3, 2 * A, O, LDO, false);
    __syncthreads();
  }
  if (t < 16 && r0 + t < a.N) {
    const int row = r0 + t;
    const uint64_t genv = (uint64_t)(a.env_offset + row), step = (uint64_t)a.ctr[2];
    float e[kSacMaxA], act[kSacMaxA], logp = 0.f;
    if (a.mode == 2) {
      for (int j = 0; j < 2; ++j) {
        uint32_t o[4];
        philox4x32_10((uint32_t)genv, (uint32_t)j, (uint32_t)step, (uint32_t)(step >> 32) ^ kSacTagWarm, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), o);
        for (int c = 0; c < 4; ++c) { act[4 * j + c] = (float)(o[c] >> 8) * (2.0f / 16777216.0f) - 1.0f; e[4 * j + c] = 0.f; }     // [-1, 1)
      }
      logp = -0.6931471805599453f * (float)A;
    } else {
      sac_normal4(a.seed, (uint32_t)genv, 0u, step, kSacTagAct, e);
      sac_normal4(a.seed, (uint32_t)genv, 1u, step, kSacTagAct, e + 4);
      logp = sac_squash(O + t * LDO, O + t * LDO + A, e, A, a.mode == 1, act);
    }
    for (int j = 0; j < A; ++j) {
      a.act_f32[(size_t)row * A + j] = act[j];
      ((T*)a.act_env)[(size_t)row * A + j] = (T)act[j];
      if (a.eps) a.eps[(size_t)row * A + j] = e[j];
    }
    if (a.logp) a.logp[row] = logp;
  }
}
// the launch of fw_sac_act (NORM = false) and fw_sac_act_norm (NORM = true) for envs of dtype T: the hidden width chooses the instantiation
template <typename T, bool NORM>
inline void sac_act_launch(hipStream_t st, const std::conditional_t<NORM, SacActNormArgs, SacActArgs>& a, int H) {
  const dim3 grid((unsigned)((a.N + 15) / 16)), block(256);
  if (H == 64) hipLaunchKernelGGL((fw_sac_act_kernel<T, 64, NORM>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((fw_sac_act_kernel<T, 256, NORM>), grid, block, 0, st, a);
}

// ---- the product kernel ----
enum { SAC_EPI_LINEAR = 0, SAC_EPI_RELU = 1, SAC_EPI_MASK = 2, SAC_EPI_ADAM = 3 };
struct SacGemmJob {
  const float* A; int sam, sak;      // A(m, k) = A[m sam + k sak]
  const float* B; int sbk, sbn;      // B(k, n) = B[k sbk + n sbn]
  float* C; int ldc;                 // C(m, n) = C[m ldc + n]
  int M, N, K;
  const float* bias;                 // LINEAR / RELU: + bias[n] (null: none)
  const float* mask; int ldm;        // MASK: C = acc where mask(m, n) > 0, else 0
  float *m1, *m2;                    // ADAM: C is the weight, these its moments (same indexing)
  float *pb, *mb1, *mb2;             // ADAM: bias[n] and its moments; its gradient is the column sum of B
};
constexpr int kSacMaxJobs = 6;
struct SacGemmArgs { SacGemmJob job[kSacMaxJobs]; int epi; const float* scal; float beta1, beta2, eps; };

__device__ __forceinline__ void sac_adam(float* p, float* m1, float* m2, float g, float step_size, float inv_bc2, float b1, float b2, float eps) {
  const float m = *m1 + (g - *m1) * (1.0f - b1);
  const float v = b2 * *m2 + (1.0f - b2) * g * g;
  *m1 = m; *m2 = v;
  *p = *p - step_size * (m / (sqrtf(v) * inv_bc2 + eps));
}

constexpr int kSgKc = 32, kSgLda = kSgKc + 1, kSgLdb = 64 + 1;
// (fw_sac_wgrad_split_kernel below carries a copy of this kernel's staging and MFMA loop with other K bounds: a change to one belongs in
// the other.  A shared inlined loop was tried; it changes this kernel's register allocation, so the existing path would have moved.)
__global__ __launch_bounds__(256) void fw_sac_gemm_kernel(SacGemmArgs G) {
  __shared__ float As[64 * kSgLda], Bs[kSgKc * kSgLdb];
  const SacGemmJob& J = G.job[blockIdx.z];
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  if (m0 >= J.M || n0 >= J.N) return;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, g = lane >> 4;
  const int left = (J.N - n0 + 15) >> 4, ntile = left < 4 ? left : 4;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_col = G.epi == SAC_EPI_ADAM && J.pb != nullptr && m0 == 0 && t < 64;
  float colsum = 0.f;
  for (int k0 = 0; k0 < J.K; k0 += kSgKc) {
    for (int idx = t; idx < 64 * kSgKc; idx += 256) {
      int m, k;
      if (J.sak == 1) { k = idx % kSgKc; m = idx / kSgKc; } else { m = idx & 63; k = idx >> 6; }
      const int gm = m0 + m, gk = k0 + k;
      As[m * kSgLda + k] = (gm < J.M && gk < J.K) ? J.A[(size_t)gm * J.sam + (size_t)gk * J.sak] : 0.f;
    }
    for (int idx = t; idx < 64 * kSgKc; idx += 256) {
      int k, n;
      if (J.sbn == 1) { n = idx & 63; k = idx >> 6; } else { k = idx % kSgKc; n = idx / kSgKc; }
      const int gk = k0 + k, gn = n0 + n;
      Bs[k * kSgLdb + n] = (gk < J.K && gn < J.N) ? J.B[(size_t)gk * J.sbk + (size_t)gn * J.sbn] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kSgKc / 4; ++s) {
      const int k = 4 * s + g;
      const float a = As[(16 * w + i) * kSgLda + k];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < ntile) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[k * kSgLdb + 16 * j + i], acc[j], 0, 0, 0);
    }
    if (do_col)
      for (int k = 0; k < kSgKc; ++k) colsum += Bs[k * kSgLdb + t];
    __syncthreads();
  }
  const float ss = G.epi == SAC_EPI_ADAM ? G.scal[SAC_S_STEP_SIZE] : 0.f, ib = G.epi == SAC_EPI_ADAM ? G.scal[SAC_S_INV_BC2] : 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j >= ntile) continue;
    const int n = n0 + 16 * j + i;
    if (n >= J.N) continue;
    const float bn = (G.epi <= SAC_EPI_RELU && J.bias) ? J.bias[n] : 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int m = m0 + 16 * w + 4 * g + v;
      if (m >= J.M) continue;
      const size_t off = (size_t)m * J.ldc + n;
      const float y = acc[j][v];
      if (G.epi == SAC_EPI_LINEAR) J.C[off] = y + bn;
      else if (G.epi == SAC_EPI_RELU) J.C[off] = fmaxf(y + bn, 0.f);
      else if (G.epi == SAC_EPI_MASK) J.C[off] = J.mask[(size_t)m * J.ldm + n] > 0.f ? y : 0.f;
      else sac_adam(J.C + off, J.m1 + off, J.m2 + off, y, ss, ib, G.beta1, G.beta2, G.eps);
    }
  }
  if (do_col && n0 + t < J.N) sac_adam(J.pb + n0 + t, J.mb1 + n0 + t, J.mb2 + n0 + t, colsum, ss, ib, G.beta1, G.beta2, G.eps);
}

// ---- the wide form's weight gradients: X^T G split over the batch, then one fold with Adam ----
// One workgroup per (64 x 64 weight tile, chunk of kSacSplitRows batch rows): fw_sac_gemm_kernel's staging and MFMA loop over the rows
// of its chunk alone, the raw accumulators (and the bias column sums of the chunk) stored to part[split][element], element = the
// offset of the weight in the image.  Every element of a family's range is written by exactly one workgroup per split.
// The loop is fw_sac_gemm_kernel's, line for line, with [kb, ke) for [0, K): keep the two in step.
struct SacSplitArgs { SacGemmJob job[kSacMaxJobs]; const float* image; float* part; int T, nsplit; };
__global__ __launch_bounds__(256) void fw_sac_wgrad_split_kernel(SacSplitArgs G) {
  __shared__ float As[64 * kSgLda], Bs[kSgKc * kSgLdb];
  const int split = blockIdx.z % G.nsplit;
  const SacGemmJob& J = G.job[blockIdx.z / G.nsplit];
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  if (m0 >= J.M || n0 >= J.N) return;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, g = lane >> 4;
  const int left = (J.N - n0 + 15) >> 4, ntile = left < 4 ? left : 4;
  const int kb = split * kSacSplitRows, ke = kb + kSacSplitRows < J.K ? kb + kSacSplitRows : J.K;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_col = J.pb != nullptr && m0 == 0 && t < 64;
  float colsum = 0.f;
  for (int k0 = kb; k0 < ke; k0 += kSgKc) {
    for (int idx = t; idx < 64 * kSgKc; idx += 256) {
      int m, k;
      if (J.sak == 1) { k = idx % kSgKc; m = idx / kSgKc; } else { m = idx & 63; k = idx >> 6; }
      const int gm = m0 + m, gk = k0 + k;
      As[m * kSgLda + k] = (gm < J.M && gk < ke) ? J.A[(size_t)gm * J.sam + (size_t)gk * J.sak] : 0.f;
    }
    for (int idx = t; idx < 64 * kSgKc; idx += 256) {
      int k, n;
      if (J.sbn == 1) { n = idx & 63; k = idx >> 6; } else { k = idx % kSgKc; n = idx / kSgKc; }
      const int gk = k0 + k, gn = n0 + n;
      Bs[k * kSgLdb + n] = (gk < ke && gn < J.N) ? J.B[(size_t)gk * J.sbk + (size_t)gn * J.sbn] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kSgKc / 4; ++s) {
      const int k = 4 * s + g;
      const float a = As[(16 * w + i) * kSgLda + k];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < ntile) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[k * kSgLdb + 16 * j + i], acc[j], 0, 0, 0);
    }
    if (do_col)
      for (int k = 0; k < kSgKc; ++k) colsum += Bs[k * kSgLdb + t];
    __syncthreads();
  }
  float* out = G.part + (size_t)split * G.T;
  const size_t woff = (size_t)(J.C - G.image);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j >= ntile) continue;
    const int n = n0 + 16 * j + i;
    if (n >= J.N) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int m = m0 + 16 * w + 4 * g + v;
      if (m < J.M) out[woff + (size_t)m * J.ldc + n] = acc[j][v];
    }
  }
  if (do_col && n0 + t < J.N) out[(size_t)(J.pb - G.image) + n0 + t] = colsum;
}
// image[e0, e1): the gradient is the sum of the splits in ascending order; Adam as in fw_sac_gemm_kernel's epilogue (a parameter and
// its moments sit at the same offset of their blocks)
struct SacAdamFoldArgs { float* image; const float* part; const float* scal; int e0, e1, T, nsplit, m, v; float beta1, beta2, eps; };
__global__ __launch_bounds__(256) void fw_sac_adam_fold_kernel(SacAdamFoldArgs F) {
  const int e = F.e0 + blockIdx.x * 256 + threadIdx.x;
  if (e >= F.e1) return;
  float g = F.part[e];
  for (int s = 1; s < F.nsplit; ++s) g += F.part[(size_t)s * F.T + e];
  sac_adam(F.image + e, F.image + F.m + e, F.image + F.v + e, g, F.scal[SAC_S_STEP_SIZE], F.scal[SAC_S_INV_BC2], F.beta1, F.beta2, F.eps);
}

// ---- the element-wise stages: one workgroup each, sums over the batch in a fixed order ----
struct SacStepArgs {
  float* image; const float* batch; float* ws; int64_t* ctr; float* out;
  int32_t d, A, H, B;
  SacHyper hp;
};
// every thread's partial -> the sum, in thread order, in thread 0 (others get garbage)
__device__ __forceinline__ float sac_block_sum(float x, float* red) {
  __syncthreads();
  red[threadIdx.x] = x;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0)
    for (int k = 0; k < 256; ++k) s += red[k];
  return s;
}
// actor head of [s; s'] -> a_pi, a', logp, logp'; cat(s, a_pi), cat(s', a'); alpha, the ent-coef step and the step's Adam scalars
__global__ __launch_bounds__(256) void fw_sac_head_kernel(SacStepArgs S) {
  __shared__ float red[256];
  const int d = S.d, A = S.A, B = S.B, Kc = d + A, R = 2 * d + A + 2, t = threadIdx.x;
  const SacWs W = sac_ws(d, A, S.H, B);
  const SacLayout L = sac_layout(d, A, S.H);
  float part = 0.f;
  for (int r = t; r < 2 * B; r += 256) {
    const int which = r >= B, b = which ? r - B : r;
    const float* o = S.ws + W.outa + (size_t)r * 2 * A;
    float* x = S.ws + (which ? W.xnext : W.xpi) + (size_t)b * Kc;
    const float* src = S.batch + (size_t)b * R + (which ? Kc + 1 : 0);
    for (int k = 0; k < d; ++k) x[k] = src[k];
    const float lp = sac_squash(o, o + A, S.ws + W.noise + ((size_t)which * B + b) * A, A, false, x + d);
    S.ws[W.logp + r] = lp;
    if (!which) part += lp;
  }
  const float sum = sac_block_sum(part, red);
  if (t == 0) {
    float* sc = S.ws + W.scal;
    const float mean_logp = sum / (float)B;
    const int step = ((const int32_t*)(S.image + L.tail))[0] + 1;
    const double bc1 = 1.0 - pow((double)S.hp.beta1, (double)step), bc2 = 1.0 - pow((double)S.hp.beta2, (double)step);
    const float step_size = (float)((double)S.hp.lr / bc1), inv_bc2 = (float)(1.0 / sqrt(bc2));
    sc[SAC_S_STEP_SIZE] = step_size; sc[SAC_S_INV_BC2] = inv_bc2;
    const int tui = S.hp.target_update_interval < 1 ? 1 : S.hp.target_update_interval;
    sc[SAC_S_POLYAK] = (step % tui) == 0 ? 1.f : 0.f;
    sc[SAC_S_MEAN_LOGP] = mean_logp;
    if (S.hp.auto_ent) {
      float* lec = S.image + L.lec;
      sc[SAC_S_ALPHA] = expf(*lec);
      sc[SAC_S_ENT_LOSS] = -(*lec * (mean_logp + S.hp.target_entropy));
      sac_adam(lec, S.image + L.m + L.lec, S.image + L.v + L.lec, -(mean_logp + S.hp.target_entropy), step_size, inv_bc2,
               S.hp.beta1, S.hp.beta2, S.hp.eps);
    } else {
      sc[SAC_S_ALPHA] = S.hp.ent_coef; sc[SAC_S_ENT_LOSS] = 0.f;
    }
  }
}
// y = r + (1 - done) gamma (min(Q1t, Q2t)(s', a') - alpha logp'); dL/dQ_i = (Q_i - y) / B; the critic loss
__global__ __launch_bounds__(256) void fw_sac_target_kernel(SacStepArgs S) {
  __shared__ float red[256];
  const int d = S.d, A = S.A, B = S.B, R = 2 * d + A + 2, t = threadIdx.x;
  const SacWs W = sac_ws(d, A, S.H, B);
  const float alpha = S.ws[W.scal + SAC_S_ALPHA], invB = 1.0f / (float)B;
  const float* q = S.ws + W.q;
  float part = 0.f;
  for (int b = t; b < B; b += 256) {
    const float* row = S.batch + (size_t)b * R;
    const float y = row[d + A] + (1.0f - row[R - 1]) * S.hp.gamma * (fminf(q[2 * B + b], q[3 * B + b]) - alpha * S.ws[W.logp + B + b]);
    const float e1 = q[b] - y, e2 = q[B + b] - y;
    S.ws[W.g3 + b] = e1 * invB; S.ws[W.g3 + B + b] = e2 * invB;
    part += e1 * e1 + e2 * e2;
  }
  const float sum = sac_block_sum(part, red);
  if (t == 0) S.ws[W.scal + SAC_S_CRITIC_LOSS] = 0.5f * sum * invB;
}
// actor loss mean(alpha logp - min(Q1, Q2)(s, a_pi)); dL/dQ_i = -1 / B on the smaller one
__global__ __launch_bounds__(256) void fw_sac_actor_q_kernel(SacStepArgs S) {
  __shared__ float red[256];
  const int B = S.B, t = threadIdx.x;
  const SacWs W = sac_ws(S.d, S.A, S.H, B);
  const float alpha = S.ws[W.scal + SAC_S_ALPHA], invB = 1.0f / (float)B;
  const float* q = S.ws + W.q;
  float part = 0.f;
  for (int b = t; b < B; b += 256) {
    const bool first = q[b] <= q[B + b];
    S.ws[W.g3 + b] = first ? -invB : 0.f; S.ws[W.g3 + B + b] = first ? 0.f : -invB;
    part += alpha * S.ws[W.logp + b] - (first ? q[b] : q[B + b]);
  }
  const float sum = sac_block_sum(part, red);
  if (t == 0) S.ws[W.scal + SAC_S_ACTOR_LOSS] = sum * invB;
}
// The wide form of the three (B > kSacMaxB; the kernels above stay as they are, so their device code does not move): workgroup k
// takes rows [k kSacStageRows, (k + 1) kSacStageRows), one per thread, with the arithmetic of the loops above, and stores its sum
// (thread order) to slot k of its stage; the fold launch behind it adds the slots in ascending order on one lane and does what thread
// 0 does above.
enum { SAC_STAGE_HEAD = 0, SAC_STAGE_TARGET = 1, SAC_STAGE_ACTOR_Q = 2 };
template <int STAGE>
__global__ __launch_bounds__(256) void fw_sac_stage_wide_kernel(SacStepArgs S) {
  static_assert(kSacStageRows == 256, "one row per thread");
  __shared__ float red[256];
  const int d = S.d, A = S.A, B = S.B, Kc = d + A, R = 2 * d + A + 2, r = blockIdx.x * kSacStageRows + threadIdx.x;
  const SacWs W = sac_ws(d, A, S.H, B);
  const float alpha = STAGE == SAC_STAGE_HEAD ? 0.f : S.ws[W.scal + SAC_S_ALPHA], invB = 1.0f / (float)B;
  const float* q = S.ws + W.q;
  float part = 0.f;
  if (STAGE == SAC_STAGE_HEAD && r < 2 * B) {
    const int which = r >= B, b = which ? r - B : r;
    const float* o = S.ws + W.outa + (size_t)r * 2 * A;
    float* x = S.ws + (which ? W.xnext : W.xpi) + (size_t)b * Kc;
    const float* src = S.batch + (size_t)b * R + (which ? Kc + 1 : 0);
    for (int k = 0; k < d; ++k) x[k] = src[k];
    const float lp = sac_squash(o, o + A, S.ws + W.noise + ((size_t)which * B + b) * A, A, false, x + d);
    S.ws[W.logp + r] = lp;
    if (!which) part = lp;
  }
  if (STAGE == SAC_STAGE_TARGET && r < B) {
    const float* row = S.batch + (size_t)r * R;
    const float y = row[d + A] + (1.0f - row[R - 1]) * S.hp.gamma * (fminf(q[2 * B + r], q[3 * B + r]) - alpha * S.ws[W.logp + B + r]);
    const float e1 = q[r] - y, e2 = q[B + r] - y;
    S.ws[W.g3 + r] = e1 * invB; S.ws[W.g3 + B + r] = e2 * invB;
    part = e1 * e1 + e2 * e2;
  }
  if (STAGE == SAC_STAGE_ACTOR_Q && r < B) {
    const bool first = q[r] <= q[B + r];
    S.ws[W.g3 + r] = first ? -invB : 0.f; S.ws[W.g3 + B + r] = first ? 0.f : -invB;
    part = alpha * S.ws[W.logp + r] - (first ? q[r] : q[B + r]);
  }
  const float sum = sac_block_sum(part, red);
  if (threadIdx.x == 0) S.ws[sac_ws_wide(d, A, S.H, B).slots + STAGE * kSacWideSlots + blockIdx.x] = sum;
}
__global__ __launch_bounds__(64) void fw_sac_stage_fold_kernel(SacStepArgs S, int stage, int nslots) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const SacWs W = sac_ws(S.d, S.A, S.H, S.B);
  const SacLayout L = sac_layout(S.d, S.A, S.H);
  const float* slot = S.ws + sac_ws_wide(S.d, S.A, S.H, S.B).slots + stage * kSacWideSlots;
  float* sc = S.ws + W.scal;
  const float invB = 1.0f / (float)S.B;
  float sum = 0.f;
  for (int k = 0; k < nslots; ++k) sum += slot[k];
  if (stage == SAC_STAGE_TARGET) { sc[SAC_S_CRITIC_LOSS] = 0.5f * sum * invB; return; }
  if (stage == SAC_STAGE_ACTOR_Q) { sc[SAC_S_ACTOR_LOSS] = sum * invB; return; }
  const float mean_logp = sum / (float)S.B;
  const int step = ((const int32_t*)(S.image + L.tail))[0] + 1;
  const double bc1 = 1.0 - pow((double)S.hp.beta1, (double)step), bc2 = 1.0 - pow((double)S.hp.beta2, (double)step);
  const float step_size = (float)((double)S.hp.lr / bc1), inv_bc2 = (float)(1.0 / sqrt(bc2));
  sc[SAC_S_STEP_SIZE] = step_size; sc[SAC_S_INV_BC2] = inv_bc2;
  const int tui = S.hp.target_update_interval < 1 ? 1 : S.hp.target_update_interval;
  sc[SAC_S_POLYAK] = (step % tui) == 0 ? 1.f : 0.f;
  sc[SAC_S_MEAN_LOGP] = mean_logp;
  if (S.hp.auto_ent) {
    float* lec = S.image + L.lec;
    sc[SAC_S_ALPHA] = expf(*lec);
    sc[SAC_S_ENT_LOSS] = -(*lec * (mean_logp + S.hp.target_entropy));
    sac_adam(lec, S.image + L.m + L.lec, S.image + L.v + L.lec, -(mean_logp + S.hp.target_entropy), step_size, inv_bc2,
             S.hp.beta1, S.hp.beta2, S.hp.eps);
  } else {
    sc[SAC_S_ALPHA] = S.hp.ent_coef; sc[SAC_S_ENT_LOSS] = 0.f;
  }
}
// dL/d(mean, raw log_std) of the actor loss from dL/da (the critics' input gradient) and the log-probability
__global__ __launch_bounds__(256) void fw_sac_actor_grad_kernel(SacStepArgs S) {
  const int d = S.d, A = S.A, B = S.B, Kc = d + A, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * A) return;
  const int b = e / A, j = e % A;
  const SacWs W = sac_ws(d, A, S.H, B);
  const float alpha = S.ws[W.scal + SAC_S_ALPHA], invB = 1.0f / (float)B;
  const float a = S.ws[W.xpi + (size_t)b * Kc + d + j], ls_raw = S.ws[W.outa + (size_t)b * 2 * A + A + j];
  const float ls = fminf(fmaxf(ls_raw, kSacLogStdMin), kSacLogStdMax), eps = S.ws[W.noise + (size_t)b * A + j];
  const float dq = S.ws[W.dx + (size_t)b * Kc + d + j] + S.ws[W.dx + (size_t)(B + b) * Kc + d + j];
  const float om = 1.0f - a * a;
  const float du = alpha * invB * (2.0f * a * om / (om + kSacTanhEps)) + dq * om;
  const bool pass = ls_raw >= kSacLogStdMin && ls_raw <= kSacLogStdMax;
  S.ws[W.gout + (size_t)b * 2 * A + j] = du;
  S.ws[W.gout + (size_t)b * 2 * A + A + j] = pass ? du * expf(ls) * eps - alpha * invB : 0.f;
}
// targets <- (1 - tau) targets + tau critics where the step asks for it; the outputs; the counters (one lane, nobody reads them here)
__global__ __launch_bounds__(256) void fw_sac_finish_kernel(SacStepArgs S) {
  const SacLayout L = sac_layout(S.d, S.A, S.H);
  const SacWs W = sac_ws(S.d, S.A, S.H, S.B);
  const float* sc = S.ws + W.scal;
  const int n = L.lec - L.q1, e = blockIdx.x * 256 + threadIdx.x;
  if (e < n && sc[SAC_S_POLYAK] != 0.f) {
    float* tp = S.image + L.t1 + e;
    *tp = *tp * (1.0f - S.hp.tau) + S.hp.tau * S.image[L.q1 + e];
  }
  if (e == 0) {
    if (S.out) {
      S.out[0] = sc[SAC_S_CRITIC_LOSS]; S.out[1] = sc[SAC_S_ACTOR_LOSS]; S.out[2] = sc[SAC_S_ENT_LOSS];
      S.out[3] = sc[SAC_S_ALPHA]; S.out[4] = sc[SAC_S_MEAN_LOGP];
    }
    int32_t* tail = (int32_t*)(S.image + L.tail);
    tail[0] = tail[0] + 1;
    S.ctr[3] = S.ctr[3] + 1;
  }
}

// ---- the launch sequence of one gradient step ----
inline void sac_launch_gemm(hipStream_t st, const SacStepArgs& S, int epi, const SacGemmJob* jobs, int n) {
  SacGemmArgs G;
  int maxM = 0, maxN = 0;
  for (int k = 0; k < kSacMaxJobs; ++k) {
    G.job[k] = jobs[k < n ? k : 0];
    if (k < n) { maxM = jobs[k].M > maxM ? jobs[k].M : maxM; maxN = jobs[k].N > maxN ? jobs[k].N : maxN; }
  }
  G.epi = epi; G.scal = S.ws + sac_ws(S.d, S.A, S.H, S.B).scal;
  G.beta1 = S.hp.beta1; G.beta2 = S.hp.beta2; G.eps = S.hp.eps;
  hipLaunchKernelGGL(fw_sac_gemm_kernel, dim3((maxN + 63) / 64, (maxM + 63) / 64, n), dim3(256), 0, st, G);
}
inline SacGemmJob sac_job(const float* A, int sam, int sak, const float* Bm, int sbk, int sbn, float* C, int ldc, int M, int N, int K) {
  SacGemmJob j{};
  j.A = A; j.sam = sam; j.sak = sak; j.B = Bm; j.sbk = sbk; j.sbn = sbn; j.C = C; j.ldc = ldc; j.M = M; j.N = N; j.K = K;
  return j;
}
// the wide form's weight gradients of the image range [e0, e1): the split grid, then the fold with Adam
inline void sac_launch_wgrad_wide(hipStream_t st, const SacStepArgs& S, const SacGemmJob* jobs, int n, int e0, int e1) {
  const SacLayout L = sac_layout(S.d, S.A, S.H);
  const SacWs W = sac_ws(S.d, S.A, S.H, S.B);
  const SacWsWide V = sac_ws_wide(S.d, S.A, S.H, S.B);
  SacSplitArgs G;
  int maxM = 0, maxN = 0;
  for (int k = 0; k < kSacMaxJobs; ++k) {
    G.job[k] = jobs[k < n ? k : 0];
    if (k < n) { maxM = jobs[k].M > maxM ? jobs[k].M : maxM; maxN = jobs[k].N > maxN ? jobs[k].N : maxN; }
  }
  G.image = S.image; G.part = S.ws + V.part; G.T = L.T; G.nsplit = sac_splits(S.B);
  hipLaunchKernelGGL(fw_sac_wgrad_split_kernel, dim3((maxN + 63) / 64, (maxM + 63) / 64, n * G.nsplit), dim3(256), 0, st, G);
  const SacAdamFoldArgs F{S.image, S.ws + V.part, S.ws + W.scal, e0, e1, L.T, G.nsplit, L.m, L.v, S.hp.beta1, S.hp.beta2, S.hp.eps};
  hipLaunchKernelGGL(fw_sac_adam_fold_kernel, dim3((e1 - e0 + 255) / 256), dim3(256), 0, st, F);
}
// One gradient step.  Up to kSacMaxB rows: 24 launches.  The wide form: 29 -- each of the three batch-sum stages is a grid and a fold
// (+3), each of the two weight-gradient launches a split grid and a fold with Adam (+2); everything else is the same launch on a
// grid that grows with B.  `after_target(st)` runs behind the target stage, in front of the critics' backward pass: fw_sac_update passes
// nothing, fw_sac_update_weighted (csrc/fwsim_per.hpp) its one launch on g3.
template <typename AfterTarget>
inline void sac_update_launch(hipStream_t st, const SacStepArgs& S, AfterTarget&& after_target) {
  const int d = S.d, A = S.A, H = S.H, B = S.B, Kc = d + A, O = 2 * A, R = 2 * d + A + 2;
  const bool wide = B > kSacMaxB;
  const SacLayout L = sac_layout(d, A, H);
  const SacWs W = sac_ws(d, A, H, B);
  const SacNet na = sac_net(d, H, O), nc = sac_net(Kc, H, 1);
  float* P = S.image; float* ws = S.ws;
  const float* bt = S.batch;
  const int crit[4] = {L.q1, L.q2, L.t1, L.t2};
  SacGemmJob jb[kSacMaxJobs];
  auto fwd = [&](int net, const SacNet& n, int layer, const float* X, int ldx, int K, float* Y, int M) {        // Y = X W_layer (+ bias)
    const int w = layer == 1 ? n.W1 : layer == 2 ? n.W2 : n.W3, b = layer == 1 ? n.b1 : layer == 2 ? n.b2 : n.b3;
    const int N = layer == 3 ? (n.n - n.b3) : H;
    SacGemmJob j = sac_job(X, ldx, 1, P + net + w, N, 1, Y, N, M, N, K);
    j.bias = P + net + b;
    return j;
  };
  auto back = [&](const float* Gm, int K, const float* Wm, int ldw, int N, const float* mask, float* C, int M) {   // C = (G W^T) masked
    SacGemmJob j = sac_job(Gm, K, 1, Wm, 1, ldw, C, N, M, N, K);
    j.mask = mask; j.ldm = N;
    return j;
  };
  auto grad = [&](int net, int w, int b, const float* X, int ldx, int Kin, const float* Gm, int N, int M) {       // W -= Adam(X^T G), b -= Adam(colsum G)
    SacGemmJob j = sac_job(X, 1, ldx, Gm, N, 1, P + net + w, N, Kin, N, M);
    j.m1 = P + L.m + net + w; j.m2 = P + L.v + net + w;
    j.pb = P + net + b; j.mb1 = P + L.m + net + b; j.mb2 = P + L.v + net + b;
    return j;
  };
  auto stage = [&](void (*one)(SacStepArgs), void (*many)(SacStepArgs), int which, int rows) {      // a batch-sum stage
    if (!wide) { hipLaunchKernelGGL(one, dim3(1), dim3(256), 0, st, S); return; }
    const int n = (rows + kSacStageRows - 1) / kSacStageRows;
    hipLaunchKernelGGL(many, dim3(n), dim3(256), 0, st, S);
    hipLaunchKernelGGL(fw_sac_stage_fold_kernel, dim3(1), dim3(64), 0, st, S, which, n);
  };
  auto step_weights = [&](const SacGemmJob* jobs, int n, int e0, int e1) {      // the weight gradients of image[e0, e1) with Adam
    if (wide) sac_launch_wgrad_wide(st, S, jobs, n, e0, e1);
    else sac_launch_gemm(st, S, SAC_EPI_ADAM, jobs, n);
  };
  // 0: the step's noise
  hipLaunchKernelGGL(fw_sac_noise_kernel, dim3((2 * B * ((A + 3) / 4) + 255) / 256), dim3(256), 0, st, S.hp.seed, (const int64_t*)S.ctr, B, A, ws + W.noise);
  // 1-4: the actor on [s; s']
  jb[0] = fwd(L.actor, na, 1, bt, R, d, ws + W.h1a, B);
  jb[1] = fwd(L.actor, na, 1, bt + Kc + 1, R, d, ws + W.h1a + (size_t)B * H, B);
  sac_launch_gemm(st, S, SAC_EPI_RELU, jb, 2);
  jb[0] = fwd(L.actor, na, 2, ws + W.h1a, H, H, ws + W.h2a, 2 * B);
  sac_launch_gemm(st, S, SAC_EPI_RELU, jb, 1);
  jb[0] = fwd(L.actor, na, 3, ws + W.h2a, H, H, ws + W.outa, 2 * B);
  sac_launch_gemm(st, S, SAC_EPI_LINEAR, jb, 1);
  stage(fw_sac_head_kernel, fw_sac_stage_wide_kernel<SAC_STAGE_HEAD>, SAC_STAGE_HEAD, 2 * B);
  // 5-8: Q1, Q2 on (s, a) and the targets on (s', a') in one grid per layer
  auto critic_forward = [&](int count, const float* x01, int ld01, const float* x23) {
    for (int k = 0; k < count; ++k) jb[k] = fwd(crit[k], nc, 1, k < 2 ? x01 : x23, k < 2 ? ld01 : Kc, Kc, ws + W.ch1 + (size_t)k * B * H, B);
    sac_launch_gemm(st, S, SAC_EPI_RELU, jb, count);
    for (int k = 0; k < count; ++k) jb[k] = fwd(crit[k], nc, 2, ws + W.ch1 + (size_t)k * B * H, H, H, ws + W.ch2 + (size_t)k * B * H, B);
    sac_launch_gemm(st, S, SAC_EPI_RELU, jb, count);
    for (int k = 0; k < count; ++k) jb[k] = fwd(crit[k], nc, 3, ws + W.ch2 + (size_t)k * B * H, H, H, ws + W.q + (size_t)k * B, B);
    sac_launch_gemm(st, S, SAC_EPI_LINEAR, jb, count);
  };
  // dL/dh2 and dL/dh1 of Q1, Q2 from g3 = dL/dQ
  auto critic_backward = [&]() {
    for (int k = 0; k < 2; ++k) jb[k] = back(ws + W.g3 + (size_t)k * B, 1, P + crit[k] + nc.W3, 1, H, ws + W.ch2 + (size_t)k * B * H, ws + W.G2 + (size_t)k * B * H, B);
    sac_launch_gemm(st, S, SAC_EPI_MASK, jb, 2);
    for (int k = 0; k < 2; ++k) jb[k] = back(ws + W.G2 + (size_t)k * B * H, H, P + crit[k] + nc.W2, H, H, ws + W.ch1 + (size_t)k * B * H, ws + W.G1 + (size_t)k * B * H, B);
    sac_launch_gemm(st, S, SAC_EPI_MASK, jb, 2);
  };
  critic_forward(4, bt, R, ws + W.xnext);
  stage(fw_sac_target_kernel, fw_sac_stage_wide_kernel<SAC_STAGE_TARGET>, SAC_STAGE_TARGET, B);
  after_target(st);
  // 9-11: the critics' backward pass, then all six weight gradients with Adam in one grid
  critic_backward();
  for (int k = 0; k < 2; ++k) {
    jb[3 * k + 0] = grad(crit[k], nc.W3, nc.b3, ws + W.ch2 + (size_t)k * B * H, H, H, ws + W.g3 + (size_t)k * B, 1, B);
    jb[3 * k + 1] = grad(crit[k], nc.W2, nc.b2, ws + W.ch1 + (size_t)k * B * H, H, H, ws + W.G2 + (size_t)k * B * H, H, B);
    jb[3 * k + 2] = grad(crit[k], nc.W1, nc.b1, bt, R, Kc, ws + W.G1 + (size_t)k * B * H, H, B);
  }
  step_weights(jb, 6, L.q1, L.lec);
  // 12-19: the stepped critics on (s, a_pi), their gradient with respect to the action
  critic_forward(2, ws + W.xpi, Kc, nullptr);
  stage(fw_sac_actor_q_kernel, fw_sac_stage_wide_kernel<SAC_STAGE_ACTOR_Q>, SAC_STAGE_ACTOR_Q, B);
  critic_backward();
  for (int k = 0; k < 2; ++k) jb[k] = sac_job(ws + W.G1 + (size_t)k * B * H, H, 1, P + crit[k] + nc.W1, 1, H, ws + W.dx + (size_t)k * B * Kc, Kc, B, Kc, H);
  sac_launch_gemm(st, S, SAC_EPI_LINEAR, jb, 2);
  hipLaunchKernelGGL(fw_sac_actor_grad_kernel, dim3((B * A + 255) / 256), dim3(256), 0, st, S);
  // 20-22: the actor's backward pass on the rows of s, its three weight gradients with Adam
  jb[0] = back(ws + W.gout, O, P + L.actor + na.W3, O, H, ws + W.h2a, ws + W.G2, B);
  sac_launch_gemm(st, S, SAC_EPI_MASK, jb, 1);
  jb[0] = back(ws + W.G2, H, P + L.actor + na.W2, H, H, ws + W.h1a, ws + W.G1, B);
  sac_launch_gemm(st, S, SAC_EPI_MASK, jb, 1);
  jb[0] = grad(L.actor, na.W3, na.b3, ws + W.h2a, H, H, ws + W.gout, O, B);
  jb[1] = grad(L.actor, na.W2, na.b2, ws + W.h1a, H, H, ws + W.G2, H, B);
  jb[2] = grad(L.actor, na.W1, na.b1, bt, R, d, ws + W.G1, H, B);
  step_weights(jb, 3, L.actor, L.q1);
  // 23: Polyak, outputs, counters
  hipLaunchKernelGGL(fw_sac_finish_kernel, dim3((2 * nc.n + 255) / 256), dim3(256), 0, st, S);
}
inline void sac_update_launch(hipStream_t st, const SacStepArgs& S) { sac_update_launch(st, S, [](hipStream_t) {}); }

}  // namespace fwsim
