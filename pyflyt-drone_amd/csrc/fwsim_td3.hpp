// TD3 for the low-level task (SB3 `TD3("MlpPolicy")`, one gradient step of `TD3.train()`): the act side of a vec-step and the gradient
// step as a fixed sequence of launches over the SAC product kernel (csrc/fwsim_sac.hpp), on the same replay ring (csrc/fwsim_replay.hpp).
//
// Networks are ReLU MLPs in -> H -> H -> out in fp32: the actor d -> H -> H -> A (tanh on its output), two critics (d + A) -> H -> H -> 1
// on cat(obs, action), and a target of each of the three.  Flat parameter image (floats; td3.py packs it), W[in][out] = torch
// Linear.weight^T, one network laid out as in the SAC image:
//   actor | q1 | q2 | actor target | q1 target | q2 target | exp_avg[T] | exp_avg_sq[T] | tail[4]
//   T = actor + 2 critics: the trained part is the front of the image, its targets the block of the same shape behind it, so a
//   parameter, its target and its moments sit at the same offset of their blocks;  tail[0] = gradient steps taken, tail[1] = actor
//   steps taken (int32 bits): the critics' Adam bias correction counts the first, the actor's the second.
//
// The gradient step (fw_td3_update) is 13 launches when only the critics train and 28 with the actor part.  Every product is a job of
// fw_sac_gemm_kernel, unchanged; the smoothing noise is the first block of fw_sac_noise_kernel; the kernels here are the element-wise
// stages between products.  Kernel boundaries are the only synchronisation between workgroups: no in-grid wait, no atomics.  The two
// sums over the batch (the critic loss, the actor loss) run in one workgroup in a fixed order (sac_block_sum), a weight gradient is
// the K loop of one workgroup of the product kernel: two runs give the same bits.  B is a multiple of 16 in [16, 512].
//
// Device counters: the ring's int64[4] (csrc/fwsim_sac.hpp); the step reads [3] for its noise and advances it in its closing launch.
#pragma once
#include "fwsim_sac.hpp"

namespace fwsim {

struct Td3Hyper {          // mirrors fw_td3_hyper (include/fwsim.h)
  float lr, gamma, tau, beta1, beta2, eps, policy_noise, noise_clip;
  uint64_t seed;
};

struct Td3Layout { int actor, q1, q2, ta, t1, t2, P, T, m, v, tail, total; };
__host__ __device__ constexpr Td3Layout td3_layout(int d, int A, int H) {
  const int na = sac_net(d, H, A).n, nc = sac_net(d + A, H, 1).n;
  Td3Layout L{};
  L.actor = 0; L.q1 = na; L.q2 = na + nc; L.T = na + 2 * nc;
  L.ta = L.T; L.t1 = L.T + na; L.t2 = L.t1 + nc; L.P = 2 * L.T;
  L.m = L.P; L.v = L.P + L.T; L.tail = L.P + 2 * L.T; L.total = L.tail + 4;
  return L;
}
inline bool td3_batch_ok(int B) { return B >= 16 && B <= kSacMaxB && B % 16 == 0; }

// workspace of fw_td3_update (floats)
struct Td3Ws { int noise, h1t, h2t, outt, xnext, ch1, ch2, q, g3, G2, G1, h1a, h2a, outa, xpi, dx, gout, scal, total; };
__host__ __device__ constexpr Td3Ws td3_ws(int d, int A, int H, int B) {
  Td3Ws w{}; int o = 0;
  auto take = [&](int n) { const int at = o; o += (n + 3) & ~3; return at; };
  w.noise = take(2 * B * A); w.h1t = take(B * H); w.h2t = take(B * H); w.outt = take(B * A); w.xnext = take(B * (d + A));
  w.ch1 = take(4 * B * H); w.ch2 = take(4 * B * H); w.q = take(4 * B); w.g3 = take(2 * B); w.G2 = take(2 * B * H); w.G1 = take(2 * B * H);
  w.h1a = take(B * H); w.h2a = take(B * H); w.outa = take(B * A); w.xpi = take(B * (d + A)); w.dx = take(B * A); w.gout = take(B * A);
  w.scal = take(16); w.total = o;
  return w;
}
static_assert(td3_ws(kSacMaxD, kSacMaxA, 256, kSacMaxB).total > 0 && td3_layout(kSacMaxD, kSacMaxA, 256).total > 0,
              "fw_td3_update's image and workspace offsets must stay inside int");
// scal: two blocks of eight in the product kernel's numbering (SAC_S_STEP_SIZE / SAC_S_INV_BC2 are what its ADAM epilogue reads):
// the critics' Adam scalars and loss at 0, the actor's at kTd3ScalActor
constexpr int kTd3ScalActor = 8;

// ---- fw_td3_act: fw_sac_act's tiling (16 envs per workgroup, activations in LDS, weights from the image) with a deterministic head ----
struct Td3ActArgs {
  const float* image; const void* obs; int32_t N, d, A, mode;     // mode 0 exploring, 1 deterministic, 2 warm-up (uniform, no forward)
  uint64_t seed; int64_t env_offset; const int64_t* ctr;
  float* act_f32; void* act_env; float* obs_stage; float* eps;
  float sigma;
};
template <typename T, int H>
__global__ __launch_bounds__(256) void fw_td3_act_kernel(Td3ActArgs a) {
  constexpr int LDX = 65, LDH = H + 1, LDO = 9;
  __shared__ float X[16 * LDX], H1[16 * LDH], H2[16 * LDH], O[16 * LDO];
  const int t = threadIdx.x, r0 = blockIdx.x * 16, d = a.d, A = a.A;
  const T* obs = (const T*)a.obs;
  for (int idx = t; idx < 16 * 64; idx += 256) {
    const int row = idx >> 6, k = idx & 63;
    float x = 0.f;
    if (r0 + row < a.N && k < d) {
      x = (float)obs[(size_t)(r0 + row) * d + k];
      a.obs_stage[(size_t)(r0 + row) * d + k] = x;
    }
    X[row * LDX + k] = x;
  }
  if (a.mode != 2) {
    const SacNet n = sac_net(d, H, A);
    const float* P = a.image;
    __syncthreads();
    sac_layer16(X, LDX, (d + 3) & ~3, d, P + n.W1, H, P + n.b1, H, H1, LDH, true);
    __syncthreads();
    sac_layer16(H1, LDH, H, H, P + n.W2, H, P + n.b2, H, H2, LDH, true);
    __syncthreads();
    sac_layer16(H2, LDH, H, H, P + n.W3, A, P + n.b3, A, O, LDO, false);
    __syncthreads();
  }
  if (t < 16 && r0 + t < a.N) {
    const int row = r0 + t;
    const uint64_t genv = (uint64_t)(a.env_offset + row), step = (uint64_t)a.ctr[2];
    float e[kSacMaxA], act[kSacMaxA];
    if (a.mode == 2) {
      for (int j = 0; j < 2; ++j) {
        uint32_t o[4];
        philox4x32_10((uint32_t)genv, (uint32_t)j, (uint32_t)step, (uint32_t)(step >> 32) ^ kSacTagWarm, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), o);
        for (int c = 0; c < 4; ++c) { act[4 * j + c] = (float)(o[c] >> 8) * (2.0f / 16777216.0f) - 1.0f; e[4 * j + c] = 0.f; }     // [-1, 1)
      }
    } else {
      sac_normal4(a.seed, (uint32_t)genv, 0u, step, kSacTagAct, e);
      sac_normal4(a.seed, (uint32_t)genv, 1u, step, kSacTagAct, e + 4);
      for (int j = 0; j < A; ++j) {
        const float m = ppo_tanh(O[t * LDO + j]);
        act[j] = a.mode == 1 ? m : fminf(fmaxf(m + a.sigma * e[j], -1.0f), 1.0f);
      }
    }
    for (int j = 0; j < A; ++j) {
      a.act_f32[(size_t)row * A + j] = act[j];
      ((T*)a.act_env)[(size_t)row * A + j] = (T)act[j];
      if (a.eps) a.eps[(size_t)row * A + j] = e[j];
    }
  }
}
template <typename T>
inline void td3_act_launch(hipStream_t st, const Td3ActArgs& a, int H) {
  const dim3 grid((unsigned)((a.N + 15) / 16)), block(256);
  if (H == 64) hipLaunchKernelGGL((fw_td3_act_kernel<T, 64>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((fw_td3_act_kernel<T, 256>), grid, block, 0, st, a);
}

// ---- the element-wise stages ----
struct Td3StepArgs {
  float* image; const float* batch; float* ws; int64_t* ctr; float* out;
  int32_t d, A, H, B, with_actor;
  Td3Hyper hp;
};
__device__ __forceinline__ void td3_adam_scalars(const Td3Hyper& hp, int step, float* sc) {
  const double bc1 = 1.0 - pow((double)hp.beta1, (double)step), bc2 = 1.0 - pow((double)hp.beta2, (double)step);
  sc[SAC_S_STEP_SIZE] = (float)((double)hp.lr / bc1); sc[SAC_S_INV_BC2] = (float)(1.0 / sqrt(bc2));
}
// a' = clamp(tanh(actor_target(s')) + clamp(policy_noise eps, +-noise_clip), +-1); the rows cat(s', a'); the step's Adam scalars
__global__ __launch_bounds__(256) void fw_td3_smooth_kernel(Td3StepArgs S) {
  const int d = S.d, A = S.A, B = S.B, Kc = d + A, R = 2 * d + A + 2, e = blockIdx.x * 256 + threadIdx.x;
  const Td3Ws W = td3_ws(d, A, S.H, B);
  if (e == 0) {
    const int32_t* tail = (const int32_t*)(S.image + td3_layout(d, A, S.H).tail);
    td3_adam_scalars(S.hp, tail[0] + 1, S.ws + W.scal);
    td3_adam_scalars(S.hp, tail[1] + 1, S.ws + W.scal + kTd3ScalActor);
  }
  if (e >= B * Kc) return;
  const int b = e / Kc, k = e % Kc;
  float x;
  if (k < d) {
    x = S.batch[(size_t)b * R + Kc + 1 + k];
  } else {
    const int j = k - d;
    const float noise = fminf(fmaxf(S.hp.policy_noise * S.ws[W.noise + (size_t)b * A + j], -S.hp.noise_clip), S.hp.noise_clip);
    x = fminf(fmaxf(ppo_tanh(S.ws[W.outt + (size_t)b * A + j]) + noise, -1.0f), 1.0f);
  }
  S.ws[W.xnext + (size_t)b * Kc + k] = x;
}
// y = r + (1 - last) gamma min(Q1t, Q2t)(s', a'); dL/dQ_i = 2 (Q_i - y) / B; the critic loss, the SUM of the two mean squared errors
__global__ __launch_bounds__(256) void fw_td3_target_kernel(Td3StepArgs S) {
  __shared__ float red[256];
  const int d = S.d, A = S.A, B = S.B, R = 2 * d + A + 2, t = threadIdx.x;
  const Td3Ws W = td3_ws(d, A, S.H, B);
  const float invB = 1.0f / (float)B;
  const float* q = S.ws + W.q;
  float part = 0.f;
  for (int b = t; b < B; b += 256) {
    const float* row = S.batch + (size_t)b * R;
    const float y = row[d + A] + (1.0f - row[R - 1]) * S.hp.gamma * fminf(q[2 * B + b], q[3 * B + b]);
    const float e1 = q[b] - y, e2 = q[B + b] - y;
    S.ws[W.g3 + b] = 2.0f * e1 * invB; S.ws[W.g3 + B + b] = 2.0f * e2 * invB;
    part += e1 * e1 + e2 * e2;
  }
  const float sum = sac_block_sum(part, red);
  if (t == 0) S.ws[W.scal + SAC_S_CRITIC_LOSS] = sum * invB;
}
// the rows cat(s, tanh(actor(s)))
__global__ __launch_bounds__(256) void fw_td3_actor_rows_kernel(Td3StepArgs S) {
  const int d = S.d, A = S.A, B = S.B, Kc = d + A, R = 2 * d + A + 2, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * Kc) return;
  const Td3Ws W = td3_ws(d, A, S.H, B);
  const int b = e / Kc, k = e % Kc;
  S.ws[W.xpi + (size_t)b * Kc + k] = k < d ? S.batch[(size_t)b * R + k] : ppo_tanh(S.ws[W.outa + (size_t)b * A + (k - d)]);
}
// actor loss -mean Q1(s, pi(s)); dL/dQ1 = -1 / B
__global__ __launch_bounds__(256) void fw_td3_actor_q_kernel(Td3StepArgs S) {
  __shared__ float red[256];
  const int B = S.B, t = threadIdx.x;
  const Td3Ws W = td3_ws(S.d, S.A, S.H, B);
  const float invB = 1.0f / (float)B;
  float part = 0.f;
  for (int b = t; b < B; b += 256) {
    S.ws[W.g3 + b] = -invB;
    part += S.ws[W.q + b];
  }
  const float sum = sac_block_sum(part, red);
  if (t == 0) S.ws[W.scal + kTd3ScalActor + SAC_S_ACTOR_LOSS] = -(sum * invB);
}
// dL/d(actor output) from dL/da (Q1's input gradient) through the tanh
__global__ __launch_bounds__(256) void fw_td3_actor_grad_kernel(Td3StepArgs S) {
  const int d = S.d, A = S.A, B = S.B, Kc = d + A, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * A) return;
  const Td3Ws W = td3_ws(d, A, S.H, B);
  const int b = e / A, j = e % A;
  const float a = S.ws[W.xpi + (size_t)b * Kc + d + j];
  S.ws[W.gout + e] = S.ws[W.dx + e] * (1.0f - a * a);
}
// the closing launch.  With the actor part: targets <- (1 - tau) targets + tau trained, all three networks (one block of the image
// onto the next); both outputs; both step counts.  Without: the critic loss and the gradient-step count alone (one workgroup).
__global__ __launch_bounds__(256) void fw_td3_finish_kernel(Td3StepArgs S) {
  const Td3Layout L = td3_layout(S.d, S.A, S.H);
  const float* sc = S.ws + td3_ws(S.d, S.A, S.H, S.B).scal;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (S.with_actor && e < L.T) {
    float* tp = S.image + L.ta + e;
    *tp = *tp * (1.0f - S.hp.tau) + S.hp.tau * S.image[e];
  }
  if (e == 0) {
    if (S.out) {
      S.out[0] = sc[SAC_S_CRITIC_LOSS];
      if (S.with_actor) S.out[1] = sc[kTd3ScalActor + SAC_S_ACTOR_LOSS];
    }
    int32_t* tail = (int32_t*)(S.image + L.tail);
    tail[0] = tail[0] + 1;
    if (S.with_actor) tail[1] = tail[1] + 1;
    S.ctr[3] = S.ctr[3] + 1;
  }
}

// ---- the launch sequence of one gradient step ----
inline void td3_launch_gemm(hipStream_t st, const Td3StepArgs& S, const float* scal, int epi, const SacGemmJob* jobs, int n) {
  SacGemmArgs G;
  int maxM = 0, maxN = 0;
  for (int k = 0; k < kSacMaxJobs; ++k) {
    G.job[k] = jobs[k < n ? k : 0];
    if (k < n) { maxM = jobs[k].M > maxM ? jobs[k].M : maxM; maxN = jobs[k].N > maxN ? jobs[k].N : maxN; }
  }
  G.epi = epi; G.scal = scal;
  G.beta1 = S.hp.beta1; G.beta2 = S.hp.beta2; G.eps = S.hp.eps;
  hipLaunchKernelGGL(fw_sac_gemm_kernel, dim3((maxN + 63) / 64, (maxM + 63) / 64, n), dim3(256), 0, st, G);
}
inline void td3_update_launch(hipStream_t st, const Td3StepArgs& S) {
  const int d = S.d, A = S.A, H = S.H, B = S.B, Kc = d + A, R = 2 * d + A + 2;
  const Td3Layout L = td3_layout(d, A, H);
  const Td3Ws W = td3_ws(d, A, H, B);
  const SacNet na = sac_net(d, H, A), nc = sac_net(Kc, H, 1);
  float* P = S.image; float* ws = S.ws;
  const float* bt = S.batch;
  const float *scal_c = ws + W.scal, *scal_a = ws + W.scal + kTd3ScalActor;
  const int crit[4] = {L.q1, L.q2, L.t1, L.t2};
  const dim3 rows_grid((B * Kc + 255) / 256), block(256);
  SacGemmJob jb[kSacMaxJobs];
  auto gemm = [&](int epi, int n, const float* scal = nullptr) { td3_launch_gemm(st, S, scal ? scal : scal_c, epi, jb, n); };
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
  // the actor network at image offset `net` on X [B, d]: three launches
  auto actor_forward = [&](int net, const float* X, int ldx, int h1, int h2, int out) {
    jb[0] = fwd(net, na, 1, X, ldx, d, ws + h1, B);
    gemm(SAC_EPI_RELU, 1);
    jb[0] = fwd(net, na, 2, ws + h1, H, H, ws + h2, B);
    gemm(SAC_EPI_RELU, 1);
    jb[0] = fwd(net, na, 3, ws + h2, H, H, ws + out, B);
    gemm(SAC_EPI_LINEAR, 1);
  };
  // the first `count` of Q1, Q2 (on x01) and their targets (on x23): one grid per layer
  auto critic_forward = [&](int count, const float* x01, int ld01, const float* x23) {
    for (int k = 0; k < count; ++k) jb[k] = fwd(crit[k], nc, 1, k < 2 ? x01 : x23, k < 2 ? ld01 : Kc, Kc, ws + W.ch1 + (size_t)k * B * H, B);
    gemm(SAC_EPI_RELU, count);
    for (int k = 0; k < count; ++k) jb[k] = fwd(crit[k], nc, 2, ws + W.ch1 + (size_t)k * B * H, H, H, ws + W.ch2 + (size_t)k * B * H, B);
    gemm(SAC_EPI_RELU, count);
    for (int k = 0; k < count; ++k) jb[k] = fwd(crit[k], nc, 3, ws + W.ch2 + (size_t)k * B * H, H, H, ws + W.q + (size_t)k * B, B);
    gemm(SAC_EPI_LINEAR, count);
  };
  // dL/dh2 and dL/dh1 of the first `count` critics from g3 = dL/dQ
  auto critic_backward = [&](int count) {
    for (int k = 0; k < count; ++k) jb[k] = back(ws + W.g3 + (size_t)k * B, 1, P + crit[k] + nc.W3, 1, H, ws + W.ch2 + (size_t)k * B * H, ws + W.G2 + (size_t)k * B * H, B);
    gemm(SAC_EPI_MASK, count);
    for (int k = 0; k < count; ++k) jb[k] = back(ws + W.G2 + (size_t)k * B * H, H, P + crit[k] + nc.W2, H, H, ws + W.ch1 + (size_t)k * B * H, ws + W.G1 + (size_t)k * B * H, B);
    gemm(SAC_EPI_MASK, count);
  };
  // 0: the smoothing noise (the first block of the step's noise: the last workgroup may run into the second, inside the buffer)
  hipLaunchKernelGGL(fw_sac_noise_kernel, dim3((B * ((A + 3) / 4) + 255) / 256), block, 0, st, S.hp.seed, (const int64_t*)S.ctr, B, A, ws + W.noise);
  // 1-4: the target actor on s', the smoothed action
  actor_forward(L.ta, bt + Kc + 1, R, W.h1t, W.h2t, W.outt);
  hipLaunchKernelGGL(fw_td3_smooth_kernel, rows_grid, block, 0, st, S);
  // 5-8: Q1, Q2 on (s, a) and the targets on (s', a') in one grid per layer; y and dL/dQ
  critic_forward(4, bt, R, ws + W.xnext);
  hipLaunchKernelGGL(fw_td3_target_kernel, dim3(1), block, 0, st, S);
  // 9-11: the critics' backward pass, then all six weight gradients with Adam in one grid
  critic_backward(2);
  for (int k = 0; k < 2; ++k) {
    jb[3 * k + 0] = grad(crit[k], nc.W3, nc.b3, ws + W.ch2 + (size_t)k * B * H, H, H, ws + W.g3 + (size_t)k * B, 1, B);
    jb[3 * k + 1] = grad(crit[k], nc.W2, nc.b2, ws + W.ch1 + (size_t)k * B * H, H, H, ws + W.G2 + (size_t)k * B * H, H, B);
    jb[3 * k + 2] = grad(crit[k], nc.W1, nc.b1, bt, R, Kc, ws + W.G1 + (size_t)k * B * H, H, B);
  }
  gemm(SAC_EPI_ADAM, 6);
  if (!S.with_actor) {
    // 12: the critic loss and the step count; the actor, its moments and the three targets stay as they are
    hipLaunchKernelGGL(fw_td3_finish_kernel, dim3(1), block, 0, st, S);
    return;
  }
  // 12-15: the actor on s, the rows cat(s, pi(s))
  actor_forward(L.actor, bt, R, W.h1a, W.h2a, W.outa);
  hipLaunchKernelGGL(fw_td3_actor_rows_kernel, rows_grid, block, 0, st, S);
  // 16-23: the stepped Q1 on them, its gradient with respect to the action
  critic_forward(1, ws + W.xpi, Kc, nullptr);
  hipLaunchKernelGGL(fw_td3_actor_q_kernel, dim3(1), block, 0, st, S);
  critic_backward(1);
  jb[0] = sac_job(ws + W.G1, H, 1, P + L.q1 + nc.W1 + (size_t)d * H, 1, H, ws + W.dx, A, B, A, H);          // the action rows of W1 alone
  gemm(SAC_EPI_LINEAR, 1);
  hipLaunchKernelGGL(fw_td3_actor_grad_kernel, dim3((B * A + 255) / 256), block, 0, st, S);
  // 24-26: the actor's backward pass, its three weight gradients with Adam (its own step count)
  jb[0] = back(ws + W.gout, A, P + L.actor + na.W3, A, H, ws + W.h2a, ws + W.G2, B);
  gemm(SAC_EPI_MASK, 1);
  jb[0] = back(ws + W.G2, H, P + L.actor + na.W2, H, H, ws + W.h1a, ws + W.G1, B);
  gemm(SAC_EPI_MASK, 1);
  jb[0] = grad(L.actor, na.W3, na.b3, ws + W.h2a, H, H, ws + W.gout, A, B);
  jb[1] = grad(L.actor, na.W2, na.b2, ws + W.h1a, H, H, ws + W.G2, H, B);
  jb[2] = grad(L.actor, na.W1, na.b1, bt, R, d, ws + W.G1, H, B);
  gemm(SAC_EPI_ADAM, 3, scal_a);
  // 27: Polyak of all three targets, outputs, counters
  hipLaunchKernelGGL(fw_td3_finish_kernel, dim3((L.T + 255) / 256), block, 0, st, S);
}

}  // namespace fwsim
