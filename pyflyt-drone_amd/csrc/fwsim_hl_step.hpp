// The high-level command task with the frozen controller at the control rate (controller_hz): the controller
// runs inside fw_step_hl's kernel, once in front of every Aviary step of the agent step, instead of once per agent step in a launch
// of its own.  That kernel is fw_step_kernel_wd (fwsim_direct.hpp) with the controller as its action source (SRC = WD_CTL): it takes
// no actions -- the command in force is the env's FW_SL_TARGET tail, which fw_command_hl / fw_collect_act_hl wrote -- and in front of
// every stepping Aviary step the env's lanes build the controller's raw row (attitude block of the current rigid state, the six
// actuator commands last issued, the command), normalise it with the frozen statistics and evaluate the policy net.  This file holds
// the controller and what that source is built from (CtlArgs, ctl_lds_bytes, ctl_load_stats, ctl_normalise, ctl_attitude_row,
// ctl_forward); the step frame is written once, in fwsim_direct.hpp, with the source's statements in place under `if constexpr`:
// moved into functions of this file they compiled to other device code in some instantiations.
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
// Included by fwsim.hip in front of fwsim_direct.hpp.
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

// LDS of fw_step_kernel_wd<..., WD_CTL> behind the observation tile, and of fw_controller_forward_kernel
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
