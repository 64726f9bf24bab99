// fwsim_probe.hpp -- fw_probe: a TEST HOOK, not used by the product.  One kernel per (op, variant) that evaluates ONE device
// building block of fwsim_device.hpp on n rows of doubles, with the constants a handle's kernels use (Params<T> as build_params
// folded it, TickC<T> / SurfC<T> through load_tick_constants) and in the handle's dtype: a row crosses the ABI as doubles and is
// converted to T in the kernel (the tests pass values that T represents exactly), the results are widened back.
//
// The probes CALL the production __device__ functions; nothing is copied here.  They are inline functions, so every probe kernel
// holds its own compiled copy: the compiler may contract products and sums into FMAs differently from the copy inside a step
// kernel.  A probe result is therefore compared with a reference under a bound, never bit for bit with a step kernel (Philox,
// pure integer arithmetic, is the exception); tests/test_directed_states_gpu.py sends the same corner cases through the step
// kernels themselves.
//
// Row -> lane mapping: one lane per row, or (the 8-lane forms) one group of 8 consecutive lanes per row with every lane of the group
// given the row's inputs.  Rows beyond n are clamped to row n - 1 for the loads (all lanes of a wave stay active: the 8-lane forms
// shuffle and ballot) and only the stores are guarded.  Workgroups are one wave (kWave threads), as the step kernels'.
#pragma once
#include <string>
#include <type_traits>

#include "fwsim_device.hpp"

namespace fwsim {
namespace probe {

// columns of a row, in / out, per (op, variant); 0 = no such variant
struct Shape { int in_cols, out_cols, lanes_per_row; };
inline Shape shape_of(int op, int variant) {
  switch (op) {
    case FW_PROBE_MATH1: return variant == 0 ? Shape{1, 7, 1} : Shape{0, 0, 0};
    case FW_PROBE_MATH2: return variant == 0 ? Shape{2, 2, 1} : Shape{0, 0, 0};
    case FW_PROBE_ROT: return variant == 0 ? Shape{5, 23, 1} : Shape{0, 0, 0};
    case FW_PROBE_EULER:
      if (variant == FW_PROBE_EULER_LANE) return Shape{4, 4, 1};
      if (variant == FW_PROBE_EULER_LANES8) return Shape{4, 32, 8};
      if (variant == FW_PROBE_EULER_INVERSE) return Shape{3, 4, 1};
      return Shape{0, 0, 0};
    case FW_PROBE_QUAT_STEP: return variant == 0 ? Shape{7, 4, 1} : Shape{0, 0, 0};
    case FW_PROBE_SURFACE:
      if (variant == FW_PROBE_SURFACE_SCALAR) return Shape{11, 6, 1};
      if (variant == FW_PROBE_SURFACE_REGS || variant == FW_PROBE_SURFACE_LDS || variant == FW_PROBE_SURFACE_AX) return Shape{11, 6, 8};
      return Shape{0, 0, 0};
    case FW_PROBE_GROUP: return variant == 0 ? Shape{16, 80, 8} : Shape{0, 0, 0};
    case FW_PROBE_RNG:
      if (variant == FW_PROBE_RNG_PHILOX) return Shape{6, 4, 1};
      if (variant == FW_PROBE_RNG_UNIFORM) return Shape{5, 1, 1};
      if (variant == FW_PROBE_RNG_NORMAL2) return Shape{4, 2, 1};
      return Shape{0, 0, 0};
    case FW_PROBE_WIND: return variant == 0 ? Shape{9, 6, 1} : Shape{0, 0, 0};
    default: return Shape{0, 0, 0};
  }
}

template <typename T, int OP, int V>
__global__ __launch_bounds__(kWave) void fw_probe_kernel(const Params<T>* __restrict__ Pp, const double* __restrict__ in, double* __restrict__ out, int n) {
  constexpr int LPR = (OP == FW_PROBE_GROUP || (OP == FW_PROBE_EULER && V == FW_PROBE_EULER_LANES8) ||
                       (OP == FW_PROBE_SURFACE && V != FW_PROBE_SURFACE_SCALAR)) ? 8 : 1;
  const Params<T>& P = *Pp;
  const int gid = blockIdx.x * kWave + threadIdx.x;
  const int row = gid / LPR, sub = gid % LPR;
  const int rowc = row < n ? row : n - 1;
  const bool live = row < n;
  (void)sub; (void)P;

  if constexpr (OP == FW_PROBE_MATH1) {
    const double* x = in + (size_t)rowc;
    double* o = out + (size_t)rowc * 7;
    const T a = (T)x[0];
    T s, c;
    M<T>::sincos_(a, &s, &c);
    const T r0 = M<T>::rcp_(a), r1 = M<T>::sqrt_(a), r2 = M<T>::sin_(a), r5 = M<T>::asin_(a), r6 = M<T>::log_(a);
    if (live) { o[0] = (double)r0; o[1] = (double)r1; o[2] = (double)r2; o[3] = (double)s; o[4] = (double)c; o[5] = (double)r5; o[6] = (double)r6; }
  } else if constexpr (OP == FW_PROBE_MATH2) {
    const double* x = in + (size_t)rowc * 2;
    double* o = out + (size_t)rowc * 2;
    const T a = (T)x[0], b = (T)x[1];
    const T r0 = M<T>::div_(a, b), r1 = M<T>::atan2_(a, b);
    if (live) { o[0] = (double)r0; o[1] = (double)r1; }
  } else if constexpr (OP == FW_PROBE_ROT) {
    const double* x = in + (size_t)rowc * 5;
    double* o = out + (size_t)rowc * 23;
    T q[4] = { (T)x[0], (T)x[1], (T)x[2], (T)x[3] };
    T m[9], mu[9];
    rot_from_quat<T>(q, m);
    rot_from_unit_quat<T>(q, mu);
    const T ton = two_over_norm2<T>((T)x[4]);
    normalize_quat<T>(q);
    if (live) {
#pragma unroll
      for (int k = 0; k < 9; ++k) { o[k] = (double)m[k]; o[9 + k] = (double)mu[k]; }
#pragma unroll
      for (int k = 0; k < 4; ++k) o[18 + k] = (double)q[k];
      o[22] = (double)ton;
    }
  } else if constexpr (OP == FW_PROBE_EULER && V == FW_PROBE_EULER_INVERSE) {
    const double* x = in + (size_t)rowc * 3;
    double* o = out + (size_t)rowc * 4;
    const T e[3] = { (T)x[0], (T)x[1], (T)x[2] };
    T q[4];
    quat_from_euler<T>(e, q);
    if (live) {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (double)q[k];
    }
  } else if constexpr (OP == FW_PROBE_EULER) {
    const double* x = in + (size_t)rowc * 4;
    // LANES8: every lane of the group stores its own copy of the handed-round result, [8][4] per row -- the callers use it on all 8
    double* o = out + (size_t)rowc * (4 * LPR) + (size_t)sub * 4;
    const T q[4] = { (T)x[0], (T)x[1], (T)x[2], (T)x[3] };
    T e[3];
    bool lock;
    if constexpr (V == FW_PROBE_EULER_LANES8) lock = euler_from_quat_lanes8<T>(q, e);
    else lock = euler_from_quat<T>(q, e);
    if (live) { o[0] = (double)e[0]; o[1] = (double)e[1]; o[2] = (double)e[2]; o[3] = lock ? 1.0 : 0.0; }
  } else if constexpr (OP == FW_PROBE_QUAT_STEP) {
    const double* x = in + (size_t)rowc * 7;
    double* o = out + (size_t)rowc * 4;
    TickC<T> C; SurfC<T> mine; T wmask;
    load_tick_constants<T, 1>(Pp, C, mine, wmask);
    Rigid<T> S;
#pragma unroll
    for (int k = 0; k < 3; ++k) { S.w[k] = (T)x[k]; S.p[k] = (T)0; S.v[k] = (T)0; }
#pragma unroll
    for (int k = 0; k < 4; ++k) S.q[k] = (T)x[3 + k];
    quat_integrate<T>(C, S);
    if (live) {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (double)S.q[k];
    }
  } else if constexpr (OP == FW_PROBE_SURFACE) {
    const double* x = in + (size_t)rowc * 11;
    double* o = out + (size_t)rowc * 6;
    int surf = (int)x[0];
    surf = surf < 0 ? 0 : (surf >= FW_NUM_SURFACES ? FW_NUM_SURFACES - 1 : surf);
    const T act = (T)x[1];
    const T v_b[3] = { (T)x[2], (T)x[3], (T)x[4] }, w_b[3] = { (T)x[5], (T)x[6], (T)x[7] }, wind_b[3] = { (T)x[8], (T)x[9], (T)x[10] };
    T f[3] = { (T)0, (T)0, (T)0 }, tq[3] = { (T)0, (T)0, (T)0 };
    bool mine_row = true;
    if constexpr (V == FW_PROBE_SURFACE_SCALAR) {
      // as the one-lane-per-env tick: a rolled loop whose index is wave-uniform, so the constants arrive by scalar loads
#pragma unroll 1
      for (int s = 0; s < FW_NUM_SURFACES; ++s)
        if (s == surf) surface_wrench<T, const SurfC<T>>(P.s[s], act, v_b, w_b, wind_b, f, tq);
    } else {
      // as the 8-lane tick: lane `sub` of the group carries surface min(sub, 4) (load_tick_constants); the row is read from the lane
      // whose surface it names
      TickC<T> C; SurfC<T> mine; T wmask;
      load_tick_constants<T, 8, true>(Pp, C, mine, wmask);
      mine_row = (sub == surf);
      if constexpr (V == FW_PROBE_SURFACE_REGS) {
        surface_wrench<T, SurfC<T>>(mine, act, v_b, w_b, wind_b, f, tq);
      } else if constexpr (V == FW_PROBE_SURFACE_LDS) {
        __shared__ SurfC<T> lds[kWave];
        constexpr int NW = (int)(sizeof(SurfC<T>) / sizeof(T));
        const T* src = reinterpret_cast<const T*>(&mine);
        volatile T* dst = reinterpret_cast<volatile T*>(&lds[threadIdx.x]);
#pragma unroll
        for (int k = 0; k < NW; ++k) dst[k] = src[k];
        volatile SurfC<T>& S = lds[threadIdx.x];
        surface_wrench<T, volatile SurfC<T>>(S, act, v_b, w_b, wind_b, f, tq);
      } else {
        if (sub >= FW_NUM_SURFACES) mine.hra = (T)0;           // as the axis-aligned step kernel: lanes 5-7 evaluate a zero wrench
        surface_wrench_ax<T>(mine, act, v_b, w_b, wind_b, f, tq);
      }
    }
    if (live && mine_row) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { o[k] = (double)f[k]; o[3 + k] = (double)tq[k]; }
    }
  } else if constexpr (OP == FW_PROBE_GROUP) {
    // in: v[8] (one per lane), b[8] (one per lane).  out, per lane [10]: sum v, min v, or of (uint32) b, any (b odd), lane_pick5 of
    // v[0..4], and act[0..4] after lane_act_scatter of v[0..4], a lane-local change (+ 1000 * sub) and lane_act_gather
    const double* x = in + (size_t)rowc * 16;
    double* o = out + (size_t)rowc * 80 + (size_t)sub * 10;
    const T v = (T)x[sub];
    const uint32_t b = (uint32_t)x[8 + sub];
    const T vs = group_sum<8, T>(v), vm = group_min<8, T>(v);
    const uint32_t bo = group_or<8>(b);
    const bool any = group_any<8>((b & 1u) != 0u);
    const T pick = lane_pick5<T>((T)x[0], (T)x[1], (T)x[2], (T)x[3], (T)x[4]);
    Rigid<T> S;
#pragma unroll
    for (int k = 0; k < FW_NUM_SURFACES; ++k) S.act[k] = (T)x[k];
    LaneAct<T> LA;
    lane_act_scatter<T>(S, LA);
    LA.a += (T)(1000 * sub);
    lane_act_gather<T>(S, LA);
    if (live) {
      o[0] = (double)vs; o[1] = (double)vm; o[2] = (double)bo; o[3] = any ? 1.0 : 0.0; o[4] = (double)pick;
#pragma unroll
      for (int k = 0; k < FW_NUM_SURFACES; ++k) o[5 + k] = (double)S.act[k];
    }
  } else if constexpr (OP == FW_PROBE_RNG && V == FW_PROBE_RNG_PHILOX) {
    const double* x = in + (size_t)rowc * 6;
    double* o = out + (size_t)rowc * 4;
    uint32_t r[4];
    philox4x32_10((uint32_t)x[0], (uint32_t)x[1], (uint32_t)x[2], (uint32_t)x[3], (uint32_t)x[4], (uint32_t)x[5], r);
    if (live) {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (double)r[k];
    }
  } else if constexpr (OP == FW_PROBE_RNG && V == FW_PROBE_RNG_UNIFORM) {
    const double* x = in + (size_t)rowc * 5;
    const double u = rng_uniform<T>(P, (uint32_t)x[0], (uint32_t)x[1], (uint32_t)x[2], x[3], x[4]);
    if (live) out[rowc] = u;
  } else if constexpr (OP == FW_PROBE_RNG) {
    const double* x = in + (size_t)rowc * 4;
    double* o = out + (size_t)rowc * 2;
    const uint64_t a = ((uint64_t)(uint32_t)x[0] << 32) | (uint32_t)x[1], b = ((uint64_t)(uint32_t)x[2] << 32) | (uint32_t)x[3];
    T z0, z1;
    normal2_from_words<T>(a, b, z0, z1);
    if (live) { o[0] = (double)z0; o[1] = (double)z1; }
  } else if constexpr (OP == FW_PROBE_WIND) {
    // gust_init at `tick`, k x gust_advance, wind_from_phase -- against wind_at at tick + k
    const double* x = in + (size_t)rowc * 9;
    double* o = out + (size_t)rowc * 6;
    const T wb[3] = { (T)x[0], (T)x[1], (T)x[2] }, wa[3] = { (T)x[3], (T)x[4], (T)x[5] };
    const T phase = (T)x[6];
    const int32_t tick = (int32_t)x[7];
    int k = (int)x[8];
    k = k < 0 ? 0 : (k > 64 ? 64 : k);
    T g[2], w1[3], w2[3];
    gust_init<T>(P, phase, tick, g);
    for (int i = 0; i < k; ++i) gust_advance<T>(P, g);
    wind_from_phase<T>(P, wb, wa, g, w1);
    wind_at<T>(P, wb, wa, phase, tick + k, w2);
    if (live) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { o[i] = (double)w1[i]; o[3 + i] = (double)w2[i]; }
    }
  }
}

template <typename T, int OP, int V>
inline hipError_t launch(const void* params_dev, const double* in, double* out, int n, hipStream_t stream) {
  const Shape sh = shape_of(OP, V);
  const long long threads = (long long)n * sh.lanes_per_row;
  const unsigned grid = (unsigned)((threads + kWave - 1) / kWave);
  hipLaunchKernelGGL((fw_probe_kernel<T, OP, V>), dim3(grid), dim3(kWave), 0, stream, (const Params<T>*)params_dev, in, out, n);
  return hipGetLastError();
}

// the (op, variant) table; `axis_ok`: the handle's geometry is the one surface_wrench_ax is written for.  Returns FW_OK after the
// launch, FW_EINVAL for an (op, variant) that does not exist, FW_EUNSUPPORTED (with `err` set) for one this handle has no kernel for.
template <typename T>
inline int dispatch(int op, int variant, bool axis_ok, const void* params_dev, const double* in, double* out, int n, hipStream_t stream,
                    hipError_t& herr, std::string& err) {
  herr = hipSuccess;
#define FW_PROBE_CASE(OP, V) if (op == (OP) && variant == (V)) { herr = launch<T, (OP), (V)>(params_dev, in, out, n, stream); return FW_OK; }
  FW_PROBE_CASE(FW_PROBE_MATH1, 0)
  FW_PROBE_CASE(FW_PROBE_MATH2, 0)
  FW_PROBE_CASE(FW_PROBE_ROT, 0)
  FW_PROBE_CASE(FW_PROBE_EULER, FW_PROBE_EULER_LANE)
  FW_PROBE_CASE(FW_PROBE_EULER, FW_PROBE_EULER_LANES8)
  FW_PROBE_CASE(FW_PROBE_EULER, FW_PROBE_EULER_INVERSE)
  FW_PROBE_CASE(FW_PROBE_QUAT_STEP, 0)
  FW_PROBE_CASE(FW_PROBE_SURFACE, FW_PROBE_SURFACE_SCALAR)
  FW_PROBE_CASE(FW_PROBE_SURFACE, FW_PROBE_SURFACE_REGS)
  FW_PROBE_CASE(FW_PROBE_SURFACE, FW_PROBE_SURFACE_LDS)
  if (op == FW_PROBE_SURFACE && variant == FW_PROBE_SURFACE_AX) {
    if constexpr (std::is_same<T, double>::value) {
      if (!axis_ok) { err = "fw_probe: the axis-aligned surface wrench needs a handle whose surfaces have forward = e_x, lift = e_y or e_z and a diagonal inertia"; return FW_EUNSUPPORTED; }
      herr = launch<T, FW_PROBE_SURFACE, FW_PROBE_SURFACE_AX>(params_dev, in, out, n, stream);
      return FW_OK;
    } else {
      err = "fw_probe: the axis-aligned surface wrench is built for float64 handles only";
      return FW_EUNSUPPORTED;
    }
  }
  FW_PROBE_CASE(FW_PROBE_GROUP, 0)
  FW_PROBE_CASE(FW_PROBE_RNG, FW_PROBE_RNG_PHILOX)
  FW_PROBE_CASE(FW_PROBE_RNG, FW_PROBE_RNG_UNIFORM)
  FW_PROBE_CASE(FW_PROBE_RNG, FW_PROBE_RNG_NORMAL2)
  FW_PROBE_CASE(FW_PROBE_WIND, 0)
#undef FW_PROBE_CASE
  err = "fw_probe: unknown (op, variant) = (" + std::to_string(op) + ", " + std::to_string(variant) + ")";
  return FW_EINVAL;
}

}  // namespace probe
}  // namespace fwsim
