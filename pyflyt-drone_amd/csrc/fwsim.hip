// fwsim.hip -- kernels + C-ABI host side of libfwsim_hip.so (gfx950 only).
// See include/fwsim.h for the contract and fwsim_device.hpp for the device code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "fwsim_device.hpp"
#include "fwsim_rollout.hpp"
#include "fwsim_ppo.hpp"
#include "fwsim_collect.hpp"
#include "fwsim_fused.hpp"
#include "fwsim_objlock.hpp"
#include "fwsim_render.hpp"

using namespace fwsim;

// ======================================================================
// kernels
// ======================================================================

// K0: mark every env as an un-reset shell (step() before reset() is inert).
template <typename T>
__global__ void fw_init_kernel(DevState<T> D, int tile) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= D.npad) return;
  for (int f = 0; f < RF_COUNT; ++f) D.r[tile_index(tile, RF_COUNT, f, env)] = (T)0;
  D.r[tile_index(tile, RF_COUNT, RF_QUAT + 3, env)] = (T)1;
  for (int f = 0; f < IF_COUNT; ++f) D.i[tile_index(tile, IF_COUNT, f, env)] = 0;
  D.i[tile_index(tile, IF_COUNT, IF_FLAGS, env)] = FL_TERM;
  D.i[tile_index(tile, IF_COUNT, IF_EPISODE, env)] = -1;
}

// Kw: one lane integrates the wind-free warm-up once; resets then copy it.
template <typename T>
__global__ void fw_warm_kernel(Params<T>* Pm) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const Params<T>& P = *Pm;
  Rigid<T> S;
  for (int k = 0; k < 3; ++k) { S.p[k] = P.start_pos[k]; S.v[k] = P.start_vel[k]; S.w[k] = (T)0; }
  for (int k = 0; k < 4; ++k) S.q[k] = P.start_quat[k];
  for (int k = 0; k < FW_NUM_ACTUATORS; ++k) S.act[k] = (T)0;
  T cmd0[FW_NUM_ACTUATORS] = {(T)0, (T)0, (T)0, (T)0, (T)0, (T)0};
  T wind0[3] = {(T)0, (T)0, (T)0};
  int ticks = P.warmup_aviary_steps * P.ticks_per_aviary;
  TickC<T> C; SurfC<T> mine; T wmask;
  load_tick_constants<T, 1>(Pm, C, mine, wmask);
  T R[9];
  normalize_quat<T>(S.q);
  rot_from_unit_quat<T>(S.q, R);
  LaneAct<T> LA; LA.a = (T)0; LA.cmd = (T)0;      // (unused by the one-lane-per-env tick)
  for (int t = 0; t < ticks; ++t) (void)physics_tick<T, false, 1>(P, C, S, R, cmd0, (T)0, wind0, mine, wmask, LA);
  for (int k = 0; k < 3; ++k) { Pm->warm[k] = S.p[k]; Pm->warm[7 + k] = S.v[k]; Pm->warm[10 + k] = S.w[k]; }
  for (int k = 0; k < 4; ++k) Pm->warm[3 + k] = S.q[k];
  for (int k = 0; k < FW_NUM_ACTUATORS; ++k) Pm->warm[13 + k] = S.act[k];
  Pm->warm_ticks = ticks;
  // the observation every cached reset returns, up to its target deltas
  const T a0[4] = {(T)0, (T)0, (T)0, (T)0};
  T Rw[9];
  (void)write_obs_attitude<T, false>(P, S, a0, Rw, [&](int k, T v) { Pm->warm_obs[k] = v; });
  for (int k = 0; k < 9; ++k) Pm->warm_R[k] = Rw[k];
}

// Ki: the step image of a handle (fwsim_device.hpp: StepImage), behind its Params.  One wave; lanes 0-7 write a row each.
template <typename T>
__global__ void fw_step_image_kernel(Params<T>* Pm) {
  if (threadIdx.x >= 8 || blockIdx.x != 0) return;
  fill_step_image<T>(*Pm, const_cast<StepImage<T>*>(step_image_of<T>(Pm)), (int)threadIdx.x);
}

// Prefetch that stays where it is written.  What a resetting env copies in the epilogue is only USED inside the divergent reset
// block, and LLVM sinks a plain load down to its only use: the round trip the prefetch was meant to hide then sits inside that
// block (tools/wave_profile.py: ~2.3 k cycles in the waves that reset -- the slowest waves of nearly every launch -- whatever was
// "requested" ahead of the observation pass).  Volatile loads are no way out (the backend waits for each at once: 20.1 -> 24.5 us
// per step).  So the load is issued by hand: `pf_issue` emits it here, `pf_wait` (one s_waitcnt for the lot, tied to the values
// through "+v") comes right before the first use.  The compiler's own vmcnt bookkeeping stays conservative-correct: loads return
// in order, extra outstanding loads only make its waits longer.
__device__ __forceinline__ void pf_issue(double& dst, const double* p) { asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(dst) : "v"(p) : "memory"); }
__device__ __forceinline__ void pf_issue(float& dst, const float* p) { asm volatile("global_load_dword %0, %1, off" : "=v"(dst) : "v"(p) : "memory"); }
template <typename T> __device__ __forceinline__ void pf_wait(T& a, T& b, T& c, T& d) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) :: "memory"); }
template <typename T> __device__ __forceinline__ void pf_tie(T& a, T& b, T& c, T& d) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }
template <typename T> __device__ __forceinline__ T vload(const T* p) { return *p; }

// action shown in the observation: src 0 = this step's input, 1 = stored (stale), 2 = zeros
template <typename T, bool COH = false>
__device__ __forceinline__ void load_action(const DevState<T>& D, const T* actions, int env, int src, T a[4]) {
  const T* ap = actions + (size_t)env * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    T cur = COH ? ld_coherent(ap + k) : ap[k], old = D.r[(size_t)(RF_ACTION + k) * D.npad + env];
    a[k] = (src == 0) ? cur : (src == 1) ? old : (T)0;
  }
}

// ------------------------------------------------------------------------------------------
// Background warm-up ("shadow") -- used when the reset warm-up cannot be cached (wind acts on
// the dynamics, or the task has a camera).  In the latency regime the launch time is the time
// of its slowest wave, and a wave that has to sample a scenario and integrate the 10 warm-up
// Aviary steps of a reset in-kernel takes several times as long as its neighbours -- with
// thousands of envs most launches contain one (rocprofv3: 27 us min, 96 us max, 61 us mean).
// Instead every env owns a shadow copy of its state holding the START of its NEXT episode.
// Extra workgroups of the same launch (blocks >= the step blocks; they land on SIMDs the
// latency mapping leaves idle) build it in chunks no longer than a stepping wave -- launch 1:
// scenario sampling, launches 2-4: <= step_ratio warm-up Aviary steps each -- and a reset
// swaps the finished shadow in (a copy).  An episode is a pure function of (seed, env,
// episode), so the result equals the in-kernel path (to rounding: the compiler contracts
// FMAs differently at the two inlining sites), which stays as the fallback while a shadow is
// not ready (episodes shorter than ~5 steps).
// Protocol (kernel-boundary visibility only, one writer per word, 8-byte words so nothing
// tears): the env's own lanes never touch the shadow arrays; they post `sreq` = (episode
// wanted, launch index).  The worker ignores a request carrying the current launch index
// (it may be half a launch old), owns the shadow arrays and `sdone` = (episode built, launch
// index, progress); the env's lanes accept a finished shadow only if it was finished in an
// EARLIER launch.
// ------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ DevState<T> shadow_view(const DevState<T>& D) {
  DevState<T> V = D; V.r = D.rs; V.i = nullptr; return V;
}
__device__ __forceinline__ unsigned long long pack_done(uint32_t ep, uint32_t epoch, int done) {
  return ((unsigned long long)ep << 32) | ((unsigned long long)(epoch & 0xFFFFFFu) << 8) | (unsigned long long)(done & 0xFF);
}

// worker: one chunk of work on the shadows of the envs of block `blk` (at most `max_chunk` warm-up Aviary steps; 0 = step_ratio)
template <typename T, int G, int TKIND>
__device__ __forceinline__ void shadow_worker(const Params<T>* __restrict__ Pp, const ObjC<T>* __restrict__ OCp, DevState<T> D, int blk, int max_chunk = 0) {
  constexpr bool OBJ = TKIND == FW_TASK_OBJLOCK, COMB = TKIND == FW_TASK_WAYPOINT_OBJLOCK, HASOBJ = OBJ || COMB;
  constexpr int EPW = kWave / G;
  const Params<T>& P = *Pp;
  const ObjC<T>& OC = *OCp;
  const int lane = threadIdx.x & (kWave - 1), sub = (G == 1) ? 0 : (lane & (G - 1)), row = lane / G;     // (the capture wave of a two-wave workgroup works here too)
  const bool leader = sub == 0;
  const int env = blk * EPW + row;
  const bool active = env < D.n;
  const int envc = active ? env : D.n - 1;
  const size_t n = D.npad;
  const int total = P.warmup_aviary_steps + 1;                  // progress 1 = scenario sampled, then one per warm-up step
  // A warm-up of no steps: the scenario pass leaves progress 0 and the next chunk is the closing pass alone (no Aviary step, only
  // end_reset()'s compute_state and the first observation), so that progress == total means "closed" for every warm-up length.
  const int sampled = P.warmup_aviary_steps > 0 ? 1 : 0;
  const unsigned long long req = D.sreq[envc], dn = D.sdone[envc];
  const uint32_t target = (uint32_t)(req >> 32);
  const bool fresh = active && (uint32_t)req != D.epoch && req != ~0ull;     // a request of an earlier launch
  int done = (int)(dn & 0xFF);
  const bool begin = fresh && (uint32_t)(dn >> 32) != target;   // new episode wanted: (re)start
  int left = (fresh && !begin) ? min(total - done, max_chunk > 0 ? max_chunk : P.step_ratio) : 0;
  if (__ballot(begin || left > 0) == 0ull) return;              // nothing to do in this wave: the common case
  const DevState<T> V = shadow_view<T>(D);
  if (begin) {
    Rigid<T> S0; int32_t tick0 = 0, episode = (int32_t)target - 1, nr = 0; T wb0[3], wa0[3], wph0;
    T tm0[3]; (void)begin_reset<T, G>(P, V, env, S0, tick0, episode, nr, wb0, wa0, wph0, tm0);     // shadow_on implies !warm_valid
    if (HASOBJ) {
      ObjState<T> O0;
      obj_reset_state<T, OBJ>(O0);
      if (OBJ) obj_spawn<T, G>(P, OC, V, env, target, leader, O0); else comb_spawn<T, G>(P, OC, V, env, target, leader, O0);
      if (leader) obj_store<T, OBJ>(V, env, O0);
    }
    if (leader) { store_rigid<T>(V, env, S0); D.is[env] = 0; D.sdone[env] = pack_done(target, D.epoch, sampled); }
  }
  if (__ballot(left > 0) == 0ull) return;
  TickC<T> C; SurfC<T> mine; T wmask;
  load_tick_constants<T, G, false>(Pp, C, mine, wmask);
  Rigid<T> S;
  load_rigid<T>(V, envc, S);
  T R[9];
  rot_from_unit_quat<T>(S.q, R);
  int32_t tick = D.is[envc];
  T wb[3], wa[3], wph;
#pragma unroll
  for (int k = 0; k < 3; ++k) { wb[k] = V.r[(RF_WIND + k) * n + envc]; wa[k] = V.r[(RF_WIND + 3 + k) * n + envc]; }
  wph = V.r[(RF_WIND + 6) * n + envc];
  T gust[2];
  gust_init<T>(P, wph, tick, gust);
  ObjState<T> O;
  if (HASOBJ) { obj_load<T, OBJ>(V, envc, O); O.near_mask = 0u; O.near_n = 0; }
  const T cmd0[FW_NUM_ACTUATORS] = {(T)0, (T)0, (T)0, (T)0, (T)0, (T)0};
  LaneAct<T> LA; LA.cmd = (T)0; LA.a = (T)0;
  if (G == 8) lane_act_scatter<T>(S, LA);
  const int chunk = left;
  int steps = sampled ? left : 0;
#pragma unroll 1
  while (__ballot(steps > 0) != 0ull) {
    const bool stepped = steps > 0;
    if (stepped) {
      (void)aviary_step<T, true, G, HASOBJ>(P, C, OC, V, envc, O, S, R, cmd0, tick, (T)0, (T)0, wb, wa, gust, mine, wmask, LA);
      steps -= 1;
    }
    if (HASOBJ) obj_capture_step<T, G>(OC, V, stepped, envc, O, S, R, tick);
  }
  if (G == 8) lane_act_gather<T>(S, LA);
  if (chunk > 0 && done + chunk == total) {
    // warm-up complete: end_reset()'s first compute_state and the observation reset() returns (zero action) are part of the
    // shadow, so that the reset that takes it is a copy (state rows, observation row) and nothing else.  The rows of the
    // shadow the worker never writes (stored action, episode return) are zero from the allocation: what a fresh episode holds.
    T nd = (T)0;
    if (OBJ) obj_compute_state<T>(O);
    else {
      T t0[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) t0[k] = V.r[(size_t)(RF_TARGETS + k) * n + envc];
      nd = end_reset<T, G>(P, V, envc, (int32_t)target, S, t0);
      if (COMB) comb_compute_state<T>(OC, O, P.num_targets == 0);
    }
    if (leader) {
      const T a0[4] = {(T)0, (T)0, (T)0, (T)0};
      T* orow = D.sobs + (size_t)env * P.obs_dim;
      if (OBJ) obj_write_obs<T>(P, O, S, a0, [&](int k, T v) { orow[k] = v; });
      else if (COMB) comb_write_obs<T>(P, V, env, O, S, a0, 0, [&](int k, T v) { orow[k] = v; });
      else write_obs<T>(P, V, env, S, a0, 0, [&](int k, T v) { orow[k] = v; });
      V.r[RF_NEW_DIST * n + env] = nd;
    }
  }
  if (chunk > 0 && leader) {
    store_rigid<T>(V, env, S);
    D.is[env] = tick;
    if (HASOBJ) obj_store<T, OBJ>(V, env, O);
    D.sdone[env] = pack_done(target, D.epoch, done + chunk);
  }
}

// Wind-free waypoints: the reset itself is cached (warm state, its observation), what remains per env is sampling the next
// episode's waypoints (3 Philox blocks + 2 sincos per waypoint).  The same hand-off as above lets a worker block do that
// ahead of time into the shadow's waypoint rows; the reset then only copies 3 words per lane (requested at launch start).
// (WAVE1: the caller is the second wave of a step workgroup working that workgroup's own tile, fw_step_kernel_g8xo; every other caller is wave 0)
template <typename T, int G, bool WAVE1 = false>
__device__ __forceinline__ void scenario_worker(const Params<T>* __restrict__ Pp, DevState<T> D, int blk) {
  constexpr int EPW = kWave / G;
  const int lane = WAVE1 ? threadIdx.x & (kWave - 1) : threadIdx.x, sub = (G == 1) ? 0 : (lane & (G - 1)), row = lane / G;
  const int env = blk * EPW + row;
  const bool active = env < D.n;
  const int envc = active ? env : D.n - 1;
  const unsigned long long req = D.sreq[envc], dn = D.sdone[envc];
  const uint32_t target = (uint32_t)(req >> 32);
  const bool fresh = active && (uint32_t)req != D.epoch && req != ~0ull;          // a request of an earlier launch
  const bool begin = fresh && (uint32_t)(dn >> 32) != target;
  if (__ballot(begin) == 0ull) return;
  if (begin) {
    const Params<T>& P = *Pp;
    Scenario<T> sc;
    sample_scenario_inl<T, G>(Pp, D.rs, (size_t)D.npad, env, target, &sc);
    // ... and the observation the new episode starts with (cached attitude block ++ deltas of the fresh waypoints, zero padded)
    // plus its first distance: the reset that takes this hand-off is then a copy (state = the cached warm state)
    T* orow = D.sobs + (size_t)env * P.obs_dim;
    for (int k = sub; k < P.att_dim; k += G) orow[k] = Pp->warm_obs[k];
    if (G > 1) {
      if (sub < P.ctx) {
        T d[3] = {(T)0, (T)0, (T)0}, b[3] = {(T)0, (T)0, (T)0};
        if (sub < P.num_targets) {
#pragma unroll
          for (int k = 0; k < 3; ++k) d[k] = sc.t_mine[k] - P.warm[k];
          mtv(P.warm_R, d, b);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) orow[P.att_dim + 3 * sub + k] = b[k];
      }
      if (sub == 0) {
        T nd = (T)0;
        if (P.num_targets > 0) {
          const T dx = sc.t_mine[0] - P.warm[0], dy = sc.t_mine[1] - P.warm[1], dz = sc.t_mine[2] - P.warm[2];
          nd = M<T>::sqrt_(dx * dx + dy * dy + dz * dz);
        }
        D.rs[(size_t)RF_NEW_DIST * D.npad + env] = nd;
      }
    }
    if (sub == 0) D.sdone[env] = pack_done(target, D.epoch, 1);
  }
}

// Dev-only per-wave cycle accounting (tools/wave_profile.py builds a second library with -DFW_PROFILE).
#ifdef FW_PROFILE
#define FWP_NOW() ((long long)__builtin_readcyclecounter())
#define FWP(...) __VA_ARGS__
constexpr int kProfSlots = 256, kProfWords = 12;
#ifdef FW_PROFILE_PHASES
constexpr bool getenv_ph = true;     // the words of the wave split carry the phases of capture_body instead (tools/wave_profile.py --phases)
#else
constexpr bool getenv_ph = false;
#endif
#else
#define FWP(...)
#endif

constexpr int kObsHandWords = 20;   // fw_step_kernel_g8xo: words per env of the LDS block the step wave hands the observation wave (step_body OBSW)

// Per-lane phase of the fused step state machine.
enum Phase : int { PH_STEP = 0, PH_WARM = 1, PH_DONE = 2 };

// K1: one agent step, everything fused.  One wave per workgroup; the wave holds 64/G envs
// (G lanes per env, see fwsim_device.hpp).
//
// The kernel is a per-env state machine around ONE inlined Aviary step:
//   PH_STEP  the env runs its (<= step_ratio) sub-steps; after each one the
//            reference's compute_state / compute_term_trunc_reward are applied;
//   PH_WARM  the env finished its episode mid-launch and (wind acting on the
//            dynamics) is integrating its reset warm-up with a zero setpoint --
//            concurrently with neighbours that are still in PH_STEP;
//   PH_DONE  results latched; the lanes idle until the wave-uniform exit.
// Outputs are latched in registers and stored once at the end.
// GENERAL = wind is on (per-env wind registers, and -- if it acts on the dynamics -- the
// PH_WARM path).  The wind-free instantiation (the headline config) carries none of that.
// OBJ = the ObjLock task (duck / analytic camera / vision shaping, fwsim_objlock.hpp); its state rides in registers.
// WPE = waves per SIMD the instantiation is built for (G = 8 only): 1 = the whole register file (359 registers: shared tick
// constants resident in VGPRs), 2 = capped at 256 registers so that two waves share a SIMD -- the constants then stay
// wave-uniform (scalar loads); used between 8 192 and 65 536 envs, where the 1-wave build would run its waves in two rounds.
// COLLECT = the step waves of fw_collect_step (fwsim_fused.hpp): block indices are offset by the act waves in front, the
// actions are waited for and read coherently, and the epilogue carries the statistics of VecNormalize.step_wait.
// HELP = the workgroup has a capture wave (fwsim_objlock.hpp, "The capture wave"): camera tasks on the 8-lane mapping.
// AUX = the workgroup has a second wave (fw_step_kernel_g8x) that draws the launch's motor noise while the step wave is in its
// prologue: the draw reads three integers per env and nothing of the launch's physics.  Same lane -> (env, sub) map on both waves;
// the values cross in LDS ([kWave][2] behind the output stash) and the waves meet at ONE __syncthreads() in front of the sub-step
// loop, which both execute unconditionally.
// SH = the shape the instantiation is compiled for (fwsim_device.hpp: ShapeOfParams reads Params, as every kernel but one does;
// ShapeTrainWaypoints is the headline config's, fw_step_kernel_g8xs): trip counts, row lengths and the reward / attitude / noise
// variants become constants, and the four numbers of the task logic that stay run-time values (max_steps, auto_reset, dome, reach) are
// loaded once in front of the sub-step loop.  Integers only: the floating-point results are those of the run-time shape, bit for
// bit (sum_squares_fma pins the two sums of squares whose FMA contraction would otherwise follow the shape of the loop around them).
// OBSW = the second wave stays to the end of the launch (fw_step_kernel_g8xo; a fixed shape with AUX only).  Behind barrier 1 it is the
// scenario worker of its own tile -- the grid has no worker half, which could not start before whole step workgroups had left -- and
// then the observation writer: the step wave leaves what the pass reads (rigid state, actuators, target index, a mode word per env:
// 0 no reset, 1 reset whose first row the worker left, 2 reset by the in-kernel fallback) in LDS behind the normals, the waves meet at
// a SECOND __syncthreads() behind the end-of-step latch, and the second wave runs the pass, the terminal-observation copy and the
// flush while the step wave stores state, counters and -- mode 2 only -- the new episode's row, straight to memory (the flush skips
// those rows: no word of `obs` has two writers).  Both waves execute both barriers unconditionally; nothing else synchronises them.
template <typename T, bool GENERAL, int G, int TKIND, int WPE = 1, bool COLLECT = false, bool HELP = false, bool AX = false, bool AUX = false,
          typename SH = ShapeOfParams, int OBSM = 0>
__device__ __forceinline__
void step_body(const Params<T>* __restrict__ Pp, const ObjC<T>* __restrict__ OCp, DevState<T> Dg,
               const T* __restrict__ actions, T* __restrict__ obs, T* __restrict__ reward,
               uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated, T* __restrict__ terminal_obs,
               int32_t* __restrict__ info, const CollectArgs* __restrict__ CAp = nullptr) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const Params<T>& P = *Pp;
  constexpr bool OBJ = TKIND == FW_TASK_OBJLOCK;              // duck only
  constexpr bool COMB = TKIND == FW_TASK_WAYPOINT_OBJLOCK;    // waypoints, then the duck
  constexpr bool HASOBJ = OBJ || COMB;
  constexpr int EPW = kWave / G;                     // envs per wave
  // Wind-free waypoints (the headline config): the episode start is the cached warm state for every env, so an
  // auto-reset is deferred to the epilogue -- the obs pass there writes the terminal observation, the new episode's
  // observation is the cached attitude block + the deltas of the freshly sampled waypoints.  No second obs pass, no
  // sampling inside the step loop, and the waves that contain a reset finish with the others.
  constexpr bool DEFER = !GENERAL && TKIND == FW_TASK_WAYPOINTS;
  static_assert(!SH::kFixed || (std::is_same<T, double>::value && DEFER && G == 8 && !COLLECT && !HELP), "a fixed shape is threaded through the wind-free 8-lane waypoints path only");
  // OBSM: 0 = no such wave; 2 = fw_step_kernel_g8xo as described above; 1 = its first half alone, for measuring part by part (-DFW_OBSW_MODE=1:
  // the grid without worker workgroups and the second wave as scenario worker, which then returns; the step wave keeps the whole epilogue)
  constexpr bool OBSG = OBSM != 0, OBSW = OBSM == 2;
  static_assert(!OBSG || (SH::kFixed && AUX), "the observation wave is the noise wave of a fixed shape");
  const int nblk = (Dg.npad + EPW - 1) / EPW;        // step blocks; blocks beyond are shadow workers
  FWP(const long long p_t0 = FWP_NOW(); long long p_reset = 0, p_avi = 0, p_task = 0, p_r1 = 0, p_r2 = 0, p_r3 = 0; int p_nreset = 0, p_nhit = 0;)
  // XCD-aware block -> env-block map (G = 8): a wave touches 64 B of every SoA row, i.e. half a 128-B L2 line, and
  // consecutive workgroups are dealt round-robin to the 8 XCDs, whose L2s are private -- with the identity map both
  // halves of every line are fetched by two different L2s (PMC: 2x the algorithmic read traffic).  Give each XCD a
  // contiguous range of env blocks instead.  (Speed only: nothing depends on where a block really lands.)
  const int bx = (int)blockIdx.x - (COLLECT ? CAp->n_act : 0);       // my index among the step (+ worker) workgroups
  // (a fixed shape: the grid of a kernel without act waves is nblk or 2 * nblk workgroups -- step_T -- so the remainder is a subtraction,
  // not the 30-instruction division emulation both waves ran at entry)
  const int wg = SH::kFixed ? (bx >= nblk ? bx - nblk : bx) : bx % nblk;
  const int blk = (G == 8 && (nblk & 7) == 0) ? (wg & 7) * (nblk >> 3) + (wg >> 3) : wg;
  const DevState<T> D = tile_view<T, EPW>(Dg, blk);  // this wave's tile: row stride EPW (a compile-time constant), global env ids
  if (!OBSG && (GENERAL || DEFER) && bx >= nblk) {    // (OBSG: the grid is the step workgroups alone)
    if (AUX && threadIdx.x >= kWave) return;        // (a worker workgroup's second wave has nothing to do)
    DevState<T> Dw = D;
    if constexpr (SH::kFixed) Dw.epoch = launch_index(Dg.lctr);     // a fixed shape numbers its launches in here (see `lctr_v` below): a worker reads its counter at once
    if (GENERAL) shadow_worker<T, G, TKIND>(Pp, OCp, Dw, blk); else scenario_worker<T, G>(Pp, Dw, blk);
    FWP(if (D.prof && threadIdx.x == 0) {
      long long* w = D.prof + ((size_t)(Dw.epoch % kProfSlots) * 2 * nblk + blockIdx.x) * kProfWords;
      w[0] = FWP_NOW() - p_t0; })
    if constexpr (SH::kFixed) launch_done(Dg.lctr, Dw.epoch);
    return;
  }
  const int lane = AUX ? (int)(threadIdx.x & (kWave - 1)) : (int)threadIdx.x;
  const int sub = (G == 1) ? 0 : (lane & (G - 1));   // my lane within the env's group
  const int row = lane / G;                          // env slot within the wave
  const bool leader = sub == 0;
  const int env0 = blk * EPW;
  const int env = env0 + row;
  const bool active = env < D.n;
  const int envc = active ? env : D.n - 1;           // inactive lanes shadow the last env and never store
  const size_t n = D.npad;
  const int Dobs = FW_SH(obs_dim);
  const int ld = Dobs + 1;

  // AUX, second wave: the normals of my lane's Aviary step -- the very call the step wave of the one-wave kernel makes below (same
  // lane map, same arguments, zeros where that wave draws nothing) -- left in LDS for the step wave; then the barrier, and done.
  T* aux_nz = AUX ? reinterpret_cast<T*>(smem_raw + Dg.mbox_off) : nullptr;     // [kWave][2], behind tile and stash (step_lds_bytes_h)
  // OBSW: the hand-off block behind the normals, kObsHandWords words per env: p, q, v, w (0-12), the five surface actuators (13-17, each
  // from the lane that owns it), the motor (18), and two integers in word 19: the target index of the last compute_state, the mode
  T* obs_hand = OBSW ? aux_nz + 2 * kWave : nullptr;
  if constexpr (AUX) {
    if (threadIdx.x >= kWave) {
      const int32_t a_tick = D.i[IF_TICK * n + envc], a_episode = D.i[IF_EPISODE * n + envc], a_flags = D.i[IF_FLAGS * n + envc];
      T a_z0 = (T)0, a_z1 = (T)0;
      if (FW_SH(has_noise) && FW_SH(step_ratio) <= G && !(a_flags & (FL_TERM | FL_TRUNC)))
        rng_normal2<T>(P, (uint32_t)(P.env_offset + envc), (uint32_t)a_episode, (uint32_t)(a_tick / FW_SH(ticks_per_aviary)) + (uint32_t)sub, a_z0, a_z1);
      aux_nz[2 * lane] = a_z0; aux_nz[2 * lane + 1] = a_z1;
      FWP(const long long o_tb1 = FWP_NOW();)          // arrival at barrier 1 (the stamp behind it, o_t1, includes the wait)
      __syncthreads();                               // barrier 1 (the step wave's is in front of its sub-step loop)
      if constexpr (OBSG) {
        // ---- the scenario worker of this tile: requests of earlier launches only (the step wave writes this launch's `sreq` behind
        // barrier 2), and nothing it writes is read in this launch (the `launch` field of `sdone`, tested by the step wave) ----
        FWP(const long long o_t1 = FWP_NOW();)
        // (the env count through a scalar register of its own: read as a part of the kernel-argument tuple it keeps all eight of that tuple's
        // registers live across the worker, and the allocator, short of scalar registers there, reserves a stack slot that it then never uses)
        int o_n = D.n;
        asm volatile("" : "+s"(o_n));
        const uint32_t o_launch = launch_index(Dg.lctr);     // the workgroup's counter: the step wave advances it at the very end, behind barrier 2
        if (D.shadow_on) {
          DevState<T> Dw = D;
          Dw.epoch = o_launch; Dw.n = o_n;
          scenario_worker<T, G, true>(Pp, Dw, blk);
        }
        FWP(const long long o_t2 = FWP_NOW();)
        if constexpr (!OBSW) {                       // (the measuring build with the first half alone: done; the counter word was read ~25 k cycles before the step wave stores it)
          FWP(if (D.prof && lane == 0) { long long* w = D.prof + ((size_t)(o_launch % kProfSlots) * 2 * nblk + nblk + blockIdx.x) * kProfWords; w[0] = o_t2 - o_t1; w[1] = o_t1 - p_t0; w[6] = o_t2 - p_t0; w[7] = p_t0; })
          return;
        } else {
        // ---- what the observation pass needs and the launch does not change, on the step wave's lane map; unconditional, so that
        // no load waits behind barrier 2 (this wave has the whole sub-step loop to spare) ----
        const int o_gbase = lane & ~(G - 1);
        T o_tmine[3] = {(T)0, (T)0, (T)0};
        if (sub < SH::num_targets) {
#pragma unroll
          for (int k = 0; k < 3; ++k) o_tmine[k] = D.r[(size_t)(RF_TARGETS + 3 * sub + k) * n + envc];
        }
        const T o_keep = actions[(size_t)envc * 4 + (sub & 3)];
        T o_act[4], o_stale[4], o_dow[4] = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
        for (int k = 0; k < 4; ++k) { o_act[k] = __shfl(o_keep, o_gbase | k, kWave); o_stale[k] = D.r[(size_t)(RF_ACTION + k) * n + envc]; }
        if (a_flags & (FL_TERM | FL_TRUNC)) {        // done at entry (bare-Gymnasium view): the stored action
#pragma unroll
          for (int k = 0; k < 4; ++k) o_act[k] = o_stale[k];
        }
        static_assert(!OBSW || SH::obs_dim <= 4 * G, "the env's eight lanes hold the worker's first row in four words each");
        static_assert(!OBSW || SH::att_dim <= 32, "the step wave's fallback row takes its cached attitude block from the env's lanes (kWO * G words): no tile write is left behind barrier 2");
        if (D.shadow_on) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { const int k = sub + j * G; if (k < Dobs) o_dow[j] = Dg.sobs[(size_t)envc * Dobs + k]; }
        }
        FWP(const long long o_t3 = FWP_NOW();)
        __syncthreads();                             // barrier 2 (the step wave's is behind its end-of-step latch)
        FWP(const long long o_t4 = FWP_NOW();)
        const T* hr = obs_hand + row * kObsHandWords;
        Rigid<T> So;
#pragma unroll
        for (int k = 0; k < 3; ++k) { So.p[k] = hr[k]; So.v[k] = hr[7 + k]; So.w[k] = hr[10 + k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) So.q[k] = hr[3 + k];
#pragma unroll
        for (int k = 0; k < FW_NUM_ACTUATORS; ++k) So.act[k] = hr[13 + k];
        const int o_tgt = reinterpret_cast<const int*>(hr + 19)[0], o_mode = reinterpret_cast<const int*>(hr + 19)[1];
        // the pass of the one-wave epilogue, call for call
        T Ro[9];
        int o = write_obs_attitude<T, true, SH>(P, So, o_act, Ro, [&](int k, T v) { if (leader) tile[row * ld + k] = v; });
#pragma unroll SH::kCtxUnroll
        for (int i = 0; i < SH::ctx; ++i) {
          const int t = o_tgt + i;
          T tw[3], d[3], b[3] = {(T)0, (T)0, (T)0};
#pragma unroll
          for (int k = 0; k < 3; ++k) tw[k] = __shfl(o_tmine[k], o_gbase | (t & (G - 1)), kWave);
          if (t < SH::num_targets) {
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = tw[k] - So.p[k];
            mtv(Ro, d, b);
          }
          if (leader) { tile[row * ld + o] = b[0]; tile[row * ld + o + 1] = b[1]; tile[row * ld + o + 2] = b[2]; }
          o += 3;
        }
        if (o_mode != 0) {                           // group-uniform: the row just written is the terminal observation
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          if (terminal_obs) {
            T* trow = terminal_obs + (size_t)env * Dobs;
            for (int k = sub; k < Dobs; k += G) trow[k] = tile[row * ld + k];
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          if (o_mode == 1) {                         // ... and the new episode's row is the one the worker left
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int k = sub + j * G; if (k < Dobs) tile[row * ld + k] = o_dow[j]; }
          }
        }
        FWP(const long long o_t5 = FWP_NOW();)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
        // flush_obs_tile on this wave's lanes, without the rows the step wave stores itself (mode 2)
        flush_obs_tile_fixed<T, SH::obs_dim, EPW>(tile, obs, env0, o_n, lane,
                                                  [&](int r) { return reinterpret_cast<const int*>(obs_hand + r * kObsHandWords + 19)[1]; },
                                                  [](int mode) { return mode != 2; });
        FWP(if (D.prof && lane == 0) {               // this wave's slot: the one a worker workgroup of the two-half grid has
          long long* w = D.prof + ((size_t)(o_launch % kProfSlots) * 2 * nblk + nblk + blockIdx.x) * kProfWords;
          const long long o_t6 = FWP_NOW();
          w[0] = o_t2 - o_t1; w[1] = o_t1 - p_t0; w[2] = o_t3 - o_t2; w[3] = o_t4 - o_t3; w[4] = o_t5 - o_t4; w[5] = o_t6 - o_t5; w[6] = o_t6 - p_t0; w[7] = p_t0;
          w[8] = o_tb1 - p_t0; w[9] = o_t3 - p_t0; })   // arrival at barrier 1 and at barrier 2, from this wave's first stamp
        }
      }
      return;
    }
  }

  // Loads first, in the order their results are needed (vmcnt retires in order): the counters that feed
  // the RNG and the target window, then the rigid state, then the launch-resident constants.
  int32_t step_count = D.i[IF_STEP * n + envc];
  int32_t tick = D.i[IF_TICK * n + envc];
  int32_t episode = D.i[IF_EPISODE * n + envc];
  int32_t flags = D.i[IF_FLAGS * n + envc];
  int32_t num_reached = D.i[IF_NUM_REACHED * n + envc];
  // G = 8, wind-free waypoints: lane j of the group keeps waypoint j (num_targets <= 8) and component j & 3 of the
  // action; the current waypoint, the obs deltas and the obs action are fetched by shuffle -- no dependent loads.
  constexpr bool LANE_T = DEFER && G == 8;
  T tmine[3] = {(T)0, (T)0, (T)0};
  T a_keep = (T)0;
  if (LANE_T) {
    if (sub < FW_SH(num_targets)) {
#pragma unroll
      for (int k = 0; k < 3; ++k) tmine[k] = D.r[(size_t)(RF_TARGETS + 3 * sub + k) * n + envc];
    }
    if (!COLLECT) a_keep = actions[(size_t)envc * 4 + (sub & 3)];
  }
  Rigid<T> S;
  load_rigid<T>(D, envc, S);
  T new_dist = D.r[RF_NEW_DIST * n + envc];
  T ep_return = D.r[RF_EP_RETURN * n + envc];
  // tick constants + this lane's lifting surface (G = 8: resident in VGPRs for the whole launch)
  TickC<T> C; SurfC<T> mine_regs; T wmask;
  // A fixed shape: this lane's row of the handle's step image and the clamp constants of quat_integrate (fwsim_device.hpp: StepImage),
  // instead of 37 loads of mixed width from three places in Params and what was rebuilt behind them.
  if constexpr (SH::kFixed) load_step_image<T>(Pp, C, mine_regs, wmask);
  else load_tick_constants<T, G, DEFER && G == 8 && WPE == 1>(Pp, C, mine_regs, wmask);
  // A fixed shape: the launch counter, by a vector load BEHIND the state and constant loads (they retire in order: nothing waits for it
  // that would not wait anyway) instead of a scalar load in front of the worker / step split, which every scalar wait of the prologue
  // paid for.  This wave first needs the launch index in the epilogue (`launch` below); it is pinned in front of the barrier so that
  // the load is not sunk to its use.  Same word, same arithmetic as launch_index: the numbering is what it was.
  uint32_t lctr_v = 0;
  if constexpr (SH::kFixed) lctr_v = vload(Dg.lctr + blockIdx.x + opaque_zero());
  // (Tried for WPE = 2: this lane's surface constants in LDS, read field by field through a volatile reference -- 54 registers
  // fewer to hold, but the allocator spilled as much elsewhere and the ds_reads sit on the tick's critical path: 40.6 -> 50.9 us
  // at 16 384 envs.  surface_wrench / physics_tick keep the template parameter that made the experiment a four-line change.)
  if (AX && !SH::kFixed && sub >= FW_NUM_SURFACES) mine_regs.hra = (T)0;    // AX: lanes 5-7 evaluate a zero wrench, no mask (surface_wrench_ax; the step image holds the zero already)
  SurfC<T>& mine = mine_regs;

  normalize_quat<T>(S.q);
  T R[9];
  // A fixed shape spells the contraction out.  In fw_step_kernel_g8xo, without the worker branch in front, the plain form came out with the
  // other product of each sum fused (one ulp in v once in a few hundred env-steps, tests/test_obs_wave_gpu.py); the spelled-out form is what
  // the compiler makes of the plain one in the prologues of the other step kernels (read from their assembly, not from their source), and
  // fw_step_kernel_g8xs compiles to the code it had with either, so the twins share the one that does not depend on the compiler's choice.
  if constexpr (OBSG || SH::kFixed) rot_from_unit_quat_fma<T>(S.q, R); else rot_from_unit_quat<T>(S.q, R);
  ObjState<T> O;
  const ObjC<T>& OC = *OCp;
  if (HASOBJ) { obj_load<T, OBJ>(D, envc, O); obj_update_near_mask<T, G>(P, OC, D, envc, O, S); }
  int32_t out_strike = 0;
  // shadow bookkeeping (kernel-boundary hand-off, see shadow_* above)
  unsigned long long sh_req = ~0ull, sh_done = 0ull;
  if ((GENERAL || DEFER) && D.shadow_on) { sh_req = D.sreq[envc]; sh_done = D.sdone[envc]; }
  T wb[3] = {(T)0, (T)0, (T)0}, wa[3] = {(T)0, (T)0, (T)0}, wphase = (T)0;
  if (GENERAL) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { wb[k] = D.r[(RF_WIND + k) * n + envc]; wa[k] = D.r[(RF_WIND + 3 + k) * n + envc]; }
    wphase = D.r[(RF_WIND + 6) * n + envc];
  }
  T gust[2] = {(T)0, (T)1};                          // sin / cos of the gust phase at `tick`
  if (GENERAL) gust_init<T>(P, wphase, tick, gust);
  // fixedwing_base_env.py:325-331
  T rew = (T)-0.1;
  T cmd[FW_NUM_ACTUATORS];
  // COLLECT: the actions of this launch come from the act waves in front of the grid; everything above was loaded while they
  // worked.  Coherent loads from here on: the rows were written (write-through) by a wave of another XCD in this same launch.
  double c_ret = 0.0;                                // COLLECT: my env's discounted-return tracker, fetched while the wave waits anyway
  if (COLLECT) {
    if (active && leader) c_ret = ld_sc1(CAp->S.returns + env);
    collect_wait_actions(*CAp, Dg.epoch, env0, min(EPW, Dg.n - env0));
  }
  {
    const T* ap = actions + (size_t)envc * 4;
    T a4[4];
    if (COLLECT) collect_load_actions<T>(*CAp, ap, a4);
    else {
#pragma unroll
      for (int k = 0; k < 4; ++k) a4[k] = ap[k];
    }
    if (COLLECT && LANE_T) a_keep = (sub & 3) == 0 ? a4[0] : (sub & 3) == 1 ? a4[1] : (sub & 3) == 2 ? a4[2] : a4[3];
    const T sp[4] = { a4[0], a4[1], a4[2], a4[3] * (T)0.5 + (T)0.5 };
#pragma unroll
    for (int c = 0; c < FW_NUM_ACTUATORS; ++c)
      cmd[c] = P.mixer[c][0] * sp[0] + P.mixer[c][1] * sp[1] + P.mixer[c][2] * sp[2] + P.mixer[c][3] * sp[3];
  }
  // G = 8: my surface's actuator state and command stay lane-local during the ticks (see LaneAct)
  LaneAct<T> LA; LA.a = (T)0; LA.cmd = (T)0;
  T cmd_mine = (T)0;
  if (G == 8) { lane_act_scatter<T>(S, LA); cmd_mine = lane_pick5<T>(cmd[0], cmd[1], cmd[2], cmd[3], cmd[4]); LA.cmd = cmd_mine; }

  // current and next waypoint stay in registers (no L2 round trip per sub-step)
  T tcur[3] = {(T)0, (T)0, (T)0}, tnext[3] = {(T)0, (T)0, (T)0};
  const int gbase = lane & ~(G - 1);                  // first lane of my group
  if (LANE_T) {
#pragma unroll
    for (int k = 0; k < 3; ++k) tcur[k] = __shfl(tmine[k], gbase | (num_reached & (G - 1)), kWave);
  } else if (!OBJ) {
    const int i0 = min(num_reached, FW_MAX_TARGETS - 1), i1 = min(num_reached + 1, FW_MAX_TARGETS - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      tcur[k] = D.r[(size_t)(RF_TARGETS + 3 * i0 + k) * n + envc];
      tnext[k] = D.r[(size_t)(RF_TARGETS + 3 * i1 + k) * n + envc];
    }
  }

  const uint32_t genv = (uint32_t)(P.env_offset + envc);
  // An env that is already done (bare-Gymnasium mode) runs no sub-step: the reference then
  // returns its stale self.state, i.e. the previous action and target view.
  const bool done_at_entry = (flags & (FL_TERM | FL_TRUNC)) != 0;
  int tgt_obs = (flags >> FL_TGT_SHIFT) & 15;        // target index the last compute_state() saw
  flags &= FL_MASK;
  // which action the returned observation shows: 0 = this step's, 1 = the stored (stale) one,
  // 2 = zeros (fresh reset).  Re-read at the end instead of held in registers across the loop.
  int act_src = done_at_entry ? 1 : 0;

  // Motor noise.  G = 8: lane j of the group draws the normals of the step's j-th Aviary
  // step up front (8 lanes -> up to 8 sub-steps, in parallel); they are fetched by shuffle.
  const uint32_t astep0 = (uint32_t)(tick / FW_SH(ticks_per_aviary));
  const bool pre_noise = (G == 8) && FW_SH(has_noise) && (FW_SH(step_ratio) <= G);
  T nz0 = (T)0, nz1 = (T)0;
  if (!AUX && pre_noise && !done_at_entry) rng_normal2<T>(P, genv, (uint32_t)episode, astep0 + (uint32_t)sub, nz0, nz1);

  int phase = active ? PH_STEP : PH_DONE;
  // STASH: the outputs of the step (reward, flags, info) wait in LDS -- four words per env behind the tile / the camera's map --
  // from the latch point to the END of the epilogue.  Stored at the latch point (round 2: to keep them out of registers) they
  // sat in front of the epilogue's loads (stored action, waypoints of the observation): vector memory operations retire in order
  // on gfx9, so those loads paid the stores' acknowledgement, ~2 k cycles in every wave.  The wind-free headline kernel has no such
  // loads (actions and waypoints ride in registers) and keeps storing at the latch point.
  // (The camera kernels would gain the same way -- but with the stash their plain builds trip the compiler hazard of section 4
  // of DESIGN.md at the mask-row join, and the hazard-free form of that join costs 3-4 us; they keep the latch-point stores.)
  constexpr bool STASH = (!DEFER && !HASOBJ) || COLLECT;
  double* latch = STASH ? reinterpret_cast<double*>(smem_raw + Dg.stash_off) : nullptr;        // [EPW][4]: reward, done, (num_reached, flags), (strike, step_count)
  int it = 0, warm_left = 0;
  // HELP: the request of the previous sub-step that is still with the capture wave (0 = none), and what this lane owes it:
  // bit 0 the frame-dependent half of that sub-step's task logic, bit 1 a frame, bit 2 "no collision / not out of bounds then",
  // bit 3 (combined) "all waypoints were reached then"; the distance to the duck of that sub-step (ObjLock's reward reads it)
  const Mbox<T> MB = mbox_at<T>(HELP ? Dg.mbox_off : 0);
  uint32_t n_posted = 0, pend_seq = 0;
  int pend = 0;
  T dist_keep = (T)0;
  bool resetting = false;                            // DEFER: auto-reset pending for the epilogue
  bool step_over = active && done_at_entry;          // nothing to simulate: finalise immediately
  // A fixed shape: what the task logic of a sub-step still reads from Params, fetched here once.  The scalar file is full in this
  // kernel and the allocator would rather load a Params field again (a round trip with its own wait, in every sub-step) than keep
  // it; a value that went through an empty asm cannot be re-derived from memory, so it is kept (or parked in a lane).
  int32_t k_max_steps = 0, k_auto_reset = 0; T k_dome = (T)0, k_reach = (T)0;
  if constexpr (SH::kFixed) {
    k_max_steps = P.max_steps; k_auto_reset = P.auto_reset; k_dome = P.dome; k_reach = P.reach;
    asm("" : "+s"(k_max_steps)); asm("" : "+s"(k_auto_reset)); asm("" : "+s"(k_dome)); asm("" : "+s"(k_reach));
  }
  if constexpr (SH::kFixed) asm volatile("" : "+v"(lctr_v));       // the counter load stays in the prologue (see above)
  FWP(const long long p_b1 = FWP_NOW(); long long p_b2 = 0;)      // arrival at barrier 1, at barrier 2 (OBSW)
  if constexpr (AUX) {                               // barrier 1: every lane of both waves, whatever its env does
    __syncthreads();
    nz0 = aux_nz[2 * lane]; nz1 = aux_nz[2 * lane + 1];
  }

  FWP(const long long p_t1 = FWP_NOW();)
  if constexpr (SH::kFixed) {
    // A fixed shape: the agent step is a counted loop.  This kernel has no in-loop reset, no warm-up phase and no camera, and its
    // step_ratio is a constant, so the phase machine below reduces to one per-lane bit: `stepping`, cleared where that machine sets
    // step_over.  Noise shuffle, Aviary step and task logic of a sub-step are those of the general loop, in its order.  The
    // end-of-step latch -- which that loop tests for at the head of every iteration -- runs once, behind the loop, for every active
    // lane: a lane that has finished reads nothing of what the latch writes (step_count is compared with max_steps by stepping
    // lanes only, and they have not latched).  A wave whose envs are all done -- at entry or early -- leaves at the ballot.
    // The loop stays rolled: unrolled twice it measured the same, unrolled four times slower (CHANGELOG).
    bool stepping = active && !done_at_entry;
#pragma unroll 1
    for (it = 0; it < SH::step_ratio; ++it) {
      FWP(const long long p_b = FWP_NOW();)
      if (__ballot(stepping) == 0ull) break;         // wave-uniform exit
      // noise of this iteration's Aviary step (all stepping envs of the wave are at sub-step `it`)
      const int src = (lane & ~(G - 1)) | (it & (G - 1));
      const T z0 = __shfl(nz0, src, kWave), z1 = __shfl(nz1, src, kWave);
      bool contact = false;
      if (stepping) contact = aviary_step<T, false, G, false, AX, SH>(P, C, OC, D, env, O, S, R, cmd, tick, z0, z1, wb, wa, gust, mine, wmask, LA);    // :339
      FWP(const long long p_c = FWP_NOW(); p_avi += p_c - p_b;)
      if (stepping) {
        // compute_state(): WaypointHandler.distance_to_targets side effects
        const int nleft = SH::num_targets - num_reached;
        const T old_dist = new_dist;
        if (nleft > 0) {
          T dx = tcur[0] - S.p[0], dy = tcur[1] - S.p[1], dz = tcur[2] - S.p[2];
          new_dist = M<T>::sqrt_(sum_squares_fma(dx, dy, dz));
        }
        tgt_obs = num_reached;
        // compute_base_term_trunc_reward(): :296-312
        if (step_count > k_max_steps) flags |= FL_TRUNC;
        if (contact) { rew = (T)-100; flags |= FL_COLLISION | FL_TERM; }
        if (sum_squares_fma(S.p[0], S.p[1], S.p[2]) > k_dome * k_dome) { rew = (T)-100; flags |= FL_OOB | FL_TERM; }
        // waypoint reward (upstream FixedwingWaypointsEnv)
        if (nleft > 0) {
          if (!SH::sparse) {
            T progress = (old_dist != (T)0) ? (old_dist - new_dist) : (T)0;
            rew += M<T>::fmax_((T)3 * progress, (T)0);
            rew += M<T>::rcp_(new_dist);
          }
          if (new_dist < k_reach) {
            rew = (T)100;
            num_reached += 1;
            if (num_reached == SH::num_targets) flags |= FL_TRUNC | FL_COMPLETE;
#pragma unroll
            for (int k = 0; k < 3; ++k) tcur[k] = __shfl(tmine[k], gbase | (num_reached & (G - 1)), kWave);   // advance_targets(): the next waypoint's lane hands it over
          }
        }
        if (flags & (FL_TERM | FL_TRUNC)) stepping = false;     // :334-337 (the last sub-step ends with the loop)
        FWP(p_task += FWP_NOW() - p_c;)
      }
    }
    // ---- end of env.step(): :346, outputs, SB3 worker auto-reset ---- once, for every env of the wave: in front of the epilogue's
    // loads as the latch always was, with the outputs leaving for memory here (see STASH)
    FWP(const long long p_a = FWP_NOW();)
    if (active) {
      step_count += 1;
      ep_return += rew;
      if (leader) {
        reward[env] = rew;
        terminated[env] = (uint8_t)((flags & FL_TERM) ? 1 : 0);
        truncated[env] = (uint8_t)((flags & FL_TRUNC) ? 1 : 0);
        if (info) {
          int4* ip = reinterpret_cast<int4*>(info + (size_t)env * FW_INFO_DIM);
          ip[0] = make_int4(num_reached, (flags & FL_COLLISION) ? 1 : 0, (flags & FL_OOB) ? 1 : 0, (flags & FL_COMPLETE) ? 1 : 0);
          ip[1] = make_int4(out_strike, 0, step_count, 0);
        }
      }
      resetting = (flags & (FL_TERM | FL_TRUNC)) && k_auto_reset;
      FWP(if (resetting) p_nreset += 1;)
    }
    FWP(p_reset += FWP_NOW() - p_a;)
  } else {
#pragma unroll 1
  for (;;) {
    FWP(const long long p_a = FWP_NOW();)
    if (phase == PH_STEP && step_over) {
      // ---- end of env.step(): :346, outputs, SB3 worker auto-reset ----
      step_count += 1;
      ep_return += rew;
      phase = PH_DONE;
      if (STASH && leader) {
        latch[4 * row] = (double)rew; latch[4 * row + 1] = (flags & (FL_TERM | FL_TRUNC)) ? 1.0 : 0.0;
        latch[4 * row + 2] = __hiloint2double(num_reached, flags); latch[4 * row + 3] = __hiloint2double(out_strike, step_count);
      }
      // DEFER: the outputs of the step leave for memory here (nothing is kept live across the rest of the loop for them)
      if (!(STASH && !DEFER) && leader) {     // (COLLECT && DEFER stashes for the statistics tail and stores here as well)
        reward[env] = rew;
        terminated[env] = (uint8_t)((flags & FL_TERM) ? 1 : 0);
        truncated[env] = (uint8_t)((flags & FL_TRUNC) ? 1 : 0);
        if (info) {
          int4* ip = reinterpret_cast<int4*>(info + (size_t)env * FW_INFO_DIM);
          ip[0] = make_int4(num_reached, (flags & FL_COLLISION) ? 1 : 0, (flags & FL_OOB) ? 1 : 0, (flags & FL_COMPLETE) ? 1 : 0);
          ip[1] = make_int4(out_strike, OBJ ? out_strike : 0, step_count, 0);
        }
      }
      if (DEFER) { resetting = (flags & (FL_TERM | FL_TRUNC)) && (SH::kFixed ? k_auto_reset : P.auto_reset); FWP(if (resetting) p_nreset += 1;) }
      // GENERAL: a reset whose pre-simulated episode is ready is a copy, done in the epilogue (the observation pass there writes
      // the terminal observation); only a reset without one runs here, with its warm-up in the loop
      const bool take_shadow = GENERAL && (flags & (FL_TERM | FL_TRUNC)) && P.auto_reset && D.shadow_on &&
                               (int)(sh_done & 0xFF) == P.warmup_aviary_steps + 1 && (uint32_t)(sh_done >> 32) == (uint32_t)(episode + 1) &&
                               (uint32_t)((sh_done >> 8) & 0xFFFFFFu) != (D.epoch & 0xFFFFFFu);
      if (take_shadow) { resetting = true; FWP(p_nreset += 1; p_nhit += 1;) }
      if (!DEFER && !take_shadow && (flags & (FL_TERM | FL_TRUNC)) && P.auto_reset) {
        if (G == 8) lane_act_gather<T>(S, LA);          // the terminal observation shows all six actuators
        if (terminal_obs && leader) {
          T* trow = terminal_obs + (size_t)env * Dobs;
          T act_t[4];
          load_action<T, COLLECT>(D, actions, env, act_src, act_t);
          if (OBJ) obj_write_obs<T>(P, O, S, act_t, [&](int k, T v) { trow[k] = v; });
          else if (COMB) comb_write_obs<T>(P, D, env, O, S, act_t, tgt_obs, [&](int k, T v) { trow[k] = v; });
          else write_obs<T>(P, D, env, S, act_t, tgt_obs, [&](int k, T v) { trow[k] = v; });
        }
        T t_mine[3] = {(T)0, (T)0, (T)0};            // first waypoint of the new episode
        FWP(const long long p_ra = FWP_NOW(); p_r1 += p_ra - p_a;)
        {
          if (leader) stat_add(D.stats, FW_CTR_FALLBACKS);
          warm_left = begin_reset<T, G>(P, D, env, S, tick, episode, num_reached, wb, wa, wphase, t_mine);
          if (G > 1) {                                          // the group's lane 0 sampled waypoint 0
            const int src = lane & ~(G - 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) t_mine[k] = __shfl(t_mine[k], src, kWave);
          }
          if (HASOBJ) {
            obj_reset_state<T, OBJ>(O);
            if (OBJ) obj_spawn<T, G>(P, OC, D, env, (uint32_t)episode, leader, O);
            else comb_spawn<T, G>(P, OC, D, env, (uint32_t)episode, leader, O);
          }
        }
        if (G > 1 && warm_left > 0) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the warm-up's camera reads the obstacles
        if (HASOBJ) obj_update_near_mask<T, G>(P, OC, D, env, O, S);                          // new position, new cylinders
        if (GENERAL) gust_init<T>(P, wphase, tick, gust);                                  // new clock, new phase
        if (G == 8) lane_act_scatter<T>(S, LA);                                             // new episode's actuator state
        FWP(const long long p_rb = FWP_NOW(); p_r2 += p_rb - p_ra;)
        step_count = 0; flags = 0; ep_return = (T)0; tgt_obs = 0;
        act_src = 2;
        if (leader) stat_add(D.stats, FW_CTR_RESETS);
        FWP(p_nreset += 1;)
        rot_from_unit_quat<T>(S.q, R);
        if (GENERAL && warm_left > 0) phase = PH_WARM;
        else if (OBJ) obj_compute_state<T>(O);                 // end_reset(): first compute_state of the episode
        else {
          new_dist = end_reset<T, G>(P, D, env, episode, S, t_mine);
          if (COMB) comb_compute_state<T>(OC, O, P.num_targets == 0);
        }
        FWP(p_r3 += FWP_NOW() - p_rb;)
      }
    }
    FWP(const long long p_b = FWP_NOW(); p_reset += p_b - p_a;)
    if (__ballot(phase != PH_DONE) == 0ull) break;   // wave-uniform exit
    // noise of this iteration's Aviary step (all stepping envs of the wave are at sub-step `it`)
    T z0 = (T)0, z1 = (T)0;
    if (pre_noise) {
      const int src = (lane & ~(G - 1)) | (it & (G - 1));
      z0 = __shfl(nz0, src, kWave); z1 = __shfl(nz1, src, kWave);
    }
    const bool stepped = phase != PH_DONE;
    const bool stepping = stepped && (!GENERAL || phase == PH_STEP);
    bool contact = false;
    if (stepped) {
      if (FW_SH(has_noise) && !pre_noise && stepping)
        rng_normal2<T>(P, genv, (uint32_t)episode, (uint32_t)(tick / FW_SH(ticks_per_aviary)), z0, z1);
      if (GENERAL) {
        T c_eff[FW_NUM_ACTUATORS];
#pragma unroll
        for (int c = 0; c < FW_NUM_ACTUATORS; ++c) c_eff[c] = stepping ? cmd[c] : (T)0;
        z0 = stepping ? z0 : (T)0; z1 = stepping ? z1 : (T)0;
        LA.cmd = stepping ? cmd_mine : (T)0;
        contact = aviary_step<T, true, G, HASOBJ, AX, SH>(P, C, OC, D, env, O, S, R, c_eff, tick, z0, z1, wb, wa, gust, mine, wmask, LA);   // :339
      } else {
        contact = aviary_step<T, false, G, HASOBJ, AX, SH>(P, C, OC, D, env, O, S, R, cmd, tick, z0, z1, wb, wa, gust, mine, wmask, LA);    // :339
      }
    }
    if constexpr (HELP) {
      // ---- the camera on the capture wave, one sub-step behind the physics ----
      const bool due = stepped && OC.camera_ratio_ticks > 0 && (tick % OC.camera_ratio_ticks) == 0;
      FWP(const long long p_c0 = FWP_NOW(); p_avi += p_c0 - p_b;)
      const uint32_t seq_cur = cap_post<T>(MB, n_posted, due, row, leader, O, S, R);
      FWP(p_r1 += FWP_NOW() - p_c0;)
      // the frame-independent half of THIS sub-step's task logic first: it reads the state as the physics left it; rew / flags
      // of the previous sub-step's other half are complete only below, and the order of their updates is the reference's:
      // (previous: frame half) comes before (this: -100 assignments), see the two halves
      FWP(const long long p_w0 = FWP_NOW();)
      cap_collect<T>(MB, pend_seq, (pend & 2) != 0, row, O, D.stats);
      FWP(p_task += FWP_NOW() - p_w0;)
      pend_seq = 0;
      auto frame_half = [&](int keep) {             // compute_state + the rewards that read the frame (fixedwing_objlock_env.py:253-287, 296-372)
        if (OBJ) {
          obj_compute_state<T>(O);
          if ((keep & 4) && obj_reward<T>(OC, P.sparse, O, dist_keep, rew)) { flags |= FL_TERM | FL_COMPLETE; out_strike = 1; }
        } else {
          comb_compute_state<T>(OC, O, (keep & 8) != 0);
          if (keep & 4) {
            if (!(keep & 8)) comb_obstacle_penalty<T>(OC, O, (T)1, rew);
            else {
              comb_obstacle_penalty<T>(OC, O, (T)0.5, rew);
              if (comb_duck_reward<T>(OC, P.sparse, O, rew)) { flags |= FL_TERM | FL_COMPLETE; out_strike = 1; }
            }
          }
        }
      };
      FWP(const long long p_f0 = FWP_NOW();)
      if (pend & 1) frame_half(pend);
      FWP(const long long p_f1 = FWP_NOW(); p_r2 += p_f1 - p_f0;)
      pend = 0;
      int keep = 0;
      bool now = false;                             // this lane needs its frame before the next sub-step's physics
      if (stepped) {
        if (stepping) {
          keep = 1 | (due ? 2 : 0);
          int nleft = 0;
          T old_dist = new_dist;
          if (COMB) {
            nleft = P.num_targets - num_reached;
            if (nleft > 0) {
              T dx = tcur[0] - S.p[0], dy = tcur[1] - S.p[1], dz = tcur[2] - S.p[2];
              new_dist = M<T>::sqrt_(dx * dx + dy * dy + dz * dz);
            }
            tgt_obs = num_reached;
            if (nleft == 0) keep |= 8;
          }
          if (step_count > P.max_steps) flags |= FL_TRUNC;
          if (contact) { rew = (T)-100; flags |= FL_COLLISION | FL_TERM; }
          if (S.p[0] * S.p[0] + S.p[1] * S.p[1] + S.p[2] * S.p[2] > P.dome * P.dome) { rew = (T)-100; flags |= FL_OOB | FL_TERM; }
          bool can_strike = false;
          if (!(flags & (FL_COLLISION | FL_OOB))) {
            keep |= 4;
            if (OBJ) {
              T dx = O.duck[0] - S.p[0], dy = O.duck[1] - S.p[1], dz = O.duck[2] - S.p[2];
              dist_keep = M<T>::sqrt_(dx * dx + dy * dy + dz * dz);
              // obj_reward: a strike needs lock_steps >= hold_steps AFTER this sub-step's (at most +1) update, and the distance
              can_strike = O.lock_steps + (T)1 >= (T)OC.hold_steps && dist_keep <= OC.strike_dist;
            } else if (nleft > 0) {
              if (!P.sparse) {
                T progress = (old_dist != (T)0) ? (old_dist - new_dist) : (T)0;
                rew += M<T>::fmax_((T)3 * progress, (T)0);
                rew += M<T>::rcp_(new_dist);
              }
              if (new_dist < P.reach) {
                rew = (T)100;
                num_reached += 1;
                if (num_reached == P.num_targets) flags &= ~(FL_TERM | FL_TRUNC);          // :297-300
                const int i1 = min(num_reached + 1, FW_MAX_TARGETS - 1);
#pragma unroll
                for (int k = 0; k < 3; ++k) { tcur[k] = tnext[k]; tnext[k] = D.r[(size_t)(RF_TARGETS + 3 * i1 + k) * n + env]; }
              }
            } else {
              flags &= ~FL_TERM;                                                            // :306
              // comb_duck_reward: a strike needs the duck phase (which this sub-step's frame may switch on) and the lock counter
              can_strike = O.lock_steps + (T)1 >= (T)OC.hold_steps;
            }
          }
          step_over = (it + 1 >= P.step_ratio) || (flags & (FL_TERM | FL_TRUNC));
          now = can_strike || step_over;
        } else {
          now = true;                               // warm-up of an in-kernel reset: its last sub-step reads the frame
        }
      }
      auto finish_now = [&]() {                     // the rest of this sub-step for a lane whose frame (if it is due one) is in O
        if (stepping) {
          frame_half(keep);
          step_over = (it + 1 >= P.step_ratio) || (flags & (FL_TERM | FL_TRUNC));
        } else {
          warm_left -= 1;
          if (warm_left == 0) {
            if (OBJ) obj_compute_state<T>(O);
            else { new_dist = end_reset<T, G>(P, D, env, episode, S); comb_compute_state<T>(OC, O, P.num_targets == 0); }
            phase = PH_DONE;
          }
        }
      };
      // Wait here if somebody's agent step ends at this sub-step (or could, by a strike) -- ObjLock: ... AND that lane reads a
      // frame of this very sub-step; a lane that ends on the frame it already has finishes at once and the others' frames come
      // back behind the next sub-step's physics.  (The combined kernel keeps the simpler rule: with the finer one its build
      // trips the spill-before-exec-restore check of tools/check_isa.py.)
      FWP(const long long p_f2 = FWP_NOW(); p_r3 += p_f2 - p_f1;)
      bool wait_here;
      if constexpr (OBJ) wait_here = __ballot(now && due) != 0ull; else wait_here = __ballot(now) != 0ull;
      if (wait_here) {
        FWP(const long long p_w1 = FWP_NOW();)
        cap_collect<T>(MB, seq_cur, due, row, O, D.stats);
        FWP(p_task += FWP_NOW() - p_w1; p_nhit += 1;)
        FWP(const long long p_f3 = FWP_NOW();)
        if (stepped) finish_now();               // ... and the sub-step is finished for everybody, as in the one-wave kernel
        FWP(p_r2 += FWP_NOW() - p_f3;)
      } else {
        FWP(const long long p_f3 = FWP_NOW();)
        if constexpr (OBJ) { if (now) finish_now(); else pend = keep; }
        else pend = keep;
        FWP(p_r2 += FWP_NOW() - p_f3;)
        pend_seq = seq_cur;
      }
    } else {
    if (HASOBJ) obj_capture_step<T, G, COLLECT>(OC, D, stepped, envc, O, S, R, tick);     // the camera, by the whole wave
    FWP(const long long p_c = FWP_NOW(); p_avi += p_c - p_b;)
    if (stepped) {
      if (stepping && OBJ) {
        obj_compute_state<T>(O);                                                                   // :342
        // compute_base_term_trunc_reward(): :296-312
        if (step_count > P.max_steps) flags |= FL_TRUNC;
        if (contact) { rew = (T)-100; flags |= FL_COLLISION | FL_TERM; }
        if (S.p[0] * S.p[0] + S.p[1] * S.p[1] + S.p[2] * S.p[2] > P.dome * P.dome) { rew = (T)-100; flags |= FL_OOB | FL_TERM; }
        if (!(flags & (FL_COLLISION | FL_OOB))) {                                                  // :293-294
          T dx = O.duck[0] - S.p[0], dy = O.duck[1] - S.p[1], dz = O.duck[2] - S.p[2];
          if (obj_reward<T>(OC, P.sparse, O, M<T>::sqrt_(dx * dx + dy * dy + dz * dz), rew)) {
            flags |= FL_TERM | FL_COMPLETE; out_strike = 1;
          }
        }
        step_over = (it + 1 >= P.step_ratio) || (flags & (FL_TERM | FL_TRUNC));
      } else if (stepping && COMB) {
        // compute_state() :197-276
        const int nleft = P.num_targets - num_reached;
        const T old_dist = new_dist;
        if (nleft > 0) {
          T dx = tcur[0] - S.p[0], dy = tcur[1] - S.p[1], dz = tcur[2] - S.p[2];
          new_dist = M<T>::sqrt_(dx * dx + dy * dy + dz * dz);
        }
        tgt_obs = num_reached;
        comb_compute_state<T>(OC, O, nleft == 0);
        // compute_term_trunc_reward() :278-343
        if (step_count > P.max_steps) flags |= FL_TRUNC;
        if (contact) { rew = (T)-100; flags |= FL_COLLISION | FL_TERM; }
        if (S.p[0] * S.p[0] + S.p[1] * S.p[1] + S.p[2] * S.p[2] > P.dome * P.dome) { rew = (T)-100; flags |= FL_OOB | FL_TERM; }
        if (!(flags & (FL_COLLISION | FL_OOB))) {
          if (nleft > 0) {
            if (!P.sparse) {
              T progress = (old_dist != (T)0) ? (old_dist - new_dist) : (T)0;
              rew += M<T>::fmax_((T)3 * progress, (T)0);
              rew += M<T>::rcp_(new_dist);
            }
            if (new_dist < P.reach) {
              rew = (T)100;
              num_reached += 1;
              if (num_reached == P.num_targets) flags &= ~(FL_TERM | FL_TRUNC);          // :297-300
              const int i1 = min(num_reached + 1, FW_MAX_TARGETS - 1);
#pragma unroll
              for (int k = 0; k < 3; ++k) { tcur[k] = tnext[k]; tnext[k] = D.r[(size_t)(RF_TARGETS + 3 * i1 + k) * n + env]; }
            }
            comb_obstacle_penalty<T>(OC, O, (T)1, rew);
          } else {
            flags &= ~FL_TERM;                                                            // :306
            comb_obstacle_penalty<T>(OC, O, (T)0.5, rew);
            if (comb_duck_reward<T>(OC, P.sparse, O, rew)) { flags |= FL_TERM | FL_COMPLETE; out_strike = 1; }
          }
        }
        step_over = (it + 1 >= P.step_ratio) || (flags & (FL_TERM | FL_TRUNC));
      } else if (stepping) {
        // compute_state(): WaypointHandler.distance_to_targets side effects
        const int nleft = FW_SH(num_targets) - num_reached;
        const T old_dist = new_dist;
        if (FW_SH(task) != FW_TASK_OBJLOCK && nleft > 0) {
          T dx = tcur[0] - S.p[0], dy = tcur[1] - S.p[1], dz = tcur[2] - S.p[2];
          if constexpr (SH::kFixed) new_dist = M<T>::sqrt_(sum_squares_fma(dx, dy, dz));
          else new_dist = M<T>::sqrt_(dx * dx + dy * dy + dz * dz);
        }
        tgt_obs = num_reached;
        // compute_base_term_trunc_reward(): :296-312
        if (step_count > (SH::kFixed ? k_max_steps : P.max_steps)) flags |= FL_TRUNC;
        if (contact) { rew = (T)-100; flags |= FL_COLLISION | FL_TERM; }
        bool oob;
        if constexpr (SH::kFixed) oob = sum_squares_fma(S.p[0], S.p[1], S.p[2]) > k_dome * k_dome;
        else oob = S.p[0] * S.p[0] + S.p[1] * S.p[1] + S.p[2] * S.p[2] > P.dome * P.dome;
        if (oob) { rew = (T)-100; flags |= FL_OOB | FL_TERM; }
        // waypoint reward (upstream FixedwingWaypointsEnv; mirrored at fixedwing_waypoint_objlock_env.py:286-294)
        if (FW_SH(task) != FW_TASK_OBJLOCK && nleft > 0) {
          if (!FW_SH(sparse)) {
            T progress = (old_dist != (T)0) ? (old_dist - new_dist) : (T)0;
            rew += M<T>::fmax_((T)3 * progress, (T)0);
            rew += M<T>::rcp_(new_dist);
          }
          if (new_dist < (SH::kFixed ? k_reach : P.reach)) {
            rew = (T)100;
            num_reached += 1;
            if (num_reached == FW_SH(num_targets)) flags |= FL_TRUNC | FL_COMPLETE;
            if (LANE_T) {                                                   // advance_targets(): the next waypoint's lane hands it over
#pragma unroll
              for (int k = 0; k < 3; ++k) tcur[k] = __shfl(tmine[k], gbase | (num_reached & (G - 1)), kWave);
            } else {
              const int i1 = min(num_reached + 1, FW_MAX_TARGETS - 1);     // advance_targets(): shift the register window
#pragma unroll
              for (int k = 0; k < 3; ++k) { tcur[k] = tnext[k]; tnext[k] = D.r[(size_t)(RF_TARGETS + 3 * i1 + k) * n + env]; }
            }
          }
        }
        step_over = (it + 1 >= FW_SH(step_ratio)) || (flags & (FL_TERM | FL_TRUNC));     // :334-337
      } else {
        warm_left -= 1;
        if (warm_left == 0) {
          if (OBJ) obj_compute_state<T>(O);
          else { new_dist = end_reset<T, G>(P, D, env, episode, S); if (COMB) comb_compute_state<T>(OC, O, P.num_targets == 0); }
          phase = PH_DONE;
        }
      }
      FWP(p_task += FWP_NOW() - p_c;)
    }
    }
    it += 1;
  }
  }
  FWP(const long long p_t2 = FWP_NOW();)
  // G = 8: waypoints sampled by sibling lanes during an in-launch reset are read back below
  if (G > 1 && !DEFER) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  if (G == 8 && !OBSW) lane_act_gather<T>(S, LA);    // S.act[0..4] current again for the observation and the state store (OBSW: through the hand-off block below)
  // DEFER: the waypoint a worker block sampled ahead of time for my next episode, requested only by resetting envs and only
  // now -- its latency hides behind the observation pass below
  T tpre[3] = {(T)0, (T)0, (T)0};
  // The launch index: D.epoch as the kernel set it at entry, or (a fixed shape) from the counter word fetched in the prologue: every lane
  // loaded the same word, so any lane's copy serves.  The step wave gets here with all its lanes and on every path: it has no early return,
  // and must not get one -- launch_done at the end of this function is what advances the workgroup's counter.
  const uint32_t launch = SH::kFixed ? 1u + (uint32_t)__builtin_amdgcn_readfirstlane((int)lctr_v) : D.epoch;
  const bool pre = DEFER && resetting && D.shadow_on && (int)(sh_done & 0xFF) == 1 && (uint32_t)(sh_done >> 32) == (uint32_t)(episode + 1) &&
                   (uint32_t)((sh_done >> 8) & 0xFFFFFFu) != (launch & 0xFFFFFFu);
  if constexpr (OBSW) {
    // What the observation pass reads, for the second wave; then barrier 2 -- every lane of both waves, whatever its env does.  From
    // here on the tile, the terminal observation and the `obs` rows of modes 0 and 1 belong to that wave.
    T* hr = obs_hand + row * kObsHandWords;
    if (leader) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { hr[k] = S.p[k]; hr[7 + k] = S.v[k]; hr[10 + k] = S.w[k]; }
#pragma unroll
      for (int k = 0; k < 4; ++k) hr[3 + k] = S.q[k];
      hr[13 + FW_NUM_SURFACES] = S.act[FW_NUM_SURFACES];
      reinterpret_cast<int*>(hr + 19)[0] = tgt_obs;
      reinterpret_cast<int*>(hr + 19)[1] = resetting ? (pre ? 1 : 2) : 0;
    }
    if (sub < FW_NUM_SURFACES) hr[13 + sub] = LA.a;
    FWP(p_r1 = p_b2 = FWP_NOW();)
    __syncthreads();
    FWP(p_r1 = FWP_NOW() - p_r1;)                    // the wait at barrier 2
#pragma unroll
    for (int k = 0; k < FW_NUM_SURFACES; ++k) S.act[k] = hr[13 + k];       // lane_act_gather, for the state store
  }
  if (pre) {      // (every lane issues: rows >= num_targets of the shadow are zero and are not stored back)
#pragma unroll
    for (int k = 0; k < 3; ++k) pf_issue(tpre[k], &D.rs[(size_t)(RF_TARGETS + 3 * sub + k) * n + env]);
  }
  // ... and so is the cached attitude block of the observation a reset returns (lane `sub` holds its words sub, sub + G, ...)
  constexpr bool WO = DEFER && G == 8;               // (one lane per env: the block is copied straight from memory below)
  constexpr int kWO = WO ? 32 / G : 1;
  T wo[kWO];
  if (WO && resetting && !(OBSW && pre)) {           // (OBSW: the step wave builds the new row on the fallback path alone)
#pragma unroll
    for (int j = 0; j < kWO; ++j) { const int k = sub + j * G; wo[j] = (k < FW_SH(att_dim)) ? vload(&Pp->warm_obs[k]) : (T)0; }
  }

  // (pre: the worker also left the first observation row and the first distance: requested here as well)
  constexpr int kDOW = 4;                            // words per lane of the first observation row (obs_dim <= 32: every waypoints config up to ctx 3)
  T dow[kDOW], dnd = (T)0;
  if (WO && pre && Dobs <= kDOW * G) {
#pragma unroll
    for (int j = 0; j < kDOW; ++j) { const int k = sub + j * G; dow[j] = (T)0; if (!OBSW && k < Dobs) pf_issue(dow[j], &Dg.sobs[(size_t)env * Dobs + k]); }     // (OBSW: the second wave has the row)
    pf_issue(dnd, &D.rs[(size_t)RF_NEW_DIST * n + env]);
  }

  // GENERAL: the rows of a shadow that is being taken, fetched by the env's G lanes before the observation pass (their round
  // trip hides behind it): word w of the [RF_COUNT] state column goes to lane w % G; the first observation likewise
  constexpr int kRows = HASOBJ ? RF_COUNT : RF_TASK;  // the waypoint task has no task tail
  constexpr int kCW = GENERAL ? (kRows + G - 1) / G : 1, kOW = GENERAL ? (kMaxObs + G - 1) / G : 1;
  constexpr bool SWAP_REGS = GENERAL && G == 8;       // G = 1: one lane would hold all 171 words; it copies through memory below
  T cw[kCW], ow[kOW];
  int32_t tick_new = 0;
  // PF_GEN: the same hand-issued form for the shadow take-over of the wind / camera kernels.  Measured on the wind kernel: 23.35 ->
  // 23.49 us (15 more values live across the observation pass cost as much as the sunk loads), so it stays off; the camera
  // kernels sit at the edge of the register file and were not tried.
  constexpr bool PF_GEN = false;
  if (GENERAL && resetting) {
    if (SWAP_REGS) {
#pragma unroll
      for (int j = 0; j < kCW; ++j) {
        const int w = sub + j * G; cw[j] = (T)0;
        if (w < kRows) { if (PF_GEN) pf_issue(cw[j], &D.rs[(size_t)w * n + env]); else cw[j] = D.rs[(size_t)w * n + env]; }
      }
#pragma unroll
      for (int j = 0; j < kOW; ++j) {
        const int k = sub + j * G; ow[j] = (T)0;
        if (k < Dobs) { if (PF_GEN) pf_issue(ow[j], &Dg.sobs[(size_t)env * Dobs + k]); else ow[j] = Dg.sobs[(size_t)env * Dobs + k]; }
      }
    }
    tick_new = D.is[env];
  }
  const int ep_want = episode + 1 + ((GENERAL && resetting) ? 1 : 0);     // a reset taken below asks for the episode after next
  if ((GENERAL || DEFER) && D.shadow_on && active && leader && (uint32_t)(sh_req >> 32) != (uint32_t)ep_want)
    D.sreq[env] = ((unsigned long long)(uint32_t)ep_want << 32) | (unsigned long long)launch;   // ask for the next episode
  T act_obs[4] = {(T)0, (T)0, (T)0, (T)0};
  if (LANE_T) {
    // every lane runs the pass (same issue cost as one lane), the leader stores; action and waypoints come by shuffle
#pragma unroll
    for (int k = 0; k < 4; ++k) act_obs[k] = __shfl(a_keep, gbase | k, kWave);
    if (act_src == 1) {                              // bare-Gymnasium stale view: the stored action
#pragma unroll
      for (int k = 0; k < 4; ++k) act_obs[k] = D.r[(size_t)(RF_ACTION + k) * n + envc];
    }
    if constexpr (!OBSW) {                           // (OBSW: the second wave runs the pass; act_obs is kept for the state store)
    T Ro[9];
    int o = write_obs_attitude<T, true, SH>(P, S, act_obs, Ro, [&](int k, T v) { if (leader) tile[row * ld + k] = v; });
#pragma unroll SH::kCtxUnroll
    for (int i = 0; i < FW_SH(ctx); ++i) {
      const int t = tgt_obs + i;
      T tw[3], d[3], b[3] = {(T)0, (T)0, (T)0};
#pragma unroll
      for (int k = 0; k < 3; ++k) tw[k] = __shfl(tmine[k], gbase | (t & (G - 1)), kWave);
      if (t < FW_SH(num_targets)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = tw[k] - S.p[k];
        mtv(Ro, d, b);
      }
      if (leader) { tile[row * ld + o] = b[0]; tile[row * ld + o + 1] = b[1]; tile[row * ld + o + 2] = b[2]; }
      o += 3;
    }
    }
  } else if (active && leader) {
    load_action<T, COLLECT>(D, actions, env, act_src, act_obs);
    if (OBJ) obj_write_obs<T>(P, O, S, act_obs, [&](int k, T v) { tile[row * ld + k] = v; });
    else if (COMB) comb_write_obs<T>(P, D, env, O, S, act_obs, tgt_obs, [&](int k, T v) { tile[row * ld + k] = v; });
    else write_obs<T>(P, D, env, S, act_obs, tgt_obs, [&](int k, T v) { tile[row * ld + k] = v; });
  }
  FWP(const long long p_e0 = FWP_NOW();)
  if (DEFER && pre) {
    // the hand-issued prefetches: ONE wait, here -- behind the observation pass and AHEAD of the terminal-observation stores below
    // (vmcnt counts stores too: a wait placed after them pays their acknowledgement, ~2 k cycles) -- tied to every value
    pf_wait(tpre[0], tpre[1], tpre[2], dnd);
    if (WO && !OBSW) pf_tie(dow[0], dow[1], dow[2], dow[3]);
  }
  if (DEFER && resetting) {                          // group-uniform: all G lanes of the env take part
    // the row just written is the terminal observation: move it out before the new episode's row replaces it (OBSW: the second wave does)
    if constexpr (!OBSW) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (terminal_obs) {
      T* trow = terminal_obs + (size_t)env * Dobs;
      for (int k = sub; k < Dobs; k += G) trow[k] = tile[row * ld + k];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    FWP(const long long p_e1 = FWP_NOW(); if (!OBSW) p_r1 = p_e1 - p_e0;)      // obs pass end -> terminal observation copied out (OBSW: p_r1 is the wait at barrier 2)
    // the new episode's row goes into the tile -- or (OBSW, where only the fallback path gets here with a row to build) straight to memory
    T* const orow = OBSW ? obs + (size_t)env * Dobs : nullptr;
    episode += 1;
    if (leader) { stat_add(D.stats, FW_CTR_RESETS); stat_add(D.stats, pre ? FW_CTR_SCENARIO_HITS : FW_CTR_FALLBACKS); }
    Scenario<T> sc;
    // (the obs pass above read the old waypoints; they are overwritten here)
    if (pre) {                                         // sampled ahead of time by a worker block of an earlier launch
#pragma unroll
      for (int k = 0; k < 3; ++k) sc.t_mine[k] = tpre[k];
      if (sub < FW_SH(num_targets)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) D.r[(size_t)(RF_TARGETS + 3 * sub + k) * n + env] = tpre[k];
      }
    } else {
      sample_scenario_inl<T, G>(Pp, D.r, n, env, (uint32_t)episode, &sc);
    }
    const int nt = min(FW_SH(ctx), FW_SH(num_targets));
    T t0[3] = {(T)0, (T)0, (T)0};
    const bool copied = WO && pre && Dobs <= kDOW * G;    // the worker left the whole first observation row: nothing to compute
    if (copied && !OBSW) {
#pragma unroll
      for (int j = 0; j < kDOW; ++j) { const int k = sub + j * G; if (k < Dobs) tile[row * ld + k] = dow[j]; }
    }
#pragma unroll 1
    for (int i = 0; i < (copied ? 0 : FW_SH(ctx)); ++i) {
      T tw[3] = {(T)0, (T)0, (T)0};
      if (G > 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) tw[k] = __shfl(sc.t_mine[k], (lane & ~(G - 1)) | (i & (G - 1)), kWave);    // lane i of the group sampled waypoint i
      } else if (i < nt) {
#pragma unroll
        for (int k = 0; k < 3; ++k) tw[k] = D.r[(size_t)(RF_TARGETS + 3 * i + k) * n + env];                      // own stores, program order
      }
      T d[3] = {(T)0, (T)0, (T)0}, b[3] = {(T)0, (T)0, (T)0};
      if (i < nt) {
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = tw[k] - P.warm[k];
        mtv(P.warm_R, d, b);
        if (i == 0) { t0[0] = tw[0]; t0[1] = tw[1]; t0[2] = tw[2]; }
      }
      if (OBSW) { if (leader) { orow[SH::att_dim + 3 * i] = b[0]; orow[SH::att_dim + 3 * i + 1] = b[1]; orow[SH::att_dim + 3 * i + 2] = b[2]; } }
      else if (leader) { tile[row * ld + FW_SH(att_dim) + 3 * i] = b[0]; tile[row * ld + FW_SH(att_dim) + 3 * i + 1] = b[1]; tile[row * ld + FW_SH(att_dim) + 3 * i + 2] = b[2]; }
    }
    FWP(const long long p_e2 = FWP_NOW(); p_r2 = p_e2 - p_e1;)      // new waypoints stored, their deltas in the tile
    if (WO && !copied) {
#pragma unroll
      for (int j = 0; j < kWO; ++j) { const int k = sub + j * G; if (k < FW_SH(att_dim)) { if (OBSW) orow[k] = wo[j]; else tile[row * ld + k] = wo[j]; } }   // the env's lanes share the cached attitude block
    }
    if (!copied) for (int k = sub + (WO ? kWO * G : 0); k < FW_SH(att_dim); k += G) tile[row * ld + k] = Pp->warm_obs[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { S.p[k] = P.warm[k]; S.v[k] = P.warm[7 + k]; S.w[k] = P.warm[10 + k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) S.q[k] = P.warm[3 + k];
#pragma unroll
    for (int k = 0; k < FW_NUM_ACTUATORS; ++k) S.act[k] = P.warm[13 + k];
    tick = P.warm_ticks;
    step_count = 0; flags = 0; ep_return = (T)0; tgt_obs = 0; num_reached = 0;
    new_dist = copied ? dnd : (T)0;
    if (FW_SH(num_targets) > 0 && !copied) {
      if (G == 1 && nt == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) t0[k] = D.r[(size_t)(RF_TARGETS + k) * n + env];
      } else if (G > 1 && nt == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) t0[k] = __shfl(sc.t_mine[k], lane & ~(G - 1), kWave);
      }
      T dx = t0[0] - S.p[0], dy = t0[1] - S.p[1], dz = t0[2] - S.p[2];
      new_dist = M<T>::sqrt_(dx * dx + dy * dy + dz * dz);                 // end_reset -> compute_state
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) act_obs[k] = (T)0;
    FWP(p_r3 = FWP_NOW() - p_e2;)                                   // cached block + warm state + first distance
  }
  if (PF_GEN && resetting) {                         // ONE wait for the hand-issued loads, ahead of the terminal-observation stores
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < kCW; ++j) asm volatile("" : "+v"(cw[j]));
#pragma unroll
    for (int j = 0; j < kOW; ++j) asm volatile("" : "+v"(ow[j]));
  }
  if (GENERAL && resetting) {                        // group-uniform: all G lanes of the env take part
    // the row just written is the terminal observation: move it out, then the new episode's row and state replace the old
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (terminal_obs) {
      T* trow = terminal_obs + (size_t)env * Dobs;
      for (int k = sub; k < Dobs; k += G) trow[k] = tile[row * ld + k];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (SWAP_REGS) {
#pragma unroll
      for (int j = 0; j < kOW; ++j) { const int k = sub + j * G; if (k < Dobs) tile[row * ld + k] = ow[j]; }
#pragma unroll
      for (int j = 0; j < kCW; ++j) { const int w = sub + j * G; if (w < kRows) D.r[(size_t)w * n + env] = cw[j]; }
    } else {
      for (int k = 0; k < Dobs; ++k) tile[row * ld + k] = Dg.sobs[(size_t)env * Dobs + k];
      copy_words<T, G>(D.r, D.rs, 0, kRows, n, env);
    }
    if (leader) { stat_add(D.stats, FW_CTR_RESETS); stat_add(D.stats, FW_CTR_SHADOW_HITS); }
    episode += 1; tick = tick_new;
    step_count = 0; flags = 0; tgt_obs = 0; num_reached = 0;
  }
  if (active && leader) {
    if (!(GENERAL && resetting)) {
      store_rigid<T>(D, env, S);
      if (HASOBJ) obj_store<T, OBJ>(D, env, O);
#pragma unroll
      for (int k = 0; k < 4; ++k) D.r[(RF_ACTION + k) * n + env] = act_obs[k];
      D.r[RF_NEW_DIST * n + env] = new_dist;
      D.r[RF_EP_RETURN * n + env] = ep_return;
    }
    D.i[IF_STEP * n + env] = step_count;
    D.i[IF_TICK * n + env] = tick;
    D.i[IF_EPISODE * n + env] = episode;
    D.i[IF_FLAGS * n + env] = flags | (tgt_obs << FL_TGT_SHIFT);
    D.i[IF_NUM_REACHED * n + env] = num_reached;
  }
  if (STASH && !DEFER && active && leader) {         // the outputs parked at the latch point: behind every load of the epilogue
    const double w2 = latch[4 * row + 2], w3 = latch[4 * row + 3];
    const int o_nr = __double2hiint(w2), o_fl = __double2loint(w2), o_st = __double2hiint(w3), o_sc = __double2loint(w3);
    reward[env] = (T)latch[4 * row];
    terminated[env] = (uint8_t)((o_fl & FL_TERM) ? 1 : 0);
    truncated[env] = (uint8_t)((o_fl & FL_TRUNC) ? 1 : 0);
    if (info) {
      int4* ip = reinterpret_cast<int4*>(info + (size_t)env * FW_INFO_DIM);
      ip[0] = make_int4(o_nr, (o_fl & FL_COLLISION) ? 1 : 0, (o_fl & FL_OOB) ? 1 : 0, (o_fl & FL_COMPLETE) ? 1 : 0);
      ip[1] = make_int4(o_st, OBJ ? o_st : 0, o_sc, 0);
    }
  }
  if (OBSW) {}                                       // (the second wave flushes the tile it wrote)
  else if (HELP || AUX) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }   // (the capture / second wave takes no part: no s_barrier)
  else __syncthreads();
  // (COLLECT: the partial sums first -- the fold waves at the end of the launch are waiting for them, nobody for the observation rows)
  if (COLLECT) collect_stats_tail<T>(*CAp, D.epoch, tile, ld, min(EPW, D.n - env0), wg, nblk, active && leader, latch[4 * row], latch[4 * row + 1] != 0.0, env, c_ret);
  if (!OBSW) flush_obs_tile<T>(tile, ld, obs, env0, EPW, D.n, Dobs);
  if (COLLECT && active && leader) collect_clear_actions<T>(const_cast<T*>(actions) + (size_t)env * 4);      // "not there yet" for the next launch
  FWP(long long p_capmax = HASOBJ ? O.p_cap : 0; const int p_ncapw = HASOBJ ? __popcll(__ballot(leader && O.p_ncap > 0)) : 0;)
  FWP(if (D.prof) {
    for (int o = 32; o > 0; o >>= 1) p_capmax = max(p_capmax, (long long)__shfl_xor((long long)p_capmax, o, kWave));
    const int nr = __popcll(__ballot(leader && p_nreset > 0)), nh = __popcll(__ballot(leader && p_nhit > 0));
    for (int o = 32; o > 0; o >>= 1) {               // the reset split is per lane (divergent region): wave max
      p_r1 = max(p_r1, (long long)__shfl_xor((long long)p_r1, o, kWave));
      p_r2 = max(p_r2, (long long)__shfl_xor((long long)p_r2, o, kWave));
      p_r3 = max(p_r3, (long long)__shfl_xor((long long)p_r3, o, kWave));
    }
    if (lane == 0) {
      long long* w = D.prof + ((size_t)(launch % kProfSlots) * 2 * nblk + blockIdx.x) * kProfWords;
      const long long t3 = FWP_NOW();
      w[0] = t3 - p_t0; w[1] = p_t1 - p_t0; w[2] = p_reset; w[3] = p_avi; w[4] = p_task; w[5] = t3 - p_t2; w[6] = it | (nr << 8) | (nh << 16); w[7] = p_t0; w[8] = p_r1; w[9] = p_r2; w[10] = p_r3;
      w[11] = p_capmax | ((long long)p_ncapw << 48);
      if (OBSW) w[11] = (p_b1 - p_t0) | ((p_b2 - p_t0) << 32);      // (no camera: the word carries the two arrivals, from this wave's first stamp, 32 bits each)
      if (HELP) { w[8] = p_nhit; w[9] = n_posted; w[7] = p_r1; w[10] = p_r2; w[11] = p_r3; }
      else if (HASOBJ) { w[8] = O.p_capm[0]; w[9] = O.p_capm[1]; w[10] = O.p_capm[2]; w[7] = O.p_capm[3];
        if (getenv_ph) { w[1] = O.p_ph[0]; w[3] = O.p_ph[1]; w[4] = O.p_ph[2]; w[5] = O.p_ph[3]; w[9] = O.p_ph[4]; w[6] = O.p_ph[5]; } }     // (the reset split is unused by these kernels)
    } })
  if constexpr (SH::kFixed) launch_done(Dg.lctr, launch);         // (the kernel does not go through FW_STEP_RUN)
}

#ifndef FW_G1_WAVES
#define FW_G1_WAVES 2   // env-per-lane mapping: cap registers for >= 2 waves/SIMD (TLP hides the scalar-load and fp64 latency)
#endif
#define FW_STEP_ARGS const Params<T>* __restrict__ Pp, const ObjC<T>* __restrict__ OCp, DevState<T> D,                  \
    const T* __restrict__ actions, T* __restrict__ obs, T* __restrict__ reward, uint8_t* __restrict__ terminated,        \
    uint8_t* __restrict__ truncated, T* __restrict__ terminal_obs, int32_t* __restrict__ info
#define FW_STEP_PASS Pp, OCp, D, actions, obs, reward, terminated, truncated, terminal_obs, info
// every step kernel: launch index from the workgroup's own device-side counter, advanced when the workgroup is finished
#define FW_STEP_RUN(...) do { D.epoch = launch_index(D.lctr); step_body<__VA_ARGS__>(FW_STEP_PASS); launch_done(D.lctr, D.epoch); } while (0)
// latency mapping (8 lanes per env): one wave per SIMD by construction, let the allocator use the whole file
// (AX: the axis-aligned geometry variant of the tick, fw_env::axis_aligned)
template <typename T, bool GENERAL, bool AX = false>
__global__ __launch_bounds__(kWave) void fw_step_kernel_g8(FW_STEP_ARGS) { FW_STEP_RUN(T, GENERAL, 8, FW_TASK_WAYPOINTS, 1, false, false, AX); }
// ... with a second wave per workgroup that draws the motor noise (step_body AUX; f64, wind-free, axis-aligned: the headline row)
template <typename T>
__global__ __launch_bounds__(2 * kWave) void fw_step_kernel_g8x(FW_STEP_ARGS) { FW_STEP_RUN(T, false, 8, FW_TASK_WAYPOINTS, 1, false, false, true, true); }
// ... and that kernel compiled for the shape of the headline training config (step_body SH; fw_env::step_shape)
template <typename T>
__global__ __launch_bounds__(2 * kWave) void fw_step_kernel_g8xs(FW_STEP_ARGS) {
  // (not FW_STEP_RUN: step_body reads and advances the launch counter itself where the shape is fixed, off the path to the state loads)
  step_body<T, false, 8, FW_TASK_WAYPOINTS, 1, false, false, true, true, ShapeTrainWaypoints>(FW_STEP_PASS);
}
#ifndef FW_OBSW_MODE
#define FW_OBSW_MODE 2   // 1: a measuring build with the grid change and the worker alone (step_body OBSM; profiles/r24_obs_wave_ab.txt)
#endif
// ... and that one with the second wave kept to the end: scenario worker of its tile, then the observation rows (step_body OBSW; fw_env::obs_wave)
template <typename T>
__global__ __launch_bounds__(2 * kWave) void fw_step_kernel_g8xo(FW_STEP_ARGS) {
  step_body<T, false, 8, FW_TASK_WAYPOINTS, 1, false, false, true, true, ShapeTrainWaypoints, FW_OBSW_MODE>(FW_STEP_PASS);
}
// ... and the same mapping capped at 256 registers: two waves per SIMD (8 192 < N <= 65 536 envs)
template <typename T, bool GENERAL>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2, 2)))
void fw_step_kernel_g8w2(FW_STEP_ARGS) { FW_STEP_RUN(T, GENERAL, 8, FW_TASK_WAYPOINTS, 2); }
// throughput mapping (one lane per env)
template <typename T, bool GENERAL>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(FW_G1_WAVES, FW_G1_WAVES)))
void fw_step_kernel_g1(FW_STEP_ARGS) { FW_STEP_RUN(T, GENERAL, 1, FW_TASK_WAYPOINTS); }
// ObjLock task (always the GENERAL path: its training config has wind)
template <typename T, int TKIND>
__global__ __launch_bounds__(kWave) void fw_step_kernel_obj_g8(FW_STEP_ARGS) { FW_STEP_RUN(T, true, 8, TKIND); }
template <typename T, int TKIND>
__global__ __launch_bounds__(kWave) void fw_step_kernel_obj_g1(FW_STEP_ARGS) { FW_STEP_RUN(T, true, 1, TKIND); }
#ifndef FW_HELP_CHUNK
#define FW_HELP_CHUNK 2      // warm-up Aviary steps of shadow work a capture wave does per launch
#endif
// ... with a capture wave beside every step wave (fwsim_objlock.hpp, "The capture wave"): 128 threads, wave 0 steps, wave 1 serves
template <typename T, int TKIND>
__global__ __launch_bounds__(2 * kWave) void fw_step_kernel_obj_g8h(FW_STEP_ARGS) {
  const Mbox<T> MB = mbox_at<T>(D.mbox_off);
  if (threadIdx.x < 4) MB.ctl[threadIdx.x] = 0u;
  __syncthreads();                                   // the ONE s_barrier both waves meet at: the mailbox words are zero
  if (threadIdx.x >= kWave) {
    // The grid of this kernel is the step workgroups alone -- with one wave per SIMD (the whole register file each) 512 step waves
    // + 512 capture waves fill the chip, and separate worker workgroups would run BEHIND them (measured: + 15 us).  The capture
    // wave is the shadow worker of its tile as well: one warm-up Aviary step per launch (instead of step_ratio), at the start,
    // while the step wave is in its prologue and first sub-step and cannot have posted anything yet.
    const int nblk = (D.npad + 7) / 8, bx = (int)blockIdx.x % nblk;
    const int blk = ((nblk & 7) == 0) ? (bx & 7) * (nblk >> 3) + (bx >> 3) : bx;       // (step_body's XCD-aware map)
    D.epoch = launch_index(D.lctr);
    const DevState<T> V = tile_view<T, 8>(D, blk);
    // (Tried: the mailbox looked at in front of every warm-up Aviary step of the shadow work, requests first -- combined 60.2 ->
    // 61.5 us: the wave is short of time, not badly ordered.)
    FWP(const long long h0 = FWP_NOW(); long long hcap = 0; int hreq = 0;)
    if (D.shadow_on) shadow_worker<T, 8, TKIND>(Pp, OCp, V, blk, FW_HELP_CHUNK);
    FWP(const long long h1 = FWP_NOW();)
    capture_server<T>(MB, 0u, *OCp, V, blk * 8 FWP(, &hcap, &hreq));
    FWP(if (D.prof && threadIdx.x == kWave) {
      long long* w = D.prof + ((size_t)(D.epoch % kProfSlots) * 2 * nblk + nblk + blockIdx.x) * kProfWords;
      w[0] = (h1 - h0) + hcap; w[1] = h1 - h0; w[2] = hcap; w[3] = hreq; w[4] = FWP_NOW() - h0; })
    return;
  }
  D.epoch = launch_index(D.lctr);
  step_body<T, true, 8, TKIND, 1, false, true>(FW_STEP_PASS);
  launch_done(D.lctr, D.epoch);
  if (threadIdx.x == 0) __hip_atomic_store(MB.ctl + 2, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);     // every path of wave 0 ends here
}

// fw_collect_step (fwsim_fused.hpp): act waves in front, then the step waves of the same step kernels with COLLECT on.  The
// 8-lane mapping at one wave per SIMD only (the collector's regime: thousands of envs per GPU).
#define FW_COLLECT_RUN(T_, ...) do {                                                                                       \
    if ((int)blockIdx.x < CA.n_act) {                                                                                  \
      /* launch index = the word of a step workgroup of MY chunk: it cannot finish (and advance its word) before I publish */ \
      const int nblk_ = (D.npad + 7) / 8, c_ = min((int)blockIdx.x >> 1, CA.n_chunks - 1);                              \
      const int blk_ = min(c_ * kCRows / 8, nblk_ - 1);                                                                 \
      const int wg_ = ((nblk_ & 7) == 0) ? (blk_ % (nblk_ >> 3)) * 8 + blk_ / (nblk_ >> 3) : blk_;   /* inverse of the XCD-aware map */ \
      collect_act_wave<T_>(CA, 1u + D.lctr[wg_]);                                                                          \
      return;                                                                                                           \
    }                                                                                                                   \
    if (CA.trace && threadIdx.x == 0) CA.trace[(size_t)blockIdx.x * 8] = collect_now();                                 \
    const int bx_ = (int)blockIdx.x - CA.n_act;                                                                         \
    if (bx_ >= CA.n_workers) {                                                                                          \
      collect_fold_wave(CA, bx_ - CA.n_workers);                                                                        \
      if (CA.trace && threadIdx.x == 0) CA.trace[(size_t)blockIdx.x * 8 + 7] = collect_now();                           \
      return;                                                                                                           \
    }                                                                                                                   \
    D.epoch = 1u + D.lctr[bx_];                                                                                         \
    step_body<T_, __VA_ARGS__>(FW_STEP_PASS, &CA);                                                                     \
    if (threadIdx.x == 0) D.lctr[bx_] = D.epoch;                                                                        \
    if (CA.trace && threadIdx.x == 0) CA.trace[(size_t)blockIdx.x * 8 + 7] = collect_now();                             \
  } while (0)
template <typename T, bool GENERAL>
__global__ __launch_bounds__(kWave) void fw_collect_kernel_g8(FW_STEP_ARGS, const CollectArgs CA) { FW_COLLECT_RUN(T, GENERAL, 8, FW_TASK_WAYPOINTS, 1, true); }
template <typename T, int TKIND>
__global__ __launch_bounds__(kWave) void fw_collect_kernel_obj_g8(FW_STEP_ARGS, const CollectArgs CA) { FW_COLLECT_RUN(T, true, 8, TKIND, 1, true); }
// ... and for the two-waves-per-SIMD build of the waypoints kernels (8 192 < N <= 24 576 envs: 12 288 with wind), so that those
// env counts keep the one-launch collector (round 3 sent them to the three-launch one)
template <typename T, bool GENERAL>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2, 2)))
void fw_collect_kernel_g8w2(FW_STEP_ARGS, const CollectArgs CA) { FW_COLLECT_RUN(T, GENERAL, 8, FW_TASK_WAYPOINTS, 2, true); }

// Caller-supplied scenario of the episodes a fw_reset starts (fw_scenario, uploaded to device memory by the host side;
// doubles indexed by the handle's local env, null = keep the env's own draw).
struct ScenOv {
  const double *targets, *duck, *obst, *nob, *wind_base, *gust_amp, *gust_phase;
};

// K2: reset (masked) + observation.  Same single-tick-site structure (warm-up only).
template <typename T, int G, int TKIND>
__global__ __launch_bounds__(kWave)
void fw_reset_kernel(const Params<T>* __restrict__ Pp, const ObjC<T>* __restrict__ OCp, DevState<T> Dg,
                     const uint8_t* __restrict__ mask, T* __restrict__ obs, int do_reset, ScenOv ov) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const Params<T>& P = *Pp;
  constexpr bool OBJ = TKIND == FW_TASK_OBJLOCK;
  constexpr bool COMB = TKIND == FW_TASK_WAYPOINT_OBJLOCK;
  constexpr bool HASOBJ = OBJ || COMB;
  constexpr int EPW = kWave / G;
  const int lane = threadIdx.x;
  const int sub = (G == 1) ? 0 : (lane & (G - 1));
  const int row = lane / G;
  const bool leader = sub == 0;
  const DevState<T> D = tile_view<T, EPW>(Dg, (int)blockIdx.x);
  const int env0 = blockIdx.x * EPW;
  const int env = env0 + row;
  const bool active = env < D.n;
  const int envc = active ? env : D.n - 1;
  const size_t n = D.npad;
  const int Dobs = P.obs_dim;
  const int ld = Dobs + 1;
  TickC<T> C; SurfC<T> mine; T wmask;
  load_tick_constants<T, G, false>(Pp, C, mine, wmask);

  Rigid<T> S;
  load_rigid<T>(D, envc, S);
  ObjState<T> O;
  const ObjC<T>& OC = *OCp;
  if (HASOBJ) obj_load<T, OBJ>(D, envc, O);
  T action[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) action[k] = D.r[(RF_ACTION + k) * n + envc];
  int32_t num_reached = D.i[IF_NUM_REACHED * n + envc];
  int tgt_obs = (D.i[IF_FLAGS * n + envc] >> FL_TGT_SHIFT) & 15;
  const bool resetting = active && do_reset && (!mask || mask[envc]);
  int32_t tick = 0, episode = D.i[IF_EPISODE * n + envc];
  T new_dist = (T)0, wb[3] = {(T)0, (T)0, (T)0}, wa[3] = {(T)0, (T)0, (T)0}, wphase = (T)0;
  int warm_left = 0;
  if (resetting) {
    T t_mine[3] = {(T)0, (T)0, (T)0};
    warm_left = begin_reset<T, G>(P, D, env, S, tick, episode, num_reached, wb, wa, wphase, t_mine);
    // ---- caller-supplied scenario: replaces what begin_reset drew, before anything depends on it ----
    if (P.wind_mode != FW_WIND_OFF && (ov.wind_base || ov.gust_amp || ov.gust_phase)) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (ov.wind_base) wb[k] = (T)ov.wind_base[3 * (size_t)env + k];
        if (ov.gust_amp) wa[k] = (T)ov.gust_amp[3 * (size_t)env + k];
      }
      if (ov.gust_phase) wphase = (T)ov.gust_phase[env];
      if (leader) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { D.r[(RF_WIND + k) * n + env] = wb[k]; D.r[(RF_WIND + 3 + k) * n + env] = wa[k]; }
        D.r[(RF_WIND + 6) * n + env] = wphase;
      }
    }
    T t_last[3] = {(T)0, (T)0, (T)0};
    if (!OBJ && ov.targets && P.num_targets > 0) {
      if (leader)
        for (int t = 0; t < P.num_targets; ++t)
#pragma unroll
          for (int k = 0; k < 3; ++k) D.r[(size_t)(RF_TARGETS + 3 * t + k) * n + env] = (T)ov.targets[((size_t)env * FW_MAX_TARGETS + t) * 3 + k];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        t_mine[k] = (T)ov.targets[(size_t)env * FW_MAX_TARGETS * 3 + k];                              // waypoint 0, for end_reset
        t_last[k] = (T)ov.targets[((size_t)env * FW_MAX_TARGETS + (P.num_targets - 1)) * 3 + k];
      }
    }
    if (HASOBJ) {
      obj_reset_state<T, OBJ>(O);
      if (OBJ) obj_spawn<T, G>(P, OC, D, env, (uint32_t)episode, leader, O); else comb_spawn<T, G>(P, OC, D, env, (uint32_t)episode, leader, O);
      if (COMB && ov.targets && P.num_targets > 0) { O.duck[0] = t_last[0]; O.duck[1] = t_last[1]; }   // the duck sits under the last waypoint
      if (ov.duck) {
#pragma unroll
        for (int k = 0; k < 3; ++k) O.duck[k] = (T)ov.duck[3 * (size_t)env + k];
      }
      if (ov.obst && ov.nob) {
        int nob = (int)ov.nob[env];
        nob = nob < 0 ? 0 : (nob > OC.num_obstacles ? OC.num_obstacles : nob);           // never more than the config (and its LDS row) allows
        if (leader)
          for (int o = 0; o < FW_MAX_OBSTACLES; ++o)
#pragma unroll
            for (int k = 0; k < 3; ++k)
              D.r[(size_t)(RF_TASK + FW_ST_OBST + 3 * o + k) * n + env] = o < nob ? (T)ov.obst[((size_t)env * FW_MAX_OBSTACLES + o) * 3 + k] : (T)0;
        O.nob = nob;
      }
      if (G > 1) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
    if (HASOBJ) obj_update_near_mask<T, G>(P, OC, D, envc, O, S);
    if (warm_left == 0) {
      if (OBJ) obj_compute_state<T>(O);
      else { new_dist = end_reset<T, G>(P, D, env, episode, S, ov.targets ? t_mine : nullptr); if (COMB) comb_compute_state<T>(OC, O, P.num_targets == 0); }
    }
  }
  // waypoint 0 of a supplied scenario, for the end_reset that follows an in-kernel warm-up
  T t_first[3] = {(T)0, (T)0, (T)0};
  const bool have_first = resetting && !OBJ && ov.targets && P.num_targets > 0;
  if (have_first) {
#pragma unroll
    for (int k = 0; k < 3; ++k) t_first[k] = (T)ov.targets[(size_t)env * FW_MAX_TARGETS * 3 + k];
  }
  const T cmd0[FW_NUM_ACTUATORS] = {(T)0, (T)0, (T)0, (T)0, (T)0, (T)0};
  T R[9];
  normalize_quat<T>(S.q);
  rot_from_unit_quat<T>(S.q, R);
  T gust[2];
  gust_init<T>(P, wphase, tick, gust);
  LaneAct<T> LA; LA.cmd = (T)0; LA.a = (T)0;
  if (G == 8) lane_act_scatter<T>(S, LA);
#pragma unroll 1
  while (__ballot(warm_left > 0) != 0ull) {
    const bool stepped = warm_left > 0;
    if (stepped) (void)aviary_step<T, true, G, HASOBJ>(P, C, OC, D, env, O, S, R, cmd0, tick, (T)0, (T)0, wb, wa, gust, mine, wmask, LA);
    if (HASOBJ) obj_capture_step<T, G>(OC, D, stepped, env, O, S, R, tick);
    if (stepped) {
      warm_left -= 1;
      if (warm_left == 0) {
        if (OBJ) obj_compute_state<T>(O);
        else { new_dist = end_reset<T, G>(P, D, env, episode, S, have_first ? t_first : nullptr); if (COMB) comb_compute_state<T>(OC, O, P.num_targets == 0); }
      }
    }
  }
  if (G > 1) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  if (G == 8) lane_act_gather<T>(S, LA);
  if (resetting) {
    action[0] = action[1] = action[2] = action[3] = (T)0;
    tgt_obs = 0;
    if (leader) {
      store_rigid<T>(D, env, S);
#pragma unroll
      for (int k = 0; k < 4; ++k) D.r[(RF_ACTION + k) * n + env] = (T)0;
      D.r[RF_NEW_DIST * n + env] = new_dist;
      D.r[RF_EP_RETURN * n + env] = (T)0;
      D.i[IF_STEP * n + env] = 0;
      D.i[IF_TICK * n + env] = tick;
      D.i[IF_EPISODE * n + env] = episode;
      D.i[IF_FLAGS * n + env] = 0;
      D.i[IF_NUM_REACHED * n + env] = num_reached;
      if (HASOBJ) obj_store<T, OBJ>(D, env, O);
    }
  }
  if (obs) {
    if (active && leader) {
      if (OBJ) obj_write_obs<T>(P, O, S, action, [&](int k, T v) { tile[row * ld + k] = v; });
      else if (COMB) comb_write_obs<T>(P, D, env, O, S, action, tgt_obs, [&](int k, T v) { tile[row * ld + k] = v; });
      else write_obs<T>(P, D, env, S, action, tgt_obs, [&](int k, T v) { tile[row * ld + k] = v; });
    }
    __syncthreads();
    flush_obs_tile<T>(tile, ld, obs, env0, EPW, D.n, Dobs);
  }
}

// the low-level task: one step and one reset kernel for its two variants (fw_step_kernel_ll / fw_reset_kernel_ll)
#include "fwsim_lowlevel.hpp"
// the low-level task's command input and trace (fw_command_ll / fw_trace_ll): the target goes to ll_target_slot above
#include "fwsim_command.hpp"
#include "fwsim_flight.hpp"
// the frozen low-level controller as a device function (fw_controller_forward, and the in-loop action source of the kernel below)
#include "fwsim_hl_step.hpp"
// the waypoints task under six direct actuator commands -- held for the agent step, or from that controller in front of every Aviary
// step (fw_step_hl) -- and the high-level command step in front of it (fw_command_hl)
#include "fwsim_direct.hpp"
// ... and the act side of its collected vec-step in one launch (fw_collect_act_hl)
#include "fwsim_collect_hl.hpp"
// ... and the test hook that evaluates the device building blocks one at a time (fw_probe)
#include "fwsim_probe.hpp"
// ... and the off-policy learner of the low-level task (fw_sac_act, fw_replay_store / _sample, fw_sac_noise, fw_sac_update)
#include "fwsim_sac.hpp"
// ... and its replay ring (fwsim_replay.hpp) with prioritized replay on it (fw_replay_per_*, fw_replay_sample_per, fw_sac_update_weighted)
#include "fwsim_per.hpp"
// ... and TD3 on the same ring and the same product kernel (fw_td3_act, fw_td3_update)
#include "fwsim_td3.hpp"

// ======================================================================
// host side
// ======================================================================
namespace {

constexpr bool kObsWaveDefault = true;    // the observation-wave row (fw_step_kernel_g8xo) is on wherever it exists: measured at 4096 and 2048 envs, profiles/r24_obs_wave_ab.txt
constexpr int kAuxWaveMaxEnvs = 4096;  // noise wave beside every step wave (fw_step_kernel_g8x): 512 two-wave workgroups, one wave per SIMD on 1024 SIMDs
constexpr int kG8MaxEnvs = 16384;   // measured crossover on MI355X: 8 lanes/env wins up to 2^14 envs (51 vs 70 us), loses at 2^15 (93 vs 76 us)
thread_local std::string g_err;

// Task predicates: what the host side asks about a task, in one place (a new task answers them here).
inline bool has_camera(int task) { return task == FW_TASK_OBJLOCK || task == FW_TASK_WAYPOINT_OBJLOCK; }
inline bool direct_actions(int task) { return task == FW_TASK_LOWLEVEL || task == FW_TASK_WAYPOINTS_DIRECT; }   // six actuator commands

struct HostDerived {
  double area, aspect, Cl3, a0b, asPb, asNb, theta_f, tau_f, tq[3];
};

int validate(const fw_config* c, std::string& msg) {
  char buf[256];
  auto fail = [&](int code) { msg = buf; return code; };
  if (!c) { snprintf(buf, sizeof buf, "null config"); return fail(FW_EINVAL); }
  if (c->abi_version != FW_ABI_VERSION) { snprintf(buf, sizeof buf, "abi_version %d != %d", c->abi_version, FW_ABI_VERSION); return fail(FW_EVERSION); }
  if (c->agent_hz <= 0 || 120 % c->agent_hz != 0) {
    int lowest = c->agent_hz > 0 ? (int)(120 / ((int)(120 / c->agent_hz) + 1)) : 1;
    int highest = (c->agent_hz > 0 && c->agent_hz <= 120) ? (int)(120 / (int)(120 / c->agent_hz)) : 120;
    snprintf(buf, sizeof buf, "`agent_hz` must be round denominator of 120, try %d or %d.", lowest, highest);
    return fail(FW_EINVAL);
  }
  if (c->angle_representation != 0 && c->angle_representation != 1) {
    snprintf(buf, sizeof buf, "angle_representation must be either `euler` or `quaternion`, not %d", c->angle_representation);
    return fail(FW_EINVAL);
  }
  if (c->wind_mode < FW_WIND_OFF || c->wind_mode > FW_WIND_GUST_SINE) { snprintf(buf, sizeof buf, "Unsupported wind mode: %d", c->wind_mode); return fail(FW_EINVAL); }
  if (c->wind_mode != FW_WIND_OFF && c->wind_randomize_on_reset) {
    for (int i = 0; i < 3; ++i) {
      if (!(c->wind_enu_mps_range[i][0] <= c->wind_enu_mps_range[i][1])) { snprintf(buf, sizeof buf, "Invalid wind_enu_mps_range"); return fail(FW_EINVAL); }
      if (!(c->gust_amp_enu_mps_range[i][0] <= c->gust_amp_enu_mps_range[i][1])) { snprintf(buf, sizeof buf, "Invalid gust_amp_enu_mps_range"); return fail(FW_EINVAL); }
    }
  }
  if (c->task < FW_TASK_WAYPOINTS || (c->task > FW_TASK_LOWLEVEL && c->task != FW_TASK_WAYPOINTS_DIRECT)) { snprintf(buf, sizeof buf, "unknown task %d", c->task); return fail(FW_EINVAL); }
  if (c->task == FW_TASK_LOWLEVEL) {
    // fixedwing_lowlevel_env.py:32-33, 46, 137: numpy's uniform(low, high) needs low < high to be a range at all
    if (!(c->lowlevel_speed_range[0] < c->lowlevel_speed_range[1])) {
      snprintf(buf, sizeof buf, "target_speed_range must be (low, high) with low < high, got (%g, %g)", c->lowlevel_speed_range[0], c->lowlevel_speed_range[1]);
      return fail(FW_EINVAL);
    }
    if (!(c->lowlevel_height_range[0] < c->lowlevel_height_range[1])) {
      snprintf(buf, sizeof buf, "target_height_range must be (low, high) with low < high, got (%g, %g)", c->lowlevel_height_range[0], c->lowlevel_height_range[1]);
      return fail(FW_EINVAL);
    }
    if (c->num_targets != 0) { snprintf(buf, sizeof buf, "the low-level task has no waypoints: num_targets must be 0, got %d", c->num_targets); return fail(FW_EINVAL); }
    if (c->lowlevel_max_episode_steps <= 0) { snprintf(buf, sizeof buf, "lowlevel_max_episode_steps must be positive, got %d", c->lowlevel_max_episode_steps); return fail(FW_EINVAL); }
    if (c->lowlevel_variant != FW_LL_VARIANT_TRACKING && c->lowlevel_variant != FW_LL_VARIANT_SAC_DEMO) {
      snprintf(buf, sizeof buf, "lowlevel_variant must be 0 (fixedwing_lowlevel_env.py) or 1 (the SAC script's env), got %d", c->lowlevel_variant);
      return fail(FW_EINVAL);
    }
    // the next two words belong to the SAC script's variant alone: the first variant ignores them, as it did while they were reserved
    if (c->lowlevel_variant == FW_LL_VARIANT_SAC_DEMO && c->lowlevel_fixed_heading != 0 && c->lowlevel_fixed_heading != 1) { snprintf(buf, sizeof buf, "lowlevel_fixed_heading must be 0 or 1, got %d", c->lowlevel_fixed_heading); return fail(FW_EINVAL); }
    if (c->lowlevel_variant == FW_LL_VARIANT_SAC_DEMO && !(std::isfinite(c->lowlevel_min_speed) && c->lowlevel_min_speed >= 0.0)) { snprintf(buf, sizeof buf, "lowlevel_min_speed must be finite and >= 0, got %g", c->lowlevel_min_speed); return fail(FW_EINVAL); }
    if (c->physics_hz != 240 || c->control_hz != 120 || c->agent_hz != 120) {
      snprintf(buf, sizeof buf, "the low-level task steps one Aviary step per agent step: physics_hz 240, control_hz 120, agent_hz 120 (got %d, %d, %d)",
               c->physics_hz, c->control_hz, c->agent_hz);
      return fail(FW_EINVAL);
    }
  }
  if (c->dtype != FW_F64 && c->dtype != FW_F32) { snprintf(buf, sizeof buf, "unknown dtype %d", c->dtype); return fail(FW_EINVAL); }
  if (c->num_targets < 0 || c->num_targets > FW_MAX_TARGETS) { snprintf(buf, sizeof buf, "num_targets must be in [0,%d]", FW_MAX_TARGETS); return fail(FW_EINVAL); }
  if (c->task != FW_TASK_OBJLOCK && (c->context_length < 0 || c->context_length > FW_MAX_TARGETS + 1)) { snprintf(buf, sizeof buf, "bad context_length"); return fail(FW_EINVAL); }
  if (c->n_collision_pts < 0 || c->n_collision_pts > FW_MAX_COLLISION_PTS) { snprintf(buf, sizeof buf, "bad n_collision_pts"); return fail(FW_EINVAL); }
  if (c->num_obstacles < 0 || c->num_obstacles > FW_MAX_OBSTACLES) { snprintf(buf, sizeof buf, "bad num_obstacles"); return fail(FW_EINVAL); }
  if (has_camera(c->task) && (c->camera_resolution < 0 || c->camera_resolution > 1024)) { snprintf(buf, sizeof buf, "camera_resolution must be in [1, 1024]"); return fail(FW_EINVAL); }
  if (c->physics_hz <= 0 || c->control_hz <= 0 || c->physics_hz % c->control_hz != 0) { snprintf(buf, sizeof buf, "physics_hz must be a multiple of control_hz"); return fail(FW_EINVAL); }
  if (!(c->mass > 0.0)) { snprintf(buf, sizeof buf, "mass must be > 0"); return fail(FW_EINVAL); }
  if (c->wind_coupling < FW_WIND_COUPLE_NONE || c->wind_coupling > FW_WIND_COUPLE_AIRSPEED) { snprintf(buf, sizeof buf, "bad wind_coupling"); return fail(FW_EINVAL); }
  return FW_OK;
}

// attitude block of the waypoint / camera observations: pose, the last action (direct waypoints: six wide), auxiliary state
int att_dim_of(const fw_config* c) { return (c->angle_representation == 0 ? 12 : 13) + (c->task == FW_TASK_WAYPOINTS_DIRECT ? 6 : 4) + 6; }
int obs_dim_of(const fw_config* c) {
  if (c->task == FW_TASK_LOWLEVEL) return 21;       // fixedwing_lowlevel_env.py:65-66
  const int att = att_dim_of(c);
  if (c->task == FW_TASK_OBJLOCK) return att + 3 + FW_VISION_FEATS * FW_VISION_HIST + (c->duck_vision_no_deltas ? 0 : 4);
  return att + 3 * c->context_length;
}

bool invert3(const double m[9], double inv[9]) {
  double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
  if (det == 0.0) return false;
  double id = 1.0 / det;
  inv[0] = (m[4] * m[8] - m[5] * m[7]) * id; inv[1] = (m[2] * m[7] - m[1] * m[8]) * id; inv[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  inv[3] = (m[5] * m[6] - m[3] * m[8]) * id; inv[4] = (m[0] * m[8] - m[2] * m[6]) * id; inv[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  inv[6] = (m[3] * m[7] - m[4] * m[6]) * id; inv[7] = (m[1] * m[6] - m[0] * m[7]) * id; inv[8] = (m[0] * m[4] - m[1] * m[3]) * id;
  return true;
}

// Geometry of the tick's axis-aligned variant (surface_wrench_ax / physics_tick, AX = true): every lifting surface has fwd = e_x and
// lift = e_y or e_z, and the inertia tensor (hence its inverse, from invert3) is diagonal.  The shipped airframe is.
bool axis_aligned_geometry(const fw_config& c) {
  for (int s = 0; s < FW_NUM_SURFACES; ++s) {
    const double* F = c.surfaces[s].forward_unit;
    const double* L = c.surfaces[s].lift_unit;
    if (!(F[0] == 1.0 && F[1] == 0.0 && F[2] == 0.0)) return false;
    if (!(L[0] == 0.0 && ((L[1] == 1.0 && L[2] == 0.0) || (L[1] == 0.0 && L[2] == 1.0)))) return false;
  }
  const double* I = c.inertia;
  const double m[9] = { I[0], I[3], I[4], I[3], I[1], I[5], I[4], I[5], I[2] };
  double mi[9];
  if (!invert3(m, mi)) return false;
  for (int k : {1, 2, 3, 5, 6, 7})
    if (m[k] != 0.0 || mi[k] != 0.0) return false;
  return true;
}

// Host twin of ShapeTrainWaypoints (fwsim_device.hpp): 1 when fill_params() gives every field that shape compiles in exactly the
// value it compiles in -- the same expressions as there.  Only fields that no call changes after fw_create are in a shape
// (auto_reset is one too, but the kernel reads it once per launch, outside the sub-step loop, and both settings are in use).
int step_shape_of(const fw_config& c) {
  return (c.task == FW_TASK_WAYPOINTS && 120 / c.agent_hz == 4 && c.physics_hz / c.control_hz == 2 && c.context_length == 2 &&
          c.num_targets == 8 && obs_dim_of(&c) == 28 && att_dim_of(&c) == 22 && c.sparse_reward != 0 && c.angle_representation == 0 &&
          c.motor.noise_ratio != 0.0 && c.gyroscopic != 0) ? 1 : 0;
}

// Fold fw_config into the wave-uniform constant block (all derivations in double).
template <typename T>
bool build_params(const fw_config& c, uint64_t seed, int64_t env_offset, Params<T>& P, std::string& err) {
  std::memset(&P, 0, sizeof P);
  const double dt = 1.0 / (double)c.physics_hz;
  const double d2r = kPi / 180.0;
  for (int s = 0; s < FW_NUM_SURFACES; ++s) {
    const fw_surface_params& sp = c.surfaces[s];
    SurfC<T>& o = P.s[s];
    double area = sp.chord * sp.span, AR = sp.span / sp.chord;
    double Cl3 = sp.Cl_alpha_2D * (AR / (AR + ((2.0 * (AR + 4.0)) / (AR + 2.0))));
    double theta_f = std::acos(2.0 * sp.flap_to_chord - 1.0);
    double tau_f = 1.0 - ((theta_f - std::sin(theta_f)) / kPi);
    double a0b = sp.alpha_0_base_deg * d2r, asPb = sp.alpha_stall_P_base_deg * d2r, asNb = sp.alpha_stall_N_base_deg * d2r;
    o.dt_tau = (T)(dt / sp.tau);
    for (int k = 0; k < 3; ++k) { o.lift[k] = (T)sp.lift_unit[k]; o.fwd[k] = (T)sp.forward_unit[k]; o.pos[k] = (T)sp.pos[k]; }
    const double* L = sp.lift_unit; const double* F = sp.forward_unit;
    o.tq[0] = (T)(L[1] * F[2] - L[2] * F[1]); o.tq[1] = (T)(L[2] * F[0] - L[0] * F[2]); o.tq[2] = (T)(L[0] * F[1] - L[1] * F[0]);
    o.hra = (T)(0.5 * c.air_density * area);
    o.chord = (T)sp.chord;
    o.Cl3 = (T)Cl3; o.inv_Cl3 = (T)(1.0 / Cl3); o.inv_piAR = (T)(1.0 / (kPi * AR));
    o.a0b = (T)a0b;
    o.defl_scale = (T)(sp.deflection_limit_deg * d2r);
    o.k_dCl = (T)(Cl3 * tau_f * sp.eta * sp.deflection_limit_deg * d2r);
    o.ClmaxPb = (T)(Cl3 * (asPb - a0b)); o.ClmaxNb = (T)(Cl3 * (asNb - a0b));
    o.ftc = (T)sp.flap_to_chord; o.Cd0 = (T)sp.Cd_0;
    o.k_exp = (T)(0.41 * (1.0 - std::exp(-17.0 / AR)));
  }
  const double max_rpm = std::sqrt(c.motor.total_thrust / c.motor.thrust_coef);
  P.motor_dt_tau = (T)(dt / c.motor.tau);
  P.noise_ratio = (T)c.motor.noise_ratio;
  P.has_noise = c.motor.noise_ratio != 0.0;
  for (int k = 0; k < 3; ++k) {
    P.m_force[k] = (T)(max_rpm * max_rpm * c.motor.thrust_coef * c.motor.thrust_unit[k]);
    P.m_torque[k] = (T)(max_rpm * max_rpm * c.motor.torque_coef * c.motor.thrust_unit[k]);
    P.m_pos[k] = (T)c.motor.pos[k];
  }
  {
    const double f[3] = { max_rpm * max_rpm * c.motor.thrust_coef * c.motor.thrust_unit[0], max_rpm * max_rpm * c.motor.thrust_coef * c.motor.thrust_unit[1], max_rpm * max_rpm * c.motor.thrust_coef * c.motor.thrust_unit[2] };
    const double* r = c.motor.pos;
    const double tq[3] = { max_rpm * max_rpm * c.motor.torque_coef * c.motor.thrust_unit[0], max_rpm * max_rpm * c.motor.torque_coef * c.motor.thrust_unit[1], max_rpm * max_rpm * c.motor.torque_coef * c.motor.thrust_unit[2] };
    P.m_wrench_t[0] = (T)(r[1] * f[2] - r[2] * f[1] + tq[0]);
    P.m_wrench_t[1] = (T)(r[2] * f[0] - r[0] * f[2] + tq[1]);
    P.m_wrench_t[2] = (T)(r[0] * f[1] - r[1] * f[0] + tq[2]);
  }
  for (int a = 0; a < FW_NUM_ACTUATORS; ++a) for (int k = 0; k < 4; ++k) P.mixer[a][k] = (T)c.mixer[a][k];
  P.inv_mass = (T)(1.0 / c.mass); P.gravity = (T)c.gravity;
  const double* I = c.inertia;
  double m[9] = { I[0], I[3], I[4], I[3], I[1], I[5], I[4], I[5], I[2] }, mi[9];
  if (!invert3(m, mi)) { err = "singular inertia"; return false; }
  for (int k = 0; k < 9; ++k) { P.I[k] = (T)m[k]; P.Iinv[k] = (T)mi[k]; }
  for (int i = 0; i < FW_MAX_COLLISION_PTS; ++i) for (int k = 0; k < 3; ++k) P.coll[i][k] = (T)c.collision_pts[i][k];
  P.n_coll = c.n_collision_pts; P.gyroscopic = c.gyroscopic;
  P.dt = (T)dt; P.inv_physics_hz = (T)dt; P.physics_hz_T = (T)c.physics_hz;
  P.dome = (T)c.flight_dome_size; P.reach = (T)c.goal_reach_distance;
  P.min_height = (T)c.waypoint_min_height; P.spawn_hi = (T)(c.waypoint_spawn_size * 0.9);
  {
    double hr = 0.5 * c.start_orn[0], hp = 0.5 * c.start_orn[1], hy = 0.5 * c.start_orn[2];
    double cr = std::cos(hr), sr = std::sin(hr), cp = std::cos(hp), sp = std::sin(hp), cy = std::cos(hy), sy = std::sin(hy);
    P.start_quat[0] = (T)(sr * cp * cy - cr * sp * sy); P.start_quat[1] = (T)(cr * sp * cy + sr * cp * sy);
    P.start_quat[2] = (T)(cr * cp * sy - sr * sp * cy); P.start_quat[3] = (T)(cr * cp * cy + sr * sp * sy);
  }
  for (int k = 0; k < 3; ++k) {
    P.start_pos[k] = (T)c.start_pos[k]; P.start_vel[k] = (T)c.start_vel[k];
    P.wind_base[k] = (T)c.wind_enu_mps[k]; P.wind_amp[k] = (T)c.gust_amp_enu_mps[k];
    for (int j = 0; j < 2; ++j) { P.wind_base_range[k][j] = c.wind_enu_mps_range[k][j]; P.wind_amp_range[k][j] = c.gust_amp_enu_mps_range[k][j]; }
  }
  P.wind_phase = (T)c.gust_phase_rad; P.gust_omega = (T)(2.0 * kPi * c.gust_freq_hz); P.wind_force_coef = (T)c.wind_force_coef;
  P.gust_sd = (T)std::sin((double)P.gust_omega * (double)P.inv_physics_hz); P.gust_cd = (T)std::cos((double)P.gust_omega * (double)P.inv_physics_hz);
  P.wind_mode = c.wind_mode; P.wind_randomize = c.wind_randomize_on_reset; P.wind_randomize_phase = c.wind_randomize_phase;
  P.wind_coupling = (c.wind_mode == FW_WIND_OFF) ? FW_WIND_COUPLE_NONE : c.wind_coupling;
  P.task = c.task; P.angle_repr = c.angle_representation;
  P.att_dim = att_dim_of(&c);
  P.obs_dim = obs_dim_of(&c); P.ctx = c.context_length;
  P.num_targets = c.num_targets; P.sparse = c.sparse_reward; P.auto_reset = c.auto_reset;
  P.max_steps = (int32_t)(c.agent_hz * c.max_duration_seconds);
  P.step_ratio = 120 / c.agent_hz;
  P.ticks_per_aviary = c.physics_hz / c.control_hz;
  P.warmup_aviary_steps = c.warmup_aviary_steps;
  // The warm-up is env-independent iff wind cannot act on the dynamics (throttle
  // stays exactly 0 under a zero setpoint, so motor noise multiplies 0).
  // ObjLock: the camera may capture during the warm-up (cadence), so it is always integrated in-kernel.
  // (direct actuator commands: the same warm-up -- all six commands zero, throttle command zero)
  P.warm_valid = (P.wind_coupling == FW_WIND_COUPLE_NONE && (c.task == FW_TASK_WAYPOINTS || c.task == FW_TASK_WAYPOINTS_DIRECT)) ? 1 : 0;   // (the duck cannot be in contact during warm-up: it spawns >= start height away only by chance; contacts there are ignored by the reference too)
  P.seed_lo = (uint32_t)seed; P.seed_hi = (uint32_t)(seed >> 32);
  P.env_offset = env_offset;
  for (int k = 0; k < 2; ++k) { P.ll_speed[k] = c.lowlevel_speed_range[k]; P.ll_height[k] = c.lowlevel_height_range[k]; }
  P.ll_max_steps = c.lowlevel_max_episode_steps;
  if (P.obs_dim > kMaxObs) { err = "obs_dim exceeds kMaxObs"; return false; }
  return true;
}

// One env kernel as a handle launches it (env_kernels_of below): the host function pointer and what of the launch follows the kernel.
struct EnvKernel {
  const void* fn = nullptr;
  unsigned block = kWave;       // 2 * kWave: a capture wave (its LDS carries the mailbox) or a noise wave (its [kWave][2] normals) beside every step wave: step_lds_bytes_h
  bool worker_half = true;      // step kernels: with shadow_on the second half of the grid are the shadow workers
  bool takes_objc = true;       // reset kernels: the argument list has the ObjC block (the low-level task's has not)
};

}  // namespace

struct fw_env {
  fw_config cfg;
  int32_t n = 0, npad = 0, device = 0;
  int32_t lanes_per_env = 1;    // 1: throughput mapping, 8: latency mapping (see fwsim_device.hpp)
  int32_t g8_waves = 1;         // 8-lane mapping, waypoints task: waves per SIMD the step kernel is built for (1 | 2)
  int32_t capture_wave = 0;     // 8-lane mapping, camera tasks: fw_step workgroups carry a capture wave (fw_step_kernel_obj_g8h)
  int32_t aux_wave = 0;         // the axis-aligned row with motor noise, up to kAuxWaveMaxEnvs envs: a second wave per step workgroup draws the noise (fw_step_kernel_g8x)
  int32_t step_shape = 0;       // the noise-wave row on the headline training config's shape (step_shape_of): that kernel with the shape compiled in (fw_step_kernel_g8xs)
  int32_t obs_wave = 0;         // the fixed-shape row with its second wave kept to the end of the launch: scenario worker of its tile, then the observation rows (fw_step_kernel_g8xo)
  int32_t axis_aligned = 0;     // f64 wind-free waypoints on the 8-lane one-wave build: the tick's axis-aligned variant (axis_aligned_geometry)
  EnvKernel step, reset, collect;   // chosen once by fw_create from the fields above (select_kernels); collect.fn is null where fw_collect_step does not serve
  EnvKernel step_hl;                // fw_step_hl's kernel (hl_step_kernel_of); null where fw_step_hl does not serve
  uint64_t seed = 0;
  int64_t env_offset = 0;
  void* params_dev = nullptr;   // Params<T>
  void* objc_dev = nullptr;     // ObjC<T>
  void* r_dev = nullptr;        // T[RF_COUNT][npad]
  int32_t* i_dev = nullptr;     // i32[IF_COUNT][npad]
  void* rs_dev = nullptr;       // shadow T[RF_COUNT][npad]   (only when shadow_on)
  int32_t* is_dev = nullptr;    // shadow ticks i32[npad]
  void* sobs_dev = nullptr;     // shadow first observations T[npad][obs_dim]
  unsigned long long* sreq_dev = nullptr;   // shadow requests / progress words, u64[npad] each
  unsigned long long* sdone_dev = nullptr;
  uint32_t* lctr_dev = nullptr;             // device-side launch index, one word per workgroup (fwsim_device.hpp: launch_index)
  unsigned long long* stats_dev = nullptr;  // hand-off counters (fw_get_counters)
  double* scen_dev = nullptr;               // staging of a caller-supplied fw_scenario (allocated on first use)
  long long* prof_dev = nullptr; // FW_PROFILE builds only
  int32_t shadow_on = 0;        // background warm-up of the next episode (see shadow_* kernels)
  const void* collect_act_seen = nullptr;   // the action buffer fw_collect_step last filled with "not there yet"
  std::string err;
};

#define HIP_TRY(h, expr)                                                                  \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      std::string m_ = std::string(#expr) + ": " + hipGetErrorString(e_);                 \
      if (h) (h)->err = m_; else g_err = m_;                                              \
      return FW_EHIP;                                                                     \
    }                                                                                     \
  } while (0)

namespace {
struct DeviceGuard {
  int prev = -1; bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) { switched = hipSetDevice(dev) == hipSuccess; }
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

// The learner-side entry points have no handle: the device is the one their buffers live on (never the thread's current
// device), and everything they launch runs under a DeviceGuard for it.
int device_of(const void* p) {
  hipPointerAttribute_t a;
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (p && hipPointerGetAttributes(&a, p) == hipSuccess && a.device >= 0) return a.device;
  (void)hipGetLastError();                     // clear the sticky error of a failed query
  return cur;
}
// Opt `kernel` into `bytes` of dynamic LDS where that is more than the 48 KB a workgroup gets without asking.  The attribute belongs
// to the (device, kernel) pair, not to a handle or a call: keep the maximum ever asked for and only ever raise it, so a later, smaller
// handle cannot lower the cap under an earlier one.  Set when a pair first sees a larger size, never again on the launch path.
int ensure_dynamic_lds(fw_env* h, int device, const void* kernel, size_t bytes) {
  if (bytes <= 48 * 1024) return FW_OK;
  static std::mutex mu;                         // (one thread per process drives launches today; the lock keeps the map whole if two ever do)
  static std::map<std::pair<int, const void*>, size_t> caps;
  std::lock_guard<std::mutex> lock(mu);
  size_t& cap = caps[{device, kernel}];
  if (bytes <= cap) return FW_OK;
  HIP_TRY(h, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  cap = bytes;
  return FW_OK;
}

// From a runtime dtype / lane mapping to template arguments: f gets a value of the type, or the lanes per env as a std::integral_constant.
template <typename F> auto with_real(bool is_f64, F&& f) { return is_f64 ? f(double{}) : f(float{}); }
template <typename F> auto with_dtype(const fw_env* h, F&& f) { return with_real(h->cfg.dtype == FW_F64, f); }
template <typename F> auto with_lanes(const fw_env* h, F&& f) { return h->lanes_per_env == 8 ? f(std::integral_constant<int, 8>{}) : f(std::integral_constant<int, 1>{}); }

template <typename T> size_t tile_bytes(const fw_env* h);
template <typename T> size_t step_lds_bytes(const fw_env* h);
template <typename T> DevState<T> dev_state(fw_env* h) {
  DevState<T> D; D.r = (T*)h->r_dev; D.i = h->i_dev; D.n = h->n; D.npad = h->npad;
  D.rs = (T*)h->rs_dev; D.is = h->is_dev; D.sobs = (T*)h->sobs_dev; D.sreq = h->sreq_dev; D.sdone = h->sdone_dev; D.epoch = 0; D.shadow_on = h->shadow_on;
  D.lctr = h->lctr_dev; D.stats = h->stats_dev;
  D.stash_off = (int32_t)((tile_bytes<T>(h) + 15) & ~(size_t)15);
  D.mbox_off = (int32_t)((step_lds_bytes<T>(h) + 15) & ~(size_t)15);
  FWP(D.prof = h->prof_dev;)
  return D;
}
int invalidate_shadow(fw_env* h) {
  if (!h->shadow_on) return FW_OK;
  HIP_TRY(h, hipDeviceSynchronize());
  HIP_TRY(h, hipMemset(h->sreq_dev, 0xFF, sizeof(unsigned long long) * h->npad));    // ~0 = nothing requested
  HIP_TRY(h, hipMemset(h->sdone_dev, 0xFF, sizeof(unsigned long long) * h->npad));   // episode 0xFFFFFFFF never matches
  HIP_TRY(h, hipMemset(h->is_dev, 0, sizeof(int32_t) * h->npad));
  return FW_OK;
}

// every device buffer of a handle, freed once and nulled (fw_destroy and the error path of fw_create)
void free_device_buffers(fw_env* h) {
  void** bufs[] = { &h->params_dev, &h->objc_dev, &h->r_dev, (void**)&h->i_dev, &h->rs_dev, (void**)&h->is_dev, &h->sobs_dev,
                    (void**)&h->sreq_dev, (void**)&h->sdone_dev, (void**)&h->lctr_dev, (void**)&h->stats_dev, (void**)&h->scen_dev,
                    (void**)&h->prof_dev };
  for (void** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
}

// words per env of the camera's LDS row buffer: the width padded so that the 4 envs of a half-wave start on different banks
inline int zrow_stride_of(int res) { return ((res + 31) / 32) * 32 + 8; }

// LDS bytes: the padded [64/G][D+1] observation tile; the camera tasks on the 8-lane mapping alias it (in time) with the
// row buffer of the analytic camera (1 / t of the nearest cylinder fragment per column), 8 envs x zrow_stride words
template <typename T> size_t tile_bytes(const fw_env* h) {
  size_t b = sizeof(T) * (size_t)(kWave / h->lanes_per_env) * (size_t)(obs_dim_of(&h->cfg) + 1);
  if (has_camera(h->cfg.task) && h->lanes_per_env == 8) {
    const int res = h->cfg.camera_resolution > 0 ? h->cfg.camera_resolution : 128;
    b = std::max(b, cam_lds(sizeof(T), zrow_stride_of(res), res, h->cfg.num_obstacles > 0).total);   // camera map (fwsim_objlock.hpp): 2 KB without, 48 KB with cylinders at 480 columns
  }
  return b;
}
// dynamic LDS of a step launch: the tile (or the camera's map) + the output stash of the envs of a wave
template <typename T> size_t step_lds_bytes(const fw_env* h) { return ((tile_bytes<T>(h) + 15) & ~(size_t)15) + sizeof(double) * 4 * (size_t)(kWave / h->lanes_per_env); }
// ... of a step launch whose workgroups carry a second wave: + the capture mailbox, or the noise wave's [kWave][2] normals in its place (DevState::mbox_off)
// ... and behind the normals, where the second wave writes the observation rows, the step wave's hand-off block ([envs per wave][kObsHandWords], step_body OBSW)
template <typename T> size_t step_lds_bytes_h(const fw_env* h) {
  const size_t hand = h->obs_wave ? sizeof(T) * (size_t)kObsHandWords * (size_t)(kWave / h->lanes_per_env) : 0;
  return ((step_lds_bytes<T>(h) + 15) & ~(size_t)15) + std::max(mbox_bytes(sizeof(T)), sizeof(T) * 2 * (size_t)kWave + hand);
}
inline dim3 grid_of(const fw_env* h) { return dim3((unsigned)(h->npad / (kWave / h->lanes_per_env))); }

// ObjLock task constants (analytic camera axes, shaping coefficients of envs/fixedwing_objlock_env.py:54-80)
template <typename T>
void build_objc(const fw_config& c, ObjC<T>& O) {
  std::memset(&O, 0, sizeof O);
  const double th = c.camera_angle_deg * kPi / 180.0;
  const double f[3] = { std::cos(th), 0.0, std::sin(th) }, r[3] = { 0.0, -1.0, 0.0 };
  const double d[3] = { f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0] };
  for (int k = 0; k < 3; ++k) { O.cam_f[k] = (T)f[k]; O.cam_r[k] = (T)r[k]; O.cam_d[k] = (T)d[k]; O.cam_off[k] = (T)c.camera_offset[k]; }
  const int res = c.camera_resolution > 0 ? c.camera_resolution : 128;
  O.W = O.H = (T)res; O.vmid = (T)(res / 2);
  O.focal = (T)(0.5 * res / std::tan(0.5 * c.camera_fov_deg * kPi / 180.0));
  O.inv_focal = (T)(1.0 / (0.5 * res / std::tan(0.5 * c.camera_fov_deg * kPi / 180.0)));
  O.near_ = (T)c.camera_near; O.far_ = (T)c.camera_far;
  O.inv_near = (T)(1.0 / c.camera_near); O.inv_far = (T)(1.0 / c.camera_far); O.db_c1 = (T)(c.camera_far / (c.camera_far - c.camera_near));
  O.zrow_stride = zrow_stride_of(res);
  O.duck_radius = (T)(c.duck_radius_per_scale * c.duck_global_scaling); O.half_dome = (T)(c.flight_dome_size / 2.0);
  O.obst_radius = (T)c.obstacle_radius; O.obst_hmin = (T)c.obstacle_height_range[0]; O.obst_hmax = (T)c.obstacle_height_range[1];
  O.safe_dist = (T)c.obstacle_safe_distance_m; O.avoid_scale = (T)c.obstacle_avoid_reward_scale; O.avoid_max = (T)c.obstacle_avoid_max_penalty;
  O.k_dist = (T)c.duck_distance_reward_scale; O.lock_radius = (T)c.duck_lock_center_radius; O.k_center = (T)c.duck_centering_reward_scale;
  O.k_visible = (T)c.duck_visible_step_reward; O.k_area = (T)c.duck_area_reward_scale; O.lost_penalty = (T)c.duck_lock_lost_penalty;
  O.approach_clip = (T)c.duck_approach_reward_clip_m; O.k_approach = (T)c.duck_approach_reward_scale;
  O.strike_dist = (T)c.duck_strike_distance_m; O.strike_reward = (T)c.duck_strike_reward; O.lock_step_reward = (T)c.duck_lock_step_reward;
  O.hold_steps = c.duck_lock_hold_steps; O.decay_steps = c.duck_lock_decay_steps; O.num_obstacles = c.num_obstacles;
  O.camera_ratio_ticks = (c.physics_hz / c.control_hz) * c.duck_camera_capture_interval_steps;
  O.switch_min_area = (T)c.duck_switch_min_area; O.switch_min_seen = c.duck_switch_min_consecutive_seen;
  {
    double rm = 0.0;
    for (int i = 0; i < c.n_collision_pts; ++i) { const double* q = c.collision_pts[i]; rm = std::max(rm, std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])); }
    O.reach_margin = (T)(rm + 0.25);
  }
}

template <typename T>
int upload_params(fw_env* h) {
  Params<T> P;
  if (!build_params<T>(h->cfg, h->seed, h->env_offset, P, h->err)) return FW_EINVAL;
  if (!h->params_dev) HIP_TRY(h, hipMalloc(&h->params_dev, lld_consts_offset<T>() + sizeof(LldC<T>)));     // Params, then the step image, then the low-level variant's constants
  HIP_TRY(h, hipMemcpy(h->params_dev, &P, sizeof P, hipMemcpyHostToDevice));
  const LldC<T> LC = { (T)h->cfg.lowlevel_min_speed, h->cfg.lowlevel_fixed_heading };
  HIP_TRY(h, hipMemcpy((unsigned char*)h->params_dev + lld_consts_offset<T>(), &LC, sizeof LC, hipMemcpyHostToDevice));
  ObjC<T> OC;
  build_objc<T>(h->cfg, OC);
  if (!h->objc_dev) HIP_TRY(h, hipMalloc(&h->objc_dev, sizeof(ObjC<T>)));
  HIP_TRY(h, hipMemcpy(h->objc_dev, &OC, sizeof OC, hipMemcpyHostToDevice));
  if (P.warm_valid) {
    hipLaunchKernelGGL(fw_warm_kernel<T>, dim3(1), dim3(kWave), 0, 0, (Params<T>*)h->params_dev);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipDeviceSynchronize());
  }
  // The step image follows Params: it is refilled wherever Params is written, and this function is the only place (fw_create and
  // fw_seed; fw_set_state, fw_reset and the command paths write state rows, never Params).  Read by the fixed-shape step kernel alone,
  // which exists in f64 only.
  if constexpr (std::is_same<T, double>::value) {
    hipLaunchKernelGGL(fw_step_image_kernel<T>, dim3(1), dim3(kWave), 0, 0, (Params<T>*)h->params_dev);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipDeviceSynchronize());
  }
  return FW_OK;
}

// ---- which kernels a handle launches: one table, looked up once by fw_create (select_kernels) ----
// A key names the fields of a handle that the choice depends on; kAny in a row matches every value.  The first row that matches
// wins, so a special case stands above the general one.  A new kernel variant is one new row.
constexpr int kAny = -1;
struct KernelKey { int task, lanes, waves, windy, axis_aligned, capture_wave, aux_wave, step_shape, obs_wave, variant; };   // variant: fw_config.lowlevel_variant
struct KernelRow { KernelKey key; EnvKernel step, reset, collect; };
template <typename... A> const void* kfn(void (*kernel)(A...)) { return (const void*)kernel; }      // the host-side pointer hipLaunchKernel takes
// The argument lists step_T / collect_step_T / reset_T build.  hipLaunchKernel takes them unchecked, so a kernel enters the table
// through the function of its family: a row whose kernel takes anything else does not compile.
template <typename T> using StepFn = void (*)(const Params<T>*, const ObjC<T>*, DevState<T>, const T*, T*, T*, uint8_t*, uint8_t*, T*, int32_t*);
template <typename T> using CollectFn = void (*)(const Params<T>*, const ObjC<T>*, DevState<T>, const T*, T*, T*, uint8_t*, uint8_t*, T*, int32_t*, CollectArgs);
template <typename T> using ResetFn = void (*)(const Params<T>*, const ObjC<T>*, DevState<T>, const uint8_t*, T*, int, ScenOv);
template <typename T> using ResetLLFn = void (*)(const Params<T>*, DevState<T>, const uint8_t*, T*, int, ScenOv);
template <typename T> EnvKernel step_k(StepFn<T> f) { return {kfn(f)}; }
template <typename T> EnvKernel two_wave(StepFn<T> f) { return {kfn(f), 2 * kWave, false}; }       // step wave + capture wave per workgroup (the capture wave is the worker)
template <typename T> EnvKernel noise_wave(StepFn<T> f) { return {kfn(f), 2 * kWave, true}; }       // step wave + noise wave per workgroup; the scenario workers stay the grid's second half
template <typename T> EnvKernel collect_k(CollectFn<T> f) { return {kfn(f)}; }
template <typename T> EnvKernel reset_k(ResetFn<T> f) { return {kfn(f)}; }
template <typename T> EnvKernel no_objc(ResetLLFn<T> f) { return {kfn(f), kWave, true, false}; }
// The axis-aligned tick exists in f64 only: its float row holds no kernel, and select_kernels refuses a handle that lands on it.
template <typename T> EnvKernel axis_aligned_step_kernel() {
  if constexpr (std::is_same<T, double>::value) return step_k<T>(fw_step_kernel_g8<T, false, true>); else return {};
}
// ... and so does its build with a noise wave
template <typename T> EnvKernel aux_wave_step_kernel() {
  if constexpr (std::is_same<T, double>::value) return noise_wave<T>(fw_step_kernel_g8x<T>); else return {};
}
// ... and that one compiled for the headline training config's shape
template <typename T> EnvKernel step_shape_step_kernel() {
  if constexpr (std::is_same<T, double>::value) return noise_wave<T>(fw_step_kernel_g8xs<T>); else return {};
}
// ... and that one with the second wave as scenario worker and observation writer: the grid has no worker half (the two-wave launch shape of the capture wave)
template <typename T> EnvKernel obs_wave_step_kernel() {
  if constexpr (std::is_same<T, double>::value) return two_wave<T>(fw_step_kernel_g8xo<T>); else return {};
}
// (fw_collect_step: the four-action tasks on the 8-lane mapping -- collect_fill says so to the others; general tick, no capture wave)
template <typename T> const KernelRow* env_kernels_of(const KernelKey& q) {
  constexpr int LL = FW_TASK_LOWLEVEL, WD = FW_TASK_WAYPOINTS_DIRECT, OBJ = FW_TASK_OBJLOCK, COMB = FW_TASK_WAYPOINT_OBJLOCK, WP = FW_TASK_WAYPOINTS;
  static const KernelRow rows[] = {
    // task lanes waves windy axis  capture aux   shape obsw  variant  fw_step                                                      fw_reset / fw_observe                                fw_collect_step
    {{LL,   8, kAny, 1,    kAny, kAny, kAny, kAny, kAny, 1   }, step_k<T>(fw_step_kernel_ll<T, 8, true, 1>),       no_objc<T>(fw_reset_kernel_ll<T, 8, 1>),      {}},
    {{LL,   8, kAny, 0,    kAny, kAny, kAny, kAny, kAny, 1   }, step_k<T>(fw_step_kernel_ll<T, 8, false, 1>),      no_objc<T>(fw_reset_kernel_ll<T, 8, 1>),      {}},
    {{LL,   1, kAny, 1,    kAny, kAny, kAny, kAny, kAny, 1   }, step_k<T>(fw_step_kernel_ll<T, 1, true, 1>),       no_objc<T>(fw_reset_kernel_ll<T, 1, 1>),      {}},
    {{LL,   1, kAny, 0,    kAny, kAny, kAny, kAny, kAny, 1   }, step_k<T>(fw_step_kernel_ll<T, 1, false, 1>),      no_objc<T>(fw_reset_kernel_ll<T, 1, 1>),      {}},
    {{LL,   8, kAny, 1,    kAny, kAny, kAny, kAny, kAny, 0   }, step_k<T>(fw_step_kernel_ll<T, 8, true, 0>),       no_objc<T>(fw_reset_kernel_ll<T, 8, 0>),      {}},
    {{LL,   8, kAny, 0,    kAny, kAny, kAny, kAny, kAny, 0   }, step_k<T>(fw_step_kernel_ll<T, 8, false, 0>),      no_objc<T>(fw_reset_kernel_ll<T, 8, 0>),      {}},
    {{LL,   1, kAny, 1,    kAny, kAny, kAny, kAny, kAny, 0   }, step_k<T>(fw_step_kernel_ll<T, 1, true, 0>),       no_objc<T>(fw_reset_kernel_ll<T, 1, 0>),      {}},
    {{LL,   1, kAny, 0,    kAny, kAny, kAny, kAny, kAny, 0   }, step_k<T>(fw_step_kernel_ll<T, 1, false, 0>),      no_objc<T>(fw_reset_kernel_ll<T, 1, 0>),      {}},
    {{WD,   8, kAny, 1,    kAny, kAny, kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_wd<T, 8, true, WD_HELD>),  reset_k<T>(fw_reset_kernel_wd<T, 8>),         {}},
    {{WD,   8, kAny, 0,    kAny, kAny, kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_wd<T, 8, false, WD_HELD>), reset_k<T>(fw_reset_kernel_wd<T, 8>),         {}},
    {{WD,   1, kAny, 1,    kAny, kAny, kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_wd<T, 1, true, WD_HELD>),  reset_k<T>(fw_reset_kernel_wd<T, 1>),         {}},
    {{WD,   1, kAny, 0,    kAny, kAny, kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_wd<T, 1, false, WD_HELD>), reset_k<T>(fw_reset_kernel_wd<T, 1>),         {}},
    {{OBJ,  8, kAny, kAny, kAny, 1,    kAny, kAny, kAny, kAny}, two_wave<T>(fw_step_kernel_obj_g8h<T, OBJ>),      reset_k<T>(fw_reset_kernel<T, 8, OBJ>),       collect_k<T>(fw_collect_kernel_obj_g8<T, OBJ>)},
    {{OBJ,  8, kAny, kAny, kAny, 0,    kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_obj_g8<T, OBJ>),         reset_k<T>(fw_reset_kernel<T, 8, OBJ>),       collect_k<T>(fw_collect_kernel_obj_g8<T, OBJ>)},
    {{OBJ,  1, kAny, kAny, kAny, kAny, kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_obj_g1<T, OBJ>),         reset_k<T>(fw_reset_kernel<T, 1, OBJ>),       {}},
    {{COMB, 8, kAny, kAny, kAny, 1,    kAny, kAny, kAny, kAny}, two_wave<T>(fw_step_kernel_obj_g8h<T, COMB>),     reset_k<T>(fw_reset_kernel<T, 8, COMB>),      collect_k<T>(fw_collect_kernel_obj_g8<T, COMB>)},
    {{COMB, 8, kAny, kAny, kAny, 0,    kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_obj_g8<T, COMB>),        reset_k<T>(fw_reset_kernel<T, 8, COMB>),      collect_k<T>(fw_collect_kernel_obj_g8<T, COMB>)},
    {{COMB, 1, kAny, kAny, kAny, kAny, kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_obj_g1<T, COMB>),        reset_k<T>(fw_reset_kernel<T, 1, COMB>),      {}},
    {{WP,   8, 1,    0,    1,    kAny, 1,    1,    1,    kAny}, obs_wave_step_kernel<T>(),                        reset_k<T>(fw_reset_kernel<T, 8, WP>),        collect_k<T>(fw_collect_kernel_g8<T, false>)},
    {{WP,   8, 1,    0,    1,    kAny, 1,    1,    kAny, kAny}, step_shape_step_kernel<T>(),                      reset_k<T>(fw_reset_kernel<T, 8, WP>),        collect_k<T>(fw_collect_kernel_g8<T, false>)},
    {{WP,   8, 1,    0,    1,    kAny, 1,    kAny, kAny, kAny}, aux_wave_step_kernel<T>(),                        reset_k<T>(fw_reset_kernel<T, 8, WP>),        collect_k<T>(fw_collect_kernel_g8<T, false>)},
    {{WP,   8, 1,    0,    1,    kAny, kAny, kAny, kAny, kAny}, axis_aligned_step_kernel<T>(),                    reset_k<T>(fw_reset_kernel<T, 8, WP>),        collect_k<T>(fw_collect_kernel_g8<T, false>)},
    {{WP,   8, 2,    1,    kAny, kAny, kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_g8w2<T, true>),          reset_k<T>(fw_reset_kernel<T, 8, WP>),        collect_k<T>(fw_collect_kernel_g8w2<T, true>)},
    {{WP,   8, 2,    0,    kAny, kAny, kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_g8w2<T, false>),         reset_k<T>(fw_reset_kernel<T, 8, WP>),        collect_k<T>(fw_collect_kernel_g8w2<T, false>)},
    {{WP,   8, 1,    1,    kAny, kAny, kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_g8<T, true>),            reset_k<T>(fw_reset_kernel<T, 8, WP>),        collect_k<T>(fw_collect_kernel_g8<T, true>)},
    {{WP,   8, 1,    0,    kAny, kAny, kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_g8<T, false>),           reset_k<T>(fw_reset_kernel<T, 8, WP>),        collect_k<T>(fw_collect_kernel_g8<T, false>)},
    {{WP,   1, kAny, 1,    kAny, kAny, kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_g1<T, true>),            reset_k<T>(fw_reset_kernel<T, 1, WP>),        {}},
    {{WP,   1, kAny, 0,    kAny, kAny, kAny, kAny, kAny, kAny}, step_k<T>(fw_step_kernel_g1<T, false>),           reset_k<T>(fw_reset_kernel<T, 1, WP>),        {}},
  };
  auto fits = [](int row, int v) { return row == kAny || row == v; };
  for (const KernelRow& r : rows)
    if (const KernelKey& k = r.key; fits(k.task, q.task) && fits(k.lanes, q.lanes) && fits(k.waves, q.waves) && fits(k.windy, q.windy) &&
                                    fits(k.axis_aligned, q.axis_aligned) && fits(k.capture_wave, q.capture_wave) && fits(k.aux_wave, q.aux_wave) &&
                                    fits(k.step_shape, q.step_shape) && fits(k.obs_wave, q.obs_wave) && fits(k.variant, q.variant)) return &r;
  return nullptr;
}

// The handle's kernels, from the fields fw_create has just fixed.  A combination without a row (or whose row holds no step or
// reset kernel) is an error here, not a launch that silently does nothing.
template <typename T> int select_kernels(fw_env* h) {
  const KernelKey q = { h->cfg.task, h->lanes_per_env, h->g8_waves, h->cfg.wind_mode != FW_WIND_OFF ? 1 : 0, h->axis_aligned, h->capture_wave, h->aux_wave, h->step_shape, h->obs_wave,
                        h->cfg.task == FW_TASK_LOWLEVEL ? h->cfg.lowlevel_variant : 0 };
  const KernelRow* r = env_kernels_of<T>(q);
  if (!r || !r->step.fn || !r->reset.fn) {
    h->err = "no kernel is built for (task, dtype, lanes per env, waves per SIMD, wind, axis_aligned, capture_wave, aux_wave, step_shape, obs_wave, lowlevel_variant) =";
    for (int x : { q.task, h->cfg.dtype, q.lanes, q.waves, q.windy, q.axis_aligned, q.capture_wave, q.aux_wave, q.step_shape, q.obs_wave, q.variant }) h->err += " " + std::to_string(x);
    return FW_EUNSUPPORTED;
  }
  h->step = r->step; h->reset = r->reset; h->collect = r->collect;
  return FW_OK;
}

// fw_step_hl's kernels, a table of their own: the direct-command waypoints task with the euler attitude (fw_command_hl's rule), by
// lane mapping and wind.  Any other handle holds no kernel, and fw_step_hl says so.
struct HlStepRow { int lanes, windy; EnvKernel step; };
template <typename T> using HlStepFn = void (*)(const Params<T>*, const ObjC<T>*, DevState<T>, fwsim_ctl::CtlArgs, T*, T*, uint8_t*, uint8_t*, T*, int32_t*);
template <typename T> EnvKernel hl_step_k(HlStepFn<T> f) { return {kfn(f)}; }
template <typename T> EnvKernel hl_step_kernel_of(const fw_env* h) {
  static const HlStepRow rows[] = {
    {8, 1, hl_step_k<T>(fw_step_kernel_wd<T, 8, true, WD_CTL>)}, {8, 0, hl_step_k<T>(fw_step_kernel_wd<T, 8, false, WD_CTL>)},
    {1, 1, hl_step_k<T>(fw_step_kernel_wd<T, 1, true, WD_CTL>)}, {1, 0, hl_step_k<T>(fw_step_kernel_wd<T, 1, false, WD_CTL>)},
  };
  if (h->cfg.task != FW_TASK_WAYPOINTS_DIRECT || h->cfg.angle_representation != 0) return {};
  const int windy = h->cfg.wind_mode != FW_WIND_OFF ? 1 : 0;
  for (const HlStepRow& r : rows) if (r.lanes == h->lanes_per_env && r.windy == windy) return r.step;
  return {};
}
// dynamic LDS of an fw_step_hl launch: the observation tile, then the controller's statistics, (8 lanes per env) its policy net, and
// one activation row per env of the wave
template <typename T> size_t hl_step_lds_bytes(const fw_env* h) {
  return ((tile_bytes<T>(h) + 15) & ~(size_t)15) + fwsim_ctl::ctl_lds_bytes(kWave / h->lanes_per_env, h->lanes_per_env == 8);
}

template <typename T>
int create_T(fw_env* h) {
  const size_t npad = (size_t)h->npad;
  int rc = select_kernels<T>(h);
  if (rc != FW_OK) return rc;
  h->step_hl = hl_step_kernel_of<T>(h);
  if (h->step_hl.fn && (rc = ensure_dynamic_lds(h, h->device, h->step_hl.fn, hl_step_lds_bytes<T>(h))) != FW_OK) return rc;
  HIP_TRY(h, hipMalloc(&h->r_dev, sizeof(T) * RF_COUNT * npad));
  HIP_TRY(h, hipMalloc((void**)&h->i_dev, sizeof(int32_t) * IF_COUNT * npad));
  rc = upload_params<T>(h);
  if (rc != FW_OK) return rc;
  const size_t nctr = 2 * (size_t)grid_of(h).x;              // step workgroups + (possibly) as many workers
  HIP_TRY(h, hipMalloc((void**)&h->lctr_dev, sizeof(uint32_t) * nctr));
  HIP_TRY(h, hipMemset(h->lctr_dev, 0, sizeof(uint32_t) * nctr));
  HIP_TRY(h, hipMalloc((void**)&h->stats_dev, sizeof(unsigned long long) * FW_CTR_DIM));
  HIP_TRY(h, hipMemset(h->stats_dev, 0, sizeof(unsigned long long) * FW_CTR_DIM));
  // shadow warm-up whenever the reset warm-up cannot be cached (wind acting on the dynamics, camera tasks)
  const bool cached = (h->cfg.task == FW_TASK_WAYPOINTS) &&
                      (h->cfg.wind_mode == FW_WIND_OFF || h->cfg.wind_coupling == FW_WIND_COUPLE_NONE);
  h->shadow_on = (!cached && h->cfg.auto_reset && !direct_actions(h->cfg.task) && !getenv("FWSIM_NO_SHADOW")) ? 1 : 0;   // (low-level: no warm-up to hand off; direct waypoints: resets run in the kernel)
  // wind-free waypoints on the latency mapping: workers only pre-sample the next episode's waypoints (scenario_worker)
  if (h->cfg.task == FW_TASK_WAYPOINTS && h->cfg.wind_mode == FW_WIND_OFF && h->cfg.auto_reset && h->lanes_per_env == 8 &&
      !getenv("FWSIM_NO_SHADOW"))
    h->shadow_on = 2;
  if (h->shadow_on) {
    HIP_TRY(h, hipMalloc(&h->rs_dev, sizeof(T) * RF_COUNT * npad));
    HIP_TRY(h, hipMemset(h->rs_dev, 0, sizeof(T) * RF_COUNT * npad));
    HIP_TRY(h, hipMalloc((void**)&h->is_dev, sizeof(int32_t) * npad));
    HIP_TRY(h, hipMalloc(&h->sobs_dev, sizeof(T) * (size_t)npad * (size_t)obs_dim_of(&h->cfg)));
    HIP_TRY(h, hipMemset(h->sobs_dev, 0, sizeof(T) * (size_t)npad * (size_t)obs_dim_of(&h->cfg)));
    HIP_TRY(h, hipMalloc((void**)&h->sreq_dev, sizeof(unsigned long long) * npad));
    HIP_TRY(h, hipMalloc((void**)&h->sdone_dev, sizeof(unsigned long long) * npad));
    rc = invalidate_shadow(h);
    if (rc != FW_OK) return rc;
  }
  // the camera's LDS map outgrows 48 KB from ~480 columns with cylinders on: opt in what this handle launches (the size, for every handle: the largest step launch, with the capture wave's mailbox)
  const size_t lds = step_lds_bytes_h<T>(h);
  if (lds > 160 * 1024) { h->err = "camera_resolution x num_obstacles needs more LDS than a CU has"; return FW_EINVAL; }
  for (const EnvKernel* k : {&h->step, &h->reset}) if ((rc = ensure_dynamic_lds(h, h->device, k->fn, lds)) != FW_OK) return rc;
  hipLaunchKernelGGL(fw_init_kernel<T>, dim3((h->npad + 255) / 256), dim3(256), 0, 0, dev_state<T>(h), kWave / h->lanes_per_env);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipDeviceSynchronize());
  return FW_OK;
}

// The argument lists of the env kernels (FW_STEP_ARGS and the reset kernels' own), launched through the pointer the handle holds.
template <typename T>
int step_T(fw_env* h, const void* actions, void* obs, void* reward, uint8_t* term, uint8_t* trunc, void* tobs,
           int32_t* info, hipStream_t st) {
  const EnvKernel& k = h->step;
  dim3 grid = grid_of(h);
  if (h->shadow_on && k.worker_half) grid.x *= 2;          // second half of the grid = shadow workers (two-wave workgroups: the capture wave is the worker)
  const Params<T>* Pp = (const Params<T>*)h->params_dev; const ObjC<T>* OCp = (const ObjC<T>*)h->objc_dev;
  DevState<T> D = dev_state<T>(h);
  void* args[] = { &Pp, &OCp, &D, &actions, &obs, &reward, &term, &trunc, &tobs, &info };
  (void)hipLaunchKernel(k.fn, grid, dim3(k.block), args, k.block == 2 * kWave ? step_lds_bytes_h<T>(h) : step_lds_bytes<T>(h), st);
  HIP_TRY(h, hipGetLastError());
  return FW_OK;
}

template <typename T>
int reset_T(fw_env* h, const uint8_t* mask, void* obs, int do_reset, hipStream_t st, ScenOv ov = ScenOv{}) {
  const EnvKernel& k = h->reset;
  const Params<T>* Pp = (const Params<T>*)h->params_dev; const ObjC<T>* OCp = (const ObjC<T>*)h->objc_dev;
  DevState<T> D = dev_state<T>(h);
  void* with_objc[] = { &Pp, &OCp, &D, &mask, &obs, &do_reset, &ov };
  void* without[] = { &Pp, &D, &mask, &obs, &do_reset, &ov };
  (void)hipLaunchKernel(k.fn, grid_of(h), dim3(k.block), k.takes_objc ? with_objc : without, tile_bytes<T>(h), st);
  HIP_TRY(h, hipGetLastError());
  return FW_OK;
}

// canonical record <-> SoA field maps
struct FieldMap { int rec; int rf; int count; };
const FieldMap kRealMap[] = {
  {FW_S_POS, RF_POS, 3}, {FW_S_QUAT, RF_QUAT, 4}, {FW_S_VEL, RF_VEL, 3}, {FW_S_OMEGA, RF_OMEGA, 3},
  {FW_S_ACT, RF_ACT, 6}, {FW_S_ACTION, RF_ACTION, 4}, {FW_S_NEW_DIST, RF_NEW_DIST, 1}, {FW_S_WIND, RF_WIND, 7},
  {FW_S_EP_RETURN, RF_EP_RETURN, 1}, {FW_S_TARGETS, RF_TARGETS, 3 * FW_MAX_TARGETS},
  {FW_S_TASK, RF_TASK, FW_STATE_DIM - FW_S_TASK},
};
const FieldMap kIntMap[] = {
  {FW_S_STEP_COUNT, IF_STEP, 1}, {FW_S_TICK_COUNT, IF_TICK, 1}, {FW_S_EPISODE, IF_EPISODE, 1},
  {FW_S_FLAGS, IF_FLAGS, 1}, {FW_S_NUM_REACHED, IF_NUM_REACHED, 1},
};

template <typename T>
int get_state_T(fw_env* h, double* out) {
  const size_t npad = (size_t)h->npad;
  const int tile = kWave / h->lanes_per_env;
  std::vector<T> r(RF_COUNT * npad);
  std::vector<int32_t> iv(IF_COUNT * npad);
  HIP_TRY(h, hipDeviceSynchronize());
  HIP_TRY(h, hipMemcpy(r.data(), h->r_dev, sizeof(T) * r.size(), hipMemcpyDeviceToHost));
  HIP_TRY(h, hipMemcpy(iv.data(), h->i_dev, sizeof(int32_t) * iv.size(), hipMemcpyDeviceToHost));
  for (int e = 0; e < h->n; ++e) {
    double* rec = out + (size_t)e * FW_STATE_DIM;
    std::memset(rec, 0, sizeof(double) * FW_STATE_DIM);
    for (const FieldMap& f : kRealMap) for (int k = 0; k < f.count; ++k) rec[f.rec + k] = (double)r[tile_index(tile, RF_COUNT, f.rf + k, e)];
    for (const FieldMap& f : kIntMap) rec[f.rec] = (double)iv[tile_index(tile, IF_COUNT, f.rf, e)];
  }
  return FW_OK;
}

template <typename T>
int set_state_T(fw_env* h, const double* in) {
  const size_t npad = (size_t)h->npad;
  const int tile = kWave / h->lanes_per_env;
  std::vector<T> r(RF_COUNT * npad, (T)0);
  std::vector<int32_t> iv(IF_COUNT * npad, 0);
  HIP_TRY(h, hipDeviceSynchronize());
  HIP_TRY(h, hipMemcpy(r.data(), h->r_dev, sizeof(T) * r.size(), hipMemcpyDeviceToHost));
  HIP_TRY(h, hipMemcpy(iv.data(), h->i_dev, sizeof(int32_t) * iv.size(), hipMemcpyDeviceToHost));
  for (int e = 0; e < h->n; ++e) {
    const double* rec = in + (size_t)e * FW_STATE_DIM;
    for (const FieldMap& f : kRealMap) for (int k = 0; k < f.count; ++k) r[tile_index(tile, RF_COUNT, f.rf + k, e)] = (T)rec[f.rec + k];
    for (const FieldMap& f : kIntMap) iv[tile_index(tile, IF_COUNT, f.rf, e)] = (int32_t)rec[f.rec];
  }
  HIP_TRY(h, hipMemcpy(h->r_dev, r.data(), sizeof(T) * r.size(), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(h->i_dev, iv.data(), sizeof(int32_t) * iv.size(), hipMemcpyHostToDevice));
  return FW_OK;
}
}  // namespace

namespace {
// The learner's kernels: one lookup per family, used by the launch and by the LDS opt-in in front of it.
// (form 1: the diagnostics form of the same row -- fw_ppo_update_diag; form 2: the KL-stop form -- fw_ppo_update_kl; the plain entry
// points never ask for either)
enum { PPO_FORM_PLAIN = 0, PPO_FORM_DIAG = 1, PPO_FORM_KL = 2 };
const void* ppo_update_kernel(int act_dim, int ch /*samples per pass*/, int ns /*blocks per network of the reduce-scatter form, 0: all-to-all*/, int form = PPO_FORM_PLAIN) {
  struct Row { int ch, ns; const void* a4; const void* a6; const void* a3; const void* d4; const void* d6; const void* d3; const void* k4; const void* k6; const void* k3; };
#define FW_PPO_ROW(CH, NS) {CH, NS, kfn(fw_ppo_update_kernel<CH, NS>), kfn(fw_ppo_update_kernel_a6<CH, NS>), kfn(fw_ppo_update_kernel_a3<CH, NS>), \
                            kfn(fw_ppo_update_diag_kernel<CH, NS, 4>), kfn(fw_ppo_update_diag_kernel<CH, NS, 6>), kfn(fw_ppo_update_diag_kernel<CH, NS, 3>), \
                            kfn(fw_ppo_update_kl_kernel<CH, NS, 4>), kfn(fw_ppo_update_kl_kernel<CH, NS, 6>), kfn(fw_ppo_update_kl_kernel<CH, NS, 3>)}
  static const Row rows[] = {
    FW_PPO_ROW(64, 8), FW_PPO_ROW(64, 4), FW_PPO_ROW(64, 0), FW_PPO_ROW(32, 8), FW_PPO_ROW(32, 4), FW_PPO_ROW(32, 0),
    FW_PPO_ROW(16, 8), FW_PPO_ROW(16, 4), FW_PPO_ROW(16, 0),
  };
#undef FW_PPO_ROW
  for (const Row& r : rows) if (r.ch == ch && r.ns == ns)
    return form == PPO_FORM_KL ? (act_dim == 6 ? r.k6 : act_dim == 3 ? r.k3 : r.k4)
         : form == PPO_FORM_DIAG ? (act_dim == 6 ? r.d6 : act_dim == 3 ? r.d3 : r.d4) : (act_dim == 6 ? r.a6 : act_dim == 3 ? r.a3 : r.a4);
  return nullptr;
}
// the pre-pass that packs the rows, and the entry point that sizes the workspace (for the message), by action width
struct PpoWidth { int act_dim; const void* pack; const char* ws_fn; };
const PpoWidth* ppo_width(int act_dim) {
  static const PpoWidth rows[] = {
    {4, kfn(fw_ppo_pack_kernel), "fw_ppo_update_workspace_bytes(n_minibatches, batch_size, obs_dim)"},
    {6, kfn(fw_ppo_pack_kernel_a6), "fw_ppo_update_workspace_bytes_a(n_minibatches, batch_size, obs_dim, act_dim)"},
    {3, kfn(fw_ppo_pack_kernel_a3), "fw_ppo_update_workspace_bytes_a3(n_minibatches, batch_size, obs_dim)"},
  };
  for (const PpoWidth& r : rows) if (r.act_dim == act_dim) return &r;
  return nullptr;
}
const void* policy_act_kernel(int act_dim) { return act_dim == 6 ? kfn(fw_policy_act_kernel<6>) : kfn(fw_policy_act_kernel<4>); }

// fw_policy_act, fw_collect_act and fw_policy_terminal_value: the same launch over N rows, under the caller's DeviceGuard for `dev`
int launch_policy_act(int dev, int act_dim, ActArgs& A, size_t lds, hipStream_t st) {
  const void* fn = policy_act_kernel(act_dim);
  if (int rc = ensure_dynamic_lds(nullptr, dev, fn, lds)) return rc;
  void* args[] = { &A };
  (void)hipLaunchKernel(fn, dim3((A.N + kPChunk - 1) / kPChunk, 2), dim3(kPThreads), args, lds, st);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}
}  // namespace

// ---- fw_collect_step: one launch per vec-step (fwsim_fused.hpp) ----
namespace {
struct CollectWs { size_t part1, tot, flag_p, flag_v, sync, total; };
CollectWs collect_ws(const fw_env* h) {
  const size_t PW = 2 * (size_t)obs_dim_of(&h->cfg) + 2, nblk = (size_t)h->npad / 8, nch = ((size_t)h->n + kCRows - 1) / kCRows;
  CollectWs w; size_t o = 0;
  w.part1 = o; o += sizeof(double) * PW * kCGroups * ((nblk + kCGroups - 1) / kCGroups);
  w.tot = o; o += sizeof(double) * PW;
  w.flag_p = o; o += sizeof(unsigned int) * nch;
  w.flag_v = o; o += sizeof(unsigned int) * nch;
  o = (o + 63) & ~(size_t)63;
  w.sync = o; o += sizeof(unsigned int) * 16;                 // the last 64 bytes of the workspace: CS_* words (status = word 3)
  w.total = o;
  return w;
}
template <typename T>
int collect_step_T(fw_env* h, CollectArgs& CA, const void* actions, void* obs, void* reward, uint8_t* term, uint8_t* trunc, void* tobs,
                   int32_t* info, hipStream_t st) {
  const size_t lds = std::max(step_lds_bytes<T>(h), collect_act_lds_bytes(CA.A.D));
  if (lds > 160 * 1024) { h->err = "fw_collect_step: the networks do not fit the LDS next to the step kernel's tile"; return FW_EINVAL; }
  if (int rc = ensure_dynamic_lds(h, h->device, h->collect.fn, lds)) return rc;      // (here, not at fw_create: the size follows the policy's width)
  CA.n_workers = (int32_t)(grid_of(h).x * (h->shadow_on ? 2u : 1u));
  dim3 grid((unsigned)(CA.n_act + CA.n_workers + 2 * CA.A.D + 2));          // + one fold wave per partial-sum word
  const Params<T>* Pp = (const Params<T>*)h->params_dev; const ObjC<T>* OCp = (const ObjC<T>*)h->objc_dev;
  DevState<T> D = dev_state<T>(h);
  void* args[] = { &Pp, &OCp, &D, &actions, &obs, &reward, &term, &trunc, &tobs, &info, &CA };
  (void)hipLaunchKernel(h->collect.fn, grid, dim3(h->collect.block), args, lds, st);
  HIP_TRY(h, hipGetLastError());
  return FW_OK;
}
}  // namespace


// ======================================================================
// C ABI
// ======================================================================
extern "C" {

int32_t fw_sizeof_config(void) { return (int32_t)sizeof(fw_config); }
int32_t fw_abi_version(void) { return FW_ABI_VERSION; }
int32_t fw_state_dim(void) { return FW_STATE_DIM; }
int32_t fw_obs_dim(const fw_config* cfg) { return cfg ? obs_dim_of(cfg) : FW_EINVAL; }
int32_t fw_act_dim(const fw_config* cfg) { return cfg ? (direct_actions(cfg->task) ? 6 : 4) : FW_EINVAL; }

int32_t fw_validate_config(const fw_config* cfg, char* msg, int32_t msg_len) {
  std::string m;
  int rc = validate(cfg, m);
  if (rc != FW_OK && msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", m.c_str());
  return rc;
}

int32_t fw_create(const fw_config* cfg, int32_t num_envs, int32_t device, uint64_t seed, int64_t global_env_offset,
                  fw_handle* out) {
  if (!cfg || !out || num_envs <= 0) { g_err = "bad arguments"; return FW_EINVAL; }
  int rc = validate(cfg, g_err);
  if (rc != FW_OK) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_err = "no HIP device available (this library has no CPU fallback)"; return FW_EHIP; }
  if (device < 0 || device >= ndev) { g_err = "device index out of range"; return FW_EINVAL; }
  fw_env* h = new (std::nothrow) fw_env();
  if (!h) return FW_ENOMEM;
  h->cfg = *cfg; h->n = num_envs; h->npad = (num_envs + kWave - 1) / kWave * kWave;
  h->device = device; h->seed = seed; h->env_offset = global_env_offset;
  // Lane mapping, by measured crossover (tools/crossover.py, profiles/r03_crossover.txt; us per eager step, fp64, median of 7 x 20):
  //   wind-free waypoints   N:  8192  12288  16384  24576  32768  65536     waypoints + wind   N:  4096  6144  8192  12288  16384
  //     8 lanes, 1 wave/SIMD    25.6   42.3   46.8   64.2   83.5  150.4                              25.5  34.8  48.8   58.1   69.8
  //     8 lanes, 2 waves/SIMD   28.0   36.8   39.1   54.0   68.1  149.6                              35.1  38.2  41.2   54.3   74.7
  //     1 lane                  57.6   58.5   59.6   63.9   66.8   80.9                              62.3  63.1  63.1   66.0   67.0
  //   8 lanes per env split an env's five lifting surfaces over lanes (latency mapping: 4096 envs are 512 waves instead of
  //   64); its full-register-file build holds ONE wave per SIMD, so above 8192 envs (1024 waves) a second round starts -- there
  //   the build capped at 256 registers (two waves per SIMD) takes over, and one lane per env above that.  The wind kernels
  //   run as many worker waves again, which lowers their thresholds.
  // FWSIM_LANES_PER_ENV=1|8 and FWSIM_G8_WAVES=1|2 override (parity tests, the benchmark sweep).
  // Camera tasks with obstacles stay on the 8-lane mapping at every size: there the cylinders are drawn by the wave from LDS
  // work lists; one lane per env tests every pixel against every cylinder (combined, 20 cylinders: 330 us vs 7.8 ms per
  // step at 32 768 envs).
  const bool camera = has_camera(cfg->task);
  const bool cyl_camera = camera && cfg->num_obstacles > 0;
  const bool wp = cfg->task == FW_TASK_WAYPOINTS, windy = wp && cfg->wind_mode != FW_WIND_OFF;
  const int one_wave_max = windy ? 6144 : 8192;                 // up to here the one-wave-per-SIMD build wins
  const int g8_max = !wp ? kG8MaxEnvs : (windy ? 12288 : 24576);   // ... and up to here the 8-lane mapping
  const bool fits8 = cfg->num_targets <= 8 && cfg->n_collision_pts <= 8;
  h->lanes_per_env = ((num_envs <= g8_max || cyl_camera) && fits8) ? 8 : 1;
  if (const char* ev = getenv("FWSIM_LANES_PER_ENV")) {
    int v = atoi(ev);
    if (v == 1 || (v == 8 && fits8)) h->lanes_per_env = v;
  }
  h->g8_waves = (h->lanes_per_env == 8 && wp && num_envs > one_wave_max) ? 2 : 1;
  if (const char* ev = getenv("FWSIM_G8_WAVES")) {
    int v = atoi(ev);
    if ((v == 1 || v == 2) && h->lanes_per_env == 8 && wp) h->g8_waves = v;
  }
  // Camera tasks on the 8-lane mapping, opt-in (FWSIM_CAPTURE_WAVE=1): a second wave per step workgroup takes the captures
  // (fwsim_objlock.hpp, "The capture wave").  Off by default: measured in round 5 it shortens the MEAN wave (ObjLock - 6 %,
  // combined - 8 %) but not the launch, which lasts as long as its slowest wave (CHANGELOG round 5).
  h->capture_wave = 0;
  if (const char* ev = getenv("FWSIM_CAPTURE_WAVE")) { if (atoi(ev) != 0 && h->lanes_per_env == 8 && camera) h->capture_wave = 1; }
  // The tick's axis-aligned variant (fw_step_kernel_g8<double, false, true>; bit-identical to the general tick, see
  // surface_wrench_ax): the f64 wind-free waypoints kernel of the one-wave 8-lane build, when the geometry allows it.
  h->axis_aligned = (h->lanes_per_env == 8 && h->g8_waves == 1 && wp && !windy && cfg->dtype == FW_F64 &&
                     axis_aligned_geometry(*cfg)) ? 1 : 0;
  // ... and its build with a noise wave (fw_step_kernel_g8x; bit-identical again): where the step wave pre-draws its motor noise
  // today (noise on, step_ratio <= 8), up to the size at which every wave of the launch still has a SIMD of its own (512 step
  // workgroups of two waves on 1024 SIMDs); measured, profiles/r15_aux_wave_ab.txt.  FWSIM_AUX_WAVE=0|1 overrides where the row exists.
  const bool aux_row = h->axis_aligned && cfg->motor.noise_ratio != 0.0 && 120 / cfg->agent_hz <= 8;      // (Params: has_noise, step_ratio)
  h->aux_wave = (aux_row && num_envs <= kAuxWaveMaxEnvs) ? 1 : 0;
  if (const char* ev = getenv("FWSIM_AUX_WAVE")) { if (aux_row) h->aux_wave = atoi(ev) != 0 ? 1 : 0; }
  // ... and the noise-wave kernel with the config's shape compiled in (fw_step_kernel_g8xs; bit-identical again), where the config
  // has the one shape that is built.  FWSIM_STEP_SHAPE=0 turns it off; no value turns it on for another shape (wrong results).
  h->step_shape = (h->aux_wave && step_shape_of(*cfg)) ? 1 : 0;
  if (const char* ev = getenv("FWSIM_STEP_SHAPE")) { if (atoi(ev) == 0) h->step_shape = 0; }
  // ... and the fixed-shape kernel with its second wave kept to the end of the launch (fw_step_kernel_g8xo; bit-identical again): that
  // wave is the scenario worker of its tile and writes the observation rows.  FWSIM_OBS_WAVE=0|1 overrides where the row exists.
  // Never above kAuxWaveMaxEnvs envs, whatever FWSIM_AUX_WAVE says: both waves of a workgroup last the whole launch.
  const bool obs_row = h->step_shape && num_envs <= kAuxWaveMaxEnvs;
  h->obs_wave = (obs_row && kObsWaveDefault) ? 1 : 0;
  if (const char* ev = getenv("FWSIM_OBS_WAVE")) { if (obs_row) h->obs_wave = atoi(ev) != 0 ? 1 : 0; }
  DeviceGuard g(device);
  rc = with_dtype(h, [&](auto t) { return create_T<decltype(t)>(h); });
  if (rc != FW_OK) {
    g_err = h->err;
    free_device_buffers(h);
    delete h;
    return rc;
  }
  *out = h;
  return FW_OK;
}

int32_t fw_reset(fw_handle h, const uint8_t* mask, const fw_scenario* scenario, void* obs_out, void* hip_stream) {
  if (!h) return FW_EINVAL;
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)hip_stream;
  ScenOv ov{};
  if (scenario) {
    if (scenario->obstacles && !scenario->num_obstacles) { h->err = "fw_scenario: obstacles without num_obstacles"; return FW_EINVAL; }
    // stage the host arrays in one device buffer owned by the handle (stream-ordered copies, then the reset kernel)
    const size_t N = (size_t)h->n;
    const size_t sz[7] = { N * FW_MAX_TARGETS * 3, N * 3, N * FW_MAX_OBSTACLES * 3, N, N * 3, N * 3, N };
    size_t total = 0;
    for (size_t v : sz) total += v;
    if (!h->scen_dev) HIP_TRY(h, hipMalloc((void**)&h->scen_dev, sizeof(double) * total));
    std::vector<double> nobd;
    if (scenario->num_obstacles) { nobd.resize(N); for (size_t i = 0; i < N; ++i) nobd[i] = (double)scenario->num_obstacles[i]; }
    const double* src[7] = { scenario->targets, scenario->duck_pos, scenario->obstacles, scenario->num_obstacles ? nobd.data() : nullptr,
                             scenario->wind_base, scenario->gust_amp, scenario->gust_phase };
    const double* dst[7];
    size_t off = 0;
    for (int k = 0; k < 7; ++k) {
      dst[k] = nullptr;
      if (src[k]) {
        HIP_TRY(h, hipMemcpyAsync(h->scen_dev + off, src[k], sizeof(double) * sz[k], hipMemcpyHostToDevice, st));
        dst[k] = h->scen_dev + off;
      }
      off += sz[k];
    }
    HIP_TRY(h, hipStreamSynchronize(st));          // the host arrays (and `nobd`) may go away as soon as we return
    ov.targets = dst[0]; ov.duck = dst[1]; ov.obst = dst[2]; ov.nob = dst[3]; ov.wind_base = dst[4]; ov.gust_amp = dst[5]; ov.gust_phase = dst[6];
    if (!ov.obst) ov.nob = nullptr;
  }
  return with_dtype(h, [&](auto t) { return reset_T<decltype(t)>(h, mask, obs_out, 1, st, ov); });
}

int32_t fw_observe(fw_handle h, void* obs_out, void* hip_stream) {
  if (!h || !obs_out) { if (h) h->err = "obs_out is NULL"; return FW_EINVAL; }
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)hip_stream;
  return with_dtype(h, [&](auto t) { return reset_T<decltype(t)>(h, nullptr, obs_out, 0, st); });
}

int32_t fw_step(fw_handle h, const void* actions, void* obs, void* reward, uint8_t* terminated, uint8_t* truncated,
                void* terminal_obs, int32_t* info_i32, void* hip_stream) {
  if (!h) return FW_EINVAL;
  if (!actions || !obs || !reward || !terminated || !truncated) { h->err = "actions/obs/reward/terminated/truncated must be non-NULL"; return FW_EINVAL; }
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)hip_stream;
  return with_dtype(h, [&](auto t) { return step_T<decltype(t)>(h, actions, obs, reward, terminated, truncated, terminal_obs, info_i32, st); });
}

int32_t fw_render(fw_handle h, int32_t res, float* out, void* hip_stream) {
  if (!h) return FW_EINVAL;
  if (!out) { h->err = "fw_render: out is NULL"; return FW_EINVAL; }
  const char* camless = h->cfg.task == FW_TASK_LOWLEVEL ? "fw_render: the low-level task has no camera" : "fw_render: the waypoints task has no camera";
  if (!has_camera(h->cfg.task)) { h->err = camless; return FW_EUNSUPPORTED; }      // (direct-command waypoints: the waypoints task's words)
  if (res < 1 || res > 1024) { h->err = "fw_render: res must be in [1, 1024]"; return FW_EINVAL; }
  DeviceGuard g(h->device);
  const fw_config& c = h->cfg;
  RenderC K;
  const double th = c.camera_angle_deg * kPi / 180.0;
  const double f[3] = { std::cos(th), 0.0, std::sin(th) }, r[3] = { 0.0, -1.0, 0.0 };
  const double d[3] = { f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0] };
  for (int k = 0; k < 3; ++k) { K.cam_f[k] = f[k]; K.cam_r[k] = r[k]; K.cam_d[k] = d[k]; K.cam_off[k] = c.camera_offset[k]; }
  K.tan_half_fov = std::tan(0.5 * c.camera_fov_deg * (kPi / 180.0));
  K.near_ = c.camera_near; K.far_ = c.camera_far; K.duck_radius = c.duck_radius_per_scale * c.duck_global_scaling; K.obst_radius = c.obstacle_radius;
  K.inv_near = 1.0 / K.near_; K.inv_far = 1.0 / K.far_; K.db_c1 = K.far_ / (K.far_ - K.near_);
  const int tile = kWave / h->lanes_per_env;
  hipStream_t st = (hipStream_t)hip_stream;
  // LDS behind the kernel's static tables: the image-plane coordinate of every pixel column / row, and from 64 x 64 pixels on a stage
  // of 2048 pixels per channel through which the image leaves as whole rows (16 KB: eight workgroups per CU keep their place).
  // Measured at 4096 envs, stage against direct stores: 32 x 32 28.1 / 26.8 us (a 1024-pixel image is two store instructions per lane
  // either way: the stage only adds its barrier), 64 x 64 62.6 / 63.5, 128 x 128 223 / 273
  int stage_px = (res >= 64 && res <= 128) ? 2048 : 0;
  if (const char* e = std::getenv("FWSIM_RENDER_STAGE")) { const int v = std::atoi(e); if (v >= 0 && v <= 4096) stage_px = v & ~3; }       // (measurement knob)
  if (((stage_px / res) & ~15) == 0) stage_px = 0;
  const size_t lds = sizeof(double) * (size_t)((res + 1) & ~1) + 2 * sizeof(float) * (size_t)stage_px;
  int threads = 256;                                     // (measured at 4096 x 32 x 32 on the 1 / t kernel with 16 x 16 tiles: 64 threads per env 52.7 us, 128: 50.8, 256: 48.2)
  if (const char* e = std::getenv("FWSIM_RENDER_THREADS")) { const int v = std::atoi(e); if (v == 64 || v == 128 || v == 256) threads = v; }   // (measurement knob)
#ifdef FW_RENDER_PROF
  static long long* rprof = nullptr; static size_t rprof_n = 0;
  const size_t rp_n = (size_t)h->n * 4 * 8;
  if (rprof_n < rp_n) { if (rprof) (void)hipFree(rprof); HIP_TRY(h, hipMalloc((void**)&rprof, rp_n * sizeof(long long))); rprof_n = rp_n; }
  HIP_TRY(h, hipMemsetAsync(rprof, 0, rp_n * sizeof(long long), st));
  HIP_TRY(h, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_render_prof), &rprof, sizeof(rprof), 0, hipMemcpyHostToDevice, st));
#endif
  with_dtype(h, [&](auto t) {
    auto kernel = stage_px ? fw_render_kernel<decltype(t), true> : fw_render_kernel<decltype(t), false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)h->n), dim3(threads), lds, st, (const decltype(t)*)h->r_dev, tile, h->n, threads / 64, K, res, out, stage_px);
  });
  HIP_TRY(h, hipGetLastError());
#ifdef FW_RENDER_PROF
  if (std::getenv("FWSIM_RENDER_PROF_DUMP")) {       // per-wave cycle stamps -> mean phase lengths, set-up waves and the others apart
    HIP_TRY(h, hipStreamSynchronize(st));
    std::vector<long long> P(rp_n);
    HIP_TRY(h, hipMemcpy(P.data(), rprof, rp_n * sizeof(long long), hipMemcpyDeviceToHost));
    const int nw = threads / 64;
    double su[6] = {0}, ot[6] = {0}; long long nsu = 0, not_ = 0; long long t0min = -1, t5max = 0; double life_su = 0, life_ot = 0;
    for (int e = 0; e < h->n; ++e) for (int w = 0; w < nw; ++w) {
      const long long* q = &P[((size_t)e * 4 + w) * 8];
      if (!q[0] || !q[5]) continue;
      if (t0min < 0 || q[0] < t0min) t0min = q[0];
      if (q[5] > t5max) t5max = q[5];
      const bool is_su = (w == (e & (nw - 1))) || (w == ((e + 1) & (nw - 1)));
      double* d = is_su ? su : ot;
      if (is_su) { d[0] += (double)(q[1] - q[0]); d[1] += (double)(q[2] - q[1]); ++nsu; life_su += (double)(q[5] - q[0]); }
      else { d[0] += 0; d[1] += (double)(q[2] - q[0]); ++not_; life_ot += (double)(q[5] - q[0]); }
      d[2] += (double)(q[3] - q[2]); d[3] += (double)(q[4] - q[3]); d[4] += (double)(q[5] - q[4]);
    }
    std::fprintf(stderr, "fw_render wave profile (cycles of the counter, mean per wave; res %d, %d envs, %d waves per env, stage %d)\n", res, h->n, nw, stage_px);
    std::fprintf(stderr, "  set-up waves (%lld): start->gather in %.0f, set-up arithmetic %.0f, at the barrier %.0f, constants %.0f, strips %.0f, life %.0f\n",
                 nsu, su[0] / nsu, su[1] / nsu, su[2] / nsu, su[3] / nsu, su[4] / nsu, life_su / nsu);
    std::fprintf(stderr, "  other waves  (%lld): start->barrier arrival %.0f, at the barrier %.0f, constants %.0f, strips %.0f, life %.0f\n",
                 not_, ot[1] / not_, ot[2] / not_, ot[3] / not_, ot[4] / not_, life_ot / not_);
    std::fprintf(stderr, "  first stamp to last stamp of the launch: %lld\n", t5max - t0min);
  }
#endif
  return FW_OK;
}

int32_t fw_seed(fw_handle h, uint64_t seed) {
  if (!h) return FW_EINVAL;
  DeviceGuard g(h->device);
  h->seed = seed;
  HIP_TRY(h, hipDeviceSynchronize());
  int rc = with_dtype(h, [&](auto t) { return upload_params<decltype(t)>(h); });
  if (rc != FW_OK) return rc;
  {
    // episode counters back to -1 (the next reset starts episode 0 of the new seed); rows are tiled, so go through a host copy
    const int tile = kWave / h->lanes_per_env;
    std::vector<int32_t> iv((size_t)IF_COUNT * h->npad);
    HIP_TRY(h, hipMemcpy(iv.data(), h->i_dev, sizeof(int32_t) * iv.size(), hipMemcpyDeviceToHost));
    for (int e = 0; e < h->npad; ++e) iv[tile_index(tile, IF_COUNT, IF_EPISODE, e)] = -1;
    HIP_TRY(h, hipMemcpy(h->i_dev, iv.data(), sizeof(int32_t) * iv.size(), hipMemcpyHostToDevice));
  }
  return invalidate_shadow(h);                 // shadows were drawn with the old seed
}

int32_t fw_get_state(fw_handle h, double* state_out) {
  if (!h || !state_out) return FW_EINVAL;
  DeviceGuard g(h->device);
  return with_dtype(h, [&](auto t) { return get_state_T<decltype(t)>(h, state_out); });
}

int32_t fw_set_state(fw_handle h, const double* state_in) {
  if (!h || !state_in) return FW_EINVAL;
  DeviceGuard g(h->device);
  return with_dtype(h, [&](auto t) { return set_state_T<decltype(t)>(h, state_in); });
}

int32_t fw_get_counters(fw_handle h, uint64_t* out) {
  if (!h || !out) return FW_EINVAL;
  DeviceGuard g(h->device);
  unsigned long long w[FW_CTR_DIM];
  uint32_t launches = 0;
  HIP_TRY(h, hipDeviceSynchronize());
  HIP_TRY(h, hipMemcpy(w, h->stats_dev, sizeof w, hipMemcpyDeviceToHost));
  HIP_TRY(h, hipMemcpy(&launches, h->lctr_dev, sizeof launches, hipMemcpyDeviceToHost));
  for (int i = 0; i < FW_CTR_DIM; ++i) out[i] = w[i];
  out[FW_CTR_LAUNCHES] = launches;
  return FW_OK;
}

int32_t fw_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values,
               const float* last_dones, float* advantages, float* returns, int32_t T, int32_t N, float gamma,
               float gae_lambda, void* hip_stream) {
  if (!rewards || !values || !episode_starts || !last_values || !last_dones || !advantages || !returns || T <= 0 || N <= 0) {
    g_err = "fw_gae: bad arguments"; return FW_EINVAL;
  }
  DeviceGuard g(device_of(rewards));
  hipLaunchKernelGGL(fw_gae_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, rewards, values,
                     episode_starts, last_values, last_dones, advantages, returns, T, N, gamma, gae_lambda);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int32_t fw_eval_track(const void* reward, int32_t reward_is_f64, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                      int32_t info_dim, const int64_t* targets, int64_t* counts, double* cur_rew, int64_t* cur_len, int64_t* step_ctr,
                      double* fin_rew, int64_t* fin_len, int64_t* fin_step, int32_t* fin_info, int32_t N, int32_t E, void* hip_stream) {
  if (!reward || !terminated || !truncated || !targets || !counts || !cur_rew || !cur_len || !step_ctr || !fin_rew || !fin_len || !fin_step ||
      N <= 0 || E <= 0 || (info && (info_dim <= 0 || !fin_info))) { g_err = "fw_eval_track: bad arguments"; return FW_EINVAL; }
  EvalTrackArgs A;
  A.reward = reward; A.reward_is_f64 = reward_is_f64; A.terminated = terminated; A.truncated = truncated; A.info = info; A.info_dim = info_dim;
  A.targets = targets; A.counts = counts; A.cur_rew = cur_rew; A.cur_len = cur_len; A.step_ctr = step_ctr;
  A.fin_rew = fin_rew; A.fin_len = fin_len; A.fin_step = fin_step; A.fin_info = fin_info; A.N = N; A.E = E;
  DeviceGuard g(device_of(reward));
  hipLaunchKernelGGL(fw_eval_track_kernel, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, A);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int64_t fw_episode_state_bytes(int32_t N, int32_t W) {
  if (N <= 0 || W <= 0) { g_err = "fw_episode_state_bytes: N and W must be positive, got N=" + std::to_string(N) + ", W=" + std::to_string(W); return FW_EINVAL; }
  return 8 * ((int64_t)EP_HEADER_WORDS + (int64_t)W * (5 + kEpInfo / 2) + 2 * (int64_t)N);
}

int32_t fw_episode_fold(const void* reward, int32_t reward_is_f64, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                        int32_t info_dim, void* state, int32_t N, int32_t W, void* hip_stream) {
  if (!reward || !terminated || !truncated || !state) { g_err = "fw_episode_fold: reward, terminated, truncated and state must be non-NULL"; return FW_EINVAL; }
  if (N <= 0 || W <= 0) { g_err = "fw_episode_fold: N and W must be positive, got N=" + std::to_string(N) + ", W=" + std::to_string(W); return FW_EINVAL; }
  if (info && info_dim <= 0) { g_err = "fw_episode_fold: info given with info_dim=" + std::to_string(info_dim); return FW_EINVAL; }
  EpisodeFoldArgs A;
  A.reward = reward; A.reward_is_f64 = reward_is_f64; A.terminated = terminated; A.truncated = truncated; A.info = info; A.info_dim = info_dim;
  A.state = reinterpret_cast<int64_t*>(state); A.N = N; A.W = W;
  DeviceGuard g(device_of(reward));
  hipLaunchKernelGGL(fw_episode_fold_kernel, dim3(1), dim3(kEpThreads), 0, (hipStream_t)hip_stream, A);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int32_t fw_episode_fold_span(void) { return kEpSpan; }

static inline int64_t ep_wide_blocks(int32_t N) { return ((int64_t)N + kEpSpan - 1) / kEpSpan; }

int64_t fw_episode_fold_workspace_bytes(int32_t N) {
  if (N <= 0) { g_err = "fw_episode_fold_workspace_bytes: N must be positive, got N=" + std::to_string(N); return FW_EINVAL; }
  const int64_t B = ep_wide_blocks(N);
  return 8 * (1 + (int64_t)kEpParts * B + (B + 1) / 2);
}

int32_t fw_episode_fold_wide(const void* reward, int32_t reward_is_f64, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                             int32_t info_dim, void* state, void* workspace, int32_t N, int32_t W, void* hip_stream) {
  if (!reward || !terminated || !truncated || !state) { g_err = "fw_episode_fold_wide: reward, terminated, truncated and state must be non-NULL"; return FW_EINVAL; }
  if (!workspace) { g_err = "fw_episode_fold_wide: workspace must be non-NULL (fw_episode_fold_workspace_bytes(N) bytes of device memory)"; return FW_EINVAL; }
  if (N <= 0 || W <= 0) { g_err = "fw_episode_fold_wide: N and W must be positive, got N=" + std::to_string(N) + ", W=" + std::to_string(W); return FW_EINVAL; }
  if (info && info_dim <= 0) { g_err = "fw_episode_fold_wide: info given with info_dim=" + std::to_string(info_dim); return FW_EINVAL; }
  EpisodeWideArgs X;
  X.F.reward = reward; X.F.reward_is_f64 = reward_is_f64; X.F.terminated = terminated; X.F.truncated = truncated; X.F.info = info;
  X.F.info_dim = info_dim; X.F.state = reinterpret_cast<int64_t*>(state); X.F.N = N; X.F.W = W;
  X.ws = reinterpret_cast<int64_t*>(workspace); X.B = (int32_t)ep_wide_blocks(N);
  DeviceGuard g(device_of(reward));
  hipStream_t s = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(fw_episode_count_kernel, dim3(X.B), dim3(kEpSpan), 0, s, X);
  hipLaunchKernelGGL(fw_episode_fold_wide_kernel, dim3(X.B), dim3(kEpSpan), 0, s, X);
  hipLaunchKernelGGL(fw_episode_finish_kernel, dim3(1), dim3(kEpFinishThreads), 0, s, X);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int32_t fw_eval_track_ll(const void* reward, int32_t reward_is_f64, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                         int32_t info_dim, const void* obs, const void* terminal_obs, int32_t obs_is_f64, int32_t obs_dim,
                         const int64_t* targets, int64_t* counts, double* cur_rew, int64_t* cur_len, int64_t* step_ctr, double* cur_track,
                         double* fin_rew, int64_t* fin_len, int64_t* fin_step, int32_t* fin_info, double* fin_track, int32_t N, int32_t E,
                         void* hip_stream) {
  if (!reward || !terminated || !truncated || !targets || !counts || !cur_rew || !cur_len || !step_ctr || !fin_rew || !fin_len || !fin_step ||
      (info && (info_dim <= 0 || !fin_info))) { g_err = "fw_eval_track_ll: bad arguments"; return FW_EINVAL; }
  if (!obs || !terminal_obs || !cur_track || !fin_track) { g_err = "fw_eval_track_ll: obs, terminal_obs, cur_track and fin_track must be non-NULL"; return FW_EINVAL; }
  if (obs_dim != 21) { g_err = "fw_eval_track_ll: obs_dim must be 21 (the low-level task's observation), got " + std::to_string(obs_dim); return FW_EINVAL; }
  if (N <= 0 || E <= 0) { g_err = "fw_eval_track_ll: N and E must be positive, got N=" + std::to_string(N) + ", E=" + std::to_string(E); return FW_EINVAL; }
  EvalTrackArgs A;
  A.reward = reward; A.reward_is_f64 = reward_is_f64; A.terminated = terminated; A.truncated = truncated; A.info = info; A.info_dim = info_dim;
  A.targets = targets; A.counts = counts; A.cur_rew = cur_rew; A.cur_len = cur_len; A.step_ctr = step_ctr;
  A.fin_rew = fin_rew; A.fin_len = fin_len; A.fin_step = fin_step; A.fin_info = fin_info; A.N = N; A.E = E;
  EvalTrackLLArgs X;
  X.obs = obs; X.terminal_obs = terminal_obs; X.obs_is_f64 = obs_is_f64; X.cur_track = cur_track; X.fin_track = fin_track;
  DeviceGuard g(device_of(reward));
  hipLaunchKernelGGL(fw_eval_track_ll_kernel, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, A, X);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int32_t fw_eval_track_hl(const void* reward, int32_t reward_is_f64, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                         int32_t info_dim, const void* obs, const void* terminal_obs, const void* command, int32_t obs_is_f64,
                         int32_t obs_dim, double alt_high, double speed_high, const int64_t* targets, int64_t* counts, double* cur_rew,
                         int64_t* cur_len, int64_t* step_ctr, double* cur_track, double* prev_cmd, double* fin_rew, int64_t* fin_len,
                         int64_t* fin_step, int32_t* fin_info, double* fin_track, int32_t N, int32_t E, void* hip_stream) {
  if (!reward || !terminated || !truncated || !targets || !counts || !cur_rew || !cur_len || !step_ctr || !fin_rew || !fin_len || !fin_step ||
      (info && (info_dim <= 0 || !fin_info))) { g_err = "fw_eval_track_hl: bad arguments"; return FW_EINVAL; }
  if (!obs || !terminal_obs || !cur_track || !fin_track) { g_err = "fw_eval_track_hl: obs, terminal_obs, cur_track and fin_track must be non-NULL"; return FW_EINVAL; }
  if (!command || !prev_cmd) { g_err = "fw_eval_track_hl: command and prev_cmd must be non-NULL"; return FW_EINVAL; }
  if (obs_dim != 30) { g_err = "fw_eval_track_hl: obs_dim must be 30 (the high-level command task's observation), got " + std::to_string(obs_dim); return FW_EINVAL; }
  if (N <= 0 || E <= 0) { g_err = "fw_eval_track_hl: N and E must be positive, got N=" + std::to_string(N) + ", E=" + std::to_string(E); return FW_EINVAL; }
  EvalTrackArgs A;
  A.reward = reward; A.reward_is_f64 = reward_is_f64; A.terminated = terminated; A.truncated = truncated; A.info = info; A.info_dim = info_dim;
  A.targets = targets; A.counts = counts; A.cur_rew = cur_rew; A.cur_len = cur_len; A.step_ctr = step_ctr;
  A.fin_rew = fin_rew; A.fin_len = fin_len; A.fin_step = fin_step; A.fin_info = fin_info; A.N = N; A.E = E;
  EvalTrackLLArgs X;
  X.obs = obs; X.terminal_obs = terminal_obs; X.obs_is_f64 = obs_is_f64; X.cur_track = cur_track; X.fin_track = fin_track;
  EvalTrackHLArgs H;
  H.command = command; H.prev_cmd = prev_cmd; H.alt_high = alt_high; H.speed_high = speed_high;
  DeviceGuard g(device_of(reward));
  hipLaunchKernelGGL(fw_eval_track_hl_kernel, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, A, X, H);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int32_t fw_command_ll(fw_handle h, const double* cmd, int32_t T, const int64_t* step_idx, const uint8_t* mask, void* obs,
                      int32_t* rejected, void* hip_stream) {
  if (!h) { g_err = "fw_command_ll: NULL handle"; return FW_EINVAL; }
  if (h->cfg.task != FW_TASK_LOWLEVEL) { h->err = "fw_command_ll: only the low-level task (FW_TASK_LOWLEVEL) takes commands"; return FW_EUNSUPPORTED; }
  if (!cmd) { h->err = "fw_command_ll: cmd must be non-NULL"; return FW_EINVAL; }
  if (T <= 0) { h->err = "fw_command_ll: T must be positive, got " + std::to_string(T); return FW_EINVAL; }
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)((h->n + 255) / 256)), block(256);
  const double dome = h->cfg.flight_dome_size;
  with_dtype(h, [&](auto t) { with_lanes(h, [&](auto lanes) {
    using R = decltype(t);
    hipLaunchKernelGGL((fw_command_ll_kernel<R, decltype(lanes)::value>), grid, block, 0, st, dev_state<R>(h), cmd, T, step_idx, mask, (R*)obs, rejected, dome);
  }); });
  HIP_TRY(h, hipGetLastError());
  return FW_OK;
}

int32_t fw_command_hl(fw_handle h, const void* action, int32_t action_is_f64, const uint8_t* mask, const void* obs, void* low_obs,
                      void* cmd_out, int32_t* rejected, void* hip_stream) {
  if (!h) { g_err = "fw_command_hl: NULL handle"; return FW_EINVAL; }
  if (h->cfg.task != FW_TASK_WAYPOINTS_DIRECT) { h->err = "fw_command_hl: only the direct-command waypoints task (FW_TASK_WAYPOINTS_DIRECT) takes high-level commands"; return FW_EUNSUPPORTED; }
  if (h->cfg.angle_representation != 0) { h->err = "fw_command_hl: the low-level controller's observation needs the euler attitude (angle_representation 0)"; return FW_EUNSUPPORTED; }
  if (!action || !obs || !low_obs) { h->err = "fw_command_hl: action, obs and low_obs must be non-NULL"; return FW_EINVAL; }
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 block(256), grid((unsigned)((h->n + 255) / 256));
  const double dome = h->cfg.flight_dome_size;
  const int32_t D = obs_dim_of(&h->cfg);
  with_dtype(h, [&](auto t) { with_lanes(h, [&](auto lanes) { with_real(action_is_f64 != 0, [&](auto ta) {
    using T = decltype(t); using TA = decltype(ta);
    hipLaunchKernelGGL((fw_command_hl_kernel<T, decltype(lanes)::value, TA>), grid, block, 0, st, dev_state<T>(h), (const TA*)action, mask,
                       (const T*)obs, D, (T*)low_obs, (T*)cmd_out, rejected, dome);
  }); }); });
  HIP_TRY(h, hipGetLastError());
  return FW_OK;
}

int32_t fw_sizeof_step_hl_args(void) { return (int32_t)sizeof(fw_step_hl_args); }
int32_t fw_step_hl(fw_handle h, const fw_step_hl_args* a, void* hip_stream) {
  if (!h) { g_err = "fw_step_hl: NULL handle"; return FW_EINVAL; }
  if (h->cfg.task != FW_TASK_WAYPOINTS_DIRECT) { h->err = "fw_step_hl: only the direct-command waypoints task (FW_TASK_WAYPOINTS_DIRECT) takes high-level commands"; return FW_EUNSUPPORTED; }
  if (h->cfg.angle_representation != 0) { h->err = "fw_step_hl: the low-level controller's observation needs the euler attitude (angle_representation 0)"; return FW_EUNSUPPORTED; }
  if (!h->step_hl.fn) { h->err = "fw_step_hl: no kernel is built for this handle"; return FW_EUNSUPPORTED; }
  if (!a) { h->err = "fw_step_hl: NULL arguments"; return FW_EINVAL; }
  if (!a->low_params || !a->low_mean || !a->low_var || !a->obs || !a->reward || !a->terminated || !a->truncated) {
    h->err = "fw_step_hl: low_params, low_mean, low_var, obs, reward, terminated and truncated must be non-NULL"; return FW_EINVAL;
  }
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)hip_stream;
  fwsim_ctl::CtlArgs CA;
  CA.params = a->low_params; CA.mean = a->low_mean; CA.var = a->low_var; CA.clip = a->low_clip; CA.eps = a->low_eps; CA.low_action = a->low_action;
  void* obs = a->obs; void* reward = a->reward; uint8_t* term = a->terminated; uint8_t* trunc = a->truncated; void* tobs = a->terminal_obs;
  int32_t* info = a->info_i32;
  with_dtype(h, [&](auto t) {
    using T = decltype(t);
    const Params<T>* Pp = (const Params<T>*)h->params_dev; const ObjC<T>* OCp = (const ObjC<T>*)h->objc_dev;
    DevState<T> D = dev_state<T>(h);
    void* args[] = { &Pp, &OCp, &D, &CA, &obs, &reward, &term, &trunc, &tobs, &info };
    (void)hipLaunchKernel(h->step_hl.fn, grid_of(h), dim3(h->step_hl.block), args, hl_step_lds_bytes<T>(h), st);
  });
  HIP_TRY(h, hipGetLastError());
  return FW_OK;
}

int32_t fw_controller_forward(const float* params, const void* raw_obs, int32_t obs_is_f64, int32_t N, const double* mean, const double* var,
                              float clip, float eps, void* act_out, int32_t act_is_f64, void* hip_stream) {
  if (!params || !raw_obs || !mean || !var || !act_out) { g_err = "fw_controller_forward: params, raw_obs, mean, var and act_out must be non-NULL"; return FW_EINVAL; }
  if (N <= 0) { g_err = "fw_controller_forward: N must be positive, got " + std::to_string(N); return FW_EINVAL; }
  DeviceGuard g(device_of(params));
  const dim3 grid((unsigned)((N + kWave - 1) / kWave)), block(kWave);
  const size_t lds = fwsim_ctl::ctl_lds_bytes(kWave, false);
  with_real(obs_is_f64 != 0, [&](auto t) { with_real(act_is_f64 != 0, [&](auto to) {
    using T = decltype(t); using TO = decltype(to);
    hipLaunchKernelGGL((fw_controller_forward_kernel<T, TO>), grid, block, lds, (hipStream_t)hip_stream, params, (const T*)raw_obs, N, mean, var,
                       clip, eps, (TO*)act_out);
  }); });
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int32_t fw_trace_ll(const void* obs, const void* terminal_obs, const uint8_t* terminated, const uint8_t* truncated, int32_t obs_is_f64,
                    int32_t N, double* trace, int32_t T, int64_t* step_idx, void* hip_stream) {
  if (!obs || !trace || !step_idx) { g_err = "fw_trace_ll: obs, trace and step_idx must be non-NULL"; return FW_EINVAL; }
  if (N <= 0 || T <= 0) { g_err = "fw_trace_ll: N and T must be positive, got N=" + std::to_string(N) + ", T=" + std::to_string(T); return FW_EINVAL; }
  DeviceGuard g(device_of(trace));
  hipLaunchKernelGGL(fw_trace_ll_kernel, dim3(1), dim3(1024), 0, (hipStream_t)hip_stream, obs, terminal_obs, terminated, truncated,
                     obs_is_f64, N, trace, T, step_idx);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int32_t fw_trace_hl(const void* obs, const void* terminal_obs, const uint8_t* terminated, const uint8_t* truncated, const void* command,
                    const int32_t* info, int32_t info_dim, int32_t obs_is_f64, int32_t N, double* trace, int32_t T, int64_t* step_idx,
                    void* hip_stream) {
  if (!obs || !command || !trace || !step_idx) { g_err = "fw_trace_hl: obs, command, trace and step_idx must be non-NULL"; return FW_EINVAL; }
  if (N <= 0 || T <= 0) { g_err = "fw_trace_hl: N and T must be positive, got N=" + std::to_string(N) + ", T=" + std::to_string(T); return FW_EINVAL; }
  if (info && info_dim <= FW_INFO_NUM_TARGETS_REACHED) { g_err = "fw_trace_hl: info_dim must cover the num_targets_reached column, got " + std::to_string(info_dim); return FW_EINVAL; }
  DeviceGuard g(device_of(trace));
  hipLaunchKernelGGL(fw_trace_hl_kernel, dim3(1), dim3(1024), 0, (hipStream_t)hip_stream, obs, terminal_obs, terminated, truncated,
                     command, info, info_dim, (int32_t)FW_INFO_NUM_TARGETS_REACHED, obs_is_f64, N, trace, T, step_idx);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int32_t fw_trace_rows(const void* obs, const void* terminal_obs, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                      int32_t info_dim, int32_t obs_is_f64, int32_t N, int32_t obs_dim, double* trace, int32_t T, int64_t* step_idx,
                      void* hip_stream) {
  if (!obs || !trace || !step_idx) { g_err = "fw_trace_rows: obs, trace and step_idx must be non-NULL"; return FW_EINVAL; }
  if (N <= 0 || T <= 0) { g_err = "fw_trace_rows: N and T must be positive, got N=" + std::to_string(N) + ", T=" + std::to_string(T); return FW_EINVAL; }
  if (obs_dim <= 0) { g_err = "fw_trace_rows: obs_dim must be positive, got " + std::to_string(obs_dim); return FW_EINVAL; }
  if (info && info_dim <= FW_INFO_NUM_TARGETS_REACHED) { g_err = "fw_trace_rows: info_dim must cover the num_targets_reached column, got " + std::to_string(info_dim); return FW_EINVAL; }
  DeviceGuard g(device_of(trace));
  hipLaunchKernelGGL(fw_trace_rows_kernel, dim3(1), dim3(1024), 0, (hipStream_t)hip_stream, obs, terminal_obs, terminated, truncated,
                     info, info_dim, (int32_t)FW_INFO_NUM_TARGETS_REACHED, obs_is_f64, N, obs_dim, trace, T, step_idx);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int32_t fw_eval_track_wp(const void* reward, int32_t reward_is_f64, const uint8_t* terminated, const uint8_t* truncated, const int32_t* info,
                         int32_t info_dim, const void* obs, const void* terminal_obs, int32_t obs_is_f64, int32_t obs_dim, int32_t att_dim,
                         int32_t act_dim, const int64_t* targets, int64_t* counts, double* cur_rew, int64_t* cur_len, int64_t* step_ctr,
                         double* cur_path, double* carry, double* fin_rew, int64_t* fin_len, int64_t* fin_step, int32_t* fin_info,
                         double* fin_path, int32_t N, int32_t E, void* hip_stream) {
  if (!reward || !terminated || !truncated || !targets || !counts || !cur_rew || !cur_len || !step_ctr || !fin_rew || !fin_len || !fin_step ||
      (info && (info_dim <= 0 || !fin_info))) { g_err = "fw_eval_track_wp: bad arguments"; return FW_EINVAL; }
  if (!obs || !terminal_obs || !cur_path || !carry || !fin_path) { g_err = "fw_eval_track_wp: obs, terminal_obs, cur_path, carry and fin_path must be non-NULL"; return FW_EINVAL; }
  if (att_dim != 12 && att_dim != 13) { g_err = "fw_eval_track_wp: att_dim must be 12 (euler) or 13 (quaternion), got " + std::to_string(att_dim); return FW_EINVAL; }
  if (act_dim != 4 && act_dim != 6) { g_err = "fw_eval_track_wp: act_dim must be 4 or 6, got " + std::to_string(act_dim); return FW_EINVAL; }
  if (obs_dim < att_dim + act_dim + 6) { g_err = "fw_eval_track_wp: obs_dim must be at least att_dim + act_dim + 6, got " + std::to_string(obs_dim); return FW_EINVAL; }
  if (N <= 0 || E <= 0) { g_err = "fw_eval_track_wp: N and E must be positive, got N=" + std::to_string(N) + ", E=" + std::to_string(E); return FW_EINVAL; }
  EvalTrackArgs A;
  A.reward = reward; A.reward_is_f64 = reward_is_f64; A.terminated = terminated; A.truncated = truncated; A.info = info; A.info_dim = info_dim;
  A.targets = targets; A.counts = counts; A.cur_rew = cur_rew; A.cur_len = cur_len; A.step_ctr = step_ctr;
  A.fin_rew = fin_rew; A.fin_len = fin_len; A.fin_step = fin_step; A.fin_info = fin_info; A.N = N; A.E = E;
  EvalTrackWPArgs W;
  W.obs = obs; W.terminal_obs = terminal_obs; W.obs_is_f64 = obs_is_f64; W.obs_dim = obs_dim; W.att_dim = att_dim; W.act_dim = act_dim;
  W.cur_path = cur_path; W.carry = carry; W.fin_path = fin_path;
  DeviceGuard g(device_of(reward));
  hipLaunchKernelGGL(fw_eval_track_wp_kernel, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, A, W);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int64_t fw_normalize_obs_workspace_bytes(int32_t D) { return D > 0 ? (int64_t)sizeof(double) * 64 * 2 * D : FW_EINVAL; }

int32_t fw_normalize_obs(const void* obs, int32_t in_is_f64, int32_t N, int32_t D, double* mean, double* var,
                         double* count, int32_t update, float clip, float eps, float* obs_out, void* workspace,
                         double* batch_acc, void* hip_stream) {
  if (!obs || !mean || !var || !count || !obs_out || N <= 0 || D <= 0 || D > 256) { g_err = "fw_normalize_obs: bad arguments"; return FW_EINVAL; }
  if (update && !workspace) { g_err = "fw_normalize_obs: update needs a workspace of fw_normalize_obs_workspace_bytes(D) bytes"; return FW_EINVAL; }
  hipStream_t st = (hipStream_t)hip_stream;
  DeviceGuard g(device_of(obs));
  if (update) {
    // per-block column sums land in the CALLER's workspace: nothing here is shared between callers or streams
    double* scratch = (double*)workspace;
    const int nblocks = N >= 64 * 64 ? 64 : (N + 63) / 64;       // >= 64 rows per block
    with_real(in_is_f64 != 0, [&](auto t) { hipLaunchKernelGGL(fw_obs_moments_kernel<decltype(t)>, dim3(nblocks), dim3(256), 0, st, (const decltype(t)*)obs, N, D, scratch); });
    hipLaunchKernelGGL(fw_obs_merge_kernel, dim3(1), dim3(256), 0, st, scratch, nblocks, N, D, mean, var, count, batch_acc);
  }
  const int total = N * D;
  with_real(in_is_f64 != 0, [&](auto t) { hipLaunchKernelGGL(fw_obs_normalize_kernel<decltype(t)>, dim3((total + 255) / 256), dim3(256), 0, st, (const decltype(t)*)obs, total, D, mean, var, clip, eps, obs_out); });
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int32_t fw_ppo_param_count(int32_t obs_dim) { return obs_dim > 0 ? ppo_total_params((obs_dim + 1) & ~1) : FW_EINVAL; }
int32_t fw_ppo_moment_count(void) { return 2 * kPMomentSlots; }   // (second half: unused since round 4 -- the moments live in registers during a call; kept for the ABI's buffer size)
int32_t fw_ppo_moment_map(int32_t obs_dim, int32_t* flat_index_of_slot) {
  if (obs_dim <= 0 || obs_dim > 64 || !flat_index_of_slot) { g_err = "fw_ppo_moment_map: bad arguments"; return FW_EINVAL; }
  ppo_moment_map(obs_dim, flat_index_of_slot);
  for (int i = kPMomentSlots; i < 2 * kPMomentSlots; ++i) flat_index_of_slot[i] = -1;
  return FW_OK;
}
// the action width of the *_a entry points: 4 (the entry points above) or 6 (the low-level control task)
static bool act_dim_ok(int32_t act_dim, const char* who) {
  if (act_dim == 4 || act_dim == 6) return true;
  g_err = std::string(who) + ": act_dim must be 4 or 6 (got " + std::to_string(act_dim) + ")";
  return false;
}
int32_t fw_ppo_param_count_a(int32_t obs_dim, int32_t act_dim) {
  if (!act_dim_ok(act_dim, "fw_ppo_param_count_a")) return FW_EINVAL;
  if (obs_dim <= 0) { g_err = "fw_ppo_param_count_a: obs_dim must be positive"; return FW_EINVAL; }
  return ppo_total_params_a((obs_dim + 1) & ~1, act_dim);
}
int32_t fw_ppo_moment_count_a(int32_t act_dim) {
  if (!act_dim_ok(act_dim, "fw_ppo_moment_count_a")) return FW_EINVAL;
  return 2 * ppo_moment_slots(act_dim);      // (the second half unused, as for fw_ppo_moment_count)
}
int32_t fw_ppo_moment_map_a(int32_t obs_dim, int32_t act_dim, int32_t* flat_index_of_slot) {
  if (!act_dim_ok(act_dim, "fw_ppo_moment_map_a")) return FW_EINVAL;
  if (obs_dim <= 0 || obs_dim > 64 || !flat_index_of_slot) { g_err = "fw_ppo_moment_map_a: bad arguments"; return FW_EINVAL; }
  const int ns = ppo_moment_slots(act_dim);
  ppo_moment_map(obs_dim, flat_index_of_slot, act_dim);
  for (int i = ns; i < 2 * ns; ++i) flat_index_of_slot[i] = -1;
  return FW_OK;
}
int32_t fw_ppo_param_count_a3(int32_t obs_dim) {
  if (obs_dim <= 0) { g_err = "fw_ppo_param_count_a3: obs_dim must be positive"; return FW_EINVAL; }
  return ppo_total_params_a((obs_dim + 1) & ~1, 3);
}
int32_t fw_ppo_moment_count_a3(void) { return 2 * ppo_moment_slots(3); }      // (the second half unused, as for fw_ppo_moment_count)
int32_t fw_ppo_moment_map_a3(int32_t obs_dim, int32_t* flat_index_of_slot) {
  if (obs_dim <= 0 || obs_dim > 64 || !flat_index_of_slot) { g_err = "fw_ppo_moment_map_a3: bad arguments"; return FW_EINVAL; }
  const int ns = ppo_moment_slots(3);
  ppo_moment_map(obs_dim, flat_index_of_slot, 3);
  for (int i = ns; i < 2 * ns; ++i) flat_index_of_slot[i] = -1;
  return FW_OK;
}

// Dev knob: FWSIM_SPIN_LOG2=k bounds every in-grid wait (fw_collect_step, fw_ppo_update) to 2^k polls instead of its default --
// tests use it to provoke the timeout paths and assert that the status words surface on the host side.
static long long spin_budget(long long dflt) {
  if (const char* e = getenv("FWSIM_SPIN_LOG2")) { const int k = atoi(e); if (k >= 0 && k < 40) return std::min(dflt, 1ll << k); }
  return dflt;
}

// workspace layout of fw_ppo_update: [0, kPpoWords x 8) exchange words (kPpoWordPaths: which exchanges shared an L2, kPpoWordStatus: include/fwsim.h) |
// gradient hand-off buffer | the packed rows of every minibatch, in walking order (fw_ppo_pack_kernel)
// (the words first -- everything that is polled -- and the data a whole 64 KB behind them: the blocks that wait spin on these lines with
// loads past their L1, and whatever part of the L2 serves the words should not also serve the first partial's tiles)
// (the KL-stop form's words, kPpoWordKl .., are part of kPpoWords -- zeroed per call with the rest -- and of this fixed region: the
// workspace-size functions cover them without growing)
static constexpr size_t kPpoWsXch = 65536;
static_assert(kPpoWords * sizeof(unsigned long long) <= kPpoWsXch, "exchange words");
static constexpr size_t kPpoWsGx = sizeof(float) * (4 * kPMaxSplit * (size_t)kPGxSlots);      // [parity][net][part]: gradient partial + weight share
static size_t ppo_ws_gx(int act_dim) { return sizeof(float) * (4 * kPMaxSplit * (size_t)ppo_gx_slots(act_dim)); }      // (4: kPpoWsGx)
int64_t fw_ppo_update_workspace_bytes(int32_t n_minibatches, int32_t batch_size, int32_t obs_dim) {
  if (n_minibatches <= 0 || batch_size <= 0 || obs_dim <= 0 || obs_dim > 64) return FW_EINVAL;
  return (int64_t)(kPpoWsXch + kPpoWsGx + sizeof(float) * (size_t)n_minibatches * (size_t)batch_size * (size_t)ppo_pack_width(obs_dim));
}
static int64_t ppo_workspace_bytes(int32_t n_minibatches, int32_t batch_size, int32_t obs_dim, int32_t act_dim) {
  return (int64_t)(kPpoWsXch + ppo_ws_gx(act_dim) + sizeof(float) * (size_t)n_minibatches * (size_t)batch_size * (size_t)ppo_pack_width(obs_dim, act_dim));
}
int64_t fw_ppo_update_workspace_bytes_a(int32_t n_minibatches, int32_t batch_size, int32_t obs_dim, int32_t act_dim) {
  if (!act_dim_ok(act_dim, "fw_ppo_update_workspace_bytes_a")) return FW_EINVAL;
  if (n_minibatches <= 0 || batch_size <= 0 || obs_dim <= 0 || obs_dim > 64) { g_err = "fw_ppo_update_workspace_bytes_a: bad arguments"; return FW_EINVAL; }
  return ppo_workspace_bytes(n_minibatches, batch_size, obs_dim, act_dim);
}
// the three-action learner (the high-level command task): the *_a family with the width fixed
int64_t fw_ppo_update_workspace_bytes_a3(int32_t n_minibatches, int32_t batch_size, int32_t obs_dim) {
  if (n_minibatches <= 0 || batch_size <= 0 || obs_dim <= 0 || obs_dim > 64) { g_err = "fw_ppo_update_workspace_bytes_a3: bad arguments"; return FW_EINVAL; }
  return ppo_workspace_bytes(n_minibatches, batch_size, obs_dim, 3);
}

// fw_ppo_update and fw_ppo_update_a (who: the entry point's name, for the messages)
static int32_t ppo_update(float* params, float* mom_m, float* mom_v, const float* obs, const float* act, const float* old_logp,
                          const float* adv, const float* ret, const int32_t* perm, int32_t n_minibatches, int32_t batch_size,
                          int32_t obs_dim, int32_t act_dim, const fw_ppo_hyper* hyper, float* loss_acc, void* workspace, int64_t workspace_bytes,
                          void* hip_stream, const char* who, float* diag = nullptr /* fw_ppo_update_diag: the diagnostics buffer, checked by the caller */,
                          const PpoKlArgs* kl = nullptr /* fw_ppo_update_kl: the limit and the count's place (its diag may be null), checked by the caller */) {
  static_assert(sizeof(fw_ppo_hyper) == sizeof(PpoHyper), "fw_ppo_hyper layout");
  const std::string w = who;
  if (!params || !mom_m || !mom_v || !obs || !act || !old_logp || !adv || !ret || !perm || !hyper || n_minibatches <= 0) {
    g_err = w + ": bad arguments"; return FW_EINVAL;
  }
  if (batch_size <= 0 || batch_size % 16 != 0) { g_err = w + ": batch_size must be a multiple of 16"; return FW_EINVAL; }
  if (obs_dim <= 0 || obs_dim > 64) { g_err = w + ": obs_dim must be in [1, 64]"; return FW_EINVAL; }
  const PpoWidth* width = ppo_width(act_dim);
  if (!width) { g_err = w + ": no learner is built for " + std::to_string(act_dim) + " actions"; return FW_EINVAL; }
  if (!workspace || workspace_bytes < ppo_workspace_bytes(n_minibatches, batch_size, obs_dim, act_dim)) {
    g_err = w + ": workspace smaller than " + width->ws_fn;
    return FW_EINVAL;
  }
  const size_t lds = ppo_lds_bytes(obs_dim, act_dim, kl != nullptr);
  if (lds > 160 * 1024) { g_err = w + ": networks do not fit the 160 KB of LDS"; return FW_EINVAL; }
  hipStream_t st = (hipStream_t)hip_stream;
  const int dev = device_of(params);
  DeviceGuard g(dev);
  // everything the blocks exchange lives in the caller's workspace: two learners (or two streams) never share a word
  unsigned long long* xch = (unsigned long long*)workspace;
  float* gx = (float*)((char*)workspace + kPpoWsXch);
  float* packed = (float*)((char*)workspace + kPpoWsXch + ppo_ws_gx(act_dim));
  HIP_TRY((fw_env*)nullptr, hipMemsetAsync(xch, 0, kPpoWords * sizeof(unsigned long long), st));
  PpoArgs A;
  A.params = params; A.mom_m = mom_m; A.mom_v = mom_v; A.packed = packed;
  A.n_mb = n_minibatches; A.B = batch_size; A.D = obs_dim; A.loss_acc = loss_acc; A.xch = xch; A.gx = gx;
  A.spin = spin_budget(kPpoSpin);
  A.flags = 0;
  if (const char* e = getenv("FWSIM_PPO_NO_L2_SWAP")) if (atoi(e) != 0) A.flags |= PPO_FLAG_NO_L2_SWAP;
  if (const char* e = getenv("FWSIM_PPO_WRITER")) if (!strcmp(e, "last")) A.flags |= PPO_FLAG_WRITER_LAST;
  std::memcpy(&A.H, hyper, sizeof A.H);
  if (batch_size <= 1 && A.H.norm_adv == 1) A.H.norm_adv = 0;      // SB3 skips the normalisation of single-sample minibatches
  // the parallel pre-pass: every minibatch's rows, in walking order, advantages normalised (one workgroup per minibatch, all CUs)
  PpoPackArgs P;
  P.obs = obs; P.act = act; P.old_logp = old_logp; P.adv = adv; P.ret = ret; P.perm = perm; P.B = batch_size; P.D = obs_dim;
  P.norm_adv = A.H.norm_adv; P.adv_mean = A.H.adv_mean; P.adv_std = A.H.adv_std; P.out = packed;
  {
    void* pargs[] = { &P };
    (void)hipLaunchKernel(width->pack, dim3(n_minibatches), dim3(256), pargs, 0, st);
  }
  // four / eight blocks per network: gradient tiles by reduce-scatter, updated weights by all-gather (FWSIM_PPO_RS=0: all-to-all, as for two
  // blocks -- written for up to four, so the cut is then chosen among round 4's)
  bool rs_env = true;
  if (const char* e = getenv("FWSIM_PPO_RS")) if (atoi(e) == 0) rs_env = false;
  PpoSplit cut = ppo_split(batch_size, rs_env ? kPMaxSplit : 4);      // samples per pass and blocks per network (128 samples: 16 x 8, 64: 16 x 4)
  if (const char* e = getenv("FWSIM_PPO_SPLIT")) {  // dev knob "CHxN" (64x2 = round 3's cut, 32x4 = round 4's for 128 samples): A / B measurements, tests of every form
    int ch = 0, ns = 0;
    if (sscanf(e, "%dx%d", &ch, &ns) == 2 && (ch == 16 || ch == 32 || ch == 64) && (ns == 1 || ns == 2 || ns == 4 || (ns == 8 && rs_env)) && batch_size % ch == 0 && batch_size / ch >= ns) {
      cut.ch = ch; cut.nsplit = ns;
    } else { g_err = w + ": FWSIM_PPO_SPLIT must be CHxN with CH in {16, 32, 64}, N in {1, 2, 4, 8} (8: not with FWSIM_PPO_RS=0), N chunks of CH samples in a minibatch"; return FW_EINVAL; }
  }
  const int ns = cut.nsplit >= 4 && rs_env ? cut.nsplit : 0;      // the kernel's NS: 0 = all-to-all swap of whole partials
  const dim3 grid(16 * cut.nsplit);                 // (every 8th block works -- see the kernel)
  const void* fn = ppo_update_kernel(act_dim, cut.ch, ns, kl ? PPO_FORM_KL : diag ? PPO_FORM_DIAG : PPO_FORM_PLAIN);
  if (!fn) { g_err = w + ": no kernel is built for " + std::to_string(cut.ch) + " samples per pass x " + std::to_string(ns) + " blocks per network"; return FW_EINVAL; }
  if (int rc = ensure_dynamic_lds(nullptr, dev, fn, lds)) return rc;
  void* args_plain[] = { &A };
  void* args_diag[] = { &A, &diag };                // (the diagnostics kernels take the buffer as a second parameter)
  PpoKlArgs K = kl ? *kl : PpoKlArgs{nullptr, nullptr, 0.f};
  void* args_kl[] = { &A, &K };                     // (the KL-stop kernels: the buffer, the count's place and the limit as one struct)
  (void)hipLaunchKernel(fn, grid, dim3(kPThreads), kl ? args_kl : diag ? args_diag : args_plain, lds, st);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}
int32_t fw_ppo_update(float* params, float* mom_m, float* mom_v, const float* obs, const float* act, const float* old_logp,
                      const float* adv, const float* ret, const int32_t* perm, int32_t n_minibatches, int32_t batch_size,
                      int32_t obs_dim, const fw_ppo_hyper* hyper, float* loss_acc, void* workspace, int64_t workspace_bytes,
                      void* hip_stream) {
  return ppo_update(params, mom_m, mom_v, obs, act, old_logp, adv, ret, perm, n_minibatches, batch_size, obs_dim, 4, hyper, loss_acc,
                    workspace, workspace_bytes, hip_stream, "fw_ppo_update");
}
int32_t fw_ppo_update_a(float* params, float* mom_m, float* mom_v, const float* obs, const float* act, const float* old_logp,
                        const float* adv, const float* ret, const int32_t* perm, int32_t n_minibatches, int32_t batch_size,
                        int32_t obs_dim, int32_t act_dim, const fw_ppo_hyper* hyper, float* loss_acc, void* workspace, int64_t workspace_bytes,
                        void* hip_stream) {
  if (!act_dim_ok(act_dim, "fw_ppo_update_a")) return FW_EINVAL;
  return ppo_update(params, mom_m, mom_v, obs, act, old_logp, adv, ret, perm, n_minibatches, batch_size, obs_dim, act_dim, hyper, loss_acc,
                    workspace, workspace_bytes, hip_stream, "fw_ppo_update_a");
}
int32_t fw_ppo_update_a3(float* params, float* mom_m, float* mom_v, const float* obs, const float* act, const float* old_logp,
                         const float* adv, const float* ret, const int32_t* perm, int32_t n_minibatches, int32_t batch_size,
                         int32_t obs_dim, const fw_ppo_hyper* hyper, float* loss_acc, void* workspace, int64_t workspace_bytes,
                         void* hip_stream) {
  return ppo_update(params, mom_m, mom_v, obs, act, old_logp, adv, ret, perm, n_minibatches, batch_size, obs_dim, 3, hyper, loss_acc,
                    workspace, workspace_bytes, hip_stream, "fw_ppo_update_a3");
}
// the diagnostics form: the same call on the diagnostics instantiation of the same kernel row
int64_t fw_ppo_diag_floats(int32_t n_minibatches) {
  if (n_minibatches <= 0) { g_err = "fw_ppo_diag_floats: n_minibatches must be positive"; return FW_EINVAL; }
  return (int64_t)ppo_diag_floats(n_minibatches);
}
int32_t fw_ppo_update_diag(float* params, float* mom_m, float* mom_v, const float* obs, const float* act, const float* old_logp,
                           const float* adv, const float* ret, const int32_t* perm, int32_t n_minibatches, int32_t batch_size,
                           int32_t obs_dim, int32_t act_dim, const fw_ppo_hyper* hyper, float* loss_acc, void* workspace, int64_t workspace_bytes,
                           void* hip_stream, float* diag, int64_t diag_floats) {
  if (act_dim != 3 && act_dim != 4 && act_dim != 6) { g_err = "fw_ppo_update_diag: act_dim must be 3, 4 or 6 (got " + std::to_string(act_dim) + ")"; return FW_EINVAL; }
  if (!diag) { g_err = "fw_ppo_update_diag: diag is NULL"; return FW_EINVAL; }
  if (n_minibatches <= 0) { g_err = "fw_ppo_update_diag: n_minibatches must be positive"; return FW_EINVAL; }
  if (diag_floats < (int64_t)ppo_diag_floats(n_minibatches)) {
    g_err = "fw_ppo_update_diag: diag smaller than fw_ppo_diag_floats(n_minibatches)"; return FW_EINVAL;
  }
  return ppo_update(params, mom_m, mom_v, obs, act, old_logp, adv, ret, perm, n_minibatches, batch_size, obs_dim, act_dim, hyper, loss_acc,
                    workspace, workspace_bytes, hip_stream, "fw_ppo_update_diag", diag);
}

// the KL-stop form: the same call on the KL-stop instantiation of the same kernel row
int32_t fw_ppo_update_kl(float* params, float* mom_m, float* mom_v, const float* obs, const float* act, const float* old_logp,
                         const float* adv, const float* ret, const int32_t* perm, int32_t n_minibatches, int32_t batch_size,
                         int32_t obs_dim, int32_t act_dim, const fw_ppo_hyper* hyper, float* loss_acc, void* workspace, int64_t workspace_bytes,
                         void* hip_stream, float* diag, int64_t diag_floats, float target_kl, int32_t* minibatches_stepped) {
  if (act_dim != 3 && act_dim != 4 && act_dim != 6) { g_err = "fw_ppo_update_kl: act_dim must be 3, 4 or 6 (got " + std::to_string(act_dim) + ")"; return FW_EINVAL; }
  if (!(target_kl > 0.f) || !std::isfinite(target_kl)) { g_err = "fw_ppo_update_kl: target_kl must be positive and finite"; return FW_EINVAL; }
  if (!minibatches_stepped) { g_err = "fw_ppo_update_kl: minibatches_stepped is NULL"; return FW_EINVAL; }
  if (n_minibatches <= 0) { g_err = "fw_ppo_update_kl: n_minibatches must be positive"; return FW_EINVAL; }
  if (diag && diag_floats < (int64_t)ppo_diag_floats(n_minibatches)) {
    g_err = "fw_ppo_update_kl: diag smaller than fw_ppo_diag_floats(n_minibatches)"; return FW_EINVAL;
  }
  const PpoKlArgs K{diag, minibatches_stepped, (float)(1.5 * (double)target_kl)};      // SB3: approx_kl > 1.5 * target_kl
  return ppo_update(params, mom_m, mom_v, obs, act, old_logp, adv, ret, perm, n_minibatches, batch_size, obs_dim, act_dim, hyper, loss_acc,
                    workspace, workspace_bytes, hip_stream, "fw_ppo_update_kl", nullptr, &K);
}

int32_t fw_ppo_update_status(const void* workspace, int64_t workspace_bytes, uint32_t* status_out, uint32_t* paths_out, void* hip_stream) {
  if (!workspace || workspace_bytes < (int64_t)kPpoWsXch || !status_out) { g_err = "fw_ppo_update_status: bad arguments"; return FW_EINVAL; }
  DeviceGuard g(device_of(workspace));
  unsigned long long w[2] = {0ull, 0ull};
  HIP_TRY((fw_env*)nullptr, hipMemcpyAsync(w, (const unsigned long long*)workspace + kPpoWordPaths, sizeof w, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  HIP_TRY((fw_env*)nullptr, hipStreamSynchronize((hipStream_t)hip_stream));
  static_assert(kPpoWordStatus == kPpoWordPaths + 1 && kPpoWordStatus < kPpoWords, "exchange-word layout");
  static_assert(FW_PPO_ST_IDS == PPO_ST_IDS && FW_PPO_ST_SWAP == PPO_ST_SWAP && FW_PPO_ST_NORM == PPO_ST_NORM && FW_PPO_ST_COMMIT == PPO_ST_COMMIT, "status bits of include/fwsim.h");
  if (paths_out) *paths_out = (uint32_t)w[0];
  *status_out = (uint32_t)w[1];
  return FW_OK;
}

// fw_policy_act / fw_collect_act and their *_a forms (who: the entry point's name, for the messages)
static int32_t policy_act(const float* params, const float* obs, int32_t N, int32_t obs_dim, int32_t act_dim, int32_t nets, int32_t deterministic,
                          const uint64_t* rng, int64_t env_offset, float* obs_copy, float* act_raw, void* act_env, int32_t act_is_f64,
                          float* logp, float* value, void* hip_stream, const char* who) {
  const std::string w = who;
  if (!params || !obs || N <= 0 || obs_dim <= 0 || obs_dim > 64 || (nets & ~3) || !nets) { g_err = w + ": bad arguments"; return FW_EINVAL; }
  if ((nets & 1) && (!act_raw || !act_env || !logp || (!deterministic && !rng))) { g_err = w + ": policy outputs missing"; return FW_EINVAL; }
  if ((nets & 2) && !value) { g_err = w + ": value output missing"; return FW_EINVAL; }
  const size_t lds = act_lds_bytes(obs_dim, act_dim);
  const int dev = device_of(params);
  DeviceGuard g(dev);
  ActArgs A;
  std::memset(&A, 0, sizeof A);
  A.params = params; A.obs = obs; A.N = N; A.D = obs_dim; A.nets = nets; A.deterministic = deterministic; A.act_is_f64 = act_is_f64;
  A.rng = rng; A.env_offset = env_offset; A.obs_copy = obs_copy; A.act_raw = act_raw; A.act_env = act_env; A.logp = logp; A.value = value;
  A.raw = nullptr; A.raw_is_f64 = 0; A.mean = A.var = nullptr; A.clip = A.eps = 0.f; A.terminated = A.truncated = nullptr;
  return launch_policy_act(dev, act_dim, A, lds, (hipStream_t)hip_stream);
}
int32_t fw_policy_act(const float* params, const float* obs, int32_t N, int32_t obs_dim, int32_t nets, int32_t deterministic,
                      const uint64_t* rng, int64_t env_offset, float* obs_copy, float* act_raw, void* act_env, int32_t act_is_f64,
                      float* logp, float* value, void* hip_stream) {
  return policy_act(params, obs, N, obs_dim, 4, nets, deterministic, rng, env_offset, obs_copy, act_raw, act_env, act_is_f64, logp, value,
                    hip_stream, "fw_policy_act");
}
int32_t fw_policy_act_a(const float* params, const float* obs, int32_t N, int32_t obs_dim, int32_t act_dim, int32_t nets, int32_t deterministic,
                        const uint64_t* rng, int64_t env_offset, float* obs_copy, float* act_raw, void* act_env, int32_t act_is_f64,
                        float* logp, float* value, void* hip_stream) {
  if (!act_dim_ok(act_dim, "fw_policy_act_a")) return FW_EINVAL;
  return policy_act(params, obs, N, obs_dim, act_dim, nets, deterministic, rng, env_offset, obs_copy, act_raw, act_env, act_is_f64, logp, value,
                    hip_stream, "fw_policy_act_a");
}

static int32_t collect_act(const float* params, const void* raw_obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim, int32_t act_dim,
                           const double* obs_mean, const double* obs_var, float clip_obs, float eps_obs, int32_t nets, int32_t deterministic,
                           const uint64_t* rng, int64_t env_offset, float* obs_copy, float* act_raw, void* act_env, int32_t act_is_f64,
                           float* logp, float* value, const void* prev_reward, const uint8_t* prev_terminated, const uint8_t* prev_truncated,
                           const void* prev_terminal_obs, const double* ret_var, int32_t norm_reward, float clip_reward, float eps_reward,
                           float gamma, float* rew_out, float* start_out, void* hip_stream, const char* who) {
  const std::string w = who;
  if (!params || !raw_obs || !obs_mean || !obs_var || N <= 0 || obs_dim <= 0 || obs_dim > 64 || (nets & ~3) || !nets) { g_err = w + ": bad arguments"; return FW_EINVAL; }
  if ((nets & 1) && (!act_raw || !act_env || !logp || (!deterministic && !rng))) { g_err = w + ": policy outputs missing"; return FW_EINVAL; }
  if ((nets & 2) && !value) { g_err = w + ": value output missing"; return FW_EINVAL; }
  if (prev_reward && (!(nets & 2) || !prev_terminated || !prev_truncated || !prev_terminal_obs || !ret_var || !rew_out || !start_out)) {
    g_err = w + ": finalising the previous step needs the value network and all of its buffers"; return FW_EINVAL;
  }
  const size_t lds = act_lds_bytes(obs_dim, act_dim);
  const int dev = device_of(params);
  DeviceGuard g(dev);
  ActArgs A;
  std::memset(&A, 0, sizeof A);
  A.params = params; A.N = N; A.D = obs_dim; A.nets = nets; A.deterministic = deterministic; A.act_is_f64 = act_is_f64;
  A.rng = rng; A.env_offset = env_offset; A.obs_copy = obs_copy; A.act_raw = act_raw; A.act_env = act_env; A.logp = logp; A.value = value;
  A.raw = raw_obs; A.raw_is_f64 = obs_is_f64; A.mean = obs_mean; A.var = obs_var; A.clip = clip_obs; A.eps = eps_obs;
  A.prev_reward = prev_reward; A.prev_term = prev_terminated; A.prev_trunc = prev_truncated; A.prev_tobs = prev_terminal_obs;
  A.ret_var = ret_var; A.norm_reward = norm_reward; A.clip_reward = clip_reward; A.rew_eps = eps_reward; A.gamma = gamma;
  A.rew_out = rew_out; A.start_out = start_out;
  return launch_policy_act(dev, act_dim, A, lds, (hipStream_t)hip_stream);
}
int32_t fw_collect_act(const float* params, const void* raw_obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim, const double* obs_mean,
                       const double* obs_var, float clip_obs, float eps_obs, int32_t nets, int32_t deterministic, const uint64_t* rng,
                       int64_t env_offset, float* obs_copy, float* act_raw, void* act_env, int32_t act_is_f64, float* logp, float* value,
                       const void* prev_reward, const uint8_t* prev_terminated, const uint8_t* prev_truncated, const void* prev_terminal_obs,
                       const double* ret_var, int32_t norm_reward, float clip_reward, float eps_reward, float gamma, float* rew_out,
                       float* start_out, void* hip_stream) {
  return collect_act(params, raw_obs, obs_is_f64, N, obs_dim, 4, obs_mean, obs_var, clip_obs, eps_obs, nets, deterministic, rng, env_offset,
                     obs_copy, act_raw, act_env, act_is_f64, logp, value, prev_reward, prev_terminated, prev_truncated, prev_terminal_obs,
                     ret_var, norm_reward, clip_reward, eps_reward, gamma, rew_out, start_out, hip_stream, "fw_collect_act");
}
int32_t fw_collect_act_a(const float* params, const void* raw_obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim, int32_t act_dim,
                         const double* obs_mean, const double* obs_var, float clip_obs, float eps_obs, int32_t nets, int32_t deterministic,
                         const uint64_t* rng, int64_t env_offset, float* obs_copy, float* act_raw, void* act_env, int32_t act_is_f64, float* logp,
                         float* value, const void* prev_reward, const uint8_t* prev_terminated, const uint8_t* prev_truncated,
                         const void* prev_terminal_obs, const double* ret_var, int32_t norm_reward, float clip_reward, float eps_reward,
                         float gamma, float* rew_out, float* start_out, void* hip_stream) {
  if (!act_dim_ok(act_dim, "fw_collect_act_a")) return FW_EINVAL;
  return collect_act(params, raw_obs, obs_is_f64, N, obs_dim, act_dim, obs_mean, obs_var, clip_obs, eps_obs, nets, deterministic, rng, env_offset,
                     obs_copy, act_raw, act_env, act_is_f64, logp, value, prev_reward, prev_terminated, prev_truncated, prev_terminal_obs,
                     ret_var, norm_reward, clip_reward, eps_reward, gamma, rew_out, start_out, hip_stream, "fw_collect_act_a");
}

// fw_collect_act_hl's kernel by (dtype, lane mapping): the table the launch and the LDS opt-in look it up in
static const void* collect_act_hl_kernel(bool f64, int lanes) {
  struct Row { bool f64; int lanes; const void* fn; };
  static const Row rows[] = {
    {true, 8, kfn(fw_collect_act_hl_kernel<double, 8>)}, {true, 1, kfn(fw_collect_act_hl_kernel<double, 1>)},
    {false, 8, kfn(fw_collect_act_hl_kernel<float, 8>)}, {false, 1, kfn(fw_collect_act_hl_kernel<float, 1>)},
  };
  for (const Row& r : rows) if (r.f64 == f64 && r.lanes == lanes) return r.fn;
  return nullptr;
}
int32_t fw_sizeof_collect_hl_args(void) { return (int32_t)sizeof(fw_collect_hl_args); }
int32_t fw_collect_act_hl(fw_handle h, const fw_collect_hl_args* a, void* hip_stream) {
  if (!h) { g_err = "fw_collect_act_hl: NULL handle"; return FW_EINVAL; }
  if (h->cfg.task != FW_TASK_WAYPOINTS_DIRECT) { h->err = "fw_collect_act_hl: only the direct-command waypoints task (FW_TASK_WAYPOINTS_DIRECT) takes high-level commands"; return FW_EUNSUPPORTED; }
  if (h->cfg.angle_representation != 0) { h->err = "fw_collect_act_hl: the low-level controller's observation needs the euler attitude (angle_representation 0)"; return FW_EUNSUPPORTED; }
  if (!a) { h->err = "fw_collect_act_hl: NULL arguments"; return FW_EINVAL; }
  const int32_t nets = a->nets;
  if (!a->params || !a->obs || !a->obs_mean || !a->obs_var || (nets & ~3) || !nets) { h->err = "fw_collect_act_hl: bad arguments"; return FW_EINVAL; }
  if ((nets & 1) && (!a->low_params || !a->low_mean || !a->low_var || !a->act_raw || !a->logp || !a->low_obs || !a->cmd_out || !a->act_env ||
                     (!a->deterministic && !a->rng))) {
    h->err = "fw_collect_act_hl: the policy block needs low_params, low_mean, low_var, act_raw, logp, low_obs, cmd_out, act_env (and rng unless deterministic)";
    return FW_EINVAL;
  }
  if ((nets & 2) && !a->value) { h->err = "fw_collect_act_hl: value output missing"; return FW_EINVAL; }
  if (a->prev_reward && (!(nets & 2) || !a->prev_terminated || !a->prev_truncated || !a->prev_terminal_obs || !a->ret_var || !a->rew_out || !a->start_out)) {
    h->err = "fw_collect_act_hl: finalising the previous step needs the value network and all of its buffers"; return FW_EINVAL;
  }
  const int D = obs_dim_of(&h->cfg), f64 = h->cfg.dtype == FW_F64;
  const size_t lds = hl_act_lds_bytes(D);
  if (lds > 160 * 1024) { h->err = "fw_collect_act_hl: the two networks do not fit the 160 KB of LDS"; return FW_EINVAL; }
  DeviceGuard g(h->device);
  HlActArgs HA;
  std::memset(&HA, 0, sizeof HA);
  ActArgs& A = HA.A;
  A.params = a->params; A.N = h->n; A.D = D; A.nets = nets; A.deterministic = a->deterministic; A.act_is_f64 = f64;
  A.rng = a->rng; A.env_offset = a->env_offset; A.obs_copy = a->obs_copy; A.act_raw = a->act_raw; A.act_env = a->act_env; A.logp = a->logp; A.value = a->value;
  A.raw = a->obs; A.raw_is_f64 = f64; A.mean = a->obs_mean; A.var = a->obs_var; A.clip = a->clip_obs; A.eps = a->eps_obs;
  A.prev_reward = a->prev_reward; A.prev_term = a->prev_terminated; A.prev_trunc = a->prev_truncated; A.prev_tobs = a->prev_terminal_obs;
  A.ret_var = a->ret_var; A.norm_reward = a->norm_reward; A.clip_reward = a->clip_reward; A.rew_eps = a->eps_reward; A.gamma = a->gamma;
  A.rew_out = a->rew_out; A.start_out = a->start_out;
  HA.low_params = a->low_params; HA.low_mean = a->low_mean; HA.low_var = a->low_var; HA.low_clip = a->low_clip; HA.low_eps = a->low_eps;
  HA.low_obs = a->low_obs; HA.cmd_out = a->cmd_out; HA.rejected = a->rejected; HA.dome = h->cfg.flight_dome_size;
  const void* fn = collect_act_hl_kernel(f64 != 0, h->lanes_per_env == 8 ? 8 : 1);
  if (int rc = ensure_dynamic_lds(h, h->device, fn, lds)) return rc;
  int rc = FW_OK;
  with_dtype(h, [&](auto t) {
    using T = decltype(t);
    DevState<T> Dg = dev_state<T>(h);
    void* args[] = { &Dg, &HA };
    (void)hipLaunchKernel(fn, dim3((unsigned)((h->n + kPChunk - 1) / kPChunk), 2), dim3(kPThreads), args, lds, (hipStream_t)hip_stream);
  });
  HIP_TRY(h, hipGetLastError());
  return rc;
}

int64_t fw_collect_step_workspace_bytes(fw_handle h) { return h ? (int64_t)collect_ws(h).total : FW_EINVAL; }

// checks and argument block shared by fw_collect_step and fw_collect_close
static int32_t collect_fill(fw_handle h, const fw_collect_args* a, const char* who, bool close, CollectArgs& CA) {
  if (h->cfg.task == FW_TASK_LOWLEVEL) {
    h->err = std::string(who) + " serves the four-action tasks; the low-level task's six actions go through the policy in torch and fw_step";
    return FW_EUNSUPPORTED;
  }
  if (h->cfg.task == FW_TASK_WAYPOINTS_DIRECT) {
    h->err = std::string(who) + " serves the four-action tasks; the direct-command waypoints task's six actions go through fw_collect_act_a and fw_step";
    return FW_EUNSUPPORTED;
  }
  if (h->lanes_per_env != 8) {
    h->err = std::string(who) + " serves the 8-lanes-per-env mapping (what fw_create picks for waypoints up to 24576 envs per GPU, 12288 with wind, and "
             "for the camera tasks up to 16384 envs or at any size with obstacles); use fw_collect_act / fw_step / fw_collect_stats";
    return FW_EUNSUPPORTED;
  }
  const int D = obs_dim_of(&h->cfg), N = h->n;
  if (D > 62) { h->err = std::string(who) + ": obs_dim must be <= 62"; return FW_EINVAL; }
  const bool pol = close || (a->act_raw && a->act_env && a->logp && (a->deterministic || a->rng));
  if (!a->params || !a->obs_mean || !a->obs_var || !a->obs_count || !a->returns || !a->ret_mean || !a->ret_var || !a->ret_count ||
      !pol || !a->value || !a->obs || !a->reward || !a->terminated || !a->truncated || !a->terminal_obs ||
      (!a->rew_out != !a->start_out) || (close && !a->rew_out)) { h->err = std::string(who) + ": missing buffers"; return FW_EINVAL; }
  const CollectWs W = collect_ws(h);
  if (!a->workspace || a->workspace_bytes < (int64_t)W.total) { h->err = std::string(who) + ": workspace smaller than fw_collect_step_workspace_bytes()"; return FW_EINVAL; }
  const int f64 = h->cfg.dtype == FW_F64;
  std::memset(&CA, 0, sizeof CA);
  CA.n_chunks = (N + kCRows - 1) / kCRows;
  CA.n_act = (2 * CA.n_chunks + 1 + 7) & ~7;                 // act waves + the merge wave, padded: the step waves keep their XCD alignment
  CA.nblk = (int32_t)(h->npad / 8);
  ActArgs& A = CA.A;
  A.params = a->params; A.N = N; A.D = D; A.nets = close ? 2 : 3; A.deterministic = a->deterministic; A.act_is_f64 = f64;
  A.rng = a->rng; A.env_offset = h->env_offset; A.obs_copy = a->obs_copy; A.act_raw = a->act_raw; A.act_env = a->act_env; A.logp = a->logp; A.value = a->value;
  A.raw = a->obs; A.raw_is_f64 = f64; A.mean = a->obs_mean; A.var = a->obs_var; A.clip = a->clip_obs; A.eps = a->eps_obs;
  if (a->rew_out) {
    A.prev_reward = a->reward; A.prev_term = a->terminated; A.prev_trunc = a->truncated; A.prev_tobs = a->terminal_obs;
    A.rew_out = a->rew_out; A.start_out = a->start_out;
  }
  A.ret_var = a->ret_var; A.norm_reward = a->norm_reward; A.clip_reward = a->clip_reward; A.rew_eps = a->eps_reward; A.gamma = (float)a->gamma;
  StatsArgs& S = CA.S;
  S.obs = a->obs; S.obs_is_f64 = f64; S.N = N; S.D = D; S.mean = a->obs_mean; S.var = a->obs_var; S.count = a->obs_count; S.update_obs = a->update_obs;
  S.reward = a->reward; S.rew_is_f64 = f64; S.terminated = a->terminated; S.truncated = a->truncated; S.returns = a->returns;
  S.ret_mean = a->ret_mean; S.ret_var = a->ret_var; S.ret_count = a->ret_count; S.update_ret = a->update_ret; S.gamma = a->gamma; S.rng = a->rng;
  S.obs_acc = a->obs_acc; S.ret_acc = a->ret_acc;
  char* ws = (char*)a->workspace;
  CA.part1 = (double*)(ws + W.part1); CA.tot = (double*)(ws + W.tot);
  CA.flag_p = (unsigned int*)(ws + W.flag_p); CA.flag_v = (unsigned int*)(ws + W.flag_v);
  CA.sync = (unsigned int*)(ws + W.sync);
  CA.trace = close ? nullptr : (long long*)a->trace;
  CA.spin = (int32_t)spin_budget(kCollectSpin);
  return FW_OK;
}

int32_t fw_collect_step(fw_handle h, const fw_collect_args* a, void* hip_stream) {
  if (!h || !a) return FW_EINVAL;
  CollectArgs CA;
  if (int32_t rc = collect_fill(h, a, "fw_collect_step", false, CA)) return rc;
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)hip_stream;
  if (h->collect_act_seen != a->act_env) {
    // a new action buffer: every word "not there yet" (NaN) -- the step waves see their actions replace it and put it back at the
    // end of a launch.  (Stream-ordered; harmless if a captured graph replays it: between launches the words are NaN anyway.)
    const size_t bytes = (size_t)h->n * 4 * (h->cfg.dtype == FW_F64 ? 8 : 4);
    HIP_TRY(h, hipMemsetAsync(a->act_env, 0xFF, bytes, st));      // all-ones words: a NaN in float32 and in float64
    h->collect_act_seen = a->act_env;
  }
  return with_dtype(h, [&](auto t) { return collect_step_T<decltype(t)>(h, CA, a->act_env, a->obs, a->reward, a->terminated, a->truncated, a->terminal_obs, a->info_i32, st); });
}

int32_t fw_collect_close(fw_handle h, const fw_collect_args* a, const fw_collect_close_args* c, void* hip_stream) {
  if (!h || !a || !c) return FW_EINVAL;
  CollectArgs CA;
  if (int32_t rc = collect_fill(h, a, "fw_collect_close", true, CA)) return rc;
  if (!c->rewards || !c->values || !c->episode_starts || !c->adv || !c->ret || c->T <= 0) { h->err = "fw_collect_close: missing GAE buffers"; return FW_EINVAL; }
  if (a->rew_out != c->rewards + (size_t)(c->T - 1) * h->n) { h->err = "fw_collect_close: rew_out must be row T - 1 of the rewards buffer"; return FW_EINVAL; }
  DeviceGuard g(h->device);
  CloseArgs GA;
  GA.rewards = c->rewards; GA.values = c->values; GA.episode_starts = c->episode_starts; GA.adv = c->adv; GA.ret = c->ret;
  GA.T = c->T; GA.gamma = c->gae_gamma; GA.lam = c->gae_lambda;
  const size_t lds = collect_act_lds_bytes(CA.A.D);
  hipStream_t st = (hipStream_t)hip_stream;
  with_dtype(h, [&](auto t) { hipLaunchKernelGGL(fw_collect_close_kernel<decltype(t)>, dim3((unsigned)CA.n_chunks + 1), dim3(64), lds, st, CA, GA); });
  HIP_TRY(h, hipGetLastError());
  return FW_OK;
}

int32_t fw_collect_workspace_init(fw_handle h, void* workspace, int64_t workspace_bytes, void* hip_stream) {
  if (!h) return FW_EINVAL;
  if (h->lanes_per_env != 8) { h->err = "fw_collect_workspace_init: this handle's lane mapping has no fw_collect_step"; return FW_EUNSUPPORTED; }
  const CollectWs W = collect_ws(h);
  if (!workspace || workspace_bytes < (int64_t)W.total) { h->err = "fw_collect_workspace_init: workspace smaller than fw_collect_step_workspace_bytes()"; return FW_EINVAL; }
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)hip_stream;
  char* ws = (char*)workspace;
  HIP_TRY(h, hipMemsetAsync(ws, 0, W.total, st));
  const size_t n = (W.tot - W.part1) / sizeof(double);
  hipLaunchKernelGGL(fw_collect_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (double*)(ws + W.part1), n, (unsigned int*)(ws + W.sync));
  HIP_TRY(h, hipGetLastError());
  return FW_OK;
}

int32_t fw_collect_finish(fw_handle h, const fw_collect_args* a, void* hip_stream) {
  if (!h || !a) return FW_EINVAL;
  if (h->lanes_per_env != 8) { h->err = "fw_collect_finish: this handle's lane mapping has no fw_collect_step"; return FW_EUNSUPPORTED; }
  if (!a->obs_mean || !a->obs_var || !a->obs_count || !a->ret_mean || !a->ret_var || !a->ret_count) { h->err = "fw_collect_finish: missing statistics buffers"; return FW_EINVAL; }
  const CollectWs W = collect_ws(h);
  if (!a->workspace || a->workspace_bytes < (int64_t)W.total) { h->err = "fw_collect_finish: workspace smaller than fw_collect_step_workspace_bytes()"; return FW_EINVAL; }
  DeviceGuard g(h->device);
  CollectArgs CA;
  std::memset(&CA, 0, sizeof CA);
  CA.n_chunks = (h->n + kCRows - 1) / kCRows; CA.nblk = (int32_t)(h->npad / 8);
  StatsArgs& S = CA.S;
  S.N = h->n; S.D = obs_dim_of(&h->cfg); S.mean = a->obs_mean; S.var = a->obs_var; S.count = a->obs_count; S.update_obs = a->update_obs;
  S.ret_mean = a->ret_mean; S.ret_var = a->ret_var; S.ret_count = a->ret_count; S.update_ret = a->update_ret; S.obs_acc = a->obs_acc; S.ret_acc = a->ret_acc;
  char* ws = (char*)a->workspace;
  CA.part1 = (double*)(ws + W.part1); CA.tot = (double*)(ws + W.tot); CA.sync = (unsigned int*)(ws + W.sync);
  hipLaunchKernelGGL(fw_collect_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, CA);
  HIP_TRY(h, hipGetLastError());
  return FW_OK;
}

int32_t fw_collect_status(fw_handle h, const void* workspace, int64_t workspace_bytes, uint32_t* status_out, void* hip_stream) {
  if (!h || !status_out) return FW_EINVAL;
  const CollectWs W = collect_ws(h);
  if (!workspace || workspace_bytes < (int64_t)W.total) { h->err = "fw_collect_status: workspace smaller than fw_collect_step_workspace_bytes()"; return FW_EINVAL; }
  static_assert(FW_COLLECT_ST_ACTIONS == CS_ST_ACTIONS && FW_COLLECT_ST_FOLD == CS_ST_FOLD && FW_COLLECT_ST_MERGE == CS_ST_MERGE &&
                FW_COLLECT_ST_NOINIT == CS_ST_NOINIT && FW_COLLECT_ST_EPOCH == CS_ST_EPOCH && FW_COLLECT_ST_NANACT == CS_ST_NANACT, "status bits of include/fwsim.h");
  DeviceGuard g(h->device);
  uint32_t w = 0;
  HIP_TRY(h, hipMemcpyAsync(&w, (const char*)workspace + W.sync + sizeof(uint32_t) * CS_STATUS, sizeof w, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  HIP_TRY(h, hipStreamSynchronize((hipStream_t)hip_stream));
  *status_out = w;
  return FW_OK;
}

static int collect_stats_blocks(int N) { return N >= 64 * 64 ? 64 : (N + 63) / 64; }
int64_t fw_collect_stats_workspace_bytes(int32_t D) { return D > 0 ? (int64_t)(sizeof(double) * 64 * (2 * (size_t)D + 2) + 64) : FW_EINVAL; }

int32_t fw_collect_stats(const void* obs, int32_t obs_is_f64, int32_t N, int32_t D, double* obs_mean, double* obs_var, double* obs_count,
                         int32_t update_obs, const void* reward, int32_t rew_is_f64, const uint8_t* terminated, const uint8_t* truncated,
                         double* returns, double* ret_mean, double* ret_var, double* ret_count, int32_t update_ret, double gamma,
                         uint64_t* rng, void* workspace, double* obs_acc, double* ret_acc, void* hip_stream) {
  if (!obs || !obs_mean || !obs_var || !obs_count || !reward || !terminated || !truncated || !returns || !ret_mean || !ret_var || !ret_count ||
      !workspace || N <= 0 || D <= 0 || D > 256) { g_err = "fw_collect_stats: bad arguments"; return FW_EINVAL; }
  DeviceGuard g(device_of(obs));
  StatsArgs A;
  A.obs = obs; A.obs_is_f64 = obs_is_f64; A.N = N; A.D = D; A.mean = obs_mean; A.var = obs_var; A.count = obs_count; A.update_obs = update_obs;
  A.reward = reward; A.rew_is_f64 = rew_is_f64; A.terminated = terminated; A.truncated = truncated; A.returns = returns;
  A.ret_mean = ret_mean; A.ret_var = ret_var; A.ret_count = ret_count; A.update_ret = update_ret; A.gamma = gamma; A.rng = rng;
  A.part = (double*)workspace; A.ticket = (unsigned int*)((char*)workspace + sizeof(double) * 64 * (2 * (size_t)D + 2));
  A.obs_acc = obs_acc; A.ret_acc = ret_acc;
  const int nb = collect_stats_blocks(N);
  with_real(obs_is_f64 != 0, [&](auto t) { hipLaunchKernelGGL(fw_collect_stats_kernel<decltype(t)>, dim3(nb), dim3(256), 0, (hipStream_t)hip_stream, A); });
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int32_t fw_policy_terminal_value(const float* params, const void* terminal_obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim,
                                 const double* mean, const double* var, float clip, float eps, const uint8_t* terminated,
                                 const uint8_t* truncated, float* value, void* hip_stream) {
  if (!params || !terminal_obs || !mean || !var || !terminated || !truncated || !value || N <= 0 || obs_dim <= 0 || obs_dim > 64) {
    g_err = "fw_policy_terminal_value: bad arguments"; return FW_EINVAL;
  }
  const size_t lds = act_lds_bytes(obs_dim);
  const int dev = device_of(params);
  DeviceGuard g(dev);
  ActArgs A;
  std::memset(&A, 0, sizeof A);
  A.params = params; A.N = N; A.D = obs_dim; A.nets = 2; A.deterministic = 1; A.value = value;
  A.raw = terminal_obs; A.raw_is_f64 = obs_is_f64; A.mean = mean; A.var = var; A.clip = clip; A.eps = eps;
  A.terminated = terminated; A.truncated = truncated;
  return launch_policy_act(dev, 4, A, lds, (hipStream_t)hip_stream);
}

int32_t fw_rollout_post(const void* reward, int32_t rew_is_f64, const uint8_t* terminated, const uint8_t* truncated, const float* tvalue,
                        double* returns, double* ret_mean, double* ret_var, double* ret_count, int32_t N, int32_t training,
                        int32_t norm_reward, double gamma, float clip_reward, float epsilon, float* rew_out, float* start_out,
                        uint64_t* rng, double* ret_acc, void* hip_stream) {
  if (!reward || !terminated || !truncated || !tvalue || !returns || !ret_mean || !ret_var || !ret_count || !rew_out || !start_out || N <= 0) {
    g_err = "fw_rollout_post: bad arguments"; return FW_EINVAL;
  }
  DeviceGuard g(device_of(returns));
  PostArgs A;
  A.reward = reward; A.rew_is_f64 = rew_is_f64; A.terminated = terminated; A.truncated = truncated; A.tvalue = tvalue; A.returns = returns;
  A.ret_mean = ret_mean; A.ret_var = ret_var; A.ret_count = ret_count; A.N = N; A.training = training; A.norm_reward = norm_reward;
  A.gamma = gamma; A.clip_reward = clip_reward; A.epsilon = epsilon; A.rew_out = rew_out; A.start_out = start_out; A.rng = rng; A.ret_acc = ret_acc;
  hipLaunchKernelGGL(fw_rollout_post_kernel, dim3(1), dim3(1024), 0, (hipStream_t)hip_stream, A);
  HIP_TRY((fw_env*)nullptr, hipGetLastError());
  return FW_OK;
}

int32_t fw_probe(fw_handle h, int32_t op, int32_t variant, const double* in, int32_t in_cols, double* out, int32_t out_cols,
                 int32_t n, void* hip_stream) {
  if (!h) { g_err = "fw_probe: the handle must be non-NULL"; return FW_EINVAL; }
  if (!in || !out) { h->err = "fw_probe: in and out must be non-NULL"; return FW_EINVAL; }
  if (n <= 0 || n > (1 << 24)) { h->err = "fw_probe: n must be in [1, 2^24], got " + std::to_string(n); return FW_EINVAL; }
  const probe::Shape sh = probe::shape_of(op, variant);
  if (sh.in_cols == 0) { h->err = "fw_probe: unknown (op, variant) = (" + std::to_string(op) + ", " + std::to_string(variant) + ")"; return FW_EINVAL; }
  if (in_cols != sh.in_cols || out_cols != sh.out_cols) {
    h->err = "fw_probe: (op, variant) = (" + std::to_string(op) + ", " + std::to_string(variant) + ") takes " + std::to_string(sh.in_cols) +
             " input and " + std::to_string(sh.out_cols) + " output columns, got " + std::to_string(in_cols) + " and " + std::to_string(out_cols);
    return FW_EINVAL;
  }
  DeviceGuard g(h->device);
  hipError_t herr = hipSuccess;
  const bool axis_ok = axis_aligned_geometry(h->cfg);
  const int rc = with_dtype(h, [&](auto t) {
    return probe::dispatch<decltype(t)>(op, variant, axis_ok, h->params_dev, in, out, n, (hipStream_t)hip_stream, herr, h->err);
  });
  if (rc != FW_OK) return rc;
  HIP_TRY(h, herr);
  return FW_OK;
}

int32_t fw_num_envs(fw_handle h) { return h ? h->n : FW_EINVAL; }
int32_t fw_capture_wave(fw_handle h) { return h ? h->capture_wave : FW_EINVAL; }
int32_t fw_aux_wave(fw_handle h) { return h ? h->aux_wave : FW_EINVAL; }
int32_t fw_step_shape(fw_handle h) { return h ? h->step_shape : FW_EINVAL; }
int32_t fw_obs_wave(fw_handle h) { return h ? h->obs_wave : FW_EINVAL; }
int32_t fw_axis_aligned(fw_handle h) { return h ? h->axis_aligned : FW_EINVAL; }
int32_t fw_lanes_per_env(fw_handle h) { return h ? (h->lanes_per_env == 8 && h->g8_waves == 2 ? 16 : h->lanes_per_env) : FW_EINVAL; }

const char* fw_last_error(fw_handle h) { return h ? h->err.c_str() : g_err.c_str(); }

int32_t fw_destroy(fw_handle h) {
  if (!h) return FW_EINVAL;
  DeviceGuard g(h->device);
  (void)hipDeviceSynchronize();
  free_device_buffers(h);
  delete h;
  return FW_OK;
}

// ---- soft actor-critic (csrc/fwsim_sac.hpp) and its replay ring (csrc/fwsim_replay.hpp) ----
#define FW_TRY(expr) do { const int32_t rc_ = (expr); if (rc_ != FW_OK) return rc_; } while (0)
static int32_t sac_fail(int32_t rc, const char* who, const std::string& what) { g_err = std::string(who) + ": " + what; return rc; }
static int32_t sac_launched() { HIP_TRY((fw_env*)nullptr, hipGetLastError()); return FW_OK; }          // the end of every entry point here
static int32_t sac_check_shape(const char* who, int32_t d, int32_t A, int32_t H) {
  if (d <= 0 || A <= 0 || H <= 0) return sac_fail(FW_EINVAL, who, "obs_dim, act_dim and hidden must be positive");
  if (!sac_shape_ok(d, A, H))
    return sac_fail(FW_EUNSUPPORTED, who, "built for obs_dim <= 64, act_dim <= 8 and hidden 64 or 256, got (" + std::to_string(d) + ", " + std::to_string(A) + ", " + std::to_string(H) + ")");
  return FW_OK;
}
static int32_t sac_check_batch(const char* who, int32_t B) {
  if (B <= 0) return sac_fail(FW_EINVAL, who, "the batch size must be positive");
  if (!sac_batch_ok(B)) return sac_fail(FW_EUNSUPPORTED, who, "built for batch sizes that are multiples of 16 in [16, 512] or multiples of 64 in (512, 8192], got " + std::to_string(B));
  return FW_OK;
}
static int32_t replay_check_ring(const char* who, int64_t capacity, int32_t row_floats, int32_t batch) {          // the ring as a sampler sees it
  const bool ok = capacity > 0 && capacity <= 0x7fffffffLL && row_floats > 0 && batch > 0;
  return ok ? FW_OK : sac_fail(FW_EINVAL, who, "capacity (below 2^31), row_floats and batch must be positive");
}
static int32_t replay_check_envs(const char* who, int64_t capacity, int32_t N) {          // the ring as whole vec-steps of N envs
  return N > 0 && capacity >= N && capacity % N == 0 ? FW_OK : sac_fail(FW_EINVAL, who, "N must be positive and capacity a positive multiple of N");
}
static_assert(sizeof(fw_her_task) == sizeof(HerTask), "HerTask mirrors fw_her_task");
static int32_t her_check(const char* who, const fw_her_task* task, int32_t obs_dim, int32_t row_floats) {
  if (task->variant != FW_LL_VARIANT_TRACKING && task->variant != FW_LL_VARIANT_SAC_DEMO) return sac_fail(FW_EINVAL, who, "task variant must be 0 (tracking) or 1 (FW_LL_VARIANT_SAC_DEMO)");
  if (obs_dim != kHerObsDim || row_floats != kHerRowFloats) return sac_fail(FW_EUNSUPPORTED, who, "built for the low-level task with Euler attitude, obs_dim 21 and row_floats 50");
  return FW_OK;
}
static int32_t sac_act_check(const char* who, bool pointers, int32_t N, int32_t mode, int64_t env_offset) {
  if (!pointers) return sac_fail(FW_EINVAL, who, "image, obs, counters, act_f32, act_env and obs_stage must be non-NULL");
  if (N <= 0 || mode < 0 || mode > 2 || env_offset < 0) return sac_fail(FW_EINVAL, who, "N must be positive, mode 0, 1 or 2 and env_offset non-negative");
  return FW_OK;
}
static int64_t sac_ws_floats(int32_t d, int32_t A, int32_t H, int32_t B) { return (int64_t)sac_ws_wide(d, A, H, B).total; }
// what fw_sac_update and fw_sac_update_weighted check behind their pointers, then the argument block both launch with
static int32_t sac_step_args(const char* who, float* image, const float* batch_rows, int32_t d, int32_t A, int32_t H, int32_t B, const fw_sac_hyper* hyper,
                             int64_t* counters, float* out, void* workspace, int64_t workspace_bytes, SacStepArgs* S) {
  FW_TRY(sac_check_shape(who, d, A, H));
  FW_TRY(sac_check_batch(who, B));
  if (workspace_bytes < sac_ws_floats(d, A, H, B) * (int64_t)sizeof(float)) return sac_fail(FW_EINVAL, who, "the workspace is smaller than fw_sac_update_workspace_bytes asks for");
  static_assert(sizeof(fw_sac_hyper) == sizeof(SacHyper), "fw_sac_hyper and SacHyper must agree");
  *S = SacStepArgs{image, batch_rows, (float*)workspace, counters, out, d, A, H, B, {}};
  std::memcpy(&S->hp, hyper, sizeof(SacHyper));
  return FW_OK;
}
int32_t fw_sizeof_sac_hyper(void) { return (int32_t)sizeof(fw_sac_hyper); }
int32_t fw_sac_param_count(int32_t obs_dim, int32_t act_dim, int32_t hidden) {
  FW_TRY(sac_check_shape("fw_sac_param_count", obs_dim, act_dim, hidden));
  return sac_layout(obs_dim, act_dim, hidden).total;
}
int64_t fw_sac_update_workspace_bytes(int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t batch) {
  FW_TRY(sac_check_shape("fw_sac_update_workspace_bytes", obs_dim, act_dim, hidden));
  FW_TRY(sac_check_batch("fw_sac_update_workspace_bytes", batch));
  return sac_ws_floats(obs_dim, act_dim, hidden, batch) * (int64_t)sizeof(float);
}
int32_t fw_sac_act(const float* image, const void* obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t mode,
                   uint64_t seed, int64_t env_offset, const int64_t* counters, float* act_f32, void* act_env, float* obs_stage, float* logp,
                   float* eps, void* hip_stream) {
  FW_TRY(sac_act_check("fw_sac_act", image && obs && counters && act_f32 && act_env && obs_stage, N, mode, env_offset));
  FW_TRY(sac_check_shape("fw_sac_act", obs_dim, act_dim, hidden));
  DeviceGuard g(device_of(image));
  const SacActArgs a{image, obs, N, obs_dim, act_dim, mode, seed, env_offset, counters, act_f32, act_env, obs_stage, logp, eps};
  with_real(obs_is_f64 != 0, [&](auto t) { sac_act_launch<decltype(t), false>((hipStream_t)hip_stream, a, hidden); });
  return sac_launched();
}
int32_t fw_sac_act_norm(const float* image, const void* obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim, int32_t act_dim, int32_t hidden,
                        int32_t mode, uint64_t seed, int64_t env_offset, const int64_t* counters, float* act_f32, void* act_env, float* obs_stage,
                        float* logp, float* eps, const double* obs_mean, const double* obs_var, float clip_obs, float eps_obs, void* hip_stream) {
  FW_TRY(sac_act_check("fw_sac_act_norm", image && obs && counters && act_f32 && act_env && obs_stage, N, mode, env_offset));
  if (mode != 2 && (!obs_mean || !obs_var)) { g_err = "fw_sac_act_norm: modes 0 and 1 need obs_mean and obs_var"; return FW_EINVAL; }
  if (mode != 2 && !(clip_obs > 0.0f && eps_obs >= 0.0f)) { g_err = "fw_sac_act_norm: clip_obs must be positive and eps_obs non-negative"; return FW_EINVAL; }
  FW_TRY(sac_check_shape("fw_sac_act_norm", obs_dim, act_dim, hidden));
  DeviceGuard g(device_of(image));
  const SacActNormArgs a{{image, obs, N, obs_dim, act_dim, mode, seed, env_offset, counters, act_f32, act_env, obs_stage, logp, eps},
                         obs_mean, obs_var, clip_obs, eps_obs};
  with_real(obs_is_f64 != 0, [&](auto t) { sac_act_launch<decltype(t), true>((hipStream_t)hip_stream, a, hidden); });
  return sac_launched();
}
int32_t fw_replay_normalize(float* batch_rows, int32_t batch, int32_t obs_dim, int32_t act_dim, const double* obs_mean, const double* obs_var,
                            float clip_obs, float eps_obs, const double* ret_var, float clip_reward, float eps_reward, void* hip_stream) {
  if (!batch_rows || (!obs_mean && !ret_var) || (!obs_mean != !obs_var)) {
    g_err = "fw_replay_normalize: batch_rows must be non-NULL, obs_mean and obs_var come together, and one of obs_mean and ret_var must be given"; return FW_EINVAL;
  }
  if (batch <= 0 || obs_dim <= 0 || act_dim <= 0) { g_err = "fw_replay_normalize: batch, obs_dim and act_dim must be positive"; return FW_EINVAL; }
  if ((obs_mean && !(clip_obs > 0.0f && eps_obs >= 0.0f)) || (ret_var && !(clip_reward > 0.0f && eps_reward >= 0.0f))) {
    g_err = "fw_replay_normalize: a clip must be positive and an epsilon non-negative"; return FW_EINVAL;
  }
  if (obs_dim > kSacMaxD || act_dim > kSacMaxA) { g_err = "fw_replay_normalize: built for obs_dim <= 64 and act_dim <= 8"; return FW_EUNSUPPORTED; }
  DeviceGuard g(device_of(batch_rows));
  SacBatchNormArgs n{batch_rows, batch, obs_dim, act_dim, obs_mean, obs_var, ret_var, clip_obs, eps_obs, clip_reward, eps_reward};
  hipLaunchKernelGGL(fw_replay_normalize_kernel, dim3((unsigned)(((int64_t)batch + kSacNormRows - 1) / kSacNormRows)), dim3(256), 0, (hipStream_t)hip_stream, n);
  return sac_launched();
}
int32_t fw_replay_store(float* ring, int64_t capacity, int64_t* counters, const float* obs_stage, const float* act_f32, const void* reward,
                        const void* next_obs, const void* terminal_obs, const uint8_t* terminated, const uint8_t* truncated, int32_t env_is_f64,
                        int32_t N, int32_t obs_dim, int32_t act_dim, void* hip_stream) {
  if (!ring || !counters || !obs_stage || !act_f32 || !reward || !next_obs || !terminal_obs || !terminated || !truncated) { g_err = "fw_replay_store: every pointer must be non-NULL"; return FW_EINVAL; }
  if (N <= 0 || obs_dim <= 0 || act_dim <= 0 || capacity < N || capacity % N != 0) { g_err = "fw_replay_store: N, obs_dim and act_dim must be positive and capacity a positive multiple of N"; return FW_EINVAL; }
  if (obs_dim > kSacMaxD || act_dim > kSacMaxA) { g_err = "fw_replay_store: built for obs_dim <= 64 and act_dim <= 8"; return FW_EUNSUPPORTED; }
  DeviceGuard g(device_of(ring));
  SacStoreArgs s{ring, capacity, counters, obs_stage, act_f32, reward, next_obs, terminal_obs, terminated, truncated, N, obs_dim, act_dim};
  const long long elems = (long long)N * (2 * obs_dim + act_dim + 2);
  with_real(env_is_f64 != 0, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((fw_replay_store_kernel<T>), dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, s);
  });
  hipLaunchKernelGGL(fw_replay_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, counters, capacity, N);
  return sac_launched();
}
int32_t fw_replay_sample(const float* ring, int64_t capacity, const int64_t* counters, uint64_t seed, int32_t row_floats, int32_t batch,
                         float* out, int32_t* idx_out, void* hip_stream) {
  if (!ring || !counters || !out) { g_err = "fw_replay_sample: ring, counters and out must be non-NULL"; return FW_EINVAL; }
  FW_TRY(replay_check_ring("fw_replay_sample", capacity, row_floats, batch));
  DeviceGuard g(device_of(ring));
  hipLaunchKernelGGL(fw_replay_sample_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, ring, capacity, counters, seed,
                     row_floats, batch, out, idx_out);
  return sac_launched();
}
int32_t fw_replay_mark_ends(uint8_t* ends, int64_t capacity, const int64_t* counters, const uint8_t* terminated, const uint8_t* truncated, int32_t N,
                            void* hip_stream) {
  if (!ends || !counters || !terminated || !truncated) { g_err = "fw_replay_mark_ends: every pointer must be non-NULL"; return FW_EINVAL; }
  FW_TRY(replay_check_envs("fw_replay_mark_ends", capacity, N));
  DeviceGuard g(device_of(ends));
  hipLaunchKernelGGL(fw_replay_mark_ends_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, ends, capacity, counters,
                     terminated, truncated, N);
  return sac_launched();
}
int32_t fw_replay_sample_nstep(const float* ring, int64_t capacity, const int64_t* counters, uint64_t seed, int32_t row_floats, int32_t batch,
                               float* out, int32_t* idx_out, const uint8_t* ends, int32_t obs_dim, int32_t N, int32_t n_steps, float gamma,
                               int32_t* k_out, void* hip_stream) {
  if (!ring || !counters || !out || !ends) { g_err = "fw_replay_sample_nstep: ring, counters, out and ends must be non-NULL"; return FW_EINVAL; }
  FW_TRY(replay_check_ring("fw_replay_sample_nstep", capacity, row_floats, batch));
  FW_TRY(replay_check_envs("fw_replay_sample_nstep", capacity, N));
  if (obs_dim <= 0 || row_floats < 2 * obs_dim + 3) { g_err = "fw_replay_sample_nstep: row_floats must be 2 obs_dim + act_dim + 2 with positive obs_dim and act_dim"; return FW_EINVAL; }
  if (n_steps < 1 || n_steps > kSacMaxNStep) { g_err = "fw_replay_sample_nstep: built for n_steps in [1, 16]"; return FW_EUNSUPPORTED; }
  DeviceGuard g(device_of(ring));
  hipLaunchKernelGGL(fw_replay_sample_nstep_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, ring, capacity, counters,
                     seed, row_floats, batch, out, idx_out, ends, obs_dim, N, n_steps, gamma, k_out);
  return sac_launched();
}
int32_t fw_sizeof_her_task(void) { return (int32_t)sizeof(fw_her_task); }
int32_t fw_replay_sample_her(const float* ring, int64_t capacity, const int64_t* counters, uint64_t seed, int32_t row_floats, int32_t batch,
                             float* out, int32_t* idx_out, const uint8_t* ends, int32_t obs_dim, int32_t N, int32_t horizon, float relabel_prob,
                             const fw_her_task* task, int32_t* j_out, void* hip_stream) {
  if (!ring || !counters || !out || !ends || !task) { g_err = "fw_replay_sample_her: ring, counters, out, ends and task must be non-NULL"; return FW_EINVAL; }
  if (capacity <= 0 || capacity > 0x7fffffffLL || row_floats <= 0 || batch <= 0 || obs_dim <= 0) { g_err = "fw_replay_sample_her: capacity (below 2^31), row_floats, batch and obs_dim must be positive"; return FW_EINVAL; }
  FW_TRY(replay_check_envs("fw_replay_sample_her", capacity, N));
  if (!(relabel_prob >= 0.0f && relabel_prob <= 1.0f)) { g_err = "fw_replay_sample_her: relabel_prob must lie in [0, 1]"; return FW_EINVAL; }
  FW_TRY(her_check("fw_replay_sample_her", task, obs_dim, row_floats));
  if (horizon < 1 || horizon > kSacMaxHerHorizon) { g_err = "fw_replay_sample_her: built for horizon in [1, 64]"; return FW_EUNSUPPORTED; }
  const HerTask T{task->variant, task->dome, task->min_speed};
  const uint64_t thresh = (uint64_t)((double)relabel_prob * 4294967296.0);
  DeviceGuard g(device_of(ring));
  hipLaunchKernelGGL(fw_replay_sample_her_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, ring, capacity, counters,
                     seed, batch, out, idx_out, ends, N, horizon, thresh, T, j_out);
  return sac_launched();
}
int32_t fw_her_reward(const float* rows, int32_t row_floats, int32_t batch, int32_t obs_dim, const float* goals, const fw_her_task* task,
                      float* reward_out, void* hip_stream) {
  if (!rows || !goals || !task || !reward_out) { g_err = "fw_her_reward: every pointer must be non-NULL"; return FW_EINVAL; }
  if (row_floats <= 0 || batch <= 0 || obs_dim <= 0) { g_err = "fw_her_reward: row_floats, batch and obs_dim must be positive"; return FW_EINVAL; }
  FW_TRY(her_check("fw_her_reward", task, obs_dim, row_floats));
  const HerTask T{task->variant, task->dome, task->min_speed};
  DeviceGuard g(device_of(rows));
  hipLaunchKernelGGL(fw_her_reward_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, rows, row_floats, batch, obs_dim,
                     goals, T, reward_out);
  return sac_launched();
}
int32_t fw_sac_noise(uint64_t seed, const int64_t* counters, int32_t batch, int32_t act_dim, float* out, void* hip_stream) {
  if (!counters || !out) { g_err = "fw_sac_noise: counters and out must be non-NULL"; return FW_EINVAL; }
  if (batch <= 0 || act_dim <= 0) { g_err = "fw_sac_noise: batch and act_dim must be positive"; return FW_EINVAL; }
  if (act_dim > kSacMaxA) { g_err = "fw_sac_noise: built for act_dim <= 8"; return FW_EUNSUPPORTED; }
  DeviceGuard g(device_of(out));
  hipLaunchKernelGGL(fw_sac_noise_kernel, dim3((unsigned)((2 * batch * ((act_dim + 3) / 4) + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, seed,
                     counters, batch, act_dim, out);
  return sac_launched();
}
int32_t fw_sac_update(float* image, const float* batch_rows, int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t batch, const fw_sac_hyper* hyper,
                      int64_t* counters, float* out, void* workspace, int64_t workspace_bytes, void* hip_stream) {
  if (!image || !batch_rows || !hyper || !counters || !workspace) { g_err = "fw_sac_update: image, batch_rows, hyper, counters and workspace must be non-NULL"; return FW_EINVAL; }
  SacStepArgs S;
  FW_TRY(sac_step_args("fw_sac_update", image, batch_rows, obs_dim, act_dim, hidden, batch, hyper, counters, out, workspace, workspace_bytes, &S));
  DeviceGuard g(device_of(image));
  sac_update_launch((hipStream_t)hip_stream, S);
  return sac_launched();
}

// ---- TD3 (csrc/fwsim_td3.hpp) ----
static int32_t td3_check_batch(const char* who, int32_t B) {
  if (B <= 0) return sac_fail(FW_EINVAL, who, "the batch size must be positive");
  if (!td3_batch_ok(B)) return sac_fail(FW_EUNSUPPORTED, who, "built for batch sizes that are multiples of 16 in [16, 512], got " + std::to_string(B));
  return FW_OK;
}
int32_t fw_sizeof_td3_hyper(void) { return (int32_t)sizeof(fw_td3_hyper); }
int32_t fw_td3_param_count(int32_t obs_dim, int32_t act_dim, int32_t hidden) {
  FW_TRY(sac_check_shape("fw_td3_param_count", obs_dim, act_dim, hidden));
  return td3_layout(obs_dim, act_dim, hidden).total;
}
int64_t fw_td3_update_workspace_bytes(int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t batch) {
  FW_TRY(sac_check_shape("fw_td3_update_workspace_bytes", obs_dim, act_dim, hidden));
  FW_TRY(td3_check_batch("fw_td3_update_workspace_bytes", batch));
  return (int64_t)td3_ws(obs_dim, act_dim, hidden, batch).total * (int64_t)sizeof(float);
}
int32_t fw_td3_act(const float* image, const void* obs, int32_t obs_is_f64, int32_t N, int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t mode,
                   uint64_t seed, int64_t env_offset, const int64_t* counters, float* act_f32, void* act_env, float* obs_stage, float sigma,
                   float* eps, void* hip_stream) {
  FW_TRY(sac_act_check("fw_td3_act", image && obs && counters && act_f32 && act_env && obs_stage, N, mode, env_offset));
  if (!(sigma >= 0.0f)) return sac_fail(FW_EINVAL, "fw_td3_act", "sigma must be non-negative");
  FW_TRY(sac_check_shape("fw_td3_act", obs_dim, act_dim, hidden));
  DeviceGuard g(device_of(image));
  const Td3ActArgs a{image, obs, N, obs_dim, act_dim, mode, seed, env_offset, counters, act_f32, act_env, obs_stage, eps, sigma};
  with_real(obs_is_f64 != 0, [&](auto t) { td3_act_launch<decltype(t)>((hipStream_t)hip_stream, a, hidden); });
  return sac_launched();
}
int32_t fw_td3_update(float* image, const float* batch_rows, int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t batch, const fw_td3_hyper* hyper,
                      int32_t with_actor, int64_t* counters, float* out, void* workspace, int64_t workspace_bytes, void* hip_stream) {
  const char* who = "fw_td3_update";
  if (!image || !batch_rows || !hyper || !counters || !workspace) return sac_fail(FW_EINVAL, who, "image, batch_rows, hyper, counters and workspace must be non-NULL");
  FW_TRY(sac_check_shape(who, obs_dim, act_dim, hidden));
  FW_TRY(td3_check_batch(who, batch));
  if (workspace_bytes < (int64_t)td3_ws(obs_dim, act_dim, hidden, batch).total * (int64_t)sizeof(float))
    return sac_fail(FW_EINVAL, who, "the workspace is smaller than fw_td3_update_workspace_bytes asks for");
  static_assert(sizeof(fw_td3_hyper) == sizeof(Td3Hyper), "fw_td3_hyper and Td3Hyper must agree");
  Td3StepArgs S{image, batch_rows, (float*)workspace, counters, out, obs_dim, act_dim, hidden, batch, with_actor != 0, {}};
  std::memcpy(&S.hp, hyper, sizeof(Td3Hyper));
  DeviceGuard g(device_of(image));
  td3_update_launch((hipStream_t)hip_stream, S);
  return sac_launched();
}

// ---- prioritized replay (csrc/fwsim_per.hpp) ----
static int32_t per_check_capacity(const char* who, int64_t capacity) {
  if (capacity <= 0) return sac_fail(FW_EINVAL, who, "capacity must be positive");
  if (capacity > kPerMaxCapacity) return sac_fail(FW_EUNSUPPORTED, who, "built for a capacity of at most 2^22 rows (64 level-2 entries), got " + std::to_string((long long)capacity));
  return FW_OK;
}
int32_t fw_replay_per_mark_new(float* prio, int64_t capacity, const int64_t* counters, const float* per_state, int32_t N, void* hip_stream) {
  if (!prio || !counters || !per_state) { g_err = "fw_replay_per_mark_new: every pointer must be non-NULL"; return FW_EINVAL; }
  FW_TRY(replay_check_envs("fw_replay_per_mark_new", capacity, N));
  FW_TRY(per_check_capacity("fw_replay_per_mark_new", capacity));
  DeviceGuard g(device_of(prio));
  hipLaunchKernelGGL(fw_replay_per_mark_new_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, prio, capacity, counters,
                     per_state, N);
  return sac_launched();
}
int32_t fw_replay_per_rebuild(const float* prio, int64_t capacity, float* sum1, float* min1, float* sum2, float* min2, float* per_state,
                              void* hip_stream) {
  if (!prio || !sum1 || !min1 || !sum2 || !min2 || !per_state) { g_err = "fw_replay_per_rebuild: every pointer must be non-NULL"; return FW_EINVAL; }
  FW_TRY(per_check_capacity("fw_replay_per_rebuild", capacity));
  DeviceGuard g(device_of(prio));
  const int n1 = per_groups(capacity);
  hipLaunchKernelGGL(fw_replay_per_level1_kernel, dim3((unsigned)((n1 + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, prio, (int)capacity, sum1, min1);
  hipLaunchKernelGGL(fw_replay_per_level2_kernel, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, (const float*)sum1, (const float*)min1, n1, sum2, min2,
                     per_state);
  return sac_launched();
}
int32_t fw_replay_sample_per(const float* ring, int64_t capacity, const int64_t* counters, uint64_t seed, int32_t row_floats, int32_t batch,
                             float* out, int32_t* idx_out, float* w_out, const float* prio, const float* sum1, const float* sum2,
                             const float* per_state, float beta0, int64_t beta_steps, void* hip_stream) {
  if (!ring || !counters || !out || !prio || !sum1 || !sum2 || !per_state) { g_err = "fw_replay_sample_per: ring, counters, out, prio, sum1, sum2 and per_state must be non-NULL"; return FW_EINVAL; }
  if (row_floats <= 0 || batch <= 0) { g_err = "fw_replay_sample_per: row_floats and batch must be positive"; return FW_EINVAL; }
  if (!(beta0 >= 0.0f && beta0 <= 1.0f) || beta_steps < 0) { g_err = "fw_replay_sample_per: beta0 must lie in [0, 1] and beta_steps must not be negative"; return FW_EINVAL; }
  FW_TRY(per_check_capacity("fw_replay_sample_per", capacity));
  DeviceGuard g(device_of(ring));
  hipLaunchKernelGGL(fw_replay_sample_per_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, ring, (int)capacity, counters,
                     seed, row_floats, batch, out, idx_out, w_out, prio, sum1, sum2, per_state, beta0, beta_steps);
  return sac_launched();
}
int32_t fw_replay_per_update(float* prio, int64_t capacity, const int32_t* idx, const float* td, int32_t batch, float alpha, float eps,
                             float* per_state, void* hip_stream) {
  if (!prio || !idx || !td || !per_state) { g_err = "fw_replay_per_update: every pointer must be non-NULL"; return FW_EINVAL; }
  if (batch <= 0) { g_err = "fw_replay_per_update: batch must be positive"; return FW_EINVAL; }
  if (!(alpha >= 0.0f && alpha <= 1.0f) || !(eps > 0.0f) || !(eps < 1e30f)) { g_err = "fw_replay_per_update: alpha must lie in [0, 1] and eps must be positive and finite"; return FW_EINVAL; }
  FW_TRY(per_check_capacity("fw_replay_per_update", capacity));
  DeviceGuard g(device_of(prio));
  const dim3 grid((unsigned)((batch + 255) / 256)), block(256);
  hipLaunchKernelGGL(fw_replay_per_clear_kernel, grid, block, 0, (hipStream_t)hip_stream, prio, (int)capacity, idx, batch);
  hipLaunchKernelGGL(fw_replay_per_max_kernel, grid, block, 0, (hipStream_t)hip_stream, prio, (int)capacity, idx, td, batch, alpha, eps, per_state);
  return sac_launched();
}
int32_t fw_sac_update_weighted(float* image, const float* batch_rows, int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t batch,
                               const fw_sac_hyper* hyper, int64_t* counters, float* out, void* workspace, int64_t workspace_bytes,
                               const float* weights, float* td_out, void* hip_stream) {
  if (!image || !batch_rows || !hyper || !counters || !workspace || !weights) { g_err = "fw_sac_update_weighted: image, batch_rows, hyper, counters, workspace and weights must be non-NULL"; return FW_EINVAL; }
  SacStepArgs S;
  FW_TRY(sac_step_args("fw_sac_update_weighted", image, batch_rows, obs_dim, act_dim, hidden, batch, hyper, counters, out, workspace, workspace_bytes, &S));
  DeviceGuard g(device_of(image));
  float* g3 = S.ws + sac_ws(obs_dim, act_dim, hidden, batch).g3;
  sac_update_launch((hipStream_t)hip_stream, S, [&](hipStream_t st) {
    hipLaunchKernelGGL(fw_sac_per_weight_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, g3, batch, weights, td_out);
  });
  return sac_launched();
}

#ifdef FW_PROFILE
// Dev-only (not part of include/fwsim.h): per-wave cycle accounting ring of the last 256 launches.
// Layout long long[256][2 * blocks][8]; returns the number of step blocks.
int32_t fw_debug_profile(fw_handle h, long long* host_out, int32_t enable) {
  if (!h) return FW_EINVAL;
  DeviceGuard g(h->device);
  const size_t nblk = grid_of(h).x, bytes = sizeof(long long) * kProfSlots * 2 * nblk * kProfWords;
  (void)hipDeviceSynchronize();
  if (enable && !h->prof_dev) { (void)hipMalloc((void**)&h->prof_dev, bytes); (void)hipMemset(h->prof_dev, 0, bytes); }
  if (host_out && h->prof_dev) (void)hipMemcpy(host_out, h->prof_dev, bytes, hipMemcpyDeviceToHost);
  return (int32_t)nblk;
}
int32_t fw_debug_epoch(fw_handle h) { uint64_t c[FW_CTR_DIM]; return (h && fw_get_counters(h, c) == FW_OK) ? (int32_t)c[FW_CTR_LAUNCHES] + 1 : 0; }
#endif

}  // extern "C"
