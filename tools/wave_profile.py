"""Dev tool: where does the slowest wave of each fw_step launch spend its cycles?

Builds nothing itself: expects tools/_build/libfwsim_prof.so (bash tools/build_prof.sh: fwsim.hip with -DFW_PROFILE, ISA-checked);
--phases expects libfwsim_prof_ph.so (bash tools/build_prof.sh phases) and splits the capture steps with 5+ envs due.
usage: python tools/wave_profile.py <waypoints|waypoints_wind|objlock|combined> [steps]
       (FWSIM_PROF_LIB=<path>: a profile build of another commit instead, for a before / after)
"""
import ctypes as C, os, sys, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyflyt_drone_amd as P
from pyflyt_drone_amd import config as K, _lib
_lib.LIB_PATH = os.environ.get("FWSIM_PROF_LIB") or os.path.join(ROOT, "tools", "_build", "libfwsim_prof.so")     # FWSIM_PROF_LIB: the profile build of another commit (A/B)
CFG = {"waypoints": K.train_waypoints_v3_config, "objlock": K.train_objlock_config, "combined": K.train_waypoint_objlock_config,
       "waypoints_wind": lambda: K.train_waypoints_v3_config(wind_config=K.TRAIN_OBJLOCK_WIND)}
PHASES = "--phases" in sys.argv
if PHASES:
    sys.argv.remove("--phases"); _lib.LIB_PATH = os.path.join(ROOT, "tools", "_build", "libfwsim_prof_ph.so")
which = sys.argv[1]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 600
N = int(os.environ.get("N", 4096))
e = P.FixedwingVecEnv(CFG[which](), N, seed=42); e.reset_tensor()
L = _lib.lib()
L.fw_debug_profile.restype = C.c_int32; L.fw_debug_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
nblk = L.fw_debug_profile(e._h, None, 1)
g = torch.Generator().manual_seed(0)
acts = [(torch.rand((N, 4), generator=g, dtype=torch.float64) * 2 - 1).cuda() for _ in range(64)]
for i in range(steps): e.step_tensor(acts[i % 64])
torch.cuda.synchronize()
buf = np.zeros((256, 2 * nblk, 12), dtype=np.int64)
L.fw_debug_profile(e._h, buf.ctypes.data, 1)
st, wk = buf[:, :nblk, :], buf[:, nblk:, 0]
tot = st[:, :, 0]
slow = tot.argmax(axis=1)
S = st[np.arange(256), slow]                      # slowest step wave of each launch
if PHASES:     # built with -DFW_PROFILE -DFW_PROFILE_PHASES: phases of capture_body in capture steps with 5+ envs due
    ne = st[:, :, 6].sum()
    print(f"{which}: capture steps with 5+ envs due: {ne / st[:, :, 6].size:.3f} per wave-step; cycles each: " + "  ".join(
        f"{nm} {st[:, :, k].sum() / max(1, ne):.0f}" for nm, k in (("set-up+screening", 1), ("duck", 3), ("ground", 4), ("clear+draw", 5), ("sums+means", 9))))
    sys.exit(0)
names = ["total", "prologue", "reset", "aviary", "task", "epilogue"]
cap_words = which in ("objlock", "combined")
print(f"{which} N={N}: {nblk} step waves/launch, last 256 of {steps} launches; cycles (s_memtime)")
print("  mean over all waves : " + "  ".join(f"{n} {st[:, :, k].mean():8.0f}" for k, n in enumerate(names)))
print("  slowest wave/launch : " + "  ".join(f"{n} {S[:, k].mean():8.0f}" for k, n in enumerate(names)))
it = st[:, :, 6] & 0xFF; nr = (st[:, :, 6] >> 8) & 0xFF; nh = (st[:, :, 6] >> 16) & 0xFF
OBSW = bool(getattr(e, "obs_wave", False))          # fw_step_kernel_g8xo: word 8 of a step wave is its wait at barrier 2, the terminal observation is wave 1's
if OBSW:
    print(f"  slowest wave behind barrier 2 (waves with a reset): waypoints and, on the fallback, the new row {S[:, 9].mean():.0f}  warm state / first distance {S[:, 10].mean():.0f}")
elif not cap_words:      # (the camera kernels use these words for their capture steps, below)
    print(f"  slowest wave reset split: terminal obs {S[:, 8].mean():.0f}  swap-in / begin_reset {S[:, 9].mean():.0f}  first compute_state {S[:, 10].mean():.0f}")
print(f"  loop iterations: mean {it.mean():.2f}  slowest-wave mean {(S[:, 6] & 0xFF).mean():.2f}  max {it.max()}")
print(f"  env resets/launch {nr.sum(axis=1).mean():.1f}  of which swapped-in shadows {nh.sum(axis=1).mean():.1f}")
print(f"  waves with a reset: {100.0 * (nr > 0).mean():.1f}%   with an in-kernel (fallback) reset: {100.0 * ((nr - nh) > 0).mean():.1f}%")
cap = st[:, :, 11] & ((1 << 48) - 1); ncap = st[:, :, 11] >> 48
if OBSW:                                            # (no camera: word 11 of a step wave carries its arrivals at the two barriers, below)
    cap = np.zeros_like(cap)
if cap.any():
    print(f"  camera: envs capturing per wave-step {ncap.mean():.2f} of {N // nblk}; cycles in captures per wave-step: mean {cap.mean():.0f}  "
          f"slowest wave {(S[:, 11] & ((1 << 48) - 1)).mean():.0f}; waves with a capture {100.0 * (ncap > 0).mean():.1f}%")
    names_m = ["1 env due", "2", "3-4", "5+"]
    for idx, nm in zip((8, 9, 10, 7), names_m):
        v = st[:, :, idx]; cyc = v & ((1 << 40) - 1); ne = v >> 40
        vs = S[:, idx]; cs = vs & ((1 << 40) - 1); ns = vs >> 40
        if ne.sum():
            print(f"    capture steps with {nm}: {ne.mean():.2f} per wave-step, {cyc.sum() / max(1, ne.sum()):.0f} cycles each (all waves); "
                  f"slowest wave: {ns.mean():.2f} per step, {cs.sum() / max(1, ns.sum()):.0f} cycles each")
# Start stamps (word 7 of a step wave's slot).  Workgroup b is dealt to XCD b % 8.  Whether the counters of different workgroups can be
# compared is not assumed: both spreads are printed.  Measured on an MI355X (profiles/r24_obs_wave_profile_*.txt): 2e8 cycles within
# the group b % 8 and 1.9e12 over the launch, against launches of 3e4 cycles -- the counters are NOT common to an XCD, let alone to
# the chip, so stamps compare only between the two waves of one workgroup (one CU), and nothing below orders workgroups by stamp.
if not cap_words:
    t0 = st[:, :, 7]
    spread = np.array([[np.ptp(t0[l, x::8]) for x in range(8)] for l in range(256)]) if nblk >= 16 else np.zeros((256, 1))
    print(f"  start stamps within an XCD (max - min over its {nblk // 8} step waves): mean {spread.mean():.0f}  worst XCD of a launch {spread.max(axis=1).mean():.0f}  max {spread.max()}")
    print(f"  start stamps over the whole launch (max - min over {nblk} step waves): mean {np.ptp(t0, axis=1).mean():.0f}  max {np.ptp(t0, axis=1).max()}")
if OBSW:
    # The second wave of workgroup b stamps slot nblk + b: noise draw up to barrier 1, worker, pre-loads, the wait at barrier 2, pass
    # (with the terminal-observation copy), flush.  The two waves of a workgroup sit on one CU: their stamps compare.
    W = buf[:, nblk:, :]
    wnames = [("noise+barrier 1", 1), ("worker", 0), ("pre-loads", 2), ("wait at barrier 2", 3), ("pass", 4), ("flush", 5), ("total", 6)]
    end_step, end_obs = st[:, :, 7] + st[:, :, 0], W[:, :, 7] + W[:, :, 6]
    later = np.maximum(end_step, end_obs)                           # the later of a workgroup's two ends, as a stamp
    wg_len = later - np.minimum(st[:, :, 7], W[:, :, 7])            # ... and from the workgroup's first stamp
    comparable = np.ptp(st[:, :, 7], axis=1).max() < 100 * wg_len.max()        # one clock for the whole launch? (see the spreads above)
    last = (later if comparable else wg_len).argmax(axis=1)          # the workgroup that finishes last -- or, without a common clock, the longest one
    lastname = "finishing last" if comparable else "that lasts longest"
    ar = np.arange(256)
    Wl, Sl = W[ar, last], st[ar, last]
    print("  observation wave, mean over all   : " + "  ".join(f"{n} {W[:, :, k].mean():7.0f}" for n, k in wnames))
    print(f"  ... of the workgroup {lastname}: " + "  ".join(f"{n} {Wl[:, k].mean():7.0f}" for n, k in wnames))
    print(f"  step wave: wait at barrier 2 mean {st[:, :, 8].mean():.0f} (last workgroup {Sl[:, 8].mean():.0f})  tail behind it mean {(st[:, :, 5] - st[:, :, 8]).mean():.0f} (last workgroup {(Sl[:, 5] - Sl[:, 8]).mean():.0f})")
    print(f"  workgroup length (first stamp to the later end): mean {wg_len.mean():.0f}  longest of a launch {wg_len.max(axis=1).mean():.0f}")
    print(f"  the observation wave ends after the step wave in {100.0 * (end_obs > end_step).mean():.1f}% of the workgroups, by {(end_obs - end_step)[end_obs > end_step].mean() if (end_obs > end_step).any() else 0:.0f} cycles; "
          f"in the workgroup {lastname} in {100.0 * (end_obs[ar, last] > end_step[ar, last]).mean():.1f}% of the launches")
    # Which wave gates each barrier: both waves stamp immediately in front of barrier 1 and barrier 2 (from their own first stamp: word 11
    # of the step wave, 32 bits each; words 8 and 9 of the observation wave), so the wait is not part of either side's figure.
    if (W[:, :, 9] > 0).any():                      # (a profile build of a commit without these stamps leaves the words zero)
        arr_step = [st[:, :, 7] + (st[:, :, 11] & 0xFFFFFFFF), st[:, :, 7] + (st[:, :, 11] >> 32)]
        arr_obs = [W[:, :, 7] + W[:, :, 8], W[:, :, 7] + W[:, :, 9]]
        for b, what in ((0, "step wave's prologue against the noise draw"), (1, "step wave's sub-steps and latch against the worker and the pre-loads")):
            d = arr_step[b] - arr_obs[b]              # > 0: the step wave arrives last
            late = d > 0
            dl = d[ar, last]
            print(f"  barrier {b + 1} ({what}): the step wave arrives last in {100.0 * late.mean():.1f}% of the workgroups, by {d[late].mean() if late.any() else 0:.0f} cycles; "
                  f"the observation wave in {100.0 * (~late).mean():.1f}%, by {(-d[~late]).mean() if (~late).any() else 0:.0f}; "
                  f"mean arrival step {(arr_step[b] - st[:, :, 7]).mean():.0f} / obs {(arr_obs[b] - W[:, :, 7]).mean():.0f} after each wave's start; "
                  f"workgroup {lastname}: step wave last in {100.0 * (dl > 0).mean():.1f}% of the launches, step - obs mean {dl.mean():.0f}")
    K = int(os.environ.get("PROF_LAUNCHES", 8))
    print(f"  per launch (the last {K}; the workgroup {lastname}): step wave total / wait b2 / tail | obs wave worker / wait b2 / pass / flush / total | later end - workgroup's first stamp, which wave")
    order = [(steps - k) % 256 for k in range(K - 1, -1, -1)]        # slots are launch % 256 and launches count from 1: the newest K
    for l in order:
        b = last[l]
        print(f"    wg {b:4d}: {st[l, b, 0]:6d} / {st[l, b, 8]:5d} / {st[l, b, 5] - st[l, b, 8]:5d} | {W[l, b, 0]:5d} / {W[l, b, 3]:6d} / {W[l, b, 4]:5d} / {W[l, b, 5]:5d} / {W[l, b, 6]:6d} | "
              f"{wg_len[l, b]:6d} {'obs' if end_obs[l, b] > end_step[l, b] else 'step'}")
elif wk.any():
    print(f"  shadow worker waves: busy {100.0 * (wk > 2000).mean():.1f}%  mean busy cycles {wk[wk > 2000].mean() if (wk > 2000).any() else 0:.0f}  max {wk.max()}")
