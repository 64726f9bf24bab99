"""Dev tool: worst deviation of the HIP path from the CPU oracle over lockstep traces (the tests only assert a bound).

    python tools/parity_margin.py            the shipped vehicle: four configs x both lane mappings, 240 steps x 256 envs
    python tools/parity_margin.py --fuzz     the fuzz set of tests/fuzz_configs.py (what tests/test_fuzz_parity_gpu.py flies):
                                             per leg and mapping the worst |obs|, |reward|, |terminal obs|, |state| and the
                                             episode ends, then which configs reached which row of the kernel table
"""
import os, sys, time, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from oracle import fw_oracle as O
from helpers import run_direct_lockstep, run_lockstep, run_lowlevel_lockstep
O.build()


def shipped():
    cases = {"waypoints (headline config)": K.train_waypoints_v3_config(),
             "waypoints + gust wind (force)": K.train_waypoints_v3_config(wind_config=K.TRAIN_OBJLOCK_WIND),
             "objlock train config": K.train_objlock_config(),
             "combined train config": K.train_waypoint_objlock_config()}
    for lanes in ("8", "1"):
        os.environ["FWSIM_LANES_PER_ENV"] = lanes
        for name, cfg in cases.items():
            n = 256
            hip, ora = P.FixedwingVecEnv(cfg, n, seed=7), O.OracleEnv(cfg, n, seed=7)
            w = run_lockstep(hip, ora, 240, np.random.default_rng(3), atol=1e-6, rtol=0, state_atol=1e-3)
            print(f"lanes/env={lanes} {name}: 240 steps x {n} envs, {w['dones']} episode ends; worst |obs| {w['obs']:.2e} |reward| {w['rew']:.2e} "
                  f"|terminal obs| {w['tobs']:.2e} |state| {w['state']:.2e}", flush=True)
            hip.close()


def fuzz():
    """Measures with the tests' own runners under bounds a thousand times wider than theirs (flags and info still exact), so that
    a leg that would fail its test is still reported with its figure."""
    import fuzz_configs as F
    mappings = {"1 lane": ("1", "1"), "8 lanes": ("8", "1"), "8 lanes, 2 waves/SIMD": ("8", "2")}
    rows = {}                                   # kernel-table row -> the configs that reached it

    def reached(task, mapping, cfg, hip, name):
        windy = "windy" if cfg.wind_mode != K.FW_WIND_OFF else "wind-free"
        key = [task, mapping]
        if task in ("waypoints", "low-level", "direct"):
            key.append(windy)
        if task == "waypoints" and int(_lib.lib().fw_axis_aligned(hip._h)):
            key.append("axis-aligned tick")
        if hip.capture_wave:
            key.append("capture wave")
        rows.setdefault(", ".join(key), []).append(name)

    def fly(name, task, mapping, cfg, mode, steps, after_reset=None):
        hip, ora = P.FixedwingVecEnv(cfg, F.NUM_ENVS, seed=F.SEED), O.OracleEnv(cfg, F.NUM_ENVS, seed=F.SEED)
        w = run_lockstep(hip, ora, steps, np.random.default_rng(F.ACTION_SEED), atol=2e-2 if cfg.task == K.FW_TASK_OBJLOCK else 1e-4, rtol=0,
                         rew_atol=1e-4, state_atol=1e-4, after_reset=after_reset, actions=lambda rng, n: F.actions_of(mode, rng, n))
        reached(task, mapping, cfg, hip, name)
        hip.close()
        return w

    def aim(hip, ora):
        s = F.aim_at_the_duck(O, ora.get_state(), np.random.default_rng(8))
        hip.set_state(s); ora.set_state(s)

    def line(leg, mapping, ws, t0):
        m = {k: max(w.get(k, 0.0) for w in ws) for k in ("obs", "rew", "tobs", "state")}
        ends = sum(w.get("dones", 0) for w in ws)
        print(f"{leg:34s} {mapping:22s} {len(ws):3d} traces, {ends:6d} episode ends; worst |obs| {m['obs']:.2e} |reward| {m['rew']:.2e} "
              f"|terminal obs| {m['tobs']:.2e} |state| {m['state']:.2e}   ({time.time() - t0:.1f} s)", flush=True)

    t_all = time.time()
    print(f"{F.NUM_ENVS} envs per trace; tolerance of the tests: 1e-7 (ObjLock observations: 2e-5)")
    for mapping, (lanes, waves) in mappings.items():
        os.environ["FWSIM_LANES_PER_ENV"], os.environ["FWSIM_G8_WAVES"] = lanes, waves
        os.environ.pop("FWSIM_CAPTURE_WAVE", None); os.environ.pop("FWSIM_NO_SHADOW", None)
        t0 = time.time()
        line(f"waypoints x {F.N_WAYPOINTS}, {F.WAYPOINT_STEPS} steps", mapping,
             [fly(f"waypoints-{i}", "waypoints", mapping, F.waypoints(i), "uniform", F.WAYPOINT_STEPS) for i in range(F.N_WAYPOINTS)], t0)
        if waves == "2":
            continue
        os.environ["FWSIM_NO_SHADOW"] = "1"
        t0 = time.time()
        line(f"waypoints x {len(F.RESET_PATH_CONFIGS)}, resets in the kernel", mapping,
             [fly(f"waypoints-{i}", "waypoints", mapping + ", in-kernel resets", F.waypoints(i), "uniform", F.WAYPOINT_STEPS) for i in F.RESET_PATH_CONFIGS], t0)
        os.environ.pop("FWSIM_NO_SHADOW")
        for cw in (False, True) if lanes == "8" else (False,):
            if cw:
                os.environ["FWSIM_CAPTURE_WAVE"] = "1"
            for task, make in (("objlock", F.objlock), ("combined", F.combined)):
                ids = [i for t, i in F.CAPTURE_WAVE_CONFIGS if t == task] if cw else range(F.N_CAMERA)
                t0 = time.time()
                line(f"{task} x {len(ids)}, own resets, {F.CAMERA_STEPS} steps" + (", capture wave" if cw else ""), mapping,
                     [fly(f"{task}-{i}", task, mapping, make(i), "gentle", F.CAMERA_STEPS) for i in ids], t0)
                t0 = time.time()
                line(f"{task} x {len(ids)}, aimed, {F.AIMED_STEPS} steps" + (", capture wave" if cw else ""), mapping,
                     [fly(f"{task}-aimed-{i}", task, mapping, make(i, aimed=True), "aimed", F.AIMED_STEPS, after_reset=aim) for i in ids], t0)
        os.environ.pop("FWSIM_CAPTURE_WAVE", None)
        t0, ws = time.time(), []
        for i, t in zip(F.DIRECT_VEHICLES, F.TRIPLES):
            wd, wp = F.direct_pair(i, t)
            hip, ora = P.FixedwingVecEnv(wd, F.NUM_ENVS, seed=F.SEED), O.OracleEnv(wp, F.NUM_ENVS, seed=F.SEED)
            ws.append(run_direct_lockstep(hip, ora, t, F.DIRECT_STEPS, np.random.default_rng(F.ACTION_SEED), atol=1e-4, actions=lambda rng, n: F.actions_of("direct", rng, n)))
            reached("direct", mapping, wd, hip, f"direct-{i}"); hip.close()
        line(f"direct commands x {F.N_DIRECT}, {F.DIRECT_STEPS} steps", mapping, ws, t0)
        t0, ws = time.time(), []
        for i, t in zip(F.DIRECT_VEHICLES, F.TRIPLES):
            ll, wp = F.lowlevel_pair(i, t)
            hip, ora = P.FixedwingVecEnv(ll, F.NUM_ENVS, seed=F.SEED), O.OracleEnv(wp, F.NUM_ENVS, seed=F.SEED)
            ws.append(run_lowlevel_lockstep(hip, ora, t, F.DIRECT_STEPS, np.random.default_rng(F.ACTION_SEED), atol=1e-4, actions=lambda rng, n: F.actions_of("lowlevel", rng, n)))
            reached("low-level", mapping, ll, hip, f"lowlevel-{i}"); hip.close()
        line(f"low-level x {F.N_DIRECT}, rigid state, {F.DIRECT_STEPS} steps", mapping, ws, t0)
    print(f"total {time.time() - t_all:.1f} s\n\nkernel-table rows (env_kernels_of) and the fuzz configs that reached them:")
    for key in sorted(rows):
        print(f"  {key}: {' '.join(rows[key])}")


if __name__ == "__main__":
    fuzz() if "--fuzz" in sys.argv[1:] else shipped()
