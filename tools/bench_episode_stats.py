"""Dev tool: what the rollout episode statistics (PPOConfig.episode_stats, fw_episode_fold) cost, and that nothing moved with the
flag off.

  fold     device time of one fw_episode_fold at 16, 4096, 24 576 and 65 536 envs (window 100): 64 folds over seeded step outputs
           (a tenth of the envs done per step, every env done once) captured in one hipGraph; a region = --replays replays between
           two device synchronisations, timed with events; median of --regions regions
  wide     fw_episode_fold against fw_episode_fold_wide (EpisodeMonitor(fold="one" / "wide")) on the same seeded step outputs at 16,
           4096, 24 576, 65 536 and 2^20 envs: the two forms alternate region by region in one process; median of --regions regions
           and the min / max of each arm.  The span is the loaded library's: run once per candidate build (FWSIM_LIB)
  collect  a collected vec-step without the flag, with it, and with it on the multi-workgroup fold (episode_fold="wide"): the
           one-launch and the three-launch collector (waypoints, 4096 envs; --collect_65536: the three-launch one at 65 536 too) and
           the high-level collector (16 envs, no wide arm).  The arms live in one process and alternate; a region = --rollouts
           replays of the captured rollout graph between two synchronisations; median of --regions regions per arm
  e2e      env-steps/s of examples/train_fixedwing_waypoints.py with and without --episode_stats over --total_timesteps steps each
           (child processes, one at a time, the arms in turn --e2e_repeats times), and a closing line with the medians
  parent   the flag-off headline step through tools/bench_lib.py with this build's library, the parent commit's (--parent_lib) and a
           second copy of the parent's (the A/A spread), child processes in turn, --e2e_repeats times each

    python tools/bench_episode_stats.py --what fold --out profiles/r14_episode_stats_bench.jsonl
    python tools/bench_episode_stats.py --what collect --out profiles/r14_episode_stats_bench.jsonl
    python tools/bench_episode_stats.py --what wide --out profiles/r25_episode_fold_wide.jsonl
    python tools/bench_episode_stats.py --what collect --collect_65536 --out profiles/r25_episode_fold_wide.jsonl
    python tools/bench_episode_stats.py --what e2e --out profiles/r14_episode_stats_bench.jsonl
    python tools/bench_episode_stats.py --what parent --parent_lib /path/to/parent/libfwsim_hip.so --out profiles/r14_episode_stats_bench.jsonl
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FOLD_ENVS = (16, 4096, 24576, 65536)
WIDE_ENVS = FOLD_ENVS + (1 << 20,)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def regions(fn, n, per_region):
    """n regions of fn() between two device synchronisations, timed with events: [us per unit of work]."""
    import torch
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / per_region)
    return out


def bench_fold(a, dev):
    import torch
    from pyflyt_drone_amd import monitor as M
    rows, T = [], 64
    for N in FOLD_ENVS:
        g = torch.Generator(device="cuda"); g.manual_seed(N)
        rew = torch.randn((T, N), device="cuda", generator=g, dtype=torch.float64)
        done = torch.rand((T, N), device="cuda", generator=g) < 0.1
        done[T // 2] = True                                  # every env meets a time limit together once per graph
        trunc = (done & (torch.rand((T, N), device="cuda", generator=g) < 0.5)).to(torch.uint8)
        term = (done & (trunc == 0)).to(torch.uint8)
        info = torch.randint(0, 2, (T, N, 8), device="cuda", generator=g, dtype=torch.int32)
        m = M.EpisodeMonitor(N, a.window, "cuda")
        for t in range(T):                                   # warm-up: the code object is loaded, the ring is full
            m.fold(rew[t], term[t], trunc[t], info[t])
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for t in range(T):
                m.fold(rew[t], term[t], trunc[t], info[t])
        gr.replay(); torch.cuda.synchronize()

        def work():
            for _ in range(a.replays):
                gr.replay()
        us = regions(work, a.regions, a.replays * T)
        rows.append({"what": "fold", "envs": N, "window": a.window, "folds_per_region": a.replays * T, "regions": a.regions,
                     "us_per_fold_median": round(median(us), 3), "us_per_fold_min": round(min(us), 3), "us_per_fold_max": round(max(us), 3),
                     "episodes_folded": m.totals()["episodes"], "device": dev})
    return rows


def _span():
    from pyflyt_drone_amd import _lib
    return int(_lib.lib().fw_episode_fold_span())


def bench_wide(a, dev):
    """Both forms of the fold on the same seeded step outputs, alternating region by region in one process; one row per env count.
    The span is the loaded library's (FWSIM_LIB: one run per candidate span)."""
    import torch
    from pyflyt_drone_amd import monitor as M
    span = _span()
    rows = []
    for N in WIDE_ENVS:
        T = 64 if N <= 65536 else 16                         # (2^20 envs: 16 steps of outputs are 0.8 GB as it is)
        g = torch.Generator(device="cuda"); g.manual_seed(N)
        rew = torch.randn((T, N), device="cuda", generator=g, dtype=torch.float64)
        done = torch.rand((T, N), device="cuda", generator=g) < 0.1
        done[T // 2] = True                                  # every env meets a time limit together once per graph
        trunc = (done & (torch.rand((T, N), device="cuda", generator=g) < 0.5)).to(torch.uint8)
        term = (done & (trunc == 0)).to(torch.uint8)
        info = torch.randint(0, 2, (T, N, 8), device="cuda", generator=g, dtype=torch.int32)
        del done
        arms, graphs = {k: M.EpisodeMonitor(N, a.window, "cuda", fold=k) for k in ("one", "wide")}, {}
        for k, m in arms.items():
            for t in range(T):                               # warm-up: the code object is loaded, the ring is full
                m.fold(rew[t], term[t], trunc[t], info[t])
            torch.cuda.synchronize()
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k]):
                for t in range(T):
                    m.fold(rew[t], term[t], trunc[t], info[t])
            graphs[k].replay(); torch.cuda.synchronize()
        replays = a.replays if N <= 65536 else 1
        times = {k: [] for k in arms}
        for _ in range(a.regions):                           # the arms alternate region by region
            for k in arms:
                def work(gr=graphs[k]):
                    for _ in range(replays):
                        gr.replay()
                times[k] += regions(work, 1, replays * T)
        med = {k: median(v) for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        same = arms["one"].totals()["episodes"] == arms["wide"].totals()["episodes"]
        rows.append({"what": "wide", "envs": N, "span": span, "workgroups": -(-N // span), "window": a.window,
                     "folds_per_region": replays * T, "regions_per_arm": a.regions,
                     "one_us_per_fold_median": round(med["one"], 3), "wide_us_per_fold_median": round(med["wide"], 3),
                     "one_min_max_us": [round(min(times["one"]), 3), round(max(times["one"]), 3)],
                     "wide_min_max_us": [round(min(times["wide"]), 3), round(max(times["wide"]), 3)],
                     "one_over_wide": round(med["one"] / med["wide"], 3),
                     "wide_faster_by_more_than_both_spreads": bool(med["one"] - med["wide"] > spread["one"] + spread["wide"]),
                     "wide_not_slower": bool(med["wide"] <= med["one"]),
                     "episodes_folded_equal": bool(same), "device": dev})
        del rew, trunc, term, info, arms, graphs
        torch.cuda.empty_cache()
    return rows


def _collector(kind, stats, fold="one", envs=4096):
    import numpy as np
    import torch
    import pyflyt_drone_amd as P
    from pyflyt_drone_amd import rollout as R
    if kind == "highlevel":
        from pyflyt_drone_amd.highlevel import HighLevelCmdVecEnv
        torch.manual_seed(21)
        pol = R.MlpPolicy(21, 6)
        rng = np.random.default_rng(21)
        mean, var = rng.normal(0.0, 1.0, 21), rng.uniform(0.5, 2.0, 21)
        env = R.VecNormalizeDevice(HighLevelCmdVecEnv(16, pol, (mean, var), seed=13), gamma=0.995)
        return R.PPO(env, R.PPOConfig(n_steps=16, batch_size=64, n_epochs=1, gamma=0.995, seed=13, fused_three_actions=True,
                                      episode_stats=stats))
    env = R.VecNormalizeDevice(P.FixedwingWaypointsVecEnv(envs, angle_representation="euler", seed=11))
    return R.PPO(env, R.PPOConfig(n_steps=16, batch_size=128, n_epochs=1, seed=11, one_launch_collect=(kind == "one_launch"),
                                  episode_stats=stats, episode_fold=fold))


def bench_collect(a, dev):
    import torch
    rows = []
    for kind, envs in (("one_launch", 4096), ("three_launch", 4096), ("highlevel", 16)) + ((("three_launch", 65536),) if a.collect_65536 else ()):
        arms = {"off": _collector(kind, False, envs=envs), "on": _collector(kind, True, envs=envs)}
        if kind != "highlevel":
            arms["wide"] = _collector(kind, True, "wide", envs=envs)
        for p in arms.values():
            for _ in range(3):                               # eager, capture, replay
                p.collect_rollouts()
            assert p._g_rollout is not None and bool(p._one_launch) == (kind == "one_launch")
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        T = 16
        for _ in range(a.regions):                           # the arms alternate region by region
            for k, p in arms.items():
                def work(p=p):
                    for _ in range(a.rollouts):
                        p._g_rollout.replay()
                times[k] += regions(work, 1, a.rollouts * T)
        med = {k: median(v) for k, v in times.items()}
        stats = arms["on"].rollout_stats
        rows.append({"what": "collect", "collector": kind, "envs": arms["on"].env.num_envs, "n_steps": T, "regions_per_arm": a.regions,
                     "vec_steps_per_region": a.rollouts * T, "off_us_per_vec_step": round(med["off"], 3),
                     "on_us_per_vec_step": round(med["on"], 3), "on_minus_off_us": round(med["on"] - med["off"], 3),
                     "on_over_off": round(med["on"] / med["off"], 4),
                     "off_min_max_us": [round(min(times["off"]), 3), round(max(times["off"]), 3)],
                     "on_min_max_us": [round(min(times["on"]), 3), round(max(times["on"]), 3)],
                     "episodes_seen": stats.get("rollout/episodes"), "device": dev})
        if "wide" in arms:                                   # the third arm: the flag on, the multi-workgroup fold
            rows[-1].update({"wide_us_per_vec_step": round(med["wide"], 3), "wide_minus_off_us": round(med["wide"] - med["off"], 3),
                             "wide_over_off": round(med["wide"] / med["off"], 4),
                             "wide_min_max_us": [round(min(times["wide"]), 3), round(max(times["wide"]), 3)],
                             "span": _span(),
                             "episodes_seen_wide": arms["wide"].rollout_stats.get("rollout/episodes")})
        for p in arms.values():
            p.env.venv.close()
    return rows


def bench_e2e(a):
    rows = []
    for stats in [False, True] * a.e2e_repeats:
        out = tempfile.mkdtemp(prefix="fw_epstats_e2e_")
        cmd = [sys.executable, os.path.join(ROOT, "examples", "train_fixedwing_waypoints.py"), "--num_envs", str(a.num_envs),
               "--total_timesteps", str(a.total_timesteps), "--out", out] + (["--episode_stats"] if stats else [])
        t0 = time.perf_counter()
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        shutil.rmtree(out, ignore_errors=True)
        if p.returncode != 0:
            raise RuntimeError(p.stderr[-2000:])
        lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{") and "timesteps" in l]
        last = lines[-1]
        rows.append({"what": "e2e", "example": "train_fixedwing_waypoints.py", "episode_stats": stats, "num_envs": a.num_envs,
                     "total_timesteps": a.total_timesteps, "env_steps_per_s_last_line": last["fps"], "timesteps_last_line": last["timesteps"],
                     "wall_s_process": round(wall, 2), "update_lines": len(lines),
                     "every_line_has_rollout_scalars": all("rollout/ep_rew_mean" in l and "rollout/interval/ep_rew_mean" in l for l in lines),
                     "last_line": last})
    med = lambda s: median([r["env_steps_per_s_last_line"] for r in rows if r["episode_stats"] == s])
    rows.append({"what": "e2e_summary", "repeats_per_arm": a.e2e_repeats, "median_env_steps_per_s_plain": med(False),
                 "median_env_steps_per_s_episode_stats": med(True), "episode_stats_over_plain": round(med(True) / med(False), 4),
                 "all_plain": [r["env_steps_per_s_last_line"] for r in rows if r["episode_stats"] is False],
                 "all_episode_stats": [r["env_steps_per_s_last_line"] for r in rows if r["episode_stats"] is True]})
    return rows


def bench_parent(a):
    if not a.parent_lib:
        raise SystemExit("--parent_lib (or FWSIM_LIB): the parent commit's libfwsim_hip.so")
    here = os.path.join(ROOT, "pyflyt-drone_amd", "csrc", "libfwsim_hip.so")
    tmp = tempfile.mkdtemp(prefix="fw_parent_copy_")
    twin = os.path.join(tmp, "libfwsim_parent_twin.so")
    shutil.copy(a.parent_lib, twin)
    arms = (("parent", os.path.abspath(a.parent_lib)), ("this", here), ("parent_twin", twin))
    times = {k: [] for k, _ in arms}
    for _ in range(a.e2e_repeats):
        for name, lib in arms:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_lib.py"), lib, "waypoints"], capture_output=True,
                               text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(p.stderr[-2000:])
            times[name].append(float(re.search(r"([\d.]+) us/step", p.stdout).group(1)))
    shutil.rmtree(tmp, ignore_errors=True)
    med = {k: median(v) for k, v in times.items()}
    aa = abs(med["parent_twin"] - med["parent"]) / med["parent"]
    ab = (med["this"] - med["parent"]) / med["parent"]
    return [{"what": "flag_off_vs_parent", "bench": "tools/bench_lib.py waypoints (4096 envs, headline step, hipGraph replays)",
             "runs_per_arm": a.e2e_repeats, "parent_us_per_step": med["parent"], "this_us_per_step": med["this"],
             "parent_twin_us_per_step": med["parent_twin"], "this_over_parent_minus_1": round(ab, 5),
             "aa_spread_parent_vs_itself": round(aa, 5), "inside_aa_spread": bool(abs(ab) <= aa),
             "run_spread_parent": round((max(times["parent"] + times["parent_twin"]) - min(times["parent"] + times["parent_twin"])) / med["parent"], 5),
             "inside_run_spread_of_the_parent": bool(min(times["parent"] + times["parent_twin"]) <= med["this"] <= max(times["parent"] + times["parent_twin"])),
             "all_us": times}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("fold", "wide", "collect", "e2e", "parent"), default="fold")
    ap.add_argument("--collect_65536", action="store_true", help="collect: the three-launch collector at 65 536 envs as well")
    ap.add_argument("--regions", type=int, default=30)
    ap.add_argument("--replays", type=int, default=4, help="fold: graph replays (64 folds each) per region")
    ap.add_argument("--rollouts", type=int, default=8, help="collect: rollout-graph replays (16 vec-steps each) per region")
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--parent_lib", type=str, default=os.environ.get("FWSIM_LIB"))
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--total_timesteps", type=int, default=120 * 65536)
    ap.add_argument("--e2e_repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.what in ("e2e", "parent"):
        rows = bench_e2e(a) if a.what == "e2e" else bench_parent(a)      # (child processes only: this process never touches the device)
    else:
        import torch
        dev = torch.cuda.get_device_name(0)
        rows = {"fold": bench_fold, "wide": bench_wide, "collect": bench_collect}[a.what](a, dev)
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
