"""Wall time per vec-step of a commanded run of the low-level controller (command.fly: fw_command_ll -> act -> fw_step -> fw_trace_ll,
captured as hipGraphs of 8 vec-steps and replayed) at 16 and 4096 envs, on the torch policy forward and on the fused six-action one
(fw_collect_act_a).

    python tools/bench_lowlevel_command.py [--envs 16 4096] [--steps 512] [--repeats 3] [--out profiles/r08_lowlevel_command.jsonl]

The figure is the whole fly() call divided by its vec-steps: reset, graph capture, the replays and the download of the [T, N, 8] trace
included.  The policy is a seeded MlpPolicy with zeroed action weights (every command 0, throttle 0.5), so no env ends early; the
schedule steps heading, altitude and airspeed twice.  Under `rocprofv3 --kernel-trace --stats` the launch statistics of
fw_command_ll_kernel and fw_trace_ll_kernel come out beside those of the step and act kernels.  One JSON line per (envs, path).
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[16, 4096])
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import pyflyt_drone_amd as P
    from pyflyt_drone_amd import command, rollout as R

    q = a.steps // 4
    segments = [(q, (0.0, 10.0, 14.0)), (q, (math.pi / 2, 14.0, 16.0)), (q, (0.0, 10.0, 14.0)), (a.steps - 3 * q, (-math.pi / 2, 14.0, 16.0))]
    lines = []
    for n in a.envs:
        for fused in (False, True):
            env = R.VecNormalizeDevice(P.FixedwingLowLevelVecEnv(num_envs=n, seed=3), training=False, norm_reward=False, clip_obs=10.0)
            torch.manual_seed(0)
            pol = R.MlpPolicy(env.obs_dim, env.act_dim).cuda()
            with torch.no_grad():
                pol.action_net.weight.zero_()
            schedule = command.step_schedule(segments, n, env.device)
            walls = []
            for rep in range(a.repeats + 1):                # the first one warms up (library, allocator, kernel attributes)
                env.venv.seed(3)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ct = command.fly(pol, env, schedule, use_fused=fused)
                torch.cuda.synchronize()
                if rep:
                    walls.append(time.perf_counter() - t0)
            wall = float(np.median(walls))
            sc = command.response_figures(ct)["summary"] if n <= 64 else {}
            line = {"path": "fused_six_actions" if fused else "torch", "envs": n, "vec_steps": a.steps, "graph_steps": 8,
                    "wall_s": round(wall, 5), "us_per_vec_step": round(wall / a.steps * 1e6, 2), "ended_early": int((ct.ended_at >= 0).sum()),
                    "repeats": a.repeats, **{k: v for k, v in sc.items() if k.endswith(("_mae", "survival_rate"))},
                    "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
            env.venv.close()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
