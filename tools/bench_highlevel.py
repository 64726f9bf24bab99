"""Wall time per vec-step of the high-level command task on one GPU.

    python tools/bench_highlevel.py [--legs step highlevel host] [--envs 16 4096] [--steps 2000] [--warmup 100] [--repeats 5]
                                    [--out profiles/r10_highlevel_bench.jsonl]

Legs (one JSON line per leg, size and launch mode):
  step       the direct-command step kernel (FW_TASK_WAYPOINTS_DIRECT) beside the four-action waypoint kernel of the same build: the headline
             config (train_waypoints_v3_config: f64, no wind) at --step-envs envs, uniform actions in [-1, 1] from a pool of 64 tensors, auto-resets
             on.  Both run the same 8 physics ticks per step; the four-action kernel has the axis-aligned tick and the scenario hand-off.
  highlevel  a whole vec-step of HighLevelCmdVecEnv (fw_command_hl -> fw_collect_act_a -> fw_step) on raw actions drawn wide of the Box;
             the controller is a seeded MlpPolicy(21, 6) with random weights.
  host       the same vec-step composed on the host as tests/test_highlevel_gpu.py composes it: numpy conditioning and normalisation,
             the torch forward of the controller, fw_step of the base env (observation download and action upload every step).
Modes: "graph" replays a captured hipGraph of 64 vec-steps, "eager" launches them one by one.  A timed region is --steps vec-steps
between two device synchronisations; --repeats regions, the median is reported with the spread.  Under `rocprofv3 --kernel-trace
--stats` the per-kernel averages of the three launches come out by name (fw_command_hl_kernel, fw_policy_act_kernel, fw_step_kernel_wd).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["step", "highlevel", "host"], choices=["step", "highlevel", "host"])
    ap.add_argument("--envs", type=int, nargs="+", default=[16, 4096])
    ap.add_argument("--step-envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--host-steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--modes", nargs="+", default=["graph", "eager"], choices=["graph", "eager"])
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import pyflyt_drone_amd as P
    from pyflyt_drone_amd import config as K, rollout as R
    from pyflyt_drone_amd.highlevel import HighLevelCmdVecEnv, condition_command
    assert torch.cuda.is_available(), "bench_highlevel.py needs a HIP device"
    dev_name = torch.cuda.get_device_name(0)
    lines = []

    def emit(line):
        line["device"] = dev_name
        print(json.dumps(line), flush=True)
        lines.append(line)

    def timed(stepper, steps):
        stepper.run(a.warmup)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            stepper.run(steps)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / steps * 1e6)
        return {"us_per_vec_step": round(float(np.median(us)), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                "vec_steps": steps, "repeats": a.repeats, "warmup": a.warmup}

    def pool_of(n, width, scale=None, shift=None, dtype=torch.float64):
        g = torch.Generator(device="cpu").manual_seed(0)
        if scale is None:
            return [(torch.rand((n, width), generator=g, dtype=torch.float64) * 2 - 1).to(dtype).cuda() for _ in range(bench.POOL)]
        return [(torch.randn((n, width), generator=g, dtype=torch.float64) * scale + shift).to(dtype).cuda() for _ in range(bench.POOL)]

    def controller(seed=21):
        torch.manual_seed(seed)
        p = R.MlpPolicy(21, 6)
        with torch.no_grad():
            for q in p.parameters():
                q.add_(0.1 * torch.randn_like(q))
        g = np.random.default_rng(seed)
        return p, g.normal(0.0, 1.0, 21), g.uniform(0.5, 4.0, 21)

    hl_scale = torch.tensor([2.0 * math.pi, 300.0, 40.0], dtype=torch.float64)
    hl_shift = torch.tensor([0.0, 60.0, 15.0], dtype=torch.float64)

    if "step" in a.legs:
        n = a.step_envs
        for name, cfg, width in (("waypoints_step", K.train_waypoints_v3_config(), 4),
                                 ("direct_step", K.waypoints_direct_config(sparse_reward=True, num_targets=8, goal_reach_distance=4.0,
                                                                           angle_representation="euler"), 6)):
            for mode in a.modes:
                env = P.FixedwingVecEnv(cfg, n, seed=42)
                env.reset_tensor()
                st = bench.Stepper(env, pool_of(n, width), use_graph=(mode == "graph"))
                r = timed(st, a.steps)
                c = env.get_counters()
                emit({"leg": name, "envs": n, "mode": mode, "lanes_per_env": env.lanes_per_env, **r,
                      "env_steps_per_s": round(n / r["us_per_vec_step"] * 1e6), "resets": c["resets"], "fallbacks": c["fallbacks"],
                      "scenario_hits": c["scenario_hits"]})
                env.close()

    if "highlevel" in a.legs:
        for n in a.envs:
            for mode in a.modes:
                pol, mean, var = controller()
                env = HighLevelCmdVecEnv(n, pol, (mean, var), seed=42)
                env.reset_tensor()
                st = bench.Stepper(env, pool_of(n, 3, hl_scale, hl_shift), use_graph=(mode == "graph"))
                r = timed(st, a.steps)
                emit({"leg": "highlevel_vec_step", "envs": n, "mode": mode, "lanes_per_env": env.lanes_per_env, **r,
                      "env_steps_per_s": round(n / r["us_per_vec_step"] * 1e6), "resets": env.get_counters()["resets"],
                      "rejected": int(env.rejected.item())})
                env.close()

    if "host" in a.legs:
        for n in a.envs:
            pol, mean, var = controller()
            pol = pol.cuda()
            B = P.FixedwingWaypointsDirectVecEnv(n, flight_dome_size=200.0, angle_representation="euler", seed=42)
            B.reset_tensor()
            pool = [p.cpu().numpy() for p in pool_of(n, 3, hl_scale, hl_shift)]

            class Host:
                i = 0
                def run(self, k):
                    for _ in range(k):
                        raw = pool[self.i % len(pool)]; self.i += 1
                        low = np.concatenate([B.obs.cpu().numpy()[:, 0:18], condition_command(raw, 200.0)], axis=1)
                        norm = np.clip((low - mean) / np.sqrt(var + 1e-8), -10.0, 10.0).astype(np.float32)
                        with torch.no_grad():
                            act = pol.action_net(pol.pi_net(torch.from_numpy(norm).cuda())).clamp(-1.0, 1.0)
                        B.step_tensor(act.to(torch.float64))
            r = timed(Host(), a.host_steps)
            emit({"leg": "host_composition", "envs": n, "mode": "eager", **r, "env_steps_per_s": round(n / r["us_per_vec_step"] * 1e6)})
            B.close()

    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
