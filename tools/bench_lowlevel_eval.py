"""Wall time of one evaluation of the low-level controller, in examples/eval_lowlevel.py's configuration (16 envs, 16 episodes,
2000-step truncation), on the two replayed paths -- the torch policy forward and the fused six-action one (fw_collect_act_a) -- both
keeping their books with fw_eval_track_ll.  A four-action evaluation at the same env count (waypoints, fw_collect_step ->
fw_eval_track) runs beside them so that, under `rocprofv3 --kernel-trace --stats`, the statistics of fw_eval_track_ll_kernel
and fw_eval_track_kernel come out side by side: what the tracking sums add to a bookkeeping launch.

    python tools/bench_lowlevel_eval.py [--repeats 3] [--out profiles/r07_lowlevel_eval.jsonl]

The policy is a seeded MlpPolicy with zeroed action weights (every command 0, throttle 0.5), so the episodes are long: the figure
is per evaluation and per vec-step of it.  One JSON line per path, printed and appended to --out.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--episodes", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import pyflyt_drone_amd as P
    from pyflyt_drone_amd import config as K, evaluate, rollout as R

    targets = np.array([(a.episodes + i) // a.envs for i in range(a.envs)])
    lines = []

    def run(name, cfg, act_dim, fused):
        venv = P.FixedwingVecEnv(cfg, a.envs, seed=3)
        env = R.VecNormalizeDevice(venv, training=False, norm_reward=False, clip_obs=10.0)
        torch.manual_seed(0)
        pol = R.MlpPolicy(env.obs_dim, act_dim).cuda()
        with torch.no_grad():
            pol.action_net.weight.zero_()
        walls = []
        for rep in range(a.repeats + 1):                    # the first one warms up (library, LDS carve-out, allocator)
            venv.seed(3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            job = evaluate.ReplayedEvaluation(pol, env, targets, use_fused=fused)
            r = job.run(None)
            torch.cuda.synchronize()
            if rep:
                walls.append(time.perf_counter() - t0)
        wall = float(np.median(walls))
        line = {"path": name, "task": "lowlevel" if act_dim == 6 else "waypoints", "envs": a.envs, "episodes": len(r.episode_lengths),
                "fused": bool(job.fused), "vec_steps": job.steps, "wall_s": round(wall, 4), "us_per_vec_step": round(wall / job.steps * 1e6, 2),
                "mean_ep_length": r.mean_ep_length, "repeats": a.repeats, **{k.split("/", 1)[1]: v for k, v in r.tracking_scalars().items()},
                "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        venv.close()

    ll = K.lowlevel_config()                                # examples/eval_lowlevel.py's env: 2000-step truncation
    run("replayed_torch", ll, 6, False)
    run("fused_six_actions", ll, 6, True)
    run("fused_four_actions_fw_eval_track", K.train_waypoints_v3_config(), 4, True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
