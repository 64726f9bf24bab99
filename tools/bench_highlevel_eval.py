"""Wall time per vec-step of an evaluation of the high-level command task (DESIGN.md section 2e "Evaluation") on one GPU, and what the
fused evaluation does to a whole training run.

    python tools/bench_highlevel_eval.py [--legs eval e2e] [--envs 16] [--steps 4096] [--repeats 5] [--total_timesteps 2000000]
                                         [--out profiles/r12_highlevel_eval.jsonl]

Legs (one JSON line each, printed and appended to --out):
  e2e   the closing line of examples/train_highlevel_cmd.py --fused_learner over --total_timesteps steps, without and with --fused_eval
        (evaluations and checkpoints included), above a controller that examples/train_lowlevel_cmd.py --fused_learner trained for
        131 072 steps: the checkpoint pair of profiles/r11_highlevel_learner_e2e.jsonl.  Each run is a child process; they run before
        this process opens the GPU.
  eval  the replayed evaluation (evaluate.ReplayedEvaluation: hipGraphs of 8 vec-steps) at --envs envs, f64, with the torch forward
        (torch forward + step_tensor's three launches + fw_eval_track_hl) and with use_fused=True (fw_collect_act_hl -> fw_step ->
        fw_eval_track_hl), in the same session.  A timed region is --steps vec-steps of graph replays between two device
        synchronisations; --repeats regions, the median is reported with the spread.  Commander and controller are seeded
        MlpPolicies with random weights.  Under `rocprofv3 --kernel-trace --stats` the averages of fw_eval_track_hl_kernel come out
        by name.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _final_line(argv, want_line=True):
    out = subprocess.run([sys.executable] + argv, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    if out.returncode != 0:
        raise RuntimeError(f"{' '.join(argv)} failed:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    if not want_line:
        return None
    for line in reversed(out.stdout.splitlines()):
        if line.startswith("{") and '"final"' in line:
            return json.loads(line)
    raise RuntimeError(f"{' '.join(argv)} printed no closing line")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["eval"], choices=["eval", "e2e"])
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--total_timesteps", type=int, default=2_000_000)
    ap.add_argument("--low_timesteps", type=int, default=131072)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    if "e2e" in a.legs:                                    # child processes first: this process has not opened the GPU yet
        with tempfile.TemporaryDirectory(prefix="hl_eval_bench_") as tmp:
            low = os.path.join(tmp, "low")
            _final_line(["examples/train_lowlevel_cmd.py", "--total_timesteps", str(a.low_timesteps), "--fused_learner", "--out", low], want_line=False)
            ck = os.path.join(low, "models", "final_model.pt")
            for fused_eval in (False, True):
                line = _final_line(["examples/train_highlevel_cmd.py", "--low_checkpoint", ck, "--total_timesteps", str(a.total_timesteps),
                                    "--fused_learner", "--out", os.path.join(tmp, f"high_{int(fused_eval)}")] + (["--fused_eval"] if fused_eval else []))
                emit({"leg": "e2e", **line})

    if "eval" in a.legs:
        import numpy as np
        import torch
        from pyflyt_drone_amd import evaluate, rollout as R
        from pyflyt_drone_amd.highlevel import HighLevelCmdVecEnv
        assert torch.cuda.is_available(), "bench_highlevel_eval.py needs a HIP device"
        dev_name = torch.cuda.get_device_name(0)
        n = a.envs
        torch.manual_seed(21)
        ctl = R.MlpPolicy(21, 6)
        with torch.no_grad():
            for q in ctl.parameters():
                q.add_(0.1 * torch.randn_like(q))
        g = np.random.default_rng(21)
        mean, var = g.normal(0.0, 1.0, 21), g.uniform(0.5, 4.0, 21)
        torch.manual_seed(31)
        pol = R.MlpPolicy(30, 3).cuda()
        with torch.no_grad():
            for q in pol.parameters():
                q.add_(0.1 * torch.randn_like(q))
            pol.action_net.bias.copy_(torch.tensor([0.0, 100.0, 15.0]))
        targets = np.ones(n, dtype=np.int64)                # (the replays run on past the episodes: the loop body is what is timed)
        replays = max(a.steps // evaluate.REPLAY_STEPS, 1)
        for name, fused in (("replayed_torch_forward", False), ("fused_three_actions", True)):
            venv = HighLevelCmdVecEnv(n, ctl, (mean, var), seed=3)
            env = R.VecNormalizeDevice(venv, training=False, norm_reward=False, clip_obs=10.0)
            job = evaluate.ReplayedEvaluation(pol, env, targets, use_fused=fused)
            job.begin()
            with torch.cuda.stream(job.side):
                for _ in range(16):                         # warm-up replays
                    job.graph.replay()
                torch.cuda.synchronize()
                us = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    for _ in range(replays):
                        job.graph.replay()
                    torch.cuda.synchronize()
                    us.append((time.perf_counter() - t0) / (replays * evaluate.REPLAY_STEPS) * 1e6)
            emit({"leg": "eval", "path": name, "fused": bool(job.fused), "fused3": job.step.kind == "act_hl", "envs": n, "dtype": "float64",
                  "us_per_vec_step": round(float(np.median(us)), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                  "vec_steps": replays * evaluate.REPLAY_STEPS, "repeats": a.repeats, "rejected_actions": int(venv.rejected.item()),
                  "device": dev_name})
            venv.close()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
