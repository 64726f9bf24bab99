"""What the flight records and path figures cost on one GPU: wall time per vec-step of a replayed evaluation of the
waypoint task with path_figures off and on, on both bodies, and of the two kernels alone.

    python tools/bench_flight.py [--envs 16 4096] [--steps 4096] [--repeats 5] [--out profiles/r15_flight_bench.jsonl]

One JSON line per measurement, printed and appended to --out:
  eval    evaluate.ReplayedEvaluation (hipGraphs of 8 vec-steps) on the headline waypoint config, f64, with the torch forward (torch
          forward + fw_step + normalisation + the bookkeeping: ~20 framework ops off, one fw_eval_track_wp launch on) and with
          use_fused=True (fw_collect_step + fw_eval_track off / fw_eval_track_wp on), in the same session.  A timed region is --steps
          vec-steps of graph replays between two device synchronisations; --repeats regions, the median with the spread.
  kernel  fw_eval_track, fw_eval_track_wp and fw_trace_rows alone on the buffers of a stepped env: hipGraphs of 64 launches.
The `off` lines launch what the parent commit launches: they are the yardstick (tools/bench_lib.py measures the step kernel of two
builds of the library side by side).  Under `rocprofv3 --kernel-trace --stats` the kernel averages come out by name.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[16, 4096])
    ap.add_argument("--steps", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import pyflyt_drone_amd as P
    from pyflyt_drone_amd import _lib, evalstep, evaluate, flight, config as K, rollout as R
    assert torch.cuda.is_available(), "bench_flight.py needs a HIP device"
    dev_name = torch.cuda.get_device_name(0)
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    def timed(replay, per_replay, replays):
        for _ in range(16):
            replay()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(replays):
                replay()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / (replays * per_replay) * 1e6)
        return {"us": round(float(np.median(us)), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}

    cfg = K.train_waypoints_v3_config()
    for n in a.envs:
        torch.manual_seed(31)
        pol = R.MlpPolicy(K.obs_dim(cfg), 4).cuda()
        targets = np.ones(n, dtype=np.int64)                # (the replays run on past the episodes: the loop body is what is timed)
        replays = max(a.steps // evaluate.REPLAY_STEPS, 1)
        for fused in (False, True):
            for on in (False, True):
                env = R.VecNormalizeDevice(P.FixedwingVecEnv(cfg, n, seed=3), training=False, norm_reward=False, clip_obs=10.0)
                if fused and not evalstep.applies("collect_step", pol, env):
                    env.venv.close()
                    continue
                job = evaluate.ReplayedEvaluation(pol, env, targets, use_fused=fused, path_figures=on)
                job.begin()
                with torch.cuda.stream(job.side):
                    t = timed(job.graph.replay, evaluate.REPLAY_STEPS, replays)
                job.step.check()
                emit({"leg": "eval", "body": "fw_collect_step" if fused else "torch_forward", "path_figures": on, "envs": n, "dtype": "float64",
                      "us_per_vec_step": t["us"], "us_min": t["us_min"], "us_max": t["us_max"], "vec_steps": replays * evaluate.REPLAY_STEPS,
                      "repeats": a.repeats, "device": dev_name})
                env.venv.close()
        # the kernels alone, on the buffers of an env that has been stepped
        venv = P.FixedwingVecEnv(cfg, n, seed=3)
        venv.reset_tensor()
        venv.step_tensor(torch.zeros((n, 4), dtype=venv.torch_dtype, device=venv.device))
        job = evaluate.ReplayedEvaluation(pol, R.VecNormalizeDevice(venv, training=False, norm_reward=False), targets, use_fused=False, path_figures=True)
        job.carry.copy_(flight.seed_carry(venv.obs, job.path_layout))
        L, T = _lib.lib(), 8
        trace = torch.zeros((T, n, venv.obs_dim + 2), dtype=torch.float64, device=venv.device)
        idx = torch.zeros((), dtype=torch.int64, device=venv.device)
        st = torch.cuda.Stream()

        def track():
            fi = job.fin_info
            _lib.check(L.fw_eval_track(venv.rewards.data_ptr(), 1, venv.terminated.data_ptr(), venv.truncated.data_ptr(), venv.info.data_ptr(),
                                       int(venv.info.shape[1]), job.tg.data_ptr(), job.counts.data_ptr(), job.cur_rew.data_ptr(), job.cur_len.data_ptr(),
                                       job.step_ctr.data_ptr(), job.fin_rew.data_ptr(), job.fin_len.data_ptr(), job.fin_step.data_ptr(), fi.data_ptr(),
                                       n, job.E, torch.cuda.current_stream().cuda_stream))

        def rows():
            _lib.check(L.fw_trace_rows(venv.obs.data_ptr(), venv.terminal_obs.data_ptr(), venv.terminated.data_ptr(), venv.truncated.data_ptr(),
                                       venv.info.data_ptr(), int(venv.info.shape[1]), 1, n, venv.obs_dim, trace.data_ptr(), T, idx.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream))

        for name, fn in (("fw_eval_track", track), ("fw_eval_track_wp", job.books), ("fw_trace_rows", rows)):
            with torch.cuda.stream(st):
                fn()
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=st):
                    for k in range(64):
                        if name == "fw_trace_rows" and k % T == 0:
                            idx.zero_()                      # (keeps the recorder writing: every launch copies a row)
                        fn()
                t = timed(gr.replay, 64, max(a.steps // 64, 1))
            emit({"leg": "kernel", "kernel": name, "envs": n, "dtype": "float64", "us_per_launch": t["us"], "us_min": t["us_min"],
                  "us_max": t["us_max"], "launches": max(a.steps // 64, 1) * 64, "repeats": a.repeats, "device": dev_name})
        venv.close()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
