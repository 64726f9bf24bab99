"""Step time of the low-level task's kernels (fw_step_kernel_ll<T, G, WIND, V>; --variant 1: V = 1, the SAC script's env), which
bench.py does not cover.

    python tools/bench_lowlevel.py [--envs 4096] [--steps 2000] [--warmup 200] [--lanes 1|8] [--dtype float64|float32] [--variant 0|1]

Eager fw_step launches on one GPU with fixed random actions in [-1, 1] (episodes end and auto-reset on the way); prints one JSON line
with the mean device time per step from HIP events.  Under `rocprofv3 --kernel-trace --stats -- python3 tools/bench_lowlevel.py` the
kernel's own launch statistics come out beside it.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--lanes", type=int, choices=(1, 8), default=None)
    ap.add_argument("--dtype", choices=("float64", "float32"), default="float64")
    ap.add_argument("--variant", type=int, choices=(0, 1), default=0, help="fw_config.lowlevel_variant: 0 the tracking env, 1 the SAC script's")
    a = ap.parse_args()
    if a.lanes is not None:
        os.environ["FWSIM_LANES_PER_ENV"] = str(a.lanes)
    import torch
    import pyflyt_drone_amd as P
    env = (P.FixedwingLowLevelDemoVecEnv if a.variant else P.FixedwingLowLevelVecEnv)(a.envs, seed=1, dtype=a.dtype)
    env.reset_tensor()
    g = torch.Generator(device="cpu").manual_seed(0)
    acts = [(torch.rand((a.envs, 6), generator=g, dtype=torch.float64) * 2 - 1).to(env.device, env.torch_dtype) for _ in range(16)]
    for t in range(a.warmup):
        env.step_tensor(acts[t % 16])
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for t in range(a.steps):
        env.step_tensor(acts[t % 16])
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / a.steps
    c = env.get_counters()
    print(json.dumps({"task": "lowlevel", **({"variant": a.variant} if a.variant else {}), "envs": a.envs, "lanes_per_env": env.lanes_per_env, "dtype": a.dtype, "steps": a.steps,
                      "us_per_step": round(us, 2), "env_steps_per_s": round(a.envs / us * 1e6), "resets": c["resets"]}))
    env.close()


if __name__ == "__main__":
    main()
