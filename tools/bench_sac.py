"""SAC on one MI355X, one JSON line per measurement (profiles/rNN_sac_bench.jsonl):

  * act / store / sample microseconds at 16 and 4096 envs;
  * one gradient step at (d 21, A 6, B 256) and H 256 / 64: fw_sac_update (as launched, and replayed from a captured graph), the torch
    step eager and the torch step replayed from a captured graph (capturable Adam) -- the baseline is this project's own torch path;
  * end-to-end env-steps/s of sac.SAC at 16 envs with gradient_steps 1 and -1.

Timing: device events around `iters` back-to-back calls after `warmup` calls, median of `repeats` such blocks.

    python tools/bench_sac.py [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import sac as S  # noqa: E402


def timed_us(fn, iters, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return {"us": round(statistics.median(out), 2), "us_min": round(min(out), 2), "us_max": round(max(out), 2), "iters": iters, "repeats": repeats}


def graphed(fn):
    fn(); fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def emit(**kw):
    print(json.dumps(kw), flush=True)


def filled_learner(H, B, fused, capturable=False, d=21, A=6, rows=4096):
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), seed=1, fused_update=fused)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        pol = S.SacPolicy(d, A, H).cuda()
    opts = S.make_optimizers(pol, cfg, capturable=capturable)
    buf = S.ReplayBufferDevice(rows, 16, d, A, "cuda")
    g = torch.Generator(device="cuda").manual_seed(2)
    buf.ring.copy_(torch.randn(buf.ring.shape, device="cuda", generator=g).clamp(-5, 5))
    buf.ring[:, -1] = (buf.ring[:, -1] > 1.5).float()
    buf.counters[S.CTR_SIZE] = rows
    return cfg, pol, opts, buf


def bench_update(H, B, it):
    shape = {"obs_dim": 21, "act_dim": 6, "hidden": H, "batch": B}
    cfg, pol, opts, buf = filled_learner(H, B, True)
    fused = S.FusedSacUpdate(pol, opts, cfg); fused.pack()
    batch = buf.sample(cfg.seed, torch.zeros((B, buf.row), device="cuda"))
    step = lambda: fused.run(batch, buf.counters)
    emit(what="gradient_step", path="fused", **shape, **timed_us(step, *it))
    emit(what="gradient_step", path="fused_graph", **shape, **timed_us(graphed(step), *it))
    for name, cap in (("torch_eager", False), ("torch_graph", True)):
        cfg, pol, opts, buf = filled_learner(H, B, False, capturable=cap)
        batch = buf.sample(cfg.seed, torch.zeros((B, buf.row), device="cuda"))
        noise = S.sac_noise(cfg.seed, buf.counters, B, 6)
        step = lambda: S.sac_update_torch(pol, opts, batch, noise[0], noise[1], cfg)
        if cap:
            # (capturable Adam keeps its step counts on the device; the captured step zeroes gradients in place)
            try:
                run = graphed(step)
            except Exception as e:          # a torch build that cannot capture the optimiser: say so instead of a figure
                emit(what="gradient_step", path=name, **shape, error=str(e)[:200])
                continue
        else:
            run = step
        emit(what="gradient_step", path=name, **shape, **timed_us(run, *it))


def bench_pieces(n, it):
    env = P.FixedwingLowLevelVecEnv(num_envs=n, seed=0)
    sac = S.SAC(env, S.SACConfig(seed=0, use_graphs=False))
    env.reset_tensor(); sac._started = True
    for _ in range(4):
        sac.collect_step(train=False)
    emit(what="act", envs=n, hidden=256, **timed_us(lambda: sac.act(S.ACT_STOCHASTIC), *it))
    emit(what="act_warmup", envs=n, **timed_us(lambda: sac.act(S.ACT_WARMUP), *it))
    emit(what="store", envs=n, **timed_us(sac._store, *it))
    emit(what="sample", envs=n, batch=256, **timed_us(lambda: sac.buffer.sample(0, sac.batch, sac.batch_idx), *it))
    emit(what="env_step", envs=n, **timed_us(lambda: env.step_tensor(sac.act_env), *it))
    env.close()


def bench_end_to_end(gradient_steps, fused, graphs, vec_steps):
    env = P.FixedwingLowLevelVecEnv(num_envs=16, seed=0)
    sac = S.SAC(env, S.SACConfig(seed=0, gradient_steps=gradient_steps, fused_update=fused, use_graphs=graphs))
    sac.learn(16 * 16)                       # warm-up steps, the first trained steps, the captures
    torch.cuda.synchronize()
    t0, n0 = time.perf_counter(), sac.num_timesteps
    sac.learn(16 * vec_steps)
    dt = time.perf_counter() - t0
    emit(what="end_to_end", envs=16, gradient_steps=sac.G, fused_update=fused, use_graphs=graphs, vec_steps=vec_steps,
         env_steps_per_s=round((sac.num_timesteps - n0) / dt, 1), gradient_steps_per_s=round(sac.G * vec_steps / dt, 1))
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a tenth of the iterations")
    a = ap.parse_args()
    it = (20, 5, 3) if a.quick else (200, 20, 5)            # iters, warmup, repeats
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__)
    for n in (16, 4096):
        bench_pieces(n, it)
    for H in (256, 64):
        bench_update(H, 256, it)
    vs = 50 if a.quick else 500
    for gs in (1, -1):
        bench_end_to_end(gs, True, True, vs)
        bench_end_to_end(gs, True, False, vs)
        bench_end_to_end(gs, False, True, max(vs // 5, 10))


if __name__ == "__main__":
    main()
