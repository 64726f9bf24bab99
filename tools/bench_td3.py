"""TD3 on one MI355X, one JSON line per measurement (profiles/rNN_td3.jsonl):

  * fw_td3_act (exploring and warm-up) at 16 and 4096 envs, with fw_sac_act beside it;
  * one gradient step at (d 21, A 6, H 256) and B 256 / 512: fw_td3_update with and without the actor part, as launched and replayed
    from a captured graph; beside them, in the same job, SAC's fused step (the yardstick) and this module's torch step with and
    without the actor part;
  * the 16-env vec-step end to end (gradient_steps 1 and -1, fused, graphs), with SAC's beside it.

Timing is tools/bench_sac.py's: device events around `iters` back-to-back calls after `warmup` calls, median of `repeats` such blocks.

    python tools/bench_td3.py [--quick] [--sections act,update,end_to_end]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import sac as S, td3 as T  # noqa: E402
from bench_sac import bench_end_to_end as sac_end_to_end, emit, filled_learner as sac_filled_learner, graphed, per_sample, timed_us  # noqa: E402


def filled_learner(H, B, d=21, A=6, rows=4096):
    """bench_sac.filled_learner's ring under a TD3 learner."""
    cfg = T.TD3Config(batch_size=B, net_arch=(H, H), seed=1)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        pol = T.Td3Policy(d, A, H).cuda()
    opts = T.make_optimizers(pol, cfg)
    _, _, _, buf = sac_filled_learner(H, B, True, d=d, A=A, rows=rows)
    return cfg, pol, opts, buf


def bench_act(n, it):
    env = P.FixedwingLowLevelVecEnv(num_envs=n, seed=0)
    td3 = T.TD3(env, T.TD3Config(seed=0, use_graphs=False))
    sac = S.SAC(env, S.SACConfig(seed=0, use_graphs=False))
    env.reset_tensor(); td3._started = sac._started = True
    for _ in range(4):
        td3.collect_step(train=False)
    emit(what="act", algo="td3", envs=n, hidden=256, **timed_us(lambda: td3.act(T.ACT_EXPLORE), *it))
    emit(what="act_warmup", algo="td3", envs=n, **timed_us(lambda: td3.act(T.ACT_WARMUP), *it))
    emit(what="act", algo="sac", envs=n, hidden=256, **timed_us(lambda: sac.act(S.ACT_STOCHASTIC), *it))
    env.close()


def bench_update(H, B, it):
    shape = {"obs_dim": 21, "act_dim": 6, "hidden": H, "batch": B}
    cfg, pol, opts, buf = filled_learner(H, B)
    fused = T.FusedTd3Update(pol, opts, cfg); fused.pack()
    batch = buf.sample(cfg.seed, torch.zeros((B, buf.row), device="cuda"))
    for with_actor in (False, True):
        step = lambda: fused.run(batch, buf.counters, with_actor)
        emit(what="gradient_step", algo="td3", path="fused", with_actor=with_actor, **shape, **per_sample(timed_us(step, *it), B))
        emit(what="gradient_step", algo="td3", path="fused_graph", with_actor=with_actor, **shape, **per_sample(timed_us(graphed(step), *it), B))
    # the yardstick, in the same job: SAC's fused step on the same rows
    scfg, spol, sopts, sbuf = sac_filled_learner(H, B, True)
    sfused = S.FusedSacUpdate(spol, sopts, scfg); sfused.pack()
    sstep = lambda: sfused.run(batch, sbuf.counters)
    emit(what="gradient_step", algo="sac", path="fused", **shape, **per_sample(timed_us(sstep, *it), B))
    emit(what="gradient_step", algo="sac", path="fused_graph", **shape, **per_sample(timed_us(graphed(sstep), *it), B))
    # this module's torch step
    cfg, pol, opts, buf = filled_learner(H, B)
    noise = S.sac_noise(cfg.seed, buf.counters, B, 6)[0]
    for with_actor in (False, True):
        step = lambda: T.td3_update_torch(pol, opts, batch, noise, cfg, with_actor=with_actor)
        emit(what="gradient_step", algo="td3", path="torch_eager", with_actor=with_actor, **shape, **per_sample(timed_us(step, *it), B))


def bench_end_to_end(gradient_steps, vec_steps):
    env = P.FixedwingLowLevelVecEnv(num_envs=16, seed=0)
    td3 = T.TD3(env, T.TD3Config(seed=0, gradient_steps=gradient_steps))
    td3.learn(16 * 16)                       # warm-up steps, the first trained steps, the captures
    torch.cuda.synchronize()
    t0, n0 = time.perf_counter(), td3.num_timesteps
    td3.learn(16 * vec_steps)
    dt = time.perf_counter() - t0
    emit(what="end_to_end", algo="td3", envs=16, gradient_steps=td3.G, policy_delay=td3.cfg.policy_delay, fused_update=True, use_graphs=True,
         graphs=len(td3._graphs), vec_steps=vec_steps, env_steps_per_s=round((td3.num_timesteps - n0) / dt, 1),
         us_per_vec_step=round(dt * 1e6 / vec_steps, 1), gradient_steps_per_s=round(td3.G * vec_steps / dt, 1))
    env.close()


SECTIONS = ("act", "update", "end_to_end")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--sections", type=str, default=",".join(SECTIONS))
    a = ap.parse_args()
    sections = [s for s in a.sections.split(",") if s]
    for s in sections:
        if s not in SECTIONS:
            ap.error(f"unknown section {s!r}; choose from {', '.join(SECTIONS)}")
    it = (20, 5, 3) if a.quick else (200, 20, 5)
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__)
    if "act" in sections:
        for n in (16, 4096):
            bench_act(n, it)
    if "update" in sections:
        for B in (256, 512):
            bench_update(256, B, (10, 3, 3) if a.quick else (100, 10, 5))
    if "end_to_end" in sections:
        steps = 50 if a.quick else 500
        for g in (1, -1):
            bench_end_to_end(g, steps)
            sac_end_to_end(g, True, True, steps)


if __name__ == "__main__":
    main()
