"""SAC on one MI355X, one JSON line per measurement (profiles/rNN_sac_bench.jsonl):

  * act / store / sample microseconds at 16 and 4096 envs, and the 1-step sample against the n-step sample (n_steps 3 and 8, B 256
    and 4096, with the ratio to the 1-step sample of the same job) and the mark + store of an n-step buffer; the hindsight-relabelling
    sample (her_goals 4, horizon 8 and 64) against the same 1-step sample;
  * one gradient step at (d 21, A 6, B 256) and H 256 / 64: fw_sac_update (as launched, and replayed from a captured graph), the torch
    step eager and the torch step replayed from a captured graph (capturable Adam) -- the baseline is this project's own torch path;
  * the same four at H 256 for every batch size of --batches (default 256 ... 8192: up to 512 rows the 24-launch form, above it the
    wide form), with microseconds per step and per sample;
  * end-to-end env-steps/s of sac.SAC at 16 envs with gradient_steps 1 and -1, and at 4096 envs with one 4096-row gradient step per
    vec-step on both env variants (the large-env recipe of examples/train_lowlevel_sac.py), the tracking variant with n_steps 3,
    with her_goals 4 and with prioritized replay too;
  * prioritized replay (`per`), on the ring of a 16-env and of a 4096-env learner: the prioritized sample against the 1-step sample
    (B 256 and 4096), mark-new + store + rebuild against the store alone, the rebuild and the priority write-back alone, and the
    weighted gradient step with its write-back and rebuild against the plain step (H 256, B 256 and 4096);
  * running normalisation (`norm`): fw_sac_act_norm against fw_sac_act at 16 and 4096 envs (same process, same observations, the
    statistics a few vec-steps made), fw_replay_normalize at B 256 and 4096 with the statistics launch beside it, and the 4096-env
    vec-step with its 4096-row gradient step with both flags on against both flags off.

Timing: device events around `iters` back-to-back calls after `warmup` calls, median of `repeats` such blocks.  --runs N repeats the
chosen sections N times (a "run" field tells them apart): the spread between runs is the run-to-run noise of a figure.

    python tools/bench_sac.py [--quick] [--sections pieces,update,batches,end_to_end,end_to_end_large,per,norm] [--batches 256,4096] [--runs 3]
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


RUN = {}


def emit(**kw):
    print(json.dumps({**kw, **RUN}), flush=True)


def per_sample(t, B):
    return {**t, "us_per_sample": round(t["us"] / B, 5)}


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
    emit(what="gradient_step", path="fused", **shape, **per_sample(timed_us(step, *it), B))
    emit(what="gradient_step", path="fused_graph", **shape, **per_sample(timed_us(graphed(step), *it), B))
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
        emit(what="gradient_step", path=name, **shape, **per_sample(timed_us(run, *it), B))


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
    bench_nstep_sample(sac, n, it)
    env.close()


def bench_nstep_sample(sac, n, it):
    """The 1-step gather against the n-step gather on the same rows and counters (d 21, A 6), B 256 and 4096; store with and without
    the mark launch.  The n-step buffers borrow the learner's ring; their ends carry an episode end every 50th row."""
    one = sac.buffer
    for B in (256, 4096):
        out, idx = torch.zeros((B, one.row), device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        base = timed_us(lambda: one.sample(0, out, idx), *it)
        emit(what="sample", envs=n, batch=B, n_steps=1, **base)
        for k in (3, 8):
            buf = S.ReplayBufferDevice(one.capacity, n, one.obs_dim, one.act_dim, "cuda", n_steps=k)
            buf.ring, buf.counters = one.ring, one.counters
            buf.ends[::50] = 1
            t = timed_us(lambda: buf.sample(0, out, idx, gamma=0.99), *it)
            emit(what="sample", envs=n, batch=B, n_steps=k, **t, ratio_to_one_step=round(t["us"] / base["us"], 3))
        for h in (8, 64):            # the relabelling gather: 4 of 5 rows walk up to h rows, read one more row and recompute the reward
            buf = S.ReplayBufferDevice(one.capacity, n, one.obs_dim, one.act_dim, "cuda", her_goals=4, her_horizon=h,
                                       her_task=S.her_task_of(sac.env.cfg))
            buf.ring, buf.counters = one.ring, one.counters
            buf.ends[::50] = 1
            t = timed_us(lambda: buf.sample(0, out, idx), *it)
            emit(what="sample", envs=n, batch=B, her_goals=4, her_horizon=h, **t, ratio_to_one_step=round(t["us"] / base["us"], 3))
    e = sac.env
    buf = S.ReplayBufferDevice(one.capacity, n, one.obs_dim, one.act_dim, "cuda", n_steps=3)
    t = timed_us(lambda: buf.store(sac.obs_stage, sac.act_f32, e.rewards, e.obs, e.terminal_obs, e.terminated, e.truncated), *it)
    emit(what="mark_and_store", envs=n, n_steps=3, **t)


def bench_per(n, it):
    """Prioritized replay on the ring of an n-env learner (the reference's 200 000-row buffer, d 21, A 6, H 256), every figure beside
    the plain one of the same process: sample, store, and the gradient step with everything prioritization adds around it."""
    env = P.FixedwingLowLevelVecEnv(num_envs=n, seed=0)
    sac = S.SAC(env, S.SACConfig(seed=0, use_graphs=False))
    env.reset_tensor(); sac._started = True
    for _ in range(4):
        sac.collect_step(train=False)
    one, e = sac.buffer, sac.env
    per = S.ReplayBufferDevice(one.capacity, n, one.obs_dim, one.act_dim, "cuda", prioritized=True)
    per.ring, per.counters = one.ring, one.counters
    g = torch.Generator(device="cuda").manual_seed(3)
    one.counters[S.CTR_SIZE] = one.capacity                      # a full ring: every group of the sum structure is in play
    per.prio.copy_(torch.rand(per.capacity, device="cuda", generator=g) * 0.99 + 0.01)
    per.rebuild()
    args = (sac.obs_stage, sac.act_f32, e.rewards, e.obs, e.terminal_obs, e.terminated, e.truncated)
    base = timed_us(lambda: one.store(*args), *it)
    emit(what="store", envs=n, **base)
    t = timed_us(lambda: per.store(*args), *it)
    emit(what="mark_new_store_rebuild", envs=n, capacity=per.capacity, **t, ratio_to_store=round(t["us"] / base["us"], 3))
    emit(what="per_rebuild", envs=n, capacity=per.capacity, **timed_us(per.rebuild, *it))
    for B in (256, 4096):
        out, idx, w = torch.zeros((B, one.row), device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, device="cuda")
        base = timed_us(lambda: one.sample(0, out, idx), *it)
        emit(what="sample", envs=n, batch=B, n_steps=1, **base)
        t = timed_us(lambda: per.sample(0, out, idx, w_out=w), *it)
        emit(what="sample", envs=n, batch=B, prioritized=True, capacity=per.capacity, **t, ratio_to_one_step=round(t["us"] / base["us"], 3))
        td = torch.rand(B, device="cuda", generator=g)
        emit(what="per_update_and_rebuild", envs=n, batch=B, capacity=per.capacity, **timed_us(lambda: per.update_priorities(idx, td), *it))
        cfg = S.SACConfig(batch_size=B, seed=1)
        fused = S.FusedSacUpdate(sac._policy, sac.optimizers, cfg); fused.pack()
        rows = one.sample(0, torch.zeros((B, one.row), device="cuda"))
        rows[:, -1] = (rows[:, -1] > 0.5).float()
        base = timed_us(lambda: fused.run(rows, one.counters), *it)
        emit(what="gradient_step", path="fused", envs=n, batch=B, hidden=256, **base)

        def weighted():
            fused.run(rows, one.counters, weights=w, td_out=td)
            per.update_priorities(idx, td)
        t = timed_us(weighted, *it)
        emit(what="gradient_step", path="fused_weighted_update_rebuild", envs=n, batch=B, hidden=256, capacity=per.capacity, **t,
             ratio_to_plain=round(t["us"] / base["us"], 3))
    env.close()


def bench_norm(n, it):
    """Running normalisation on an n-env learner (d 21, A 6, H 256): the normalising act against the plain act on the same
    observations, the statistics launch, and the in-place normalisation of a gathered batch."""
    env = P.FixedwingLowLevelVecEnv(num_envs=n, seed=0)
    sac = S.SAC(env, S.SACConfig(seed=0, use_graphs=False, normalize_obs=True, normalize_reward=True))
    for _ in range(4):
        sac.collect_step(train=False)
    plain = S.SAC(env, S.SACConfig(seed=0, use_graphs=False))            # the same env buffers, the plain act launch
    plain._started = True
    base = timed_us(lambda: plain.act(S.ACT_STOCHASTIC), *it)
    emit(what="act", envs=n, hidden=256, **base)
    t = timed_us(lambda: sac.act(S.ACT_STOCHASTIC), *it)
    emit(what="act_norm", envs=n, hidden=256, **t, ratio_to_act=round(t["us"] / base["us"], 3))
    emit(what="collect_stats", envs=n, **timed_us(sac._update_statistics, *it))
    for B in (256, 4096):
        rows = sac.buffer.sample(0, torch.zeros((B, sac.buffer.row), device="cuda"))
        emit(what="sample", envs=n, batch=B, n_steps=1, **timed_us(lambda: sac.buffer.sample(0, rows), *it))
        emit(what="replay_normalize", envs=n, batch=B, **timed_us(lambda: sac.normalize_batch(rows), *it))
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


def bench_end_to_end_large(variant, envs, batch, vec_steps, n_steps=1, her_goals=0, prioritized=False, normalize=False):
    """The large-env recipe: one `batch`-row gradient step per vec-step of `envs` envs, fused, one captured graph per vec-step."""
    make = P.FixedwingLowLevelDemoVecEnv if variant == "demo" else P.FixedwingLowLevelVecEnv
    env = make(num_envs=envs, seed=0)
    sac = S.SAC(env, S.SACConfig(seed=0, batch_size=batch, gradient_steps=1, learning_starts=envs, n_steps=n_steps, her_goals=her_goals,
                                 **({"prioritized": True} if prioritized else {}),
                                 **({"normalize_obs": True, "normalize_reward": True} if normalize else {})))
    sac.learn(envs * 8)                      # the warm-up step, the first trained steps, the captures
    torch.cuda.synchronize()
    t0, n0 = time.perf_counter(), sac.num_timesteps
    sac.learn(envs * vec_steps)
    dt = time.perf_counter() - t0
    emit(what="end_to_end", env=variant, envs=envs, batch=batch, n_steps=n_steps, **({"her_goals": her_goals} if her_goals else {}), **({"prioritized": True} if prioritized else {}), **({"normalize": True} if normalize else {}), gradient_steps=sac.G, fused_update=True, use_graphs=True, vec_steps=vec_steps,
         env_steps_per_s=round((sac.num_timesteps - n0) / dt, 1), us_per_vec_step=round(dt * 1e6 / vec_steps, 1))
    env.close()


SECTIONS = ("pieces", "update", "batches", "end_to_end", "end_to_end_large", "per", "norm")
BATCHES = (256, 512, 576, 1024, 2048, 4096, 8192)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a tenth of the iterations")
    ap.add_argument("--sections", type=str, default=",".join(SECTIONS), help="comma-separated, of " + ", ".join(SECTIONS))
    ap.add_argument("--batches", type=str, default=",".join(str(b) for b in BATCHES),
                    help="batch sizes of the `batches` section (H 256, d 21, A 6): one gradient step fused, torch eager and torch graph-captured")
    ap.add_argument("--runs", type=int, default=1, help="repeat the chosen sections this many times")
    a = ap.parse_args()
    sections = [s for s in a.sections.split(",") if s]
    unknown = [s for s in sections if s not in SECTIONS]
    if unknown:
        ap.error(f"unknown sections {unknown}")
    it = (20, 5, 3) if a.quick else (200, 20, 5)            # iters, warmup, repeats
    if os.environ.get("FWSIM_LIB"):          # an A/B build of the library (pyflyt_drone_amd/_lib.py): every line says so
        RUN["lib"] = os.path.basename(os.environ["FWSIM_LIB"])
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__)
    vs = 50 if a.quick else 500
    for run in range(a.runs):
        if a.runs > 1:
            RUN["run"] = run
        if "pieces" in sections:
            for n in (16, 4096):
                bench_pieces(n, it)
        if "update" in sections:
            for H in (256, 64):
                bench_update(H, 256, it)
        if "batches" in sections:
            for B in (int(b) for b in a.batches.split(",")):
                bench_update(256, B, it)
        if "end_to_end" in sections:
            for gs in (1, -1):
                bench_end_to_end(gs, True, True, vs)
                bench_end_to_end(gs, True, False, vs)
                bench_end_to_end(gs, False, True, max(vs // 5, 10))
        if "end_to_end_large" in sections:
            for variant in ("tracking", "demo"):
                bench_end_to_end_large(variant, 4096, 4096, max(vs // 2, 20))
            bench_end_to_end_large("tracking", 4096, 4096, max(vs // 2, 20), n_steps=3)
            if hasattr(S._lib.lib(), "fw_replay_sample_her"):      # (an A/B library of an older commit predates it)
                bench_end_to_end_large("tracking", 4096, 4096, max(vs // 2, 20), her_goals=4)
            if hasattr(S._lib.lib(), "fw_replay_sample_per"):      # (likewise)
                bench_end_to_end_large("tracking", 4096, 4096, max(vs // 2, 20), prioritized=True)
        if "per" in sections:
            for n in (16, 4096):
                bench_per(n, it)
        if "norm" in sections:
            if hasattr(S._lib.lib(), "fw_replay_normalize"):       # (an A/B library of an older commit predates it: the plain vec-step alone)
                for n in (16, 4096):
                    bench_norm(n, it)
                bench_end_to_end_large("tracking", 4096, 4096, max(vs // 2, 20), normalize=True)
            bench_end_to_end_large("tracking", 4096, 4096, max(vs // 2, 20))


if __name__ == "__main__":
    main()
