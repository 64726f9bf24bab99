"""Dev tool: the six-action learner against the four-action one and the torch path (the low-level control task's shapes).

  update   fw_ppo_update_a per minibatch at (obs 21, batch 64) for A = 6 and A = 4 (one launch of n_mb minibatches, device
           time from events, median of --reps launches), and the torch path's minibatch at the same shape (PPO.train() with
           fused_update=False: autograd + torch.optim.Adam, replayed as a hipGraph per minibatch)
  e2e      env-steps/s of examples/train_lowlevel_cmd.py's configuration (batch 64, 10 epochs, 65 536 samples per update) at
           --num_envs envs, PPOConfig.fused_six_actions on and off: --updates timed updates after one warm-up update

    python tools/bench_wide_learner.py --what update --out profiles/r06_lowlevel_learner_update.jsonl
    python tools/bench_wide_learner.py --what e2e --num_envs 4096 --updates 3 --out profiles/r06_lowlevel_learner_e2e.jsonl
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import _lib, rollout as R  # noqa: E402


def fused_update_us(D, A, B, n_mb, reps):
    """Device time per minibatch of one fw_ppo_update_a launch of n_mb minibatches (median over reps launches, fresh images)."""
    L = _lib.lib()
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    S = n_mb * B
    flat0 = torch.randn(L.fw_ppo_param_count_a(D, A), device="cuda", generator=g) * 0.1
    ns = L.fw_ppo_moment_count_a(A)
    obs, act = torch.randn((S, D), device="cuda", generator=g), torch.randn((S, A), device="cuda", generator=g)
    lp, adv, ret = (torch.randn(S, device="cuda", generator=g) for _ in range(3))
    perm = torch.randperm(S, device="cuda", generator=g).to(torch.int32)
    ws = torch.zeros(int(L.fw_ppo_update_workspace_bytes_a(n_mb, B, D, A)), dtype=torch.uint8, device="cuda")
    loss = torch.zeros(16, device="cuda")
    H = R._PpoHyper(lr=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, beta1=0.9, beta2=0.999, eps=1e-5,
                    adv_mean=0.0, adv_std=1.0, norm_adv=1, step0=0)
    times = []
    for r in range(reps + 1):
        flat, m, v = flat0.clone(), torch.zeros(ns, device="cuda"), torch.zeros(ns, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(L.fw_ppo_update_a(*[R._p(x) for x in (flat, m, v, obs, act, lp, adv, ret, perm)], n_mb, B, D, A, C.byref(H), R._p(loss),
                                     R._p(ws), ws.numel(), None))
        e1.record(); torch.cuda.synchronize()
        st = C.c_uint32(0)
        _lib.check(L.fw_ppo_update_status(R._p(ws), ws.numel(), C.byref(st), None, None))
        assert st.value == 0, st.value
        if r:                                   # (the first launch: warm-up)
            times.append(e0.elapsed_time(e1) * 1e3 / n_mb)
    times.sort()
    return times[len(times) // 2], times


class _BufEnv:
    def __init__(self, n, d, a):
        self.device, self.num_envs, self.obs_dim, self.act_dim = torch.device("cuda"), n, d, a


def torch_update_us(D, A, B, n_mb):
    """Wall time per minibatch of PPO.train() on the torch path (hipGraph per minibatch), over n_mb minibatches after a warm-up call."""
    T, n = 4, n_mb * B // 4
    ppo = R.PPO(_BufEnv(n, D, A), R.PPOConfig(n_steps=T, batch_size=B, n_epochs=1, use_graphs=True, fused_update=False, ent_coef=0.0))
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    ppo.buf_obs.copy_(torch.randn(ppo.buf_obs.shape, device="cuda", generator=g))
    ppo.buf_act.copy_(torch.randn(ppo.buf_act.shape, device="cuda", generator=g))
    ppo.buf_logp.copy_(torch.randn(ppo.buf_logp.shape, device="cuda", generator=g) - 5)
    ppo.adv = torch.randn((T, n), device="cuda", generator=g)
    ppo.ret = torch.randn((T, n), device="cuda", generator=g)
    ppo.train()                                  # warm-up + graph capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ppo.train()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n_mb


def e2e(num_envs, fused, updates):
    spu = 32 * 2048
    env = R.VecNormalizeDevice(P.FixedwingLowLevelVecEnv(num_envs=num_envs, seed=42, device=0), norm_obs=True, norm_reward=True, clip_obs=10.0)
    n_steps = R.n_steps_for(spu, num_envs)
    ppo = R.PPO(env, R.PPOConfig(n_steps=n_steps, batch_size=64, n_epochs=10, learning_rate=3e-4, gamma=0.99, gae_lambda=0.95,
                                 clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, seed=42, fused_six_actions=fused))
    ppo.collect_rollouts(); ppo.train()          # warm-up update (allocations, graph captures)
    torch.cuda.synchronize()
    t_roll = t_upd = 0.0
    for _ in range(updates):
        t0 = time.perf_counter(); ppo.collect_rollouts(); torch.cuda.synchronize()
        t1 = time.perf_counter(); ppo.train(); torch.cuda.synchronize()
        t_roll += t1 - t0; t_upd += time.perf_counter() - t1
    steps = updates * n_steps * num_envs
    assert all(torch.isfinite(p).all() for p in ppo.policy.parameters())
    return {"fused_six_actions": fused, "collect_fused": ppo._collect_fused, "num_envs": num_envs, "n_steps": n_steps, "updates": updates,
            "env_steps_per_s": round(steps / (t_roll + t_upd)), "rollout_s_per_update": round(t_roll / updates, 4),
            "update_s_per_update": round(t_upd / updates, 4), "minibatches_per_update": 10 * spu // 64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("update", "e2e", "kernels"), default="update")
    ap.add_argument("--obs_dim", type=int, default=21)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n_mb", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    rows = []
    dev = torch.cuda.get_device_name(0)
    if a.what == "update":
        for A in (6, 4):
            med, all_ = fused_update_us(a.obs_dim, A, a.batch, a.n_mb, a.reps)
            rows.append({"path": "fw_ppo_update_a", "act_dim": A, "obs_dim": a.obs_dim, "batch": a.batch, "n_mb": a.n_mb,
                         "us_per_minibatch": round(med, 3), "all_us": [round(x, 3) for x in all_], "device": dev})
        rows.append({"path": "torch (autograd + Adam, hipGraph per minibatch)", "act_dim": 6, "obs_dim": a.obs_dim, "batch": a.batch,
                     "n_mb": a.n_mb, "us_per_minibatch": round(torch_update_us(a.obs_dim, 6, a.batch, a.n_mb), 3), "device": dev})
    elif a.what == "kernels":                   # a short run of every new kernel, for rocprofv3 --kernel-trace --stats
        fused_update_us(a.obs_dim, 6, a.batch, 256, 2)
        fused_update_us(a.obs_dim, 4, a.batch, 256, 2)
        rows.append(e2e(a.num_envs, True, 1))
    else:
        for fused in (True, False):
            rows.append(e2e(a.num_envs, fused, a.updates))
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
