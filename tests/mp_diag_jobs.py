"""Ranks of the world_size-2 ``gloo`` jobs of tests/test_learner_diag_cpu.py (CPU tensors, the torch path of the learner): started
with the ``spawn`` context by the test itself; each puts its result on the queue it was given."""
import os


class BufEnv:
    """Just enough env for PPO.__init__ / train(): the update runs on hand-filled rollout buffers."""
    def __init__(self, n, d, a, device="cpu"):
        import torch
        self.device, self.num_envs, self.obs_dim, self.act_dim = torch.device(device), n, d, a


def filled_ppo(d, a, bs, n_epochs, T=4, n=256, seed=5, device="cpu", fill_seed=None, **cfg):
    """The buffers of the learner tests: T x n samples, actions 0.3 sigma off-policy, old log-probs jittered by 0.2 (about a third
    of the samples end outside the clip range), plus value predictions for the explained variance."""
    import torch
    from pyflyt_drone_amd import rollout as R
    kw = dict(n_steps=T, batch_size=bs, n_epochs=n_epochs, seed=seed, use_graphs=False, ent_coef=0.01)
    kw.update(cfg)
    ppo = R.PPO(BufEnv(n, d, a, device), R.PPOConfig(**kw))
    g = torch.Generator(device=device); g.manual_seed(seed if fill_seed is None else fill_seed)
    ppo.buf_obs.copy_(torch.randn(ppo.buf_obs.shape, device=device, generator=g).clamp(-10, 10))
    with torch.no_grad():
        act, _, _ = ppo.policy(ppo.buf_obs.reshape(-1, d), generator=g)
        ppo.buf_act.copy_((act + 0.3 * torch.randn(act.shape, device=device, generator=g)).reshape(ppo.buf_act.shape))
        _, lp2, _ = ppo.policy.evaluate_actions(ppo.buf_obs.reshape(-1, d), ppo.buf_act.reshape(-1, a))
        ppo.buf_logp.copy_((lp2 + 0.2 * torch.randn(lp2.shape, device=device, generator=g)).reshape(T, n))
    ppo.adv = torch.randn((T, n), device=device, generator=g) * 2.0 + 0.5
    ppo.ret = torch.randn((T, n), device=device, generator=g) * 3.0
    ppo.buf_val.copy_(ppo.ret - ppo.adv)           # (GAE's identity: returns = advantages + values)
    return ppo


def diag_rank(rank, world, port, q, dist_update):
    """One rank: its own buffers (filled from seed + rank), two train() calls with diagnostics on."""
    import numpy as np
    import torch
    import torch.distributed as td
    from pyflyt_drone_amd import rollout as R
    torch.set_num_threads(1)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ppo = filled_ppo(12, 4, 32, 2, T=2, n=64, fill_seed=5 + rank, diagnostics=True, dist_update=dist_update)
        sent, calls = [], [0]
        reduce_ = R.all_reduce_sum_

        def spy(t):                                # what this rank hands to the one all-reduce of the diagnostics
            calls[0] += 1
            if t.dtype == torch.float64 and t.numel() > 1:
                sent.append(t.clone().numpy())
            return reduce_(t)
        R.all_reduce_sum_ = spy
        ppo.train()
        first = dict(ppo.diagnostics)
        ppo.train()
        local_ev = R.explained_variance(ppo.buf_val.numpy(), ppo.ret.numpy())
        q.put((rank, dict(replicated=bool(ppo._replicated), first=first, scalars=dict(ppo.diagnostics),
                          series={k: np.array(v) for k, v in ppo.diagnostic_series.items()}, sent=sent, reduces=calls[0],
                          local_ev=local_ev, logs=dict(ppo.logs), ret=ppo.ret.reshape(-1).numpy(), adv=ppo.adv.reshape(-1).numpy(),
                          weights=torch.cat([p.detach().reshape(-1) for p in ppo.policy.parameters()]).numpy())))
    finally:
        td.destroy_process_group()
