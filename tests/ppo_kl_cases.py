"""Shared pieces of the target_kl tests (tests/test_ppo_target_kl_cpu.py, tests/test_ppo_target_kl_gpu.py): the pinned inputs, a second
statement of SB3's ``PPO.train()`` loop with ``target_kl`` in float64 -- written from the formulas alone: torch.autograd.grad and a
hand-written Adam, no nn.Module and no torch.optim -- and the helper that picks ``target_kl`` so that the stop falls on a wanted
minibatch.

The inputs.  Rollout buffers of 2 minibatches x 4 epochs (n_mb = 8) with a learning rate of 1e-2, so that the KL grows within a few
steps; shapes (obs, actions, batch): SHAPES.  The old log-probs are jittered by JITTER = 0.05 (tests/mp_diag_jobs.py uses 0.2): the KL of
the untouched policy is then about 1e-3 and what the optimiser steps add stands clear of it.

The condition on the inputs (not a tolerance on the kernel).  A case asks for the stop at minibatch j; the limit L = float32(1.5 *
target_kl) is put between the KL of minibatch j and the largest KL before it.  For every minibatch up to and including j, the KL sits
at least MARGIN = 5 % of L away from L -- in the float64 restatement AND in the float32 torch step.  5 % is far above what float32
summation order moves a mean of 64-128 terms (about 1e-6 relative) and above what the learner tolerances of sac_cases.TOL (2e-3 on the
parameters) let the trajectory move it, so every correct learner reaches the same verdict at every minibatch.  A (shape, seed) whose
KL series does not allow that for some case is replaced by the next seed, and the replacement is recorded in SEEDS below; the 5 % is
never touched.
"""
import copy
import math

import numpy as np
import torch

import mp_diag_jobs as J
import sac_cases as SC

TOL = SC.TOL
SHAPES = [(28, 4, 128), (21, 6, 64), (30, 3, 128)]        # (obs_dim, act_dim, batch_size)
N_EPOCHS, MB_PER_EPOCH = 4, 2
N_MB = N_EPOCHS * MB_PER_EPOCH
LR = 1e-2
JITTER = 0.05
MARGIN = 0.05
# the stop index j of every case (None: never): the middle of epoch 2, the first minibatch of an epoch, the very last minibatch
CASES = {"mid_epoch_2": 3, "first_of_epoch": 4, "last_minibatch": 7, "never": None}
# seed per shape: the first of 5, 6, 7, ... whose KL series meets the condition for every case (test_ppo_target_kl_cpu.py checks it);
# replacements are recorded here as "shape: tried -> taken"
#   (28, 4, 128): 5 .. 11 -> 12   (seeds 5 - 11: the KL of the last minibatch is below, or within 5 % of the limit of, the one before it,
#                                  so no limit puts the stop of "last_minibatch" there with the margin)
SEEDS = {(28, 4, 128): 12, (21, 6, 64): 5, (30, 3, 128): 5}


def make_ppo(d, a, bs, device="cpu", seed=None, **cfg):
    """A learner over hand-filled buffers of 2 x bs samples (tests/mp_diag_jobs.py's fill with the smaller jitter).  The buffers are
    drawn and worked out on the CPU whatever ``device`` is, so a learner on the GPU holds the very inputs the CPU reference saw (the
    initial weights are the same anyway: the module is built on the CPU under the seed).  The minibatch order is the generator's of
    the device: ``permutation``."""
    from pyflyt_drone_amd import rollout as R
    seed = SEEDS[(d, a, bs)] if seed is None else seed
    kw = dict(n_steps=2, batch_size=bs, n_epochs=N_EPOCHS, seed=seed, use_graphs=False, ent_coef=0.01, learning_rate=LR,
              fused_six_actions=True, fused_three_actions=True)
    kw.update(cfg)
    ppo = R.PPO(J.BufEnv(bs, d, a, device), R.PPOConfig(**kw))
    g = torch.Generator(); g.manual_seed(seed)
    pol = copy.deepcopy(ppo.policy).cpu()
    obs = torch.randn(tuple(ppo.buf_obs.shape), generator=g).clamp(-10, 10)
    with torch.no_grad():
        act, _, _ = pol(obs.reshape(-1, d), generator=g)
        act = act + 0.3 * torch.randn(act.shape, generator=g)
        _, lp, _ = pol.evaluate_actions(obs.reshape(-1, d), act)
        lp = lp + JITTER * torch.randn(lp.shape, generator=g)
    adv = torch.randn((2, bs), generator=g) * 2.0 + 0.5
    ret = torch.randn((2, bs), generator=g) * 3.0
    ppo.buf_obs.copy_(obs); ppo.buf_act.copy_(act.reshape(ppo.buf_act.shape)); ppo.buf_logp.copy_(lp.reshape(2, bs))
    ppo.adv, ppo.ret = adv.to(ppo.device), ret.to(ppo.device)
    ppo.buf_val.copy_(ppo.ret - ppo.adv)
    return ppo


def permutation(ppo):
    """The minibatch order the next train() of ``ppo`` will walk (a twin of its generator: ``ppo`` itself is left alone), int64 [N_MB * bs]."""
    g = torch.Generator(device=ppo.device); g.set_state(ppo.perm_gen.get_state())
    B = ppo.cfg.n_steps * ppo.env.num_envs
    return torch.cat([torch.randperm(B, device=ppo.device, generator=g) for _ in range(ppo.cfg.n_epochs)])


class Restated:
    """SB3's ``PPO.train()`` with ``target_kl`` from its formulas, in float64 on the CPU: two 64-64 tanh networks as plain tensors in
    torch's Linear layout, the diagonal Gaussian written out, gradients from torch.autograd.grad, the joint gradient-norm clip and Adam
    by hand."""

    def __init__(self, ppo):
        pol, cfg = ppo.policy, ppo.cfg
        f = lambda t: t.detach().double().cpu().clone()      # noqa: E731
        self.names = [n for n, _ in pol.named_parameters()]
        self.p = {n: f(q) for n, q in pol.named_parameters()}
        self.m = {n: torch.zeros_like(q) for n, q in self.p.items()}
        self.v = {n: torch.zeros_like(q) for n, q in self.p.items()}
        self.cfg, self.steps = cfg, 0
        pg = ppo.optimizer.param_groups[0]
        self.lr, self.betas, self.eps = float(pg["lr"]), tuple(pg["betas"]), float(pg["eps"])
        B = cfg.n_steps * ppo.env.num_envs
        self.obs, self.act = f(ppo.buf_obs).reshape(B, -1), f(ppo.buf_act).reshape(B, -1)
        self.old, self.adv, self.ret = f(ppo.buf_logp).reshape(B), f(ppo.adv).reshape(B), f(ppo.ret).reshape(B)

    @staticmethod
    def losses(p, obs, act, old, adv, ret, cfg):
        h = torch.tanh(torch.tanh(obs @ p["pi_net.0.weight"].t() + p["pi_net.0.bias"]) @ p["pi_net.2.weight"].t() + p["pi_net.2.bias"])
        mean = h @ p["action_net.weight"].t() + p["action_net.bias"]
        g = torch.tanh(torch.tanh(obs @ p["vf_net.0.weight"].t() + p["vf_net.0.bias"]) @ p["vf_net.2.weight"].t() + p["vf_net.2.bias"])
        value = (g @ p["value_net.weight"].t() + p["value_net.bias"])[:, 0]
        ls = p["log_std"]
        logp = (-((act - mean) ** 2) / (2.0 * torch.exp(2.0 * ls)) - ls - 0.5 * math.log(2.0 * math.pi)).sum(-1)
        a = (adv - adv.mean()) / (adv.std() + 1e-8)
        log_ratio = logp - old
        ratio = torch.exp(log_ratio)
        lo, hi = torch.full_like(ratio, 1.0 - cfg.clip_range), torch.full_like(ratio, 1.0 + cfg.clip_range)
        policy_loss = -torch.minimum(a * ratio, a * torch.minimum(torch.maximum(ratio, lo), hi)).sum() / ratio.numel()
        value_loss = ((ret - value) ** 2).sum() / ratio.numel()
        entropy_loss = -(0.5 + 0.5 * math.log(2.0 * math.pi) + ls).sum()
        approx_kl = ((ratio - 1.0) - log_ratio).sum().detach() / ratio.numel()
        return policy_loss, value_loss, entropy_loss, approx_kl

    def train(self, perm, bs, target_kl=None):
        """One update over ``perm`` (the concatenated epoch permutations).  Returns dict(kl [computed], losses [computed, 3], stepped,
        epochs_run, stopped)."""
        cfg = self.cfg
        perm = perm.cpu().long()
        n_mb, per_epoch = perm.numel() // bs, perm.numel() // bs // cfg.n_epochs
        limit = None if target_kl is None else float(np.float32(1.5 * target_kl))
        kl, losses, stepped, stopped, epochs = [], [], 0, False, 0
        for mb in range(n_mb):
            if mb % per_epoch == 0:
                epochs += 1
            idx = perm[mb * bs:(mb + 1) * bs]
            q = {n: t.clone().requires_grad_(True) for n, t in self.p.items()}
            pl, vl, el, k = self.losses(q, self.obs[idx], self.act[idx], self.old[idx], self.adv[idx], self.ret[idx], cfg)
            kl.append(float(k)); losses.append([float(pl.detach()), float(vl.detach()), float(el.detach())])
            if limit is not None and float(k) > limit:
                stopped = True
                break
            grads = torch.autograd.grad(pl + cfg.ent_coef * el + cfg.vf_coef * vl, [q[n] for n in self.names], allow_unused=True)
            grads = [torch.zeros_like(self.p[n]) if g is None else g for n, g in zip(self.names, grads)]
            norm = math.sqrt(sum(float((g * g).sum()) for g in grads))
            clip = min(cfg.max_grad_norm / (norm + 1e-6), 1.0)
            self.steps += 1
            b1, b2 = self.betas
            for n, g in zip(self.names, grads):
                g = g * clip
                self.m[n] = b1 * self.m[n] + (1.0 - b1) * g
                self.v[n] = b2 * self.v[n] + (1.0 - b2) * g * g
                denom = self.v[n].sqrt() / math.sqrt(1.0 - b2 ** self.steps) + self.eps
                self.p[n] = self.p[n] - (self.lr / (1.0 - b1 ** self.steps)) * self.m[n] / denom
            stepped += 1
        return dict(kl=np.array(kl), losses=np.array(losses), stepped=stepped, epochs_run=epochs, stopped=stopped)


def pick_target_kl(series, j):
    """``target_kl`` for a stop at minibatch ``j`` of the no-stop KL ``series`` (None: never): the limit 1.5 * target_kl is the geometric
    mean of the KL of minibatch j and the largest KL before it (never: ten times the largest of the series)."""
    series = np.asarray(series, dtype=np.float64)
    if j is None:
        return 10.0 * float(series.max()) / 1.5
    before = float(series[:j].max()) if j > 0 else float(series[j]) / 4.0
    return math.sqrt(before * float(series[j])) / 1.5


def margins(series, j, target_kl):
    """|KL - L| / L of every minibatch up to and including the stop (never: all of them), L = float32(1.5 * target_kl); and whether the
    series puts the stop where the case wants it."""
    series = np.asarray(series, dtype=np.float64)
    L = float(np.float32(1.5 * target_kl))
    upto = series if j is None else series[:j + 1]
    over = np.nonzero(series > L)[0]
    first = None if over.size == 0 else int(over[0])
    return np.abs(upto - L) / L, first == j


def first_clear_stop(series, start=2):
    """(j, target_kl) of the first minibatch from ``start`` on at which a no-stop KL series admits a stop under the condition above:
    for inputs whose minibatch order is not pinned (a device generator's permutation, a collected rollout)."""
    for j in range(start, len(series)):
        t = pick_target_kl(series, j)
        if t > 0 and math.isfinite(t):
            m, where = margins(series, j, t)
            if where and m.min() >= MARGIN:
                return j, t
    raise AssertionError(f"no minibatch of {np.asarray(series)} admits a stop with the {MARGIN:.0%} margin: choose another seed")


def compare_with_restated(ppo, ref, tol=TOL):
    """Module parameters and Adam moments of ``ppo`` against the restatement, with no element left out; the optimiser's step count."""
    for n, q in ppo.policy.named_parameters():
        SC._close(n, q, ref.p[n], *tol["param"])
        st = ppo.optimizer.state.get(q)
        if ref.steps == 0:
            assert not st or (float(st["exp_avg"].abs().sum()) == 0.0 and float(st["exp_avg_sq"].abs().sum()) == 0.0)
            continue
        assert float(st["step"]) == ref.steps, (n, float(st["step"]), ref.steps)
        SC._close(n + " exp_avg", st["exp_avg"], ref.m[n], *tol["exp_avg"])
        SC._close(n + " exp_avg_sq", st["exp_avg_sq"], ref.v[n], *tol["exp_avg_sq"])
