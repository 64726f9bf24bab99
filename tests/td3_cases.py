"""Shared pieces of the TD3 tests (tests/test_td3_cpu.py, tests/test_td3_gpu.py): the pinned inputs of the update-parity cases (those of
tests/sac_cases.py, with an actor whose output sits away from zero so that the action clamp of the smoothed target is reached), the
comparison of two learners under the project's learner tolerances, and a second statement of the gradient step written with
torch.autograd.grad and its own Adam."""
import copy

import torch

from pyflyt_drone_amd import td3 as T

import sac_cases as SC

SHAPES, SEEDS, TOL, make_batch = SC.SHAPES, SC.SEEDS, SC.TOL, SC.make_batch


def make_policy(d, A, H, seed, perturb=0.0, bias=1.0):
    """torch's default initialisation under `seed` (the global generator is left alone); `perturb` adds perturb x N(0, 1) to the trained
    networks; `bias` goes onto the actor's output bias with alternating sign, so tanh(actor) sits near +-tanh(bias) and smoothing noise
    pushes part of the target actions past +-1.  The targets are copies."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        pol = T.Td3Policy(d, A, H)
        with torch.no_grad():
            if perturb:
                for name in T.TRAINED:
                    for q in getattr(pol, name).parameters():
                        q.add_(perturb * torch.randn_like(q))
            pol.actor[4].bias.add_(bias * torch.tensor([1.0 if j % 2 == 0 else -1.0 for j in range(A)]))
            for name in T.TRAINED:
                getattr(pol, name + "_target").load_state_dict(getattr(pol, name).state_dict())
    return pol


def make_noise(A, B, seed, step, scale=1.0):
    g = torch.Generator().manual_seed(3000 + 17 * seed + step)
    return scale * torch.randn((B, A), generator=g)


def learner(pol, cfg, dtype=None, device=None):
    """A deep copy of `pol` in `dtype` on `device` and its two optimisers."""
    p = copy.deepcopy(pol)
    if dtype is not None:
        p = p.to(dtype)
    if device is not None:
        p = p.to(device)
    return p, T.make_optimizers(p, cfg)


def compare(pa, oa, pb, ob, tol=TOL):
    """Every parameter of all six networks, every Adam moment and both step counts of learner a against learner b, with no element
    left out.  The critics' optimiser has taken n_updates steps, the actor's n_actor_updates."""
    assert pa.n_updates == pb.n_updates and pa.n_actor_updates == pb.n_actor_updates
    for net in T.NETS:
        for (n, x), (_, y) in zip(getattr(pa, net).named_parameters(), getattr(pb, net).named_parameters()):
            SC._close(f"{net}.{n}", x, y, *tol["param"])
    for key, steps in (("actor", pa.n_actor_updates), ("critic", pa.n_updates)):
        for ga, gb in zip(oa[key].param_groups, ob[key].param_groups):
            assert len(ga["params"]) == len(gb["params"])
            for x, y in zip(ga["params"], gb["params"]):
                sa, sb = oa[key].state.get(x), ob[key].state.get(y)
                if steps == 0:
                    for st in (sa, sb):
                        assert not st or (float(st["exp_avg"].abs().sum()) == 0.0 and float(st["exp_avg_sq"].abs().sum()) == 0.0)
                    continue
                assert float(sa["step"]) == float(sb["step"]) == steps
                SC._close(f"{key} exp_avg", sa["exp_avg"], sb["exp_avg"], *tol["exp_avg"])
                SC._close(f"{key} exp_avg_sq", sa["exp_avg_sq"], sb["exp_avg_sq"], *tol["exp_avg_sq"])


class Restated:
    """The TD3 gradient step from its formulas alone: plain tensors per network ([W1, b1, W2, b2, W3, b3] in torch's Linear layout),
    gradients from torch.autograd.grad, Adam written out, no nn.Module and no torch.optim."""

    def __init__(self, pol, lr, betas=(0.9, 0.999), eps=1e-8):
        self.p = {name: [q.detach().clone() for q in getattr(pol, name).parameters()] for name in T.NETS}
        self.m = {name: [torch.zeros_like(q) for q in self.p[name]] for name in T.TRAINED}
        self.v = {name: [torch.zeros_like(q) for q in self.p[name]] for name in T.TRAINED}
        self.lr, self.betas, self.eps = lr, betas, eps
        self.n_updates = self.n_actor_updates = 0

    @staticmethod
    def mlp(ps, x):
        w1, b1, w2, b2, w3, b3 = ps
        return torch.relu(torch.relu(x @ w1.t() + b1) @ w2.t() + b2) @ w3.t() + b3

    def adam(self, names, grads, t):
        b1, b2 = self.betas
        flat = [(n, k) for n in names for k in range(6)]
        for (n, k), g in zip(flat, grads):
            self.m[n][k] = b1 * self.m[n][k] + (1.0 - b1) * g
            self.v[n][k] = b2 * self.v[n][k] + (1.0 - b2) * g * g
            denom = self.v[n][k].sqrt() / (1.0 - b2 ** t) ** 0.5 + self.eps
            self.p[n][k] = self.p[n][k] - (self.lr / (1.0 - b1 ** t)) * self.m[n][k] / denom

    def step(self, rows, eps, cfg, with_actor, d, A):
        """Returns (critic loss, actor loss or None, the fraction of noise elements the smoothing clip held, the fraction of target
        action elements the action clamp held)."""
        B = rows.shape[0]
        s, a, r, s2, last = rows[:, :d], rows[:, d:d + A], rows[:, d + A], rows[:, d + A + 1:2 * d + A + 1], rows[:, 2 * d + A + 1]
        scaled = cfg.target_policy_noise * eps
        noise = torch.minimum(torch.maximum(scaled, torch.full_like(eps, -cfg.target_noise_clip)), torch.full_like(eps, cfg.target_noise_clip))
        raw = torch.tanh(self.mlp(self.p["actor_target"], s2)) + noise
        a2 = torch.minimum(torch.maximum(raw, -torch.ones_like(raw)), torch.ones_like(raw))
        x2 = torch.cat([s2, a2], 1)
        qt = torch.minimum(self.mlp(self.p["q1_target"], x2), self.mlp(self.p["q2_target"], x2))[:, 0]
        y = r + (1.0 - last) * cfg.gamma * qt
        crit = [q.clone().requires_grad_(True) for n in ("q1", "q2") for q in self.p[n]]
        x = torch.cat([s, a], 1)
        loss = ((self.mlp(crit[:6], x)[:, 0] - y) ** 2).sum() / B + ((self.mlp(crit[6:], x)[:, 0] - y) ** 2).sum() / B
        grads = torch.autograd.grad(loss, crit)
        self.n_updates += 1
        self.adam(("q1", "q2"), grads, self.n_updates)
        actor_loss = None
        if with_actor:
            act = [q.clone().requires_grad_(True) for q in self.p["actor"]]
            la = -self.mlp(self.p["q1"], torch.cat([s, torch.tanh(self.mlp(act, s))], 1)).sum() / B
            grads = torch.autograd.grad(la, act)
            self.n_actor_updates += 1
            self.adam(("actor",), grads, self.n_actor_updates)
            for n in T.TRAINED:
                self.p[n + "_target"] = [(1.0 - cfg.tau) * t + cfg.tau * q for t, q in zip(self.p[n + "_target"], self.p[n])]
            actor_loss = la.detach()
        return loss.detach(), actor_loss, float((scaled.abs() > cfg.target_noise_clip).float().mean()), float((raw.abs() > 1.0).float().mean())
