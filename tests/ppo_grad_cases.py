"""Shared pieces of the per-gradient tests of the PPO learner (tests/test_ppo_grad_cpu.py, tests/test_ppo_grad_gpu.py): the inputs, a
float64 restatement of ONE minibatch of SB3's ``PPO.train()`` and the read-back of the gradient a learner applied.

The handle.  ``PPO.train()`` over a buffer of exactly one minibatch (``T * n == batch_size``, ``n_epochs = 1``) with a fresh optimiser
takes one Adam step from zero moments: afterwards ``exp_avg == (1 - beta1) * clipc * g`` and ``exp_avg_sq == (1 - beta2) * (clipc * g)**2``
for every parameter tensor, so dividing by ``1 - beta`` in float64 gives back the clipped gradient the learner applied -- through the
product's own host path (FusedPpoUpdate.run / store_to_torch, the moment map, the transposes), with no entry point of its own.  With
``max_grad_norm = 1e30`` the clip factor is 1 and what comes back is the raw gradient.  ``1 - beta`` is taken as the path took it
(ONE_MINUS): the kernel forms ``1.0f - beta`` in float32 (0.100000024, 0.00099998713), torch.optim.Adam rounds the double ``1 - beta``
to float32 (0.1f, 0.001f); the two differ by 2.4e-7 and 1.3e-5 relative, which belongs to the moments and not to the gradient.

The inputs.  Observations, actions, returns as tests/mp_diag_jobs.py fills them (drawn on the CPU, whatever device the learner is on,
so the CPU reference and a learner on the GPU hold the same bits).  KINDS:

* ``mixed``, ``dead``, ``live``: the branch of the clipped surrogate is decided by construction.  ``old_logp = float32(logp64 - l)``
  with ``logp64`` the float64 log-prob of the restatement and ``l`` from {+0.5, -0.5, +0.05, -0.05}: ratios of about 1.65, 0.61, 1.05,
  0.95, each at least 0.05 from the edge of every clip range used (0.1, 0.2, 0.3) -- five orders of magnitude above the float32
  rounding of a log-prob.  The advantages carry their signs by hand (magnitudes in [0.5, 2]) and are not normalised.
  ``mixed``: the eight (sign of A) x (l) combinations in equal shares plus ZEROS samples with A == +0.0 / -0.0 exactly.
  ``dead``: A > 0 with l = +0.5 or A < 0 with l = -0.5 -- the surrogate passes no gradient.
  ``live``: A > 0 with l = -0.5 or A < 0 with l = +0.5 -- outside the range, the gradient still flows through ``A * ratio``.
* ``random``: the buffers of mp_diag_jobs.filled_ppo as they are, advantages normalised per minibatch.  Here float32 rounding decides
  the branch of a sample that sits on the edge of the range: ``band_count`` counts the samples with ``| |r64 - 1| - clip | <= 8 x`` the
  measured float32-against-float64 difference of the log-ratio (the bracket of tests/test_learner_diag_gpu.py), the CPU test requires
  that count to be 0 for the seeds used, and a seed that fails is replaced (SEEDS), never the cap.

Left out: the exact float32 tie ``ratio == 1 +- clip``.  The ratio is ``expf`` of a float32 difference; no input makes it land on the
float32 value of ``1 +- clip`` on every ``expf`` (libm, the device's), so a test of that tie would test the ``expf`` and not the branch.

The tolerance of the GPU tests comes from ``measure(case)``: the float32 torch path (``PPO._minibatch_step`` on the CPU) against the
restatement on the same case, per tensor -- E32.  The kernel may be K = 8 x E32 off (the factor of the lr = 0 diagnostics test) plus
FLOOR_EPS float32 epsilons of the tensor's largest gradient (the floor of tests/test_device_functions_gpu.py: a tensor whose torch
gradient happens to round to the float64 one has E32 = 0 and still owes the kernel its own rounding).
"""
import functools
import math

import numpy as np
import torch

import mp_diag_jobs as J

EPS32 = float(np.finfo(np.float32).eps)
K = 8.0
FLOOR_EPS = 4.0
KINDS = ("mixed", "dead", "live", "random")
L_VALUES = (0.5, -0.5, 0.05, -0.05)
ZEROS = 8                                  # samples of a mixed minibatch with A == 0.0 exactly (alternating +0.0 / -0.0)
BIG = 1e30                                 # max_grad_norm of the raw-gradient runs: the clip factor is exactly 1
# fill seed per (obs, actions, batch): the first of 5, 6, ... whose ``random`` buffers leave no sample in the band (replacements are
# recorded here as "shape: tried -> taken"); shapes not listed take 5
SEEDS = {}

# the hyper-parameter runs: (kind, PPOConfig fields).  ``mixed`` keeps every ratio clear of all three clip ranges, so there the clip
# range must NOT reach the gradient; on ``random`` it does (the band precondition is checked for 0.1 and 0.3 as well)
HYPER = ([("mixed", dict(clip_range=v)) for v in (0.1, 0.3)] + [("random", dict(clip_range=v)) for v in (0.1, 0.3)]
         + [("mixed", dict(vf_coef=v)) for v in (0.25, 1.0)] + [("mixed", dict(ent_coef=v)) for v in (0.0, 0.05)]
         + [("mixed", dict(normalize_advantage=False)), ("mixed", dict(normalize_advantage=True, adv_norm_scope="minibatch")),
            ("mixed", dict(normalize_advantage=True, adv_norm_scope="global"))])
HYPER_IDS = [k + "-" + "-".join(f"{n}={v}" for n, v in h.items()) for k, h in HYPER]
HYPER_SHAPES = [(28, 4, 128), (21, 6, 64)]

_B1, _B2 = np.float32(0.9), np.float32(0.999)
ONE_MINUS = {"kernel": (float(np.float32(1.0) - _B1), float(np.float32(1.0) - _B2)),
             "torch": (float(np.float32(1.0 - 0.9)), float(np.float32(1.0 - 0.999)))}


def restated(p, obs, act, old, adv, ret, clip_range=0.2, vf_coef=0.5, ent_coef=0.01, norm="minibatch", mean=0.0, std=1.0):
    """One SB3 minibatch in float64 on the CPU from the formulas alone.  ``p``: name -> float64 tensor in torch's Linear layout;
    ``norm``: "off", "minibatch" (unbiased std, + 1e-8) or "given" (``mean`` / ``std``, + 1e-8).  Returns dict(grads, norm, log_ratio,
    logp, adv_used, losses)."""
    q = {n: t.detach().clone().requires_grad_(True) for n, t in p.items()}
    h = torch.tanh(torch.tanh(obs @ q["pi_net.0.weight"].t() + q["pi_net.0.bias"]) @ q["pi_net.2.weight"].t() + q["pi_net.2.bias"])
    mu = h @ q["action_net.weight"].t() + q["action_net.bias"]
    g = torch.tanh(torch.tanh(obs @ q["vf_net.0.weight"].t() + q["vf_net.0.bias"]) @ q["vf_net.2.weight"].t() + q["vf_net.2.bias"])
    value = (g @ q["value_net.weight"].t() + q["value_net.bias"])[:, 0]
    ls = q["log_std"]
    logp = (-((act - mu) ** 2) / (2.0 * torch.exp(2.0 * ls)) - ls - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    if norm == "minibatch":
        a = (adv - adv.mean()) / (adv.std() + 1e-8)
    elif norm == "given":
        a = (adv - mean) / (std + 1e-8)
    else:
        assert norm == "off", norm
        a = adv
    log_ratio = logp - old
    ratio = torch.exp(log_ratio)
    policy_loss = -torch.min(a * ratio, a * ratio.clamp(1.0 - clip_range, 1.0 + clip_range)).mean()
    value_loss = ((ret - value) ** 2).mean()
    entropy_loss = -(0.5 + 0.5 * math.log(2.0 * math.pi) + ls).sum()
    names = list(q)
    grads = torch.autograd.grad(policy_loss + ent_coef * entropy_loss + vf_coef * value_loss, [q[n] for n in names], allow_unused=True)
    grads = {n: (torch.zeros_like(q[n]) if gr is None else gr).detach() for n, gr in zip(names, grads)}
    total = math.sqrt(sum(float((gr * gr).sum()) for gr in grads.values()))
    return dict(grads=grads, norm=total, log_ratio=log_ratio.detach(), logp=logp.detach(), adv_used=a.detach(),
                losses=(float(policy_loss.detach()), float(value_loss.detach()), float(entropy_loss.detach())))


def _params64(policy):
    return {n: q.detach().double().cpu().clone() for n, q in policy.named_parameters()}


class Case:
    """The buffers of one minibatch (float32, CPU) and the initial policy they were filled from."""

    def __init__(self, d, a, bs, kind, seed=None):
        assert kind in KINDS, kind
        self.d, self.a, self.bs, self.kind = d, a, bs, kind
        self.seed = SEEDS.get((d, a, bs), 5) if seed is None else seed
        ppo = J.filled_ppo(d, a, bs, 1, T=1, n=bs, seed=self.seed, device="cpu", fused_update=False)
        self.obs, self.act = ppo.buf_obs.reshape(bs, d).clone(), ppo.buf_act.reshape(bs, a).clone()
        self.old, self.adv, self.ret = ppo.buf_logp.reshape(bs).clone(), ppo.adv.reshape(bs).clone(), ppo.ret.reshape(bs).clone()
        self.p64 = _params64(ppo.policy)
        self.l = None
        if kind != "random":
            g = torch.Generator(); g.manual_seed(1000 + self.seed)
            mag = 0.5 + 1.5 * torch.rand(bs, generator=g)
            i = torch.arange(bs)
            if kind == "mixed":
                zeros = (torch.arange(ZEROS) * (bs // ZEROS) + (bs // ZEROS) // 2)       # spread over the buffer (every block of a cut)
                live = torch.ones(bs, dtype=torch.bool); live[zeros] = False
                combo = torch.zeros(bs, dtype=torch.long)
                combo[live] = torch.arange(bs - ZEROS) % 8                               # (bs - ZEROS) / 8 samples of each combination
                sign = torch.where(combo < 4, 1.0, -1.0)
                l = torch.tensor(L_VALUES, dtype=torch.float64)[combo % 4]
                mag[zeros] = 0.0
                sign[zeros] = torch.tensor([1.0, -1.0]).repeat(ZEROS // 2)               # +0.0 and -0.0 in turn
                self.zeros, self.combo = zeros, combo
            else:
                sign = torch.where(i % 2 == 0, 1.0, -1.0)
                l = sign.double() * (0.5 if kind == "dead" else -0.5)
            self.adv = (sign * mag).float()                     # (the zeros: +0.0 and -0.0 in turn)
            logp64 = restated(self.p64, self.obs.double(), self.act.double(), torch.zeros(bs, dtype=torch.float64),
                              self.adv.double(), self.ret.double(), norm="off")["logp"]
            self.old = (logp64 - l).float()
            self.l = l
        self.norm = "minibatch" if kind == "random" else "off"

    def cfg(self, **over):
        """PPOConfig fields of the case: one minibatch, one epoch, the raw gradient unless ``max_grad_norm`` says otherwise."""
        kw = dict(max_grad_norm=BIG, normalize_advantage=self.norm != "off")
        kw.update(over)
        return kw

    def make(self, device="cpu", **over):
        """A learner holding the case: the torch path on the CPU, the fused kernels on the GPU."""
        fused = torch.device(device).type == "cuda"
        ppo = J.filled_ppo(self.d, self.a, self.bs, 1, T=1, n=self.bs, seed=self.seed, device=device, fused_update=fused,
                           fused_six_actions=True, fused_three_actions=True, **self.cfg(**over))
        bs = self.bs
        ppo.buf_obs.copy_(self.obs.reshape(1, bs, -1)); ppo.buf_act.copy_(self.act.reshape(1, bs, -1)); ppo.buf_logp.copy_(self.old.reshape(1, bs))
        ppo.adv, ppo.ret = self.adv.reshape(1, bs).to(ppo.device), self.ret.reshape(1, bs).to(ppo.device)
        ppo.buf_val.copy_(ppo.ret - ppo.adv)
        for (n, q), w in zip(ppo.policy.named_parameters(), self.p64.values()):
            assert torch.equal(q.detach().cpu().double(), w), n          # the module is built on the CPU under the seed: the same bits everywhere
        return ppo

    def reference(self, **over):
        """The restatement on this case under the hyper-parameters ``make(**over)`` would run."""
        from pyflyt_drone_amd import rollout as R
        kw = dict(ent_coef=0.01)                                # (the default of mp_diag_jobs.filled_ppo)
        kw.update(self.cfg(**over))
        c = R.PPOConfig(**kw)
        norm, mean, std = "off", 0.0, 1.0
        if c.normalize_advantage:
            norm = "given" if c.adv_norm_scope == "global" else "minibatch"
            # the statistics of the whole buffer, exact: what train() hands to either learner is their float32 rounding, which
            # counts as that learner's error (the torch path's is part of E32)
            mean, std = float(self.adv.double().mean()), float(self.adv.double().std())
        return restated(self.p64, self.obs.double(), self.act.double(), self.old.double(), self.adv.double(), self.ret.double(),
                        clip_range=c.clip_range, vf_coef=c.vf_coef, ent_coef=c.ent_coef, norm=norm, mean=mean, std=std)

    def band_count(self, clip_range=0.2):
        """(samples where float32 rounding may decide the branch, the measured log-ratio difference): see the module docstring."""
        ppo = self.make()
        with torch.no_grad():
            _, lp32, _ = ppo.policy.evaluate_actions(self.obs, self.act)
        lr64 = self.reference()["log_ratio"]
        measured = float(((lp32 - self.old).double() - lr64).abs().max())
        dist = (torch.exp(lr64) - 1.0).abs()
        return int(((dist - clip_range).abs() <= 8.0 * measured).sum()), measured


@functools.lru_cache(maxsize=None)
def case(d, a, bs, kind):
    return Case(d, a, bs, kind)


def recovered(ppo, path):
    """name -> (gradient from exp_avg, gradient squared from exp_avg_sq) in float64 on the CPU, and the optimiser's step count."""
    o1, o2 = ONE_MINUS[path]
    out, steps = {}, set()
    for n, q in ppo.policy.named_parameters():
        st = ppo.optimizer.state[q]
        out[n] = (st["exp_avg"].detach().double().cpu() / o1, st["exp_avg_sq"].detach().double().cpu() / o2)
        steps.add(float(st["step"]))
    assert len(steps) == 1
    return out, steps.pop()


def torch_total_norm(grads32):
    """The total of ``clip_grad_norm_`` over float32 gradients, as the torch path forms it."""
    ts = []
    for gr in grads32:
        t = torch.zeros_like(gr, requires_grad=True)
        t.grad = gr.clone()
        ts.append(t)
    return float(torch.nn.utils.clip_grad_norm_(ts, BIG))


_HASH = lambda kw: tuple(sorted(kw.items()))      # noqa: E731


@functools.lru_cache(maxsize=None)
def _measure(d, a, bs, kind, over):
    c = case(d, a, bs, kind)
    over = dict(over)
    ref = c.reference(**over)
    ppo = c.make("cpu", **over)
    ppo.train()
    got, step = recovered(ppo, "torch")
    assert step == 1.0
    e32, scale, grads32 = {}, {}, []
    for n, q in ppo.policy.named_parameters():
        e32[n] = float((got[n][0] - ref["grads"][n]).abs().max())
        scale[n] = float(ref["grads"][n].abs().max())
        grads32.append(q.grad.detach().clone())
    n32 = torch_total_norm(grads32)
    return dict(ref=ref, e32=e32, scale=scale, got=got, grads32=grads32, norm32=n32,
                norm_err=abs(n32 - ref["norm"]) / ref["norm"] if ref["norm"] > 0 else 0.0)


def measure(d, a, bs, kind, **over):
    """The float32 torch path against the restatement on one case (one CPU ``train()``, cached): E32 and the largest |g64| per tensor,
    the torch path's recovered gradients and its ``clip_grad_norm_`` total with its relative error against the restated norm."""
    return _measure(d, a, bs, kind, _HASH(over))


def tolerance(m, name):
    return K * m["e32"][name] + FLOOR_EPS * EPS32 * m["scale"][name]
