"""Soft actor-critic for the low-level control task (the reference's ``examples/lowlevel.py``: SB3 ``SAC("MlpPolicy")`` with
``net_arch=[256, 256]``, a 200 000-row buffer, batches of 256, ``gamma=0.99``, ``tau=0.02``, one gradient step per env step, an
automatic entropy coefficient and no ``VecNormalize``).

Everything between two env steps runs on the device (csrc/fwsim_sac.hpp, include/fwsim.h; the replay ring is :mod:`.replay`, importable from here):

* ``fw_sac_act``       the actor on the env's observations, the squashed-Gaussian sample (or SB3's uniform ``learning_starts``
                       actions), the fp32 staging copy of the observation the step is about to overwrite;
* ``fw_sac_noise``     the two noise blocks of a gradient step;
* ``fw_sac_update``    one gradient step of SB3's ``SAC.train()`` on a flat image of all five networks and their Adam moments;
* ``fw_sac_update_weighted``  (``SACConfig.prioritized`` only) the same step with the importance weights on the critic loss; it
                       reports the per-row TD errors the new priorities are made of.

:func:`sac_update_torch` is the same gradient step in plain torch (CPU tensors too): the reference the kernels are tested against
and the ``fused_update=False`` path.

Two departures from SB3, both only visible away from the reference's settings: the Polyak step is taken when the *total* number of
gradient steps is a multiple of ``target_update_interval`` (SB3 counts inside one ``train()`` call), and a vec-step is a warm-up step
-- uniform actions, no gradient step -- exactly while ``num_timesteps < learning_starts`` (SB3 starts training one vec-step later
when ``learning_starts`` is not a multiple of the env count).
"""
from __future__ import annotations

import ctypes as C
import math
import time
from dataclasses import dataclass, asdict
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _lib
from .replay import (  # noqa: F401  (the ring's names stay importable from here)
    CTR_CURSOR, CTR_GRAD, CTR_SIZE, CTR_STEPS, END_TERMINATED, END_TRUNCATED, HER_OBS_DIM, HER_ROW_FLOATS, HER_TAG, MAX_HER_HORIZON, MAX_N_STEPS, PER_GROUP,
    PER_MAX, PER_MAX_CAPACITY, PER_MIN, PER_TOTAL, HerTask, ReplayBufferDevice, _p, _stream, _walk, check_sampler_options, her_achieved_goal,
    her_reward_reference, her_rows_reference, her_task_of, normalize_obs_reference, normalize_rows_reference, nstep_rows_reference, per_beta_reference,
    per_draw_reference, per_group_sums, per_sums_reference, per_update_reference, per_weights_reference, ring_capacity, row_floats, running_moments_reference,
    split_rows, stats_step_reference)

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
MAX_OBS_DIM, MAX_ACT_DIM, HIDDEN_WIDTHS, MAX_BATCH = 64, 8, (64, 256), 512
MAX_BATCH_WIDE, WIDE_BATCH_MULTIPLE = 8192, 64                  # above MAX_BATCH: the wide form of the gradient step


@dataclass
class SACConfig:
    """The reference's hyper-parameters (examples/lowlevel.py) as defaults."""
    learning_rate: float = 3e-4
    buffer_size: int = 200_000
    batch_size: int = 256
    gamma: float = 0.99
    tau: float = 0.02
    gradient_steps: int = 1              # per vec-step; -1: one per env (update-to-data 1, SB3's meaning)
    target_update_interval: int = 1
    learning_starts: int = 100
    ent_coef: object = "auto"            # or a fixed float
    net_arch: Tuple[int, int] = (256, 256)
    seed: int = 0
    use_graphs: bool = True
    fused_update: bool = True
    episode_stats: bool = False          # SB3's rollout/* figures: SAC.rollout_stats (monitor.EpisodeMonitor folded behind every env step,
                                         # one more launch per vec-step, inside the captured graphs); off: nothing changes
    stats_window_size: int = 100         #     SB3's stats_window_size: episodes in the window
    episode_fold: str = "one"            #     the fold's device form: "one", "wide" or "auto" (monitor.EpisodeMonitor)
    n_steps: int = 1                     # n-step returns from the ring (1 ... 16); 1: the 1-step target, nothing changes
    her_goals: int = 0                   # hindsight goal relabelling, SB3's n_sampled_goal: a sampled row is relabelled with probability
                                         # her_goals / (her_goals + 1); 0: off, nothing changes.  Not built together with n_steps > 1
    her_horizon: int = 64                #     the relabelled goal comes from at most her_horizon - 1 steps ahead (1 ... 64)
    prioritized: bool = False            # prioritized replay (Schaul et al. 2016, proportional); off: nothing changes.  Not built together
                                         # with n_steps > 1 or her_goals > 0
    per_alpha: float = 0.6               #     a row's priority is (|td| + per_eps)^per_alpha, in [0, 1]; 0: uniform over the filled rows
    per_beta: float = 0.4                #     exponent of the importance weights, in [0, 1]; 0: no correction
    per_beta_steps: int = 0              #     > 0: the exponent grows linearly from per_beta to 1 over this many gradient steps
    per_eps: float = 1e-6
    normalize_obs: bool = False          # SB3's VecNormalize(norm_obs) in front of an off-policy learner: running statistics of the env's
                                         # observations; the ring keeps raw rows, the actor and every sampled batch read normalised ones.
                                         # Off (both flags): nothing changes
    normalize_reward: bool = False       #     VecNormalize(norm_reward): a sampled reward is divided by the std of the discounted return
    clip_obs: float = 10.0               #     a normalised observation is clipped to +-clip_obs ...
    clip_reward: float = 10.0            #     ... and a normalised reward to +-clip_reward
    norm_epsilon: float = 1e-8           #     added to a variance under the square root

    def __post_init__(self):
        self.normalize_obs, self.normalize_reward = bool(self.normalize_obs), bool(self.normalize_reward)
        for name in ("clip_obs", "clip_reward", "norm_epsilon"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(float(v)) and float(v) > 0.0):
                raise ValueError(f"{name} must be a positive finite number, got {v!r}")
            setattr(self, name, float(v))
        (self.n_steps, self.her_goals, self.her_horizon, self.prioritized, self.per_alpha, self.per_beta, self.per_beta_steps,
         self.per_eps) = check_sampler_options(self.n_steps, self.her_goals, self.her_horizon, self.prioritized, self.per_alpha, self.per_beta,
                                               self.per_beta_steps, self.per_eps)
        if self.episode_fold not in ("one", "wide", "auto"):
            raise ValueError(f"episode_fold must be 'one', 'wide' or 'auto', got {self.episode_fold!r}")
        if int(self.stats_window_size) <= 0:
            raise ValueError("stats_window_size must be positive")
        self.net_arch = tuple(int(h) for h in self.net_arch)
        if len(self.net_arch) != 2 or self.net_arch[0] != self.net_arch[1] or self.net_arch[0] <= 0:
            raise ValueError(f"net_arch must be two equal positive widths, got {self.net_arch}")
        if self.gradient_steps != -1 and self.gradient_steps < 0:
            raise ValueError("gradient_steps must be non-negative, or -1 for one per env")
        if self.batch_size <= 0 or self.buffer_size <= 0 or self.target_update_interval <= 0 or self.learning_starts < 0:
            raise ValueError("batch_size, buffer_size and target_update_interval must be positive, learning_starts non-negative")
        if not (0.0 <= self.gamma <= 1.0 and 0.0 < self.tau <= 1.0 and self.learning_rate > 0.0):
            raise ValueError("gamma must be in [0, 1], tau in (0, 1] and learning_rate positive")
        if self.ent_coef != "auto":
            self.ent_coef = float(self.ent_coef)
            if self.ent_coef < 0.0:
                raise ValueError("a fixed ent_coef must be non-negative")

    @property
    def hidden(self) -> int:
        return self.net_arch[0]

    @property
    def auto_ent(self) -> bool:
        return self.ent_coef == "auto"

    @property
    def her_relabel_prob(self) -> float:
        """SB3's ``her_ratio``: ``1 - 1 / (n_sampled_goal + 1)``."""
        return self.her_goals / (self.her_goals + 1.0)

    @property
    def normalizes(self) -> bool:
        return self.normalize_obs or self.normalize_reward

    def resolved_gradient_steps(self, num_envs: int) -> int:
        return int(num_envs) if self.gradient_steps == -1 else int(self.gradient_steps)


def fits(obs_dim: int, act_dim: int, hidden: int, batch_size: int) -> bool:
    """What the kernels are built for (include/fwsim.h): anything else is ``FW_EUNSUPPORTED``.  Batches: multiples of 16 in
    [16, ``MAX_BATCH``], or multiples of ``WIDE_BATCH_MULTIPLE`` in (``MAX_BATCH``, ``MAX_BATCH_WIDE``] (the wide form)."""
    batch_ok = ((16 <= batch_size <= MAX_BATCH and batch_size % 16 == 0)
                or (MAX_BATCH < batch_size <= MAX_BATCH_WIDE and batch_size % WIDE_BATCH_MULTIPLE == 0))
    return 1 <= obs_dim <= MAX_OBS_DIM and 1 <= act_dim <= MAX_ACT_DIM and hidden in HIDDEN_WIDTHS and batch_ok


# ---------------------------------------------------------------------------------------------
# the torch modules
# ---------------------------------------------------------------------------------------------
def _mlp(n_in: int, hidden: int, n_out: int) -> nn.Sequential:
    return nn.Sequential(nn.Linear(n_in, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, n_out))


class SacPolicy(nn.Module):
    """Actor ``d -> H -> H -> 2A`` (mean | log_std, clamped to [-20, 2]), two critics ``(d + A) -> H -> H -> 1`` on
    ``cat(obs, action)`` and their targets (copies at construction), ``log_ent_coef`` (log 1.0): ReLU MLPs, torch's default
    initialisation."""

    def __init__(self, obs_dim: int, act_dim: int, hidden: int = 256):
        super().__init__()
        self.obs_dim, self.act_dim, self.hidden = int(obs_dim), int(act_dim), int(hidden)
        self.actor = _mlp(obs_dim, hidden, 2 * act_dim)
        self.q1, self.q2 = _mlp(obs_dim + act_dim, hidden, 1), _mlp(obs_dim + act_dim, hidden, 1)
        self.q1_target, self.q2_target = _mlp(obs_dim + act_dim, hidden, 1), _mlp(obs_dim + act_dim, hidden, 1)
        self.q1_target.load_state_dict(self.q1.state_dict()); self.q2_target.load_state_dict(self.q2.state_dict())
        for q in list(self.q1_target.parameters()) + list(self.q2_target.parameters()):
            q.requires_grad_(False)
        self.log_ent_coef = nn.Parameter(torch.zeros(()))
        self.n_updates = 0               # gradient steps taken (the Polyak schedule counts them)

    def dist(self, obs):
        out = self.actor(obs)
        return out[..., :self.act_dim], out[..., self.act_dim:].clamp(LOG_STD_MIN, LOG_STD_MAX)

    def sample(self, obs, eps):
        """a = tanh(mean + exp(log_std) eps) and its log-probability."""
        mean, log_std = self.dist(obs)
        a = torch.tanh(mean + torch.exp(log_std) * eps)
        logp = (-0.5 * eps * eps - log_std - 0.5 * math.log(2.0 * math.pi)).sum(-1) - torch.log(1.0 - a * a + 1e-6).sum(-1)
        return a, logp

    def q_min(self, obs, act, target: bool = False):
        x = torch.cat([obs, act], dim=-1)
        q1, q2 = (self.q1_target, self.q2_target) if target else (self.q1, self.q2)
        return torch.min(torch.cat([q1(x), q2(x)], dim=-1), dim=-1).values

    def forward(self, obs, deterministic: bool = False, generator=None):
        """``(actions, values, log_prob)`` like :class:`~.rollout.MlpPolicy`: values are min(Q1, Q2)(obs, action)."""
        p = self.actor[0].weight
        obs = obs.to(dtype=p.dtype)
        mean, _ = self.dist(obs)
        eps = (torch.zeros_like(mean) if deterministic
               else torch.randn(mean.shape, device=mean.device, dtype=mean.dtype, generator=generator))
        a, logp = self.sample(obs, eps)
        return a, self.q_min(obs, a), logp


def make_optimizers(policy: SacPolicy, cfg: SACConfig, capturable: bool = False) -> Dict[str, Optional[torch.optim.Adam]]:
    """SB3's three optimisers: Adam(eps 1e-8, betas (0.9, 0.999)) for the actor, for both critics together and for log_ent_coef."""
    kw = dict(lr=cfg.learning_rate, eps=1e-8, betas=(0.9, 0.999), capturable=capturable)
    return {"actor": torch.optim.Adam(policy.actor.parameters(), **kw),
            "critic": torch.optim.Adam(list(policy.q1.parameters()) + list(policy.q2.parameters()), **kw),
            "ent": torch.optim.Adam([policy.log_ent_coef], **kw) if cfg.auto_ent else None}


def sac_update_torch(policy: SacPolicy, optimizers, batch, eps, eps_next, cfg: SACConfig, weights=None) -> Dict[str, torch.Tensor]:
    """One gradient step of SB3's ``SAC.train()`` in the order DESIGN.md section 4c spells out (the numbers at the right).  ``batch``: ``(s, a, r, s', done)`` or
    rows ``[B, 2d + A + 2]``; ``eps`` / ``eps_next``: N(0, 1) of shape ``[B, A]``.  Returns the five scalars ``fw_sac_update``
    reports (tensors, no host read) and ``"td"`` [B], the rows' ``(|Q1 - y| + |Q2 - y|) / 2``.  ``weights`` [B] (prioritized replay's
    importance weights, ``fw_sac_update_weighted``): the critics train on ``mean(w (Q_i - y)^2) / 2``; the actor and entropy losses
    are not weighted and the critic loss reported stays the unweighted one."""
    if torch.is_tensor(batch):
        batch = split_rows(batch, policy.obs_dim, policy.act_dim)
    s, a, r, s2, done = batch
    a_pi, logp = policy.sample(s, eps)                                                          # 1, 2
    if cfg.auto_ent:
        alpha = torch.exp(policy.log_ent_coef.detach())                                        # 3: the value before this step
        ent_loss = -(policy.log_ent_coef * (logp.detach() + float(-policy.act_dim))).mean()    # 4
        optimizers["ent"].zero_grad(set_to_none=True); ent_loss.backward(); optimizers["ent"].step()
    else:
        alpha = torch.as_tensor(float(cfg.ent_coef), dtype=s.dtype, device=s.device)
        ent_loss = torch.zeros((), dtype=s.dtype, device=s.device)
    with torch.no_grad():
        a2, logp2 = policy.sample(s2, eps_next)                                                # 5
        y = r + (1.0 - done) * cfg.gamma * (policy.q_min(s2, a2, target=True) - alpha * logp2)   # 6
    x = torch.cat([s, a], dim=-1)
    q1, q2 = policy.q1(x).squeeze(-1), policy.q2(x).squeeze(-1)
    critic_loss = 0.5 * (((q1 - y) ** 2).mean() + ((q2 - y) ** 2).mean())                       # 7
    trained = critic_loss if weights is None else 0.5 * ((weights * (q1 - y) ** 2).mean() + (weights * (q2 - y) ** 2).mean())
    td = 0.5 * ((q1 - y).abs() + (q2 - y).abs()).detach()
    optimizers["critic"].zero_grad(set_to_none=True); trained.backward(); optimizers["critic"].step()
    actor_loss = (alpha * logp - policy.q_min(s, a_pi)).mean()                                 # 8: the critics after their step
    optimizers["actor"].zero_grad(set_to_none=True); actor_loss.backward(); optimizers["actor"].step()
    optimizers["critic"].zero_grad(set_to_none=True)      # (the actor loss left gradients in the critics: they are not theirs)
    policy.n_updates += 1
    if policy.n_updates % cfg.target_update_interval == 0:                                      # 9
        with torch.no_grad():
            for net, tgt in ((policy.q1, policy.q1_target), (policy.q2, policy.q2_target)):
                for p, t in zip(net.parameters(), tgt.parameters()):
                    t.mul_(1.0 - cfg.tau).add_(p, alpha=cfg.tau)
    return {"critic_loss": critic_loss.detach(), "actor_loss": actor_loss.detach(), "ent_coef_loss": ent_loss.detach(),
            "ent_coef": alpha.detach(), "mean_logp": logp.detach().mean(), "td": td}


SCALARS = ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef", "mean_logp")


# ---------------------------------------------------------------------------------------------
# the flat image of fw_sac_update
# ---------------------------------------------------------------------------------------------
class _SacHyper(C.Structure):
    _fields_ = [("lr", C.c_float), ("gamma", C.c_float), ("tau", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("target_entropy", C.c_float), ("ent_coef", C.c_float), ("auto_ent", C.c_int32),
                ("target_update_interval", C.c_int32), ("seed", C.c_uint64)]


def net_floats(n_in: int, hidden: int, n_out: int) -> int:
    return n_in * hidden + hidden + hidden * hidden + hidden + hidden * n_out + n_out


def image_layout(obs_dim: int, act_dim: int, hidden: int) -> Dict[str, int]:
    """Offsets (floats) of the blocks of the flat image (include/fwsim.h)."""
    na, nc = net_floats(obs_dim, hidden, 2 * act_dim), net_floats(obs_dim + act_dim, hidden, 1)
    L = {"actor": 0, "q1": na, "q2": na + nc, "log_ent_coef": na + 2 * nc}
    L["q1_target"] = L["log_ent_coef"] + 1
    L["q2_target"] = L["q1_target"] + nc
    L["params"] = L["q2_target"] + nc
    L["trained"] = L["log_ent_coef"] + 1
    L["exp_avg"], L["exp_avg_sq"] = L["params"], L["params"] + L["trained"]
    L["tail"] = L["params"] + 2 * L["trained"]
    L["total"] = L["tail"] + 4
    return L


class FusedSacUpdate:
    """Host side of ``fw_sac_update``: the flat float32 image of the five networks, ``log_ent_coef``, the Adam moments and the step
    count, and its pack / unpack against the modules and the three optimisers (CPU tensors too).  The image is a cache of them,
    guarded by the tensors' version counters as :class:`~.rollout.FusedPpoUpdate` does."""

    def __init__(self, policy: SacPolicy, optimizers, cfg: SACConfig):
        self.policy, self.opts, self.cfg = policy, optimizers, cfg
        self.d, self.A, self.H = policy.obs_dim, policy.act_dim, policy.hidden
        self.L = image_layout(self.d, self.A, self.H)
        dev = policy.log_ent_coef.device
        self.image = torch.zeros(self.L["total"], dtype=torch.float32, device=dev)
        self.out = torch.zeros(8, dtype=torch.float32, device=dev)
        self._ws = None
        self._sig = None
        self.ahead = 0                   # gradient steps the image has taken since it was last equal to modules and optimisers

    def _slots(self):
        """(tensor, offset in the image, needs transpose, optimiser or None) per parameter, in layout order."""
        p, out = self.policy, []
        for name, net, opt in (("actor", p.actor, self.opts["actor"]), ("q1", p.q1, self.opts["critic"]), ("q2", p.q2, self.opts["critic"]),
                               ("q1_target", p.q1_target, None), ("q2_target", p.q2_target, None)):
            off = self.L[name]
            for lin in (net[0], net[2], net[4]):
                out.append((lin.weight, off, True, opt)); off += lin.weight.numel()
                out.append((lin.bias, off, False, opt)); off += lin.bias.numel()
        out.append((p.log_ent_coef, self.L["log_ent_coef"], False, self.opts.get("ent")))
        return out

    def signature(self):
        sig = [self.policy.n_updates]
        for t, _, _, opt in self._slots():
            sig.append((t.data_ptr(), t._version))
            st = opt.state.get(t) if opt is not None else None
            if st:
                sig += [(st[k].data_ptr(), st[k]._version) if torch.is_tensor(st[k]) else (k, st[k]) for k in ("exp_avg", "exp_avg_sq", "step")]
        return tuple(sig)

    def current(self) -> bool:
        return self._sig is not None and self._sig == self.signature()

    @torch.no_grad()
    def pack(self) -> None:
        """Modules and optimisers -> image."""
        img, L = self.image, self.L
        img.zero_()
        for t, off, tr, opt in self._slots():
            n = t.numel()
            img[off:off + n].copy_((t.t() if tr else t).reshape(-1))
            st = opt.state.get(t) if opt is not None else None
            if st:
                for key in ("exp_avg", "exp_avg_sq"):
                    img[L[key] + off:L[key] + off + n].copy_((st[key].t() if tr else st[key]).reshape(-1))
        img[L["tail"]:].view(torch.int32)[0] = int(self.policy.n_updates)
        self._sig, self.ahead = self.signature(), 0

    @torch.no_grad()
    def unpack(self, n_updates: Optional[int] = None) -> None:
        """Image -> modules and optimisers.  ``n_updates``: the step count when the caller already knows it (no host read)."""
        img, L = self.image, self.L
        step = int(img[L["tail"]:].view(torch.int32)[0].item()) if n_updates is None else int(n_updates)
        for t, off, tr, opt in self._slots():
            n = t.numel()
            shape = (t.shape[1], t.shape[0]) if tr else t.shape

            def get(base):
                v = img[base + off:base + off + n].view(shape)
                return v.t() if tr else v
            t.data.copy_(get(0))
            if opt is None or (step == 0 and not opt.state.get(t)):
                continue
            st = opt.state[t]
            if not st:
                cap = bool(opt.param_groups[0].get("capturable", False))
                st["step"] = torch.zeros((), dtype=torch.float32, device=t.device if cap else "cpu")
                st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(t), torch.zeros_like(t)
            st["exp_avg"].copy_(get(L["exp_avg"])); st["exp_avg_sq"].copy_(get(L["exp_avg_sq"]))
            if torch.is_tensor(st["step"]):
                st["step"].fill_(float(step))
            else:
                st["step"] = step
        self.policy.n_updates = step
        self._sig, self.ahead = self.signature(), 0

    def hyper(self) -> _SacHyper:
        pg = self.opts["actor"].param_groups[0]
        cfg = self.cfg
        return _SacHyper(lr=pg["lr"], gamma=cfg.gamma, tau=cfg.tau, beta1=pg["betas"][0], beta2=pg["betas"][1], eps=pg["eps"],
                         target_entropy=float(-self.A), ent_coef=0.0 if cfg.auto_ent else float(cfg.ent_coef),
                         auto_ent=int(cfg.auto_ent), target_update_interval=cfg.target_update_interval, seed=int(cfg.seed) & (2**64 - 1))

    def workspace(self, batch: int) -> torch.Tensor:
        need = int(_lib.lib().fw_sac_update_workspace_bytes(self.d, self.A, self.H, batch))
        if need < 0:
            _lib.check(need)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.zeros(need, dtype=torch.uint8, device=self.image.device)
        return self._ws

    def run(self, rows: torch.Tensor, counters: torch.Tensor, weights: Optional[torch.Tensor] = None,
            td_out: Optional[torch.Tensor] = None) -> None:
        """One gradient step on the image (the caller packs before, counts the step in ``ahead`` and unpacks when the modules are
        wanted; nothing here reads the device).  With ``weights`` [B] it is ``fw_sac_update_weighted``: the critic loss is weighted
        row by row and ``td_out`` [B] (optional) receives the rows' TD errors."""
        assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.shape[1] == row_floats(self.d, self.A)
        B = rows.shape[0]
        ws = self.workspace(B) if fits(self.d, self.A, self.H, B) else self.out          # (an unsupported shape: let the ABI say so)
        H = self.hyper()
        args = (_p(self.image), _p(rows), self.d, self.A, self.H, B, C.byref(H), _p(counters), _p(self.out), _p(ws), ws.numel())
        if weights is not None:
            assert weights.dtype == torch.float32 and weights.is_contiguous() and weights.numel() == B
            assert td_out is None or (td_out.dtype == torch.float32 and td_out.is_contiguous() and td_out.numel() == B)
            _lib.check(_lib.lib().fw_sac_update_weighted(*args, _p(weights), _p(td_out), _stream(rows.device)))
        elif td_out is not None:
            raise ValueError("td_out is written by the weighted step: pass weights (ones for an unweighted one)")
        else:
            _lib.check(_lib.lib().fw_sac_update(*args, _stream(rows.device)))

    def scalars(self) -> Dict[str, float]:
        return dict(zip(SCALARS, self.out[:5].tolist()))


def sac_noise(seed: int, counters: torch.Tensor, batch: int, act_dim: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """eps and eps' ``[2, B, A]`` of the gradient step ``counters[3]`` (``fw_sac_noise``): the values ``fw_sac_update`` draws inside."""
    if out is None:
        out = torch.empty((2, batch, act_dim), dtype=torch.float32, device=counters.device)
    _lib.check(_lib.lib().fw_sac_noise(int(seed) & (2**64 - 1), _p(counters), batch, act_dim, _p(out), _stream(counters.device)))
    return out


# ---------------------------------------------------------------------------------------------
# the learner
# ---------------------------------------------------------------------------------------------
ACT_STOCHASTIC, ACT_DETERMINISTIC, ACT_WARMUP = 0, 1, 2


class SAC:
    """SAC on a bare device env (``FixedwingLowLevelVecEnv``; the reference uses no normaliser).  A vec-step is act -> ``env.step_tensor``
    -> store -> G x (sample -> update); with ``use_graphs`` and the fused update it is one captured graph, with a second one for the
    warm-up steps (with the torch update the graph ends behind the store and the gradient steps run eagerly).

    ``SACConfig.normalize_obs`` / ``normalize_reward``: SB3's ``VecNormalize`` with an off-policy buffer.  ``normalizer`` (a
    :class:`~.rollout.VecNormalizeDevice` over the train env, used as the holder of the statistics only: the learner never steps through
    it) owns ``obs_rms``, ``ret_rms`` and ``returns``; a vec-step becomes act (normalising on load) -> step -> [episode fold] -> stats ->
    store (raw rows) -> G x (sample -> normalise -> update [-> priorities]).  :meth:`eval_env` wraps an evaluation env around the same
    statistics tensors."""

    def __init__(self, env, cfg: SACConfig = SACConfig(), policy: Optional[SacPolicy] = None):
        self.env, self.cfg = env, cfg
        self.device = torch.device(env.device)
        self.N, self.d, self.A = env.num_envs, env.obs_dim, env.act_dim
        if policy is None:
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(int(cfg.seed))
                policy = SacPolicy(self.d, self.A, cfg.hidden)
        self._policy = policy.to(self.device)
        self.optimizers = make_optimizers(self._policy, cfg)
        self.G = cfg.resolved_gradient_steps(self.N)
        if not fits(self.d, self.A, cfg.hidden, cfg.batch_size):
            raise ValueError(f"the SAC kernels take obs_dim <= {MAX_OBS_DIM}, act_dim <= {MAX_ACT_DIM}, hidden in {HIDDEN_WIDTHS} and batch "
                             f"sizes that are multiples of 16 in [16, {MAX_BATCH}] or multiples of {WIDE_BATCH_MULTIPLE} in "
                             f"({MAX_BATCH}, {MAX_BATCH_WIDE}]; got ({self.d}, {self.A}, {cfg.hidden}, {cfg.batch_size})")
        if cfg.buffer_size < self.N:
            raise ValueError(f"buffer_size {cfg.buffer_size} cannot hold one vec-step of {self.N} envs")
        her_task = her_task_of(getattr(env, "cfg", None)) if cfg.her_goals > 0 else None      # (ValueError unless it is the low-level task)
        self.buffer = ReplayBufferDevice.from_config(cfg, self.N, self.d, self.A, self.device, her_task)
        self.fused = FusedSacUpdate(self._policy, self.optimizers, cfg)
        kw = dict(dtype=torch.float32, device=self.device)
        self.obs_stage, self.act_f32 = torch.zeros((self.N, self.d), **kw), torch.zeros((self.N, self.A), **kw)
        self.act_env = torch.zeros((self.N, self.A), dtype=env.torch_dtype, device=self.device)
        self.batch = torch.zeros((cfg.batch_size, self.buffer.row), **kw)
        self.batch_idx = torch.zeros(cfg.batch_size, dtype=torch.int32, device=self.device)
        self.noise = torch.zeros((2, cfg.batch_size, self.A), **kw)
        self.batch_w = torch.ones(cfg.batch_size, **kw) if cfg.prioritized else None        # the batch's importance weights ...
        self.batch_td = torch.zeros(cfg.batch_size, **kw) if cfg.prioritized else None      # ... and TD errors (prioritized only)
        self.scal = torch.zeros(5, **kw)          # the torch path's last scalars
        self.num_timesteps = 0
        self.env_offset = int(getattr(env, "global_env_offset", 0))
        self._started = False
        self._graphs = {}
        self.logs: Dict[str, float] = {}
        # SACConfig.episode_stats: the device-side episode monitor, folded once per vec-step behind the env step
        self.episode_monitor = None
        if cfg.episode_stats:
            from .monitor import EpisodeMonitor
            missing = [k for k in ("rewards", "terminated", "truncated") if not hasattr(env, k)]
            if missing:
                raise ValueError("SACConfig.episode_stats reads the env's output buffers after every step: the env has no " + ", ".join(missing))
            self.episode_monitor = EpisodeMonitor(self.N, int(cfg.stats_window_size), self.device, cfg.episode_fold)
        # SACConfig.normalize_obs / normalize_reward: the running statistics, moved once per vec-step behind the env step
        self.normalizer = None
        if cfg.normalizes:
            from .rollout import VecNormalizeDevice
            missing = [k for k in ("obs", "rewards", "terminated", "truncated") if not hasattr(env, k)]
            if missing:
                raise ValueError("SACConfig.normalize_obs / normalize_reward read the env's output buffers after every step: the env has no "
                                 + ", ".join(missing))
            self.normalizer = VecNormalizeDevice(env, training=True, norm_obs=cfg.normalize_obs, norm_reward=cfg.normalize_reward,
                                                 clip_obs=cfg.clip_obs, clip_reward=cfg.clip_reward, gamma=cfg.gamma, epsilon=cfg.norm_epsilon,
                                                 use_fused_kernel=True)

    @property
    def rollout_stats(self) -> Dict[str, float]:
        """``EpisodeMonitor.scalars()`` (SACConfig.episode_stats; ``{}`` with the flag off): SB3's ``rollout/ep_rew_mean`` /
        ``ep_len_mean`` / ``success_rate`` over the window, ``rollout/episodes`` and the ``rollout/interval/*`` means over the episodes
        finished since the figures were last read.  One small host read when somebody looks, like ``read_logs()``."""
        return {} if self.episode_monitor is None else self.episode_monitor.scalars()

    @property
    def policy(self) -> SacPolicy:
        """The torch modules, brought up to date with the image first: the fused gradient steps train the image and leave the
        modules (and the optimisers) alone until somebody asks for them."""
        self.sync_policy()
        return self._policy

    def sync_policy(self) -> None:
        if self.fused.ahead:
            self.fused.unpack(self._policy.n_updates + self.fused.ahead)

    @property
    def n_updates(self) -> int:
        return self._policy.n_updates + self.fused.ahead

    # ------------------------------------------------------------------ the pieces of a vec-step
    def _ensure_started(self) -> None:
        if not self._started:
            self.env.reset_tensor()
            self._started = True
            if self.normalizer is not None:        # VecNormalize.reset(): the returns start at 0, the reset observations enter obs_rms once
                self.normalizer.returns.zero_()
                if self.cfg.normalize_obs:
                    self._update_statistics(update_ret=False)

    def _image_for_act(self) -> torch.Tensor:
        if not self.fused.current():
            self.fused.pack()
        return self.fused.image

    def act(self, mode: int = ACT_STOCHASTIC, logp: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        env, cfg = self.env, self.cfg
        args = (_p(self._image_for_act()), _p(env.obs), int(env.torch_dtype == torch.float64), self.N, self.d, self.A, cfg.hidden, int(mode),
                int(cfg.seed) & (2**64 - 1), self.env_offset, _p(self.buffer.counters), _p(self.act_f32), _p(self.act_env), _p(self.obs_stage),
                _p(logp), _p(eps))
        if cfg.normalize_obs:            # the same launch with the observation normalised on load; obs_stage stays raw
            rms = self.normalizer.obs_rms
            _lib.check(_lib.lib().fw_sac_act_norm(*args, _p(rms.mean), _p(rms.var), cfg.clip_obs, cfg.norm_epsilon, _stream(self.device)))
        else:
            _lib.check(_lib.lib().fw_sac_act(*args, _stream(self.device)))
        return self.act_env

    def _store(self) -> None:
        e = self.env
        self.buffer.store(self.obs_stage, self.act_f32, e.rewards, e.obs, e.terminal_obs, e.terminated, e.truncated)

    def _update_statistics(self, update_ret: Optional[bool] = None) -> None:
        """``fw_collect_stats`` on the env's output buffers: the new observations into ``obs_rms`` (``normalize_obs``), ``returns gamma +
        reward`` into ``ret_rms`` (``normalize_reward``; ``update_ret=False``: the reset's call), ``returns = 0`` where an episode ended.
        It writes what the act and normalise launches read, on the same stream and never in the same launch."""
        e, nz, cfg = self.env, self.normalizer, self.cfg
        f64 = int(e.torch_dtype == torch.float64)
        upd_ret = cfg.normalize_reward if update_ret is None else bool(update_ret)
        _lib.check(_lib.lib().fw_collect_stats(_p(e.obs), f64, self.N, self.d, _p(nz.obs_rms.mean), _p(nz.obs_rms.var), _p(nz.obs_rms.count),
                                               int(cfg.normalize_obs), _p(e.rewards), int(e.rewards.dtype == torch.float64), _p(e.terminated),
                                               _p(e.truncated), _p(nz.returns), _p(nz.ret_rms.mean), _p(nz.ret_rms.var), _p(nz.ret_rms.count),
                                               int(upd_ret), float(cfg.gamma), None, _p(nz._ws_stats), None, None, _stream(self.device)))

    def normalize_batch(self, rows: torch.Tensor) -> torch.Tensor:
        """``fw_replay_normalize`` in place on gathered rows, with the statistics as they are now (nothing with both flags off)."""
        nz, cfg = self.normalizer, self.cfg
        if nz is None:
            return rows
        assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.shape[1] == self.buffer.row
        _lib.check(_lib.lib().fw_replay_normalize(_p(rows), rows.shape[0], self.d, self.A,
                                                  _p(nz.obs_rms.mean) if cfg.normalize_obs else None,
                                                  _p(nz.obs_rms.var) if cfg.normalize_obs else None, cfg.clip_obs, cfg.norm_epsilon,
                                                  _p(nz.ret_rms.var) if cfg.normalize_reward else None, cfg.clip_reward, cfg.norm_epsilon,
                                                  _stream(self.device)))
        return rows

    def _gradient_step_fused(self) -> None:
        self.buffer.sample(self.cfg.seed, self.batch, self.batch_idx, gamma=self.cfg.gamma, w_out=self.batch_w)
        self.normalize_batch(self.batch)     # (behind the gather: hindsight rewards and n-step sums are formed on raw values)
        self.fused.run(self.batch, self.buffer.counters, weights=self.batch_w, td_out=self.batch_td)      # (both None unless prioritized)
        if self.cfg.prioritized:         # sample -> weighted update -> priorities -> rebuild, all stream-ordered: one graph still
            self.buffer.update_priorities(self.batch_idx, self.batch_td)

    def _gradient_step_torch(self) -> None:
        pri = self.cfg.prioritized
        self.buffer.sample(self.cfg.seed, self.batch, self.batch_idx, gamma=self.cfg.gamma, w_out=self.batch_w)
        self.normalize_batch(self.batch)
        sac_noise(self.cfg.seed, self.buffer.counters, self.cfg.batch_size, self.A, out=self.noise)
        s = sac_update_torch(self._policy, self.optimizers, self.batch, self.noise[0], self.noise[1], self.cfg,
                             weights=self.batch_w if pri else None)
        self.scal.copy_(torch.stack([s[k].float() for k in SCALARS]))
        self.buffer.counters[CTR_GRAD] += 1
        if pri:
            self.batch_td.copy_(s["td"].float())
            self.buffer.update_priorities(self.batch_idx, self.batch_td)

    def _vec_step_body(self, warm: bool, with_train: bool) -> None:
        self.act(ACT_WARMUP if warm else ACT_STOCHASTIC)
        self.env.step_tensor(self.act_env)
        if self.episode_monitor is not None:       # (same stream: the env's output buffers hold the step until the next launch)
            e = self.env
            self.episode_monitor.fold(e.rewards, e.terminated, e.truncated, getattr(e, "info", None))
        if self.normalizer is not None:
            self._update_statistics()
        self._store()
        if with_train:
            for _ in range(self.G):
                self._gradient_step_fused()

    def _replay(self, key, warm: bool, with_train: bool) -> None:
        """The vec-step of this form as a graph replay.  Its first call runs eagerly (it loads the kernels and is the vec-step
        itself), its second call captures -- a capture runs nothing -- and replays."""
        g = self._graphs.get(key)
        if g is None:
            self._vec_step_body(warm, with_train)
            self._graphs[key] = "ran"
            return
        if g == "ran":
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._vec_step_body(warm, with_train)
            self._graphs[key] = g
        g.replay()

    def collect_step(self, train: bool = True) -> None:
        """One vec-step: act (uniform while ``num_timesteps < learning_starts``) -> env step -> store, then -- unless it was a warm-up
        step or ``train`` is off -- the configured number of gradient steps."""
        self._ensure_started()
        warm = self.num_timesteps < self.cfg.learning_starts
        do_train = train and not warm and self.G > 0
        fused_train = do_train and self.cfg.fused_update
        if fused_train and not self.fused.current():
            self.fused.pack()
        if self.cfg.use_graphs:
            if not warm:
                self._image_for_act()
            self._replay((warm, fused_train), warm, fused_train)
        else:
            self._vec_step_body(warm, fused_train)
        if fused_train:
            self.fused.ahead += self.G
        elif do_train:
            self.train(self.G)
        self.num_timesteps += self.N

    def train(self, gradient_steps: int) -> None:
        """``gradient_steps`` x (sample -> update) on the current buffer."""
        if gradient_steps <= 0:
            return
        if self.cfg.fused_update:
            if not self.fused.current():
                self.fused.pack()
            for _ in range(gradient_steps):
                self._gradient_step_fused()
            self.fused.ahead += gradient_steps
        else:
            self.sync_policy()
            for _ in range(gradient_steps):
                self._gradient_step_torch()

    def read_logs(self) -> Dict[str, float]:
        """The last gradient step's scalars (one host read)."""
        src = self.fused.out[:5] if self.cfg.fused_update else self.scal
        self.logs = dict(zip(SCALARS, src.tolist()))
        self.logs["n_updates"] = self.n_updates
        self.logs["num_timesteps"] = self.num_timesteps
        return self.logs

    def learn(self, total_timesteps: int, callbacks: Sequence = ()):
        """Vec-steps until ``num_timesteps`` has grown by ``total_timesteps``; every callback is called as ``cb(self)`` after each
        vec-step and stops the run by returning ``False``."""
        end = self.num_timesteps + int(total_timesteps)
        t0, n0 = time.perf_counter(), self.num_timesteps
        while self.num_timesteps < end:
            self.collect_step()
            if any(cb(self) is False for cb in callbacks):
                break
        torch.cuda.synchronize(self.device)
        self.read_logs()
        self.logs["env_steps_per_s"] = (self.num_timesteps - n0) / max(time.perf_counter() - t0, 1e-9)
        return self

    def eval_env(self, venv):
        """An evaluation wrapper of ``venv`` for :func:`~.evaluate.evaluate_policy` on ``self.policy``: a frozen
        :class:`~.rollout.VecNormalizeDevice` (``training=False``, ``norm_reward=False``) whose ``obs_rms`` IS the learner's -- the same
        tensors, so every evaluation sees the statistics as they are then.  With ``normalize_obs`` off it passes observations through."""
        from .rollout import VecNormalizeDevice
        cfg = self.cfg
        ev = VecNormalizeDevice(venv, training=False, norm_obs=cfg.normalize_obs, norm_reward=False, clip_obs=cfg.clip_obs,
                                clip_reward=cfg.clip_reward, gamma=cfg.gamma, epsilon=cfg.norm_epsilon)
        if self.normalizer is not None:
            if ev.obs_dim != self.d:
                raise ValueError(f"the evaluation env has {ev.obs_dim} observations, the learner's statistics {self.d}")
            ev.obs_rms = self.normalizer.obs_rms
        return ev

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self, include_buffer: bool = False):
        self.sync_policy()
        sd = {"policy": self._policy.state_dict(), "n_updates": self._policy.n_updates,
              "optimizers": {k: (o.state_dict() if o is not None else None) for k, o in self.optimizers.items()},
              "buffer": self.buffer.state_dict(include_buffer), "num_timesteps": self.num_timesteps, "config": asdict(self.cfg)}
        if self.episode_monitor is not None:
            sd["episode_stats"] = self.episode_monitor.state_dict()
        if self.normalizer is not None:
            nz = self.normalizer
            sd["normalizer"] = {"obs_rms": nz.obs_rms.state_dict(), "ret_rms": nz.ret_rms.state_dict(), "returns": nz.returns.cpu().clone()}
        return sd

    def load_state_dict(self, sd) -> None:
        self.fused.ahead = 0
        self._policy.load_state_dict(sd["policy"])
        self._policy.n_updates = int(sd["n_updates"])
        for k, o in self.optimizers.items():
            if o is not None and sd["optimizers"].get(k) is not None:
                o.load_state_dict(sd["optimizers"][k])
        self.buffer.load_state_dict(sd["buffer"])
        self.num_timesteps = int(sd["num_timesteps"])
        self.fused._sig = None
        if self.episode_monitor is not None and sd.get("episode_stats") is not None:
            self.episode_monitor.load_state_dict(sd["episode_stats"])
        if self.normalizer is not None and sd.get("normalizer") is not None:       # in place: the captured graphs hold these addresses
            nz, st = self.normalizer, sd["normalizer"]                              # (a checkpoint without them: the statistics stay)
            nz.obs_rms.load_state_dict(st["obs_rms"]); nz.ret_rms.load_state_dict(st["ret_rms"])
            nz.returns.copy_(st["returns"])
