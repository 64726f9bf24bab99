"""TD3 for the low-level control task (SB3 ``TD3("MlpPolicy")``): a deterministic actor, two critics, a target of each, delayed actor
and target steps, target policy smoothing.  The second off-policy learner beside :mod:`.sac`, on the same device replay ring
(:mod:`.replay`) and the same product kernel.

Everything between two env steps runs on the device (csrc/fwsim_td3.hpp, include/fwsim.h):

* ``fw_td3_act``     the actor on the env's observations: ``tanh(mean)``, the exploring ``clamp(tanh(mean) + sigma eps, -1, 1)`` or SB3's
                     uniform ``learning_starts`` actions; the fp32 staging copy of the observation the step is about to overwrite;
* ``fw_sac_noise``   the smoothing noise of a gradient step (its first block);
* ``fw_td3_update``  one gradient step of SB3's ``TD3.train()`` on a flat image of all six networks and their Adam moments, with or
                     without the actor part.

:func:`td3_update_torch` is the same gradient step in plain torch (CPU tensors too): the reference the kernels are tested against and
the ``fused_update=False`` path.

Two departures from SB3's defaults, both owned by this build: ``net_arch=(256, 256)`` instead of (400, 300), because the kernels are
built for hidden widths 64 and 256 only, and ``action_noise_sigma=0.1`` (Gaussian exploration noise on the tanh action) instead of
``action_noise=None``, because a deterministic actor that never explores is not a usable default.  As in :mod:`.sac`, the delayed step
counts the *total* number of gradient steps (SB3 counts the same ``_n_updates``), and a vec-step is a warm-up step exactly while
``num_timesteps < learning_starts``.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass, asdict
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _lib
from .replay import CTR_GRAD, ReplayBufferDevice, _p, _stream, check_sampler_options, her_task_of, row_floats, split_rows
from .sac import HIDDEN_WIDTHS, MAX_ACT_DIM, MAX_BATCH, MAX_OBS_DIM, _mlp, net_floats, sac_noise

ACT_EXPLORE, ACT_DETERMINISTIC, ACT_WARMUP = 0, 1, 2          # fw_sac_act's integers
MAX_POLICY_DELAY = 8
SCALARS = ("critic_loss", "actor_loss")


@dataclass
class TD3Config:
    """SB3's ``TD3`` defaults, but for ``net_arch`` ((256, 256), not (400, 300): the kernels' hidden widths are 64 and 256) and
    ``action_noise_sigma`` (0.1, not SB3's ``action_noise=None``: a deterministic actor needs exploration noise to be usable)."""
    learning_rate: float = 1e-3
    buffer_size: int = 1_000_000
    batch_size: int = 256
    gamma: float = 0.99
    tau: float = 0.005
    policy_delay: int = 2                # the actor and the three targets step on every policy_delay-th gradient step (1 ... 8)
    target_policy_noise: float = 0.2     # target policy smoothing: clamp(target_policy_noise eps, +-target_noise_clip) on a'
    target_noise_clip: float = 0.5
    action_noise_sigma: float = 0.1      # exploration: clamp(tanh(mean) + action_noise_sigma eps, -1, 1); 0: none
    learning_starts: int = 100
    gradient_steps: int = 1              # per vec-step; -1: one per env (SB3's meaning)
    net_arch: Tuple[int, int] = (256, 256)
    seed: int = 0
    use_graphs: bool = True
    fused_update: bool = True
    episode_stats: bool = False          # as SACConfig: SB3's rollout/* figures (TD3.rollout_stats)
    stats_window_size: int = 100
    episode_fold: str = "one"
    n_steps: int = 1                     # n-step returns from the ring (1 ... 16)
    her_goals: int = 0                   # hindsight goal relabelling (SB3's n_sampled_goal); not built together with n_steps > 1
    her_horizon: int = 64
    prioritized: bool = False            # not built for TD3 (the step has no weighted form): True is refused
    normalize_obs: bool = False          # not built for TD3 (the act kernel does not normalise): True is refused
    normalize_reward: bool = False       #     likewise

    # what ReplayBufferDevice.from_config reads of prioritized replay (no fields: the option is refused above)
    per_alpha, per_beta, per_beta_steps, per_eps = 0.6, 0.4, 0, 1e-6

    def __post_init__(self):
        if self.prioritized:
            raise ValueError("prioritized replay under TD3 is not built: the gradient step has no weighted form")
        if self.normalize_obs or self.normalize_reward:
            raise ValueError("normalize_obs / normalize_reward under TD3 are not built: the act kernel does not normalise its input")
        self.n_steps, self.her_goals, self.her_horizon = check_sampler_options(self.n_steps, self.her_goals, self.her_horizon, False,
                                                                               self.per_alpha, self.per_beta, self.per_beta_steps, self.per_eps)[:3]
        if isinstance(self.policy_delay, bool) or int(self.policy_delay) != self.policy_delay or not 1 <= int(self.policy_delay) <= MAX_POLICY_DELAY:
            raise ValueError(f"policy_delay must be a whole number in [1, {MAX_POLICY_DELAY}], got {self.policy_delay!r}")
        self.policy_delay = int(self.policy_delay)
        if self.episode_fold not in ("one", "wide", "auto"):
            raise ValueError(f"episode_fold must be 'one', 'wide' or 'auto', got {self.episode_fold!r}")
        if int(self.stats_window_size) <= 0:
            raise ValueError("stats_window_size must be positive")
        self.net_arch = tuple(int(h) for h in self.net_arch)
        if len(self.net_arch) != 2 or self.net_arch[0] != self.net_arch[1] or self.net_arch[0] <= 0:
            raise ValueError(f"net_arch must be two equal positive widths, got {self.net_arch}")
        if self.gradient_steps != -1 and self.gradient_steps < 0:
            raise ValueError("gradient_steps must be non-negative, or -1 for one per env")
        if self.batch_size <= 0 or self.buffer_size <= 0 or self.learning_starts < 0:
            raise ValueError("batch_size and buffer_size must be positive, learning_starts non-negative")
        if not (0.0 <= self.gamma <= 1.0 and 0.0 < self.tau <= 1.0 and self.learning_rate > 0.0):
            raise ValueError("gamma must be in [0, 1], tau in (0, 1] and learning_rate positive")
        for name in ("target_policy_noise", "target_noise_clip", "action_noise_sigma"):
            v = float(getattr(self, name))
            if not (v >= 0.0 and v < float("inf")):
                raise ValueError(f"{name} must be a non-negative finite number, got {getattr(self, name)!r}")
            setattr(self, name, v)

    @property
    def hidden(self) -> int:
        return self.net_arch[0]

    @property
    def her_relabel_prob(self) -> float:
        return self.her_goals / (self.her_goals + 1.0)

    def resolved_gradient_steps(self, num_envs: int) -> int:
        return int(num_envs) if self.gradient_steps == -1 else int(self.gradient_steps)


def fits(obs_dim: int, act_dim: int, hidden: int, batch_size: int) -> bool:
    """What the kernels are built for (include/fwsim.h): anything else is ``FW_EUNSUPPORTED``.  No wide form: batches are multiples of
    16 in [16, ``MAX_BATCH``]."""
    return (1 <= obs_dim <= MAX_OBS_DIM and 1 <= act_dim <= MAX_ACT_DIM and hidden in HIDDEN_WIDTHS
            and 16 <= batch_size <= MAX_BATCH and batch_size % 16 == 0)


# ---------------------------------------------------------------------------------------------
# the torch modules
# ---------------------------------------------------------------------------------------------
TRAINED = ("actor", "q1", "q2")
NETS = TRAINED + ("actor_target", "q1_target", "q2_target")


class Td3Policy(nn.Module):
    """Actor ``d -> H -> H -> A`` with ``tanh`` on its output, two critics ``(d + A) -> H -> H -> 1`` on ``cat(obs, action)`` and a
    target of each of the three (copies at construction): ReLU MLPs, torch's default initialisation."""

    def __init__(self, obs_dim: int, act_dim: int, hidden: int = 256):
        super().__init__()
        self.obs_dim, self.act_dim, self.hidden = int(obs_dim), int(act_dim), int(hidden)
        self.actor = _mlp(obs_dim, hidden, act_dim)
        self.q1, self.q2 = _mlp(obs_dim + act_dim, hidden, 1), _mlp(obs_dim + act_dim, hidden, 1)
        self.actor_target = _mlp(obs_dim, hidden, act_dim)
        self.q1_target, self.q2_target = _mlp(obs_dim + act_dim, hidden, 1), _mlp(obs_dim + act_dim, hidden, 1)
        for name in TRAINED:
            tgt = getattr(self, name + "_target")
            tgt.load_state_dict(getattr(self, name).state_dict())
            for q in tgt.parameters():
                q.requires_grad_(False)
        self.n_updates = 0               # gradient steps taken (the delay counts them) ...
        self.n_actor_updates = 0         # ... and those of them that stepped the actor and the targets

    def pi(self, obs, target: bool = False):
        return torch.tanh((self.actor_target if target else self.actor)(obs))

    def q_min(self, obs, act, target: bool = False):
        x = torch.cat([obs, act], dim=-1)
        q1, q2 = (self.q1_target, self.q2_target) if target else (self.q1, self.q2)
        return torch.min(q1(x), q2(x)).squeeze(-1)

    def forward(self, obs, deterministic: bool = True, generator=None):
        """``(actions, values, log_prob)`` like :class:`~.sac.SacPolicy`: the action is ``tanh(actor(obs))`` either way (exploration noise
        is the learner's, not the policy's), values are min(Q1, Q2)(obs, action), ``log_prob`` is zero."""
        obs = obs.to(dtype=self.actor[0].weight.dtype)
        a = self.pi(obs)
        return a, self.q_min(obs, a), torch.zeros(a.shape[:-1], dtype=a.dtype, device=a.device)


def make_optimizers(policy: Td3Policy, cfg: TD3Config, capturable: bool = False) -> Dict[str, torch.optim.Adam]:
    """SB3's two optimisers: Adam(eps 1e-8, betas (0.9, 0.999)) for the actor and for both critics together."""
    kw = dict(lr=cfg.learning_rate, eps=1e-8, betas=(0.9, 0.999), capturable=capturable)
    return {"actor": torch.optim.Adam(policy.actor.parameters(), **kw),
            "critic": torch.optim.Adam(list(policy.q1.parameters()) + list(policy.q2.parameters()), **kw)}


def td3_update_torch(policy: Td3Policy, optimizers, batch, eps, cfg: TD3Config, with_actor: Optional[bool] = None) -> Dict[str, torch.Tensor]:
    """One gradient step of SB3's ``TD3.train()`` in the order DESIGN.md section 4d spells out.  ``batch``: ``(s, a, r, s', last)`` or
    rows ``[B, 2d + A + 2]``; ``eps``: N(0, 1) of shape ``[B, A]``, the smoothing noise before scale and clip.  ``with_actor``: whether
    this step also steps the actor and the three targets; by default ``(n_updates + 1) % policy_delay == 0``.  Returns the critic loss
    and, on a step with the actor part, the actor loss (tensors, no host read)."""
    if torch.is_tensor(batch):
        batch = split_rows(batch, policy.obs_dim, policy.act_dim)
    s, a, r, s2, last = batch
    if with_actor is None:
        with_actor = (policy.n_updates + 1) % cfg.policy_delay == 0
    with torch.no_grad():
        noise = (cfg.target_policy_noise * eps).clamp(-cfg.target_noise_clip, cfg.target_noise_clip)
        a2 = (policy.pi(s2, target=True) + noise).clamp(-1.0, 1.0)
        y = r + (1.0 - last) * cfg.gamma * policy.q_min(s2, a2, target=True)
    x = torch.cat([s, a], dim=-1)
    q1, q2 = policy.q1(x).squeeze(-1), policy.q2(x).squeeze(-1)
    critic_loss = ((q1 - y) ** 2).mean() + ((q2 - y) ** 2).mean()          # SB3: the sum of the two, no 1/2
    optimizers["critic"].zero_grad(set_to_none=True); critic_loss.backward(); optimizers["critic"].step()
    policy.n_updates += 1
    out = {"critic_loss": critic_loss.detach()}
    if with_actor:
        actor_loss = -policy.q1(torch.cat([s, policy.pi(s)], dim=-1)).mean()          # the critic after its step
        optimizers["actor"].zero_grad(set_to_none=True); actor_loss.backward(); optimizers["actor"].step()
        optimizers["critic"].zero_grad(set_to_none=True)      # (the actor loss left gradients in Q1: they are not its own)
        policy.n_actor_updates += 1
        with torch.no_grad():
            for name in TRAINED:
                for p, t in zip(getattr(policy, name).parameters(), getattr(policy, name + "_target").parameters()):
                    t.mul_(1.0 - cfg.tau).add_(p, alpha=cfg.tau)
        out["actor_loss"] = actor_loss.detach()
    return out


# ---------------------------------------------------------------------------------------------
# the flat image of fw_td3_update
# ---------------------------------------------------------------------------------------------
class _Td3Hyper(C.Structure):
    _fields_ = [("lr", C.c_float), ("gamma", C.c_float), ("tau", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("policy_noise", C.c_float), ("noise_clip", C.c_float), ("seed", C.c_uint64)]


def image_layout(obs_dim: int, act_dim: int, hidden: int) -> Dict[str, int]:
    """Offsets (floats) of the blocks of the flat image (include/fwsim.h)."""
    na, nc = net_floats(obs_dim, hidden, act_dim), net_floats(obs_dim + act_dim, hidden, 1)
    T = na + 2 * nc
    L = {"actor": 0, "q1": na, "q2": na + nc, "trained": T, "actor_target": T, "q1_target": T + na, "q2_target": T + na + nc,
         "params": 2 * T, "exp_avg": 2 * T, "exp_avg_sq": 3 * T, "tail": 4 * T}
    L["total"] = L["tail"] + 4
    return L


class FusedTd3Update:
    """Host side of ``fw_td3_update``: the flat float32 image of the six networks, the Adam moments and the two step counts, and its
    pack / unpack against the modules and the two optimisers (CPU tensors too).  The image is a cache of them, guarded by the tensors'
    version counters as :class:`~.sac.FusedSacUpdate` is."""

    def __init__(self, policy: Td3Policy, optimizers, cfg: TD3Config):
        self.policy, self.opts, self.cfg = policy, optimizers, cfg
        self.d, self.A, self.H = policy.obs_dim, policy.act_dim, policy.hidden
        self.L = image_layout(self.d, self.A, self.H)
        dev = policy.actor[0].weight.device
        self.image = torch.zeros(self.L["total"], dtype=torch.float32, device=dev)
        self.out = torch.zeros(8, dtype=torch.float32, device=dev)
        self._ws = None
        self._sig = None
        self.ahead = 0                   # gradient steps the image has taken since it was last equal to modules and optimisers ...
        self.ahead_actor = 0             # ... and actor steps among them

    def _slots(self):
        """(tensor, offset in the image, needs transpose, optimiser or None) per parameter, in layout order."""
        p, out = self.policy, []
        for name, opt in (("actor", self.opts["actor"]), ("q1", self.opts["critic"]), ("q2", self.opts["critic"]),
                          ("actor_target", None), ("q1_target", None), ("q2_target", None)):
            net, off = getattr(p, name), self.L[name]
            for lin in (net[0], net[2], net[4]):
                out.append((lin.weight, off, True, opt)); off += lin.weight.numel()
                out.append((lin.bias, off, False, opt)); off += lin.bias.numel()
        return out

    def signature(self):
        sig = [self.policy.n_updates, self.policy.n_actor_updates]
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
        tail = img[L["tail"]:].view(torch.int32)
        tail[0], tail[1] = int(self.policy.n_updates), int(self.policy.n_actor_updates)
        self._sig, self.ahead, self.ahead_actor = self.signature(), 0, 0

    @torch.no_grad()
    def unpack(self, n_updates: Optional[int] = None, n_actor_updates: Optional[int] = None) -> None:
        """Image -> modules and optimisers.  The two step counts when the caller already knows them (no host read)."""
        img, L = self.image, self.L
        if n_updates is None or n_actor_updates is None:
            n_updates, n_actor_updates = (int(v) for v in img[L["tail"]:].view(torch.int32)[:2].tolist())
        steps = {id(self.opts["actor"]): int(n_actor_updates), id(self.opts["critic"]): int(n_updates)}
        for t, off, tr, opt in self._slots():
            n = t.numel()
            shape = (t.shape[1], t.shape[0]) if tr else t.shape

            def get(base):
                v = img[base + off:base + off + n].view(shape)
                return v.t() if tr else v
            t.data.copy_(get(0))
            if opt is None:
                continue
            step = steps[id(opt)]
            if step == 0 and not opt.state.get(t):
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
        self.policy.n_updates, self.policy.n_actor_updates = int(n_updates), int(n_actor_updates)
        self._sig, self.ahead, self.ahead_actor = self.signature(), 0, 0

    def hyper(self) -> _Td3Hyper:
        pg = self.opts["actor"].param_groups[0]
        cfg = self.cfg
        return _Td3Hyper(lr=pg["lr"], gamma=cfg.gamma, tau=cfg.tau, beta1=pg["betas"][0], beta2=pg["betas"][1], eps=pg["eps"],
                         policy_noise=cfg.target_policy_noise, noise_clip=cfg.target_noise_clip, seed=int(cfg.seed) & (2**64 - 1))

    def workspace(self, batch: int) -> torch.Tensor:
        need = int(_lib.lib().fw_td3_update_workspace_bytes(self.d, self.A, self.H, batch))
        if need < 0:
            _lib.check(need)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.zeros(need, dtype=torch.uint8, device=self.image.device)
        return self._ws

    def run(self, rows: torch.Tensor, counters: torch.Tensor, with_actor: bool) -> None:
        """One gradient step on the image (the caller packs before, counts the step in ``ahead`` / ``ahead_actor`` and unpacks when
        the modules are wanted; nothing here reads the device)."""
        assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.shape[1] == row_floats(self.d, self.A)
        B = rows.shape[0]
        ws = self.workspace(B) if fits(self.d, self.A, self.H, B) else self.out          # (an unsupported shape: let the ABI say so)
        H = self.hyper()
        _lib.check(_lib.lib().fw_td3_update(_p(self.image), _p(rows), self.d, self.A, self.H, B, C.byref(H), int(bool(with_actor)), _p(counters),
                                            _p(self.out), _p(ws), ws.numel(), _stream(rows.device)))

    def scalars(self) -> Dict[str, float]:
        return dict(zip(SCALARS, self.out[:2].tolist()))


# ---------------------------------------------------------------------------------------------
# the learner
# ---------------------------------------------------------------------------------------------
class TD3:
    """TD3 on a bare device env (``FixedwingLowLevelVecEnv``).  A vec-step is act -> ``env.step_tensor`` -> store -> G x (sample ->
    update), and which of the G updates carry the actor part depends on ``n_updates % policy_delay`` at the start of the vec-step: with
    ``use_graphs`` and the fused update there is one captured graph per (warm-up, training, that residue), at most ``policy_delay``
    training graphs, and no host read on the training path."""

    def __init__(self, env, cfg: TD3Config = TD3Config(), policy: Optional[Td3Policy] = None):
        self.env, self.cfg = env, cfg
        self.device = torch.device(env.device)
        self.N, self.d, self.A = env.num_envs, env.obs_dim, env.act_dim
        if policy is None:
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(int(cfg.seed))
                policy = Td3Policy(self.d, self.A, cfg.hidden)
        self._policy = policy.to(self.device)
        self.optimizers = make_optimizers(self._policy, cfg)
        self.G = cfg.resolved_gradient_steps(self.N)
        if not fits(self.d, self.A, cfg.hidden, cfg.batch_size):
            raise ValueError(f"the TD3 kernels take obs_dim <= {MAX_OBS_DIM}, act_dim <= {MAX_ACT_DIM}, hidden in {HIDDEN_WIDTHS} and batch "
                             f"sizes that are multiples of 16 in [16, {MAX_BATCH}]; got ({self.d}, {self.A}, {cfg.hidden}, {cfg.batch_size})")
        if cfg.buffer_size < self.N:
            raise ValueError(f"buffer_size {cfg.buffer_size} cannot hold one vec-step of {self.N} envs")
        her_task = her_task_of(getattr(env, "cfg", None)) if cfg.her_goals > 0 else None      # (ValueError unless it is the low-level task)
        self.buffer = ReplayBufferDevice.from_config(cfg, self.N, self.d, self.A, self.device, her_task)
        self.fused = FusedTd3Update(self._policy, self.optimizers, cfg)
        kw = dict(dtype=torch.float32, device=self.device)
        self.obs_stage, self.act_f32 = torch.zeros((self.N, self.d), **kw), torch.zeros((self.N, self.A), **kw)
        self.act_env = torch.zeros((self.N, self.A), dtype=env.torch_dtype, device=self.device)
        self.batch = torch.zeros((cfg.batch_size, self.buffer.row), **kw)
        self.batch_idx = torch.zeros(cfg.batch_size, dtype=torch.int32, device=self.device)
        self.noise = torch.zeros((2, cfg.batch_size, self.A), **kw)
        self.scal = torch.zeros(2, **kw)          # the torch path's last scalars
        self.num_timesteps = 0
        self.env_offset = int(getattr(env, "global_env_offset", 0))
        self._started = False
        self._graphs = {}
        self.logs: Dict[str, float] = {}
        self.episode_monitor = None
        if cfg.episode_stats:
            from .monitor import EpisodeMonitor
            missing = [k for k in ("rewards", "terminated", "truncated") if not hasattr(env, k)]
            if missing:
                raise ValueError("TD3Config.episode_stats reads the env's output buffers after every step: the env has no " + ", ".join(missing))
            self.episode_monitor = EpisodeMonitor(self.N, int(cfg.stats_window_size), self.device, cfg.episode_fold)

    @property
    def rollout_stats(self) -> Dict[str, float]:
        """``EpisodeMonitor.scalars()`` (TD3Config.episode_stats; ``{}`` with the flag off), as :attr:`.sac.SAC.rollout_stats`."""
        return {} if self.episode_monitor is None else self.episode_monitor.scalars()

    @property
    def policy(self) -> Td3Policy:
        """The torch modules, brought up to date with the image first."""
        self.sync_policy()
        return self._policy

    def sync_policy(self) -> None:
        if self.fused.ahead:
            self.fused.unpack(self._policy.n_updates + self.fused.ahead, self._policy.n_actor_updates + self.fused.ahead_actor)

    @property
    def n_updates(self) -> int:
        return self._policy.n_updates + self.fused.ahead

    @property
    def n_actor_updates(self) -> int:
        return self._policy.n_actor_updates + self.fused.ahead_actor

    def _with_actor(self, n_updates: int) -> bool:
        """Whether the gradient step that follows ``n_updates`` earlier ones carries the actor part (SB3: ``_n_updates % policy_delay == 0``
        after the increment)."""
        return (n_updates + 1) % self.cfg.policy_delay == 0

    # ------------------------------------------------------------------ the pieces of a vec-step
    def _ensure_started(self) -> None:
        if not self._started:
            self.env.reset_tensor()
            self._started = True

    def _image_for_act(self) -> torch.Tensor:
        if not self.fused.current():
            self.fused.pack()
        return self.fused.image

    def act(self, mode: int = ACT_EXPLORE, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        env, cfg = self.env, self.cfg
        _lib.check(_lib.lib().fw_td3_act(_p(self._image_for_act()), _p(env.obs), int(env.torch_dtype == torch.float64), self.N, self.d, self.A,
                                         cfg.hidden, int(mode), int(cfg.seed) & (2**64 - 1), self.env_offset, _p(self.buffer.counters),
                                         _p(self.act_f32), _p(self.act_env), _p(self.obs_stage), cfg.action_noise_sigma, _p(eps),
                                         _stream(self.device)))
        return self.act_env

    def _store(self) -> None:
        e = self.env
        self.buffer.store(self.obs_stage, self.act_f32, e.rewards, e.obs, e.terminal_obs, e.terminated, e.truncated)

    def _gradient_step_fused(self, with_actor: bool) -> None:
        self.buffer.sample(self.cfg.seed, self.batch, self.batch_idx, gamma=self.cfg.gamma)
        self.fused.run(self.batch, self.buffer.counters, with_actor)

    def _gradient_step_torch(self) -> None:
        self.buffer.sample(self.cfg.seed, self.batch, self.batch_idx, gamma=self.cfg.gamma)
        sac_noise(self.cfg.seed, self.buffer.counters, self.cfg.batch_size, self.A, out=self.noise)
        s = td3_update_torch(self._policy, self.optimizers, self.batch, self.noise[0], self.cfg)
        self.scal[0] = s["critic_loss"].float()
        if "actor_loss" in s:
            self.scal[1] = s["actor_loss"].float()
        self.buffer.counters[CTR_GRAD] += 1

    def _vec_step_body(self, warm: bool, with_train: bool, residue: int) -> None:
        self.act(ACT_WARMUP if warm else ACT_EXPLORE)
        self.env.step_tensor(self.act_env)
        if self.episode_monitor is not None:
            e = self.env
            self.episode_monitor.fold(e.rewards, e.terminated, e.truncated, getattr(e, "info", None))
        self._store()
        if with_train:
            for k in range(self.G):
                self._gradient_step_fused(self._with_actor(residue + k))

    def _replay(self, key, warm: bool, with_train: bool, residue: int) -> None:
        """The vec-step of this form as a graph replay: its first call runs eagerly (it loads the kernels and is the vec-step itself),
        its second call captures -- a capture runs nothing -- and replays."""
        g = self._graphs.get(key)
        if g is None:
            self._vec_step_body(warm, with_train, residue)
            self._graphs[key] = "ran"
            return
        if g == "ran":
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._vec_step_body(warm, with_train, residue)
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
        residue = self.n_updates % self.cfg.policy_delay if fused_train else 0
        if self.cfg.use_graphs:
            if not warm:
                self._image_for_act()
            self._replay((warm, fused_train, residue), warm, fused_train, residue)
        else:
            self._vec_step_body(warm, fused_train, residue)
        if fused_train:
            self._count_ahead(self.G)
        elif do_train:
            self.train(self.G)
        self.num_timesteps += self.N

    def _count_ahead(self, steps: int) -> None:
        n = self.n_updates
        self.fused.ahead_actor += sum(self._with_actor(n + k) for k in range(steps))
        self.fused.ahead += steps

    def train(self, gradient_steps: int) -> None:
        """``gradient_steps`` x (sample -> update) on the current buffer."""
        if gradient_steps <= 0:
            return
        if self.cfg.fused_update:
            if not self.fused.current():
                self.fused.pack()
            n = self.n_updates
            for k in range(gradient_steps):
                self._gradient_step_fused(self._with_actor(n + k))
            self._count_ahead(gradient_steps)
        else:
            self.sync_policy()
            for _ in range(gradient_steps):
                self._gradient_step_torch()

    def read_logs(self) -> Dict[str, float]:
        """The last gradient steps' scalars (one host read): the critic loss of the last step, the actor loss of the last step that had
        the actor part."""
        src = self.fused.out[:2] if self.cfg.fused_update else self.scal
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

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self, include_buffer: bool = False):
        self.sync_policy()
        sd = {"policy": self._policy.state_dict(), "n_updates": self._policy.n_updates, "n_actor_updates": self._policy.n_actor_updates,
              "optimizers": {k: o.state_dict() for k, o in self.optimizers.items()},
              "buffer": self.buffer.state_dict(include_buffer), "num_timesteps": self.num_timesteps, "config": asdict(self.cfg)}
        if self.episode_monitor is not None:
            sd["episode_stats"] = self.episode_monitor.state_dict()
        return sd

    def load_state_dict(self, sd) -> None:
        self.fused.ahead = self.fused.ahead_actor = 0
        self._policy.load_state_dict(sd["policy"])
        self._policy.n_updates, self._policy.n_actor_updates = int(sd["n_updates"]), int(sd["n_actor_updates"])
        for k, o in self.optimizers.items():
            if sd["optimizers"].get(k) is not None:
                o.load_state_dict(sd["optimizers"][k])
        self.buffer.load_state_dict(sd["buffer"])
        self.num_timesteps = int(sd["num_timesteps"])
        self.fused._sig = None
        if self.episode_monitor is not None and sd.get("episode_stats") is not None:
            self.episode_monitor.load_state_dict(sd["episode_stats"])
