"""One deterministic, statistics-frozen vec-step -- "act, then step the env once" -- and the replay driver of the flight recorders.

What ``evaluate.ReplayedEvaluation`` and the three ``fly`` functions (``flight``, ``command``, ``highlevel``) put in front of their own
bookkeeping or trace kernel.  A step comes in four kinds (``KINDS``):

    collect_step   ONE ``fw_collect_step`` launch: the four-action MlpPolicy on the 8-lane mapping (:class:`CollectStep`)
    act_a          ``fw_collect_act_a`` -> ``fw_step``: the low-level task's six-action MlpPolicy (:class:`ActAStep`)
    act_hl         ``fw_collect_act_hl`` -> ``fw_step`` (``step_low``): the high-level command task's three-action MlpPolicy
                   (:class:`ActHlStep`)
    torch          the torch forward of any policy (:class:`TorchStep`)

Every kind has ``step()``, ``prepare()`` -- what must run once outside a capture: a forward that warms the libraries up, the workspace
initialisation; it changes no env state -- and ``check()`` -- what must be looked at once the stream has drained: ``fw_collect_step``'s
status word.  :func:`select` names the kind for a policy, an env and the caller's ``use_fused``; :func:`make` builds it.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import config as K
from ._lib import stream as _stream
from .rollout import FusedPpoUpdate, clip_actions, policy_inputs

KINDS = ("collect_step", "act_a", "act_hl", "torch")
FUSED_KINDS = KINDS[:3]


def is_highlevel(venv) -> bool:
    """a ``HighLevelCmdVecEnv`` with the 30-value observation: the env of the command figures, of ``highlevel.fly`` and of ``act_hl``"""
    return (hasattr(venv, "command") and hasattr(venv, "step_low") and hasattr(venv, "rejected") and hasattr(venv, "terminal_obs")
            and int(venv.obs.shape[1]) == 30)


def _frozen_on_gpu(env) -> bool:
    return torch.device(env.device).type == "cuda" and not env.training and bool(env.norm_obs)


def _collect_step_applies(policy, env) -> bool:
    venv, dev = env.venv, torch.device(env.device)
    if not (hasattr(venv, "_h") and hasattr(venv, "step_tensor") and _frozen_on_gpu(env) and FusedPpoUpdate.fits(policy, env.obs_dim, dev)):
        return False
    if env.obs_dim > 62:                   # fw_collect_step's act waves take up to 62 features (fits() allows the update's 64)
        return False
    return int(_lib.lib().fw_lanes_per_env(venv._h)) in (8, 16)


def _act_a_applies(policy, env) -> bool:
    """the low-level task's six-action MlpPolicy (either lane mapping)"""
    venv = env.venv
    if not (hasattr(venv, "_h") and hasattr(venv, "step_tensor") and _frozen_on_gpu(env)):
        return False
    if getattr(getattr(venv, "cfg", None), "task", None) != K.FW_TASK_LOWLEVEL:
        return False
    return FusedPpoUpdate.fits(policy, env.obs_dim, torch.device(env.device), act_dims=(6,))


def _act_hl_applies(policy, env) -> bool:
    """the high-level command task's three-action MlpPolicy on its 30-value observation (either lane mapping)"""
    venv = env.venv
    if not (hasattr(venv, "collect_act_hl") and is_highlevel(venv) and _frozen_on_gpu(env) and env.obs_dim == 30):
        return False
    return FusedPpoUpdate.fits(policy, 30, torch.device(env.device), act_dims=(3,))


_APPLIES = {"collect_step": _collect_step_applies, "act_a": _act_a_applies, "act_hl": _act_hl_applies}


def applies(kind: str, policy, env) -> bool:
    """whether the fused ``kind`` can serve ``policy`` on ``env`` (its kernel's shapes, the lane mapping, a frozen normaliser on the GPU)"""
    return _APPLIES[kind](policy, env)


def select(policy, env, use_fused: Optional[bool], accept: Sequence[str], refusal: str, default: Optional[str] = None) -> str:
    """The kind of step for ``policy`` on ``env``.  ``accept``: the fused kinds the caller can drive, in the order they are tried.
    ``use_fused=True``: the first of them that applies, ``ValueError(refusal)`` when none does; ``False``: ``"torch"``; ``None``:
    ``default`` where it applies (the evaluation's ``"collect_step"``; a recorder has none), else ``"torch"``.  Touches no device."""
    if use_fused is None:
        return default if default is not None and applies(default, policy, env) else "torch"
    if not use_fused:
        return "torch"
    for kind in accept:
        if applies(kind, policy, env):
            return kind
    raise ValueError(refusal)


class _Step:
    kind = "torch"

    def __init__(self, policy, env):
        self.policy, self.env, self.venv, self.n, self.dev = policy, env, env.venv, env.num_envs, env.device

    def __call__(self) -> None:
        self.step()

    def prepare(self) -> None:
        pass

    def check(self) -> None:
        pass


class TorchStep(_Step):
    """The torch forward, in its two forms.  The recorders' (``through_wrapper=False``): normalise ``venv.obs`` with the frozen
    statistics, forward, clip, ``venv.step_tensor``.  The evaluation's (``through_wrapper=True``): forward on ``self.obs`` -- the fixed
    buffer the caller sets to a copy of ``env.reset()`` -- then ``env.step``, whose normalised observation is copied back into it;
    ``self.dones`` is the mask that step returned."""

    def __init__(self, policy, env, through_wrapper: bool = False):
        super().__init__(policy, env)
        self.obs = self.dones = None
        self.through_wrapper = bool(through_wrapper)

    @torch.no_grad()
    def actions(self, obs_n: Optional[torch.Tensor] = None, **kw) -> torch.Tensor:
        """the clipped deterministic actions for normalised rows ``obs_n`` (default: ``venv.obs`` normalised here, statistics untouched)"""
        if obs_n is None:
            obs_n = self.env._process_obs(self.venv.obs, update=False)
        a, _, _ = self.policy(obs_n, deterministic=True, **kw, **policy_inputs(self.policy, self.env))
        return clip_actions(a, self.venv).to(self.venv.torch_dtype)

    def step(self) -> None:
        if not self.through_wrapper:
            self.venv.step_tensor(self.actions())
            return
        o, _, self.dones, _, _ = self.env.step(self.actions(self.obs, generator=None))
        self.obs.copy_(o)

    def prepare(self) -> None:
        self.actions()


class _FusedStep(_Step):
    def __init__(self, policy, env):
        super().__init__(policy, env)
        f = FusedPpoUpdate(policy, None, env.obs_dim)
        f.load_params_from_torch()
        self._flat = f.flat                                         # the kernels' parameter image of the frozen policy
        self._logp = torch.zeros(self.n, dtype=torch.float32, device=self.dev)      # (a rollout row the launch fills: unread)


class CollectStep(_FusedStep):
    """act + env step of the four-action policy as ONE ``fw_collect_step`` launch in its deterministic, statistics-frozen form"""
    kind = "collect_step"

    def __init__(self, policy, env):
        super().__init__(policy, env)
        venv, n, dev = self.venv, self.n, self.dev
        self._act_env = torch.full((n, 4), float("nan"), dtype=venv.torch_dtype, device=dev)      # NaN = "not there yet" (fw_collect_step)
        self._act_raw = torch.zeros((n, 4), dtype=torch.float32, device=dev)                     # rollout-buffer rows the launch fills: not looked at
        self._val = torch.zeros(n, dtype=torch.float32, device=dev)
        self._rng = torch.zeros(2, dtype=torch.int64, device=dev)
        nb = int(_lib.lib().fw_collect_step_workspace_bytes(venv._h))
        self._ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)
        self._ws_ready = False

    def prepare(self) -> None:
        """the workspace, initialised once (in front of the first launch, outside any capture)"""
        if not self._ws_ready:
            h = self.venv._h
            _lib.check(_lib.lib().fw_collect_workspace_init(h, self._ws.data_ptr(), self._ws.numel() * 8, _stream(self.dev)), h)
            self._ws_ready = True

    def step(self) -> None:
        env, venv = self.env, self.venv
        self.prepare()
        a = K.FwCollectArgs()
        a.params = self._flat.data_ptr()
        a.obs_mean, a.obs_var, a.obs_count = env.obs_rms.mean.data_ptr(), env.obs_rms.var.data_ptr(), env.obs_rms.count.data_ptr()
        a.returns = env.returns.data_ptr()
        a.ret_mean, a.ret_var, a.ret_count = env.ret_rms.mean.data_ptr(), env.ret_rms.var.data_ptr(), env.ret_rms.count.data_ptr()
        a.rng = self._rng.data_ptr()
        a.act_raw, a.logp, a.value = self._act_raw.data_ptr(), self._logp.data_ptr(), self._val.data_ptr()
        a.act_env = self._act_env.data_ptr()
        a.obs, a.reward = venv.obs.data_ptr(), venv.rewards.data_ptr()
        a.terminated, a.truncated = venv.terminated.data_ptr(), venv.truncated.data_ptr()
        a.terminal_obs, a.info_i32 = venv.terminal_obs.data_ptr(), venv.info.data_ptr()
        a.workspace, a.workspace_bytes = self._ws.data_ptr(), self._ws.numel() * 8
        a.gamma = float(env.gamma)
        a.clip_obs, a.eps_obs, a.clip_reward, a.eps_reward = float(env.clip_obs), float(env.epsilon), float(env.clip_reward), float(env.epsilon)
        a.update_obs, a.update_ret, a.norm_reward, a.deterministic = 0, 0, 0, 1
        _lib.check(_lib.lib().fw_collect_step(venv._h, C.byref(a), _stream(self.dev)), venv._h)

    def check(self) -> None:
        """the status word: a wait inside one of the launches ran out -> the run is void ("returns or raises")"""
        if not self._ws_ready:
            return
        h, stw = self.venv._h, C.c_uint32(0)
        _lib.check(_lib.lib().fw_collect_status(h, self._ws.data_ptr(), self._ws.numel() * 8, C.byref(stw), _stream(self.dev)), h)
        if stw.value:
            raise RuntimeError(f"fw_collect_step: status word {stw.value} during the evaluation; its figures are void")


class ActAStep(_FusedStep):
    """``fw_collect_act_a`` (policy net only, deterministic, frozen statistics, nothing of a previous step to finalise) ->
    ``fw_step``, one after the other on the stream"""
    kind = "act_a"

    def __init__(self, policy, env):
        super().__init__(policy, env)
        self._act_env = torch.zeros((self.n, 6), dtype=self.venv.torch_dtype, device=self.dev)      # the clipped actions fw_step takes
        self._act_raw = torch.zeros((self.n, 6), dtype=torch.float32, device=self.dev)             # (unread)

    def act(self) -> None:
        env, venv = self.env, self.venv
        _lib.collect_act_a(self._flat, venv.obs, self.n, env.obs_dim, 6, env.obs_rms.mean, env.obs_rms.var, env.clip_obs, env.epsilon,
                           nets=1, deterministic=1, env_offset=getattr(venv, "global_env_offset", 0), act_raw=self._act_raw,
                           act_env=self._act_env, logp=self._logp, stream=_stream(self.dev))

    def step(self) -> None:
        self.act()
        self.venv.step_tensor(self._act_env)

    prepare = act            # (one launch outside the capture sets the kernel's attributes; it touches no env state)


class ActHlStep(_FusedStep):
    """``fw_collect_act_hl`` (commander and controller, policy nets only, deterministic, frozen statistics, nothing of a previous step
    to finalise) -> ``fw_step`` (``step_low``), one after the other on the stream"""
    kind = "act_hl"

    def __init__(self, policy, env):
        super().__init__(policy, env)
        self._act_raw = torch.zeros((self.n, 3), dtype=torch.float32, device=self.dev)      # (unread: the env owns command / low_action)

    def step(self) -> None:
        env, venv = self.env, self.venv
        a = K.FwCollectHlArgs()
        a.params, a.nets, a.deterministic = self._flat.data_ptr(), 1, 1
        a.obs_mean, a.obs_var = env.obs_rms.mean.data_ptr(), env.obs_rms.var.data_ptr()
        a.clip_obs, a.eps_obs = float(env.clip_obs), float(env.epsilon)
        a.act_raw, a.logp = self._act_raw.data_ptr(), self._logp.data_ptr()
        venv.collect_act_hl(a)
        venv.step_low()


_CLASSES = {"collect_step": CollectStep, "act_a": ActAStep, "act_hl": ActHlStep}


def make(kind: str, policy, env, through_wrapper: bool = False) -> _Step:
    """the step object of ``kind`` (what :func:`select` returned); ``through_wrapper``: the evaluation's form of the torch forward"""
    return TorchStep(policy, env, through_wrapper) if kind == "torch" else _CLASSES[kind](policy, env)


def replay_flight(env, trace: torch.Tensor, graph_steps: int, body: Callable[[], None], once: Callable[[], None],
                  start_row: Callable[[], torch.Tensor], flag_col: int, finish: Optional[Callable[[], None]] = None):
    """The three recorders' flight, on a side stream: ``env.reset()``; ``start_row()``; ``T = trace.shape[0]`` calls of ``body`` (act,
    step, one trace kernel that fills row k of the device tensor ``trace``) -- ``T // graph_steps`` replays of a hipGraph of
    ``graph_steps`` bodies, captured after ``once()`` has run outside the capture, then the remaining steps eagerly
    (``graph_steps <= 0`` or ``> T``: all of them); ``finish()``, still on the side stream.  Returns the host copies of ``trace`` and of
    the start rows and ``ended_at [N]``: the first step whose ``flag_col`` is not 0, -1 where there is none."""
    dev, T = env.device, int(trace.shape[0])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        env.reset()
        start = start_row()
        reps = T // graph_steps if graph_steps and graph_steps > 0 else 0
        if reps:
            once()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                for _ in range(graph_steps):
                    body()
            for _ in range(reps):
                graph.replay()
        for _ in range(T - reps * (graph_steps if reps else 0)):
            body()
        if finish is not None:
            finish()
    torch.cuda.current_stream(dev).wait_stream(side)
    tr = trace.cpu().numpy()
    done = tr[:, :, flag_col] != 0
    ended_at = np.where(done.any(axis=0), done.argmax(axis=0), -1).astype(np.int64)
    return tr, start.cpu().numpy(), ended_at
