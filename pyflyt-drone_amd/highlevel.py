"""The reference's high-level command task (train/train_highlevel_cmd.py:35-181, ``HighLevelCmdEnv``), vectorised.

A policy outputs (heading, altitude, airspeed) commands; a frozen low-level controller (the six-action ``MlpPolicy`` that
``examples/train_lowlevel_cmd.py`` trains) turns each command into six actuator commands; the waypoint task runs underneath.
Which parts of that the reference states and which this build owns is DESIGN.md section 2e.  A vec-step is three launches on the
env's stream, with no host synchronisation (capturable in a hipGraph):

    fw_command_hl     clip to the action Box, condition (:164-166), low_obs = (obs[:, 0:18], command)
    fw_collect_act_a  the controller: VecNormalize statistics (frozen), policy net, deterministic, clipped to [-1, 1]
    fw_step           the waypoints task under six direct actuator commands (FW_TASK_WAYPOINTS_DIRECT)

With ``controller_hz=120`` (the config's ``control_hz``, the rate the controller was trained at) a vec-step is two launches: the
controller runs inside the step kernel, in front of every Aviary step of the agent step, on the state of that moment:

    fw_command_hl     as above
    fw_step_hl        the same task; per Aviary step the controller's row (attitude, last actuator commands, command) and forward

``condition_command`` restates the first of them in numpy.  A collected vec-step of ``rollout.PPO`` under
``PPOConfig.fused_three_actions`` replaces the first two -- and the policy's own forward and sampling in front of them -- by one
launch, ``fw_collect_act_hl`` (``collect_act_hl``), and steps the base env with ``step_low``.

:func:`fly` records a flight of a commander, one row per env and vec-step (``fw_trace_hl``, :class:`HighLevelTrace`); the
evaluation figures of the task are ``evaluate.EvalResult.command_scalars`` (DESIGN.md section 2e "Evaluation").
"""
from __future__ import annotations

import copy
import ctypes as C
import os
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import torch
from torch import nn

from . import _lib
from . import config as K
from .spaces import Box
from .vec_env import FixedwingWaypointsDirectVecEnv, FusedVecEnv, _VecEnvBase, _devptr

LOW_OBS_DIM = 21          # the low-level task's observation: 18 shared columns + (psi, h, V)
LOW_ACT_DIM = 6
AIRSPEED_HIGH = 30.0      # the action Box's airspeed bound (train/train_highlevel_cmd.py:96-99)


def condition_command(a, dome: float) -> np.ndarray:
    """The conditioned (heading, altitude, airspeed) command of raw high-level actions ``a[..., 3]``, in double: SB3's clip to the
    action Box ``[-pi, 0, 0] .. [pi, dome, 30]`` (train/train_highlevel_cmd.py:97-101), then the env's own conditioning (:164-166:
    heading ``(a + pi) % 2 pi - pi``, altitude clipped to ``[0, dome]``, airspeed clipped to ``[0, 100]``)."""
    a = np.asarray(a, dtype=np.float64)
    low, high = np.array([-np.pi, 0.0, 0.0]), np.array([np.pi, float(dome), AIRSPEED_HIGH])
    b = np.clip(a, low, high)
    out = np.empty_like(b)
    out[..., 0] = (b[..., 0] + np.pi) % (2 * np.pi) - np.pi
    out[..., 1] = np.clip(b[..., 1], 0.0, float(dome))
    out[..., 2] = np.clip(b[..., 2], 0.0, 100.0)
    return out


def _check_controller(policy) -> None:
    """The controller the kernels serve: the 21 -> 64 -> 64 -> 6 ``MlpPolicy``."""
    ok = hasattr(policy, "pi_net") and hasattr(policy, "action_net") and isinstance(policy.action_net, nn.Linear)
    if ok:
        lin = [m for m in policy.pi_net if isinstance(m, nn.Linear)]
        act = [m for m in policy.pi_net if not isinstance(m, nn.Linear)]
        ok = (len(lin) == 2 and len(act) == 2 and all(isinstance(m, nn.Tanh) for m in act)
              and (lin[0].in_features, lin[0].out_features) == (LOW_OBS_DIM, 64) and (lin[1].in_features, lin[1].out_features) == (64, 64)
              and (policy.action_net.in_features, policy.action_net.out_features) == (64, LOW_ACT_DIM))
    if not ok:
        raise ValueError("the low-level controller must be the 21 -> 64 -> 64 -> 6 MlpPolicy (rollout.MlpPolicy(21, 6): what "
                         "examples/train_lowlevel_cmd.py trains)")


def _rms_arrays(rms):
    """(mean, var) as float64 numpy arrays from a RunningMeanStd, a ``{"mean", "var"}`` mapping or a ``(mean, var)`` pair."""
    if hasattr(rms, "mean") and hasattr(rms, "var"):
        m, v = rms.mean, rms.var
    elif isinstance(rms, dict):
        m, v = rms["mean"], rms["var"]
    else:
        m, v = rms
    m, v = (np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float64).reshape(-1) for x in (m, v))
    if m.shape != (LOW_OBS_DIM,) or v.shape != (LOW_OBS_DIM,):
        raise ValueError(f"the low-level observation statistics must have {LOW_OBS_DIM} entries, got {m.shape[0]} and {v.shape[0]}")
    return m, v


def load_low_checkpoint(path: str):
    """(policy, (mean, var), clip_obs, epsilon) of a checkpoint written by ``checkpoint.save`` (``examples/train_lowlevel_cmd.py``:
    ``final_model.pt`` / ``best_model.pt``).  A missing file raises ``FileNotFoundError`` as the reference does (:110-121)."""
    from .rollout import MlpPolicy
    if not os.path.exists(path):
        raise FileNotFoundError(f"low-level controller checkpoint not found: {path}; train the low-level controller first "
                                "(examples/train_lowlevel_cmd.py)")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if "policy" not in sd or "vecnormalize" not in sd:
        raise ValueError(f"{path} is not a training checkpoint (no policy / vecnormalize entries)")
    w1, wo = sd["policy"].get("pi_net.0.weight"), sd["policy"].get("action_net.weight")
    if w1 is None or wo is None or tuple(w1.shape) != (64, LOW_OBS_DIM) or tuple(wo.shape) != (LOW_ACT_DIM, 64):
        raise ValueError(f"{path} does not hold the 21 -> 64 -> 64 -> 6 MlpPolicy of the low-level task")
    policy = MlpPolicy(LOW_OBS_DIM, LOW_ACT_DIM)
    policy.load_state_dict(sd["policy"])
    vn = sd["vecnormalize"]
    return policy, _rms_arrays(vn["obs_rms"]), float(vn.get("clip_obs", 10.0)), float(vn.get("epsilon", 1e-8))


CONTROL_HZ = 120          # the config's control_hz: one Aviary step, the rate the low-level task runs its controller at


def check_controller_hz(controller_hz: Optional[int], agent_hz: int) -> bool:
    """True when the controller runs at the control rate inside the step (``controller_hz == 120 != agent_hz``), False for the
    reference's once-per-agent-step controller (``None`` or ``agent_hz``); any other rate raises ``ValueError``."""
    if controller_hz is None:
        return False
    if isinstance(controller_hz, bool) or int(controller_hz) != controller_hz:
        raise ValueError(f"controller_hz must be None, agent_hz ({agent_hz}) or {CONTROL_HZ}, got {controller_hz!r}")
    if int(controller_hz) == int(agent_hz):
        return False
    if int(controller_hz) == CONTROL_HZ:
        return True
    raise ValueError(f"controller_hz must be None, agent_hz ({agent_hz}) or {CONTROL_HZ}, got {controller_hz!r}")


class HighLevelCmdVecEnv(FusedVecEnv):
    """``HighLevelCmdEnv`` x N on one MI355X: three actions in the reference's Box (``action_low`` / ``action_high``), the
    30-value observation of the base env, its reward, termination, truncation and info.

    ``low_policy`` + ``low_obs_rms`` (a ``RunningMeanStd``, a ``{"mean", "var"}`` mapping or a ``(mean, var)`` pair), or
    ``low_checkpoint`` (a file ``examples/train_lowlevel_cmd.py`` saved), give the frozen controller; the policy is copied.  The other
    keywords are the reference constructor's.  ``low_action`` holds the controller's clipped output of the last step,
    ``command`` the conditioned triple, ``low_obs`` the controller's raw observation.

    ``controller_hz``: the rate the controller runs at.  ``None`` or ``agent_hz``: once per agent step, its six commands held for
    the Aviary steps of the agent step (the reference's behaviour).  ``120`` (the config's ``control_hz``): once per Aviary step,
    inside the step kernel (``fw_step_hl``) -- the rate ``examples/train_lowlevel_cmd.py`` trains it at; ``low_action`` is then the
    output of the last Aviary step, ``low_obs`` the row ``fw_command_hl`` wrote.  Anything else raises ``ValueError``.  The knob is a
    constructor argument, not state: a checkpoint moves across it."""

    metadata = {"render_modes": ["human", "rgb_array"], "render_fps": 30}

    def __init__(self, num_envs: int, low_policy=None, low_obs_rms=None, *, low_checkpoint: Optional[str] = None,
                 clip_obs: float = 10.0, epsilon: float = 1e-8, render_mode: Optional[str] = None, flight_dome_size: float = 200.0,
                 max_duration_seconds: float = 120.0, agent_hz: int = 30, context_length: int = 2, wind_config: Optional[dict] = None,
                 dtype: str = "float64", motor_noise: bool = True, device=None, seed: int = 0, global_env_offset: int = 0,
                 controller_hz: Optional[int] = None):
        if render_mode is not None:
            raise ValueError(f"Invalid render mode {render_mode}, rendering is not part of the device env.")
        self.controller_in_step = check_controller_hz(controller_hz, agent_hz)
        # ---- the controller: everything that needs no device first ----
        if low_checkpoint is not None:
            if low_policy is not None or low_obs_rms is not None:
                raise ValueError("give either low_checkpoint or low_policy + low_obs_rms")
            low_policy, (mean, var), clip_obs, epsilon = load_low_checkpoint(low_checkpoint)
        else:
            if low_policy is None or low_obs_rms is None:
                raise ValueError("HighLevelCmdVecEnv needs the low-level controller: low_policy + low_obs_rms, or low_checkpoint")
            _check_controller(low_policy)
            mean, var = _rms_arrays(low_obs_rms)
        _check_controller(low_policy)
        if wind_config is not None and not bool(wind_config.get("enabled", False)):
            wind_config = None                                       # (:86-87)
        self.base = FixedwingWaypointsDirectVecEnv(
            num_envs, flight_dome_size=flight_dome_size, max_duration_seconds=max_duration_seconds, agent_hz=agent_hz,
            context_length=context_length, angle_representation="euler", wind_config=wind_config, dtype=dtype,
            motor_noise=motor_noise, device=device, seed=seed, global_env_offset=global_env_offset)
        b = self.base
        self.device, self.cfg, self.num_envs = b.device, b.cfg, b.num_envs
        self.obs_dim, self.act_dim = b.obs_dim, 3
        self.np_dtype, self.torch_dtype = b.np_dtype, b.torch_dtype
        self.global_env_offset, self.lanes_per_env = b.global_env_offset, b.lanes_per_env
        self.render_mode = None
        self.clip_obs, self.epsilon = float(clip_obs), float(epsilon)
        low = np.array([-np.pi, 0.0, 0.0], dtype=np.float32)
        high = np.array([np.pi, flight_dome_size, AIRSPEED_HIGH], dtype=np.float32)
        _VecEnvBase.__init__(self, self.num_envs, Box(-np.inf, np.inf, (self.obs_dim,), self.np_dtype), Box(low, high, (3,), np.float32))
        dev, n = self.device, self.num_envs
        self.action_low, self.action_high = torch.as_tensor(low, device=dev), torch.as_tensor(high, device=dev)
        # the frozen controller: a copy of the module (what the tests' torch forward uses) and the kernels' flat parameter image
        from .rollout import FusedPpoUpdate
        self.low_policy = copy.deepcopy(low_policy).to(dev).eval()
        for p in self.low_policy.parameters():
            p.requires_grad_(False)
        f = FusedPpoUpdate(self.low_policy, None, LOW_OBS_DIM)
        f.load_params_from_torch()
        self._flat = f.flat
        self.low_mean = torch.as_tensor(mean, dtype=torch.float64, device=dev)
        self.low_var = torch.as_tensor(var, dtype=torch.float64, device=dev)
        self.low_obs = torch.zeros((n, LOW_OBS_DIM), dtype=self.torch_dtype, device=dev)
        self.low_action = torch.zeros((n, LOW_ACT_DIM), dtype=self.torch_dtype, device=dev)
        self.command = torch.zeros((n, 3), dtype=self.torch_dtype, device=dev)
        self.rejected = torch.zeros(1, dtype=torch.int32, device=dev)       # rows with a non-finite action so far (they kept their command)
        self._act_raw = torch.zeros((n, LOW_ACT_DIM), dtype=torch.float32, device=dev)
        self._logp = torch.zeros(n, dtype=torch.float32, device=dev)
        self._actions_dev = torch.zeros((n, 3), dtype=self.torch_dtype, device=dev)
        self.controller_hz = CONTROL_HZ if self.controller_in_step else int(agent_hz)

    # the base env's output tensors are this env's
    obs = property(lambda self: self.base.obs)
    rewards = property(lambda self: self.base.rewards)
    terminated = property(lambda self: self.base.terminated)
    truncated = property(lambda self: self.base.truncated)
    terminal_obs = property(lambda self: self.base.terminal_obs)
    info = property(lambda self: self.base.info)
    seed_value = property(lambda self: self.base.seed_value)

    # ------------------------------------------------------------------ device fast path
    def reset_tensor(self, mask: Optional[torch.Tensor] = None, scenario: Optional[dict] = None) -> torch.Tensor:
        return self.base.reset_tensor(mask, scenario)

    def observe_tensor(self) -> torch.Tensor:
        return self.base.observe_tensor()

    def step_tensor(self, actions: torch.Tensor):
        """One agent step from raw high-level actions ``[N, 3]`` (float32 or float64 device tensor; anything else is converted to
        the env dtype): ``fw_command_hl -> fw_collect_act_a -> fw_step`` on the current stream (``controller_hz=120``:
        ``fw_command_hl -> fw_step_hl``).  Returns the base env's ``(obs, rewards, terminated, truncated)``."""
        b, L, n = self.base, _lib.lib(), self.num_envs
        if actions.device != self.device or actions.dtype not in (torch.float32, torch.float64) or not actions.is_contiguous():
            dt = actions.dtype if actions.dtype in (torch.float32, torch.float64) else self.torch_dtype
            actions = actions.to(device=self.device, dtype=dt).contiguous()
        if actions.shape != (n, 3):
            raise ValueError(f"actions must have shape ({n}, 3), got {tuple(actions.shape)}")
        st = b._stream()
        _lib.check(L.fw_command_hl(b._h, _devptr(actions), int(actions.dtype == torch.float64), None, _devptr(b.obs),
                                   _devptr(self.low_obs), _devptr(self.command), _devptr(self.rejected), st), b._h)
        if self.controller_in_step:
            return self.step_low()
        # the controller: policy net only, deterministic, frozen statistics, nothing of a previous step to finalise
        _lib.collect_act_a(self._flat, self.low_obs, n, LOW_OBS_DIM, LOW_ACT_DIM, self.low_mean, self.low_var, self.clip_obs, self.epsilon,
                           nets=1, deterministic=1, env_offset=self.global_env_offset, act_raw=self._act_raw, act_env=self.low_action,
                           logp=self._logp, stream=st)
        return b.step_tensor(self.low_action)

    # ------------------------------------------------------------------ the fused collector (rollout.PPO, fused_three_actions)
    def collect_act_hl(self, a: "K.FwCollectHlArgs") -> None:
        """The act side of a collected vec-step in one launch (``fw_collect_act_hl``) on the current stream.  The caller fills the
        commander's half of ``a`` -- its flat image, the statistics of its observation, ``nets`` / ``deterministic`` / ``rng``, the
        rollout rows, the previous-step block; the env adds its own: the raw observation buffer, the controller's image and frozen
        statistics, ``low_obs`` / ``command`` / ``low_action`` / ``rejected``.  ``step_low`` then steps the base env with
        ``low_action``.  ``nets == 2`` (the end of a rollout) runs the value block only and leaves the env's tensors alone."""
        b = self.base
        a.obs, a.env_offset = b.obs.data_ptr(), int(self.global_env_offset)
        a.low_params, a.low_mean, a.low_var = self._flat.data_ptr(), self.low_mean.data_ptr(), self.low_var.data_ptr()
        a.low_clip, a.low_eps = self.clip_obs, self.epsilon
        a.low_obs, a.cmd_out, a.act_env = self.low_obs.data_ptr(), self.command.data_ptr(), self.low_action.data_ptr()
        a.rejected = self.rejected.data_ptr()
        _lib.check(_lib.lib().fw_collect_act_hl(b._h, C.byref(a), b._stream()), b._h)

    def step_low(self):
        """``fw_step`` of the base env with ``low_action`` as it stands (the controller's output of ``collect_act_hl``): the second
        half of a vec-step whose act side has already run.  With ``controller_hz=120`` it is ``fw_step_hl``: the command the act
        side left in the env's tail is flown with the controller inside the kernel, and ``low_action`` is an output.  Returns the
        base env's ``(obs, rewards, terminated, truncated)``."""
        b = self.base
        if not self.controller_in_step:
            return b.step_tensor(self.low_action)
        a = K.FwStepHlArgs()
        a.low_params, a.low_mean, a.low_var = self._flat.data_ptr(), self.low_mean.data_ptr(), self.low_var.data_ptr()
        a.low_clip, a.low_eps = self.clip_obs, self.epsilon
        a.obs, a.reward, a.terminated, a.truncated = b.obs.data_ptr(), b.rewards.data_ptr(), b.terminated.data_ptr(), b.truncated.data_ptr()
        a.terminal_obs, a.info_i32, a.low_action = b.terminal_obs.data_ptr(), b.info.data_ptr(), self.low_action.data_ptr()
        _lib.check(_lib.lib().fw_step_hl(b._h, C.byref(a), b._stream()), b._h)
        return b.obs, b.rewards, b.terminated, b.truncated

    # ------------------------------------------------------------------ SB3 VecEnv surface (numpy)
    def reset(self) -> np.ndarray:
        obs = self.base.reset()
        self.reset_infos = [{} for _ in range(self.num_envs)]
        return obs

    def _finish_step(self):
        obs, rewards, dones, infos = self.base._finish_step()
        cmd = self.command.cpu().numpy().astype(np.float64)
        for i, d in enumerate(infos):
            d["command"] = cmd[i].copy()
        return obs, rewards, dones, infos

    def seed(self, seed: Optional[int] = None):
        self._seeds = self.base.seed(seed)
        return self._seeds

    def close(self) -> None:
        b = self.__dict__.get("base")
        if b is not None:
            b.close()

    def _inherited_attr(self, attr_name: str) -> Any:
        """What is not this env's own is the base env's (its attributes, then the fields of its fw_config)."""
        if "base" not in self.__dict__:
            raise AttributeError(f"{type(self).__name__} envs have no attribute {attr_name!r}")
        return self.base.get_attr(attr_name, 0)[0]

    # ------------------------------------------------------------------ state access (parity tests / checkpoints)
    def get_state(self) -> np.ndarray:
        return self.base.get_state()

    def set_state(self, state: np.ndarray) -> None:
        self.base.set_state(state)

    def get_counters(self) -> dict:
        return self.base.get_counters()


# ---------------------------------------------------------------------- the flight record (fw_trace_hl)
# columns of a trace row: commanded / actual heading, altitude, airspeed, angular-rate norm, roll, pitch, waypoints reached, flag
HL_TRACE_COLS = ("heading_cmd", "heading", "altitude_cmd", "altitude", "airspeed_cmd", "airspeed", "ang_vel", "roll", "pitch",
                 "targets_reached", "flag")
FLAG_RUNNING, FLAG_TERMINATED, FLAG_TRUNCATED = 0, 1, 2


def trace_rows_hl(obs: torch.Tensor, cmd: torch.Tensor, info: Optional[torch.Tensor] = None,
                  flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N, 11] trace rows (HL_TRACE_COLS) of observation rows ``obs`` [N, 30] and conditioned commands ``cmd`` [N, 3], in double:
    the torch statement of one fw_trace_hl row.  ``info`` [N, >= 1] int rows (None: 0 waypoints reached), ``flag`` [N] (None: 0)."""
    o, c = obs.to(torch.float64), cmd.to(torch.float64)
    v = torch.sqrt(o[:, 6] * o[:, 6] + o[:, 7] * o[:, 7] + o[:, 8] * o[:, 8])
    w = torch.sqrt(o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] + o[:, 2] * o[:, 2])
    r = torch.zeros_like(v) if info is None else info[:, K.INFO_NUM_TARGETS_REACHED].to(torch.float64)
    f = torch.zeros_like(v) if flag is None else flag.to(torch.float64)
    return torch.stack([c[:, 0], o[:, 5], c[:, 1], o[:, 11], c[:, 2], v, w, o[:, 9], o[:, 10], r, f], dim=1)


@dataclass
class HighLevelTrace:
    """What :func:`fly` recorded.  ``trace [T, N, 11]`` (host, float64): per vec-step and env the post-step row (HL_TRACE_COLS) -- on
    the step that ends an episode the terminal observation -- with the conditioned command that was in force during the step.
    ``start [N, 11]``: the rows after ``env.reset()``, their command the one the env holds then (0, start height, start speed).
    ``dt``: seconds per vec-step.  ``ended_at [N]``: the first step whose row carries a done flag, -1 if the env flew all T steps
    in one episode (the rows behind it belong to the env's next episodes)."""
    trace: np.ndarray
    start: np.ndarray
    dt: float
    ended_at: np.ndarray


def fly(policy, env, n_steps: int, use_fused: Optional[bool] = None, graph_steps: int = 8) -> HighLevelTrace:
    """Fly the commander ``policy`` (deterministic, frozen normaliser statistics) for ``n_steps`` vec-steps on ``env``, a
    ``VecNormalizeDevice(training=False)`` around a :class:`HighLevelCmdVecEnv` with the 30-value observation.  ``env.reset()``
    first; then per vec-step k: act -> step -> ``fw_trace_hl`` (row k of the trace).  The act is the torch forward followed by
    ``step_tensor`` (``use_fused`` None / False) or ``fw_collect_act_hl`` followed by ``step_low`` (``use_fused=True``, the launches
    of ``evalstep.ActHlStep``).  With ``graph_steps > 0`` the body is captured as a hipGraph of that many vec-steps and
    replayed (the trace row is picked on the device); the steps that do not fill a whole graph run eagerly after it.
    ``graph_steps <= 0`` runs every step eagerly; both give the same trace bit for bit."""
    from . import evalstep
    venv = getattr(env, "venv", None)
    if venv is None or not evalstep.is_highlevel(venv):
        raise ValueError("fly needs a VecNormalizeDevice around a HighLevelCmdVecEnv with the 30-value observation")
    if getattr(env, "training", True):
        raise ValueError("fly needs an evaluation normaliser (training=False): the statistics stay frozen")
    T = int(n_steps)
    if T <= 0:
        raise ValueError(f"n_steps must be positive, got {n_steps}")
    n, dev = env.num_envs, env.device
    kind = evalstep.select(policy, env, use_fused, ("act_hl",),
                           "use_fused=True needs the three-action MlpPolicy and an evaluation normaliser (training=False) on the GPU")
    step = evalstep.make(kind, policy, env)
    L = _lib.lib()
    step_idx = torch.zeros((), dtype=torch.int64, device=dev)
    trace = torch.zeros((T, n, len(HL_TRACE_COLS)), dtype=torch.float64, device=dev)
    is_f64 = int(venv.obs.dtype == torch.float64)

    def body():
        step()
        _lib.check(L.fw_trace_hl(_devptr(venv.obs), _devptr(venv.terminal_obs), _devptr(venv.terminated), _devptr(venv.truncated),
                                 _devptr(venv.command), _devptr(venv.info), int(venv.info.shape[1]), is_f64, n, _devptr(trace), T,
                                 _devptr(step_idx), _lib.stream(dev)))

    def start_row():
        torch.cuda.current_stream(dev).synchronize()      # (the side stream the flight runs on: get_state copies on the default stream)
        stored = torch.as_tensor(venv.get_state()[:, K.S_TASK:K.S_TASK + 3], dtype=torch.float64, device=dev)   # the FW_SL_TARGET tail
        return trace_rows_hl(venv.obs, stored)

    tr, start, ended_at = evalstep.replay_flight(env, trace, graph_steps, body, step.prepare, start_row, len(HL_TRACE_COLS) - 1)
    return HighLevelTrace(trace=tr, start=start, dt=1.0 / float(venv.cfg.agent_hz), ended_at=ended_at)
