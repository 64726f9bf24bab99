"""Commanding the low-level controller: caller-set heading / altitude / airspeed and the response to them.

The reference trains its low-level controller (train/train_lowlevel_cmd.py) to be driven from above: its high-level env writes
``target_heading`` / ``target_altitude`` / ``target_airspeed`` on every step (train/train_highlevel_cmd.py:164-166) and rebuilds
the observation the policy sees (:169).  Here that input is ``fw_command_ll`` (``FixedwingLowLevelVecEnv.command`` /
``command_tensor``), and ``fw_trace_ll`` records how the controller answers, one row per env and vec-step:

* :func:`step_schedule` builds a piecewise-constant ``[T, N, 3]`` schedule of (psi, h, V) commands;
* :func:`fly` flies a policy through it -- ``fw_command_ll`` -> act -> ``fw_step`` -> ``fw_trace_ll`` per vec-step, replayed as
  hipGraphs on the device -- and returns a :class:`CommandTrace`;
* :func:`response_figures` turns the trace into step-response figures (t90, overshoot, settling time, steady-state error) and the
  run's tracking errors and survival (definitions in DESIGN.md section 2d, "Commanding the controller").
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import config as K

# columns of a trace row (fw_trace_ll): commanded / actual heading, altitude, airspeed, angular-rate norm, flag
TRACE_COLS = ("heading_cmd", "heading", "altitude_cmd", "altitude", "airspeed_cmd", "airspeed", "ang_vel", "flag")
AXES = ("heading", "altitude", "airspeed")
FLOORS = (0.05, 0.5, 0.5)           # smallest |commanded change| that counts as a step: rad, m, m/s
FLAG_RUNNING, FLAG_TERMINATED, FLAG_TRUNCATED = 0, 1, 2
AGENT_DT = 1.0 / 120.0              # the task's agent rate (one Aviary step per agent step at 120 Hz)


def _wrap(a):
    """Python's (a + pi) % (2 pi) - pi: the heading wrap of the env's reward and of the command conditioning."""
    return np.remainder(np.asarray(a, dtype=np.float64) + math.pi, 2 * math.pi) - math.pi


def trace_rows(obs: torch.Tensor, flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N, 8] trace rows of observation rows ``obs`` [N, 21] in double: the torch statement of one fw_trace_ll row."""
    o = obs.to(torch.float64)
    v = torch.sqrt(o[:, 6] * o[:, 6] + o[:, 7] * o[:, 7] + o[:, 8] * o[:, 8])
    w = torch.sqrt(o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] + o[:, 2] * o[:, 2])
    f = torch.zeros_like(v) if flag is None else flag.to(torch.float64)
    return torch.stack([o[:, 18], o[:, 5], o[:, 19], o[:, 11], o[:, 20], v, w, f], dim=1)


def step_schedule(segments: Sequence, num_envs: int, device=None) -> torch.Tensor:
    """The piecewise-constant float64 ``[T, N, 3]`` schedule of ``segments``: ``(n_steps, value)`` pairs in order, ``value`` a
    (psi, h, V) triple for every env or an ``[N, 3]`` array / tensor of per-env commands.  T is the sum of the ``n_steps``."""
    parts = []
    for seg in segments:
        n_steps, value = seg
        n_steps = int(n_steps)
        if n_steps <= 0:
            raise ValueError(f"a segment must last at least one step, got {n_steps}")
        v = torch.as_tensor(value, dtype=torch.float64)
        if v.shape == (3,):
            v = v.expand(num_envs, 3)
        if v.shape != (num_envs, 3):
            raise ValueError(f"a segment's value must have shape (3,) or ({num_envs}, 3), got {tuple(v.shape)}")
        parts.append(v.to(device=device).unsqueeze(0).expand(n_steps, num_envs, 3))
    if not parts:
        raise ValueError("step_schedule needs at least one segment")
    return torch.cat(parts, dim=0).contiguous()


@dataclass
class CommandTrace:
    """What :func:`fly` recorded.  ``trace [T, N, 8]`` (host, float64): per vec-step and env the post-step row (TRACE_COLS); on the
    step that ends an episode it is the terminal observation.  ``start [N, 8]``: the rows after ``env.reset()``.  ``schedule``:
    the ``[T, N, 3]`` commands as given.  ``dt``: seconds per vec-step.  ``ended_at [N]``: the first step whose row carries a
    done flag, -1 if the env flew the whole schedule in one episode."""
    trace: np.ndarray
    start: np.ndarray
    schedule: np.ndarray
    dt: float
    ended_at: np.ndarray


def _check_fly_args(env, schedule) -> int:
    venv = getattr(env, "venv", None)
    cfg = getattr(venv, "cfg", None)
    if cfg is None or cfg.task != K.FW_TASK_LOWLEVEL:
        raise ValueError("fly needs a VecNormalizeDevice around a low-level task env (FW_TASK_LOWLEVEL)")
    if getattr(env, "training", True):
        raise ValueError("fly needs an evaluation normaliser (training=False): the statistics stay frozen")
    if schedule.dim() != 3 or schedule.shape[1:] != (env.num_envs, 3):
        raise ValueError(f"schedule must have shape (T, {env.num_envs}, 3), got {tuple(schedule.shape)}")
    T = int(schedule.shape[0])
    if T <= 0:
        raise ValueError("schedule has no steps")
    if T > int(cfg.lowlevel_max_episode_steps):
        raise ValueError(f"a schedule of {T} steps is longer than an episode ({cfg.lowlevel_max_episode_steps} steps): only "
                         f"a termination may end an episode inside a commanded run")
    return T


def fly(policy, env, schedule: torch.Tensor, use_fused: Optional[bool] = None, graph_steps: int = 8) -> CommandTrace:
    """Fly ``policy`` (deterministic, frozen normaliser statistics) through ``schedule`` ([T, N, 3], see :func:`step_schedule`) on
    ``env``, a ``VecNormalizeDevice(training=False)`` around a low-level task env.  ``env.reset()`` first; then per vec-step k:
    ``fw_command_ll`` (row k of the schedule, conditioned) -> act -> ``fw_step`` -> ``fw_trace_ll`` (row k of the trace).  The act
    is the torch forward (``use_fused`` None / False, as ``evaluate`` does for six actions) or ``fw_collect_act_a``
    (``use_fused=True``, the launch of ``evalstep.ActAStep``).  With ``graph_steps > 0`` the body is captured as a
    hipGraph of that many vec-steps and replayed (the schedule row and the trace row are picked on the device); the steps that do
    not fill a whole graph run eagerly after it.  ``graph_steps <= 0`` runs every step eagerly; both give the same trace bit for
    bit.  T may not exceed the episode length: inside a run only a termination ends an episode."""
    if not torch.is_tensor(schedule):
        schedule = torch.as_tensor(schedule, dtype=torch.float64)
    T = _check_fly_args(env, schedule)
    from . import evalstep
    venv, n, dev = env.venv, env.num_envs, env.device
    kind = evalstep.select(policy, env, use_fused, ("act_a",),
                           "use_fused=True needs the six-action MlpPolicy and an evaluation normaliser (training=False) on the GPU")
    step = evalstep.make(kind, policy, env)
    sched = schedule.to(device=dev, dtype=torch.float64).contiguous()
    L, p = _lib.lib(), _lib.devptr
    step_idx = torch.zeros((), dtype=torch.int64, device=dev)
    trace = torch.zeros((T, n, len(TRACE_COLS)), dtype=torch.float64, device=dev)
    is_f64 = int(venv.obs.dtype == torch.float64)

    def body():
        venv.command_tensor(sched, T, step_idx)
        step()
        _lib.check(L.fw_trace_ll(p(venv.obs), p(venv.terminal_obs), p(venv.terminated), p(venv.truncated), is_f64, n, p(trace), T,
                                 p(step_idx), _lib.stream(dev)))

    # (step.prepare: one act outside the capture warms its libraries / kernel attributes up, the fused act's too; no env state)
    tr, start, ended_at = evalstep.replay_flight(env, trace, graph_steps, body, step.prepare, lambda: trace_rows(venv.obs), 7)
    return CommandTrace(trace=tr, start=start, schedule=schedule.detach().cpu().numpy(), dt=AGENT_DT, ended_at=ended_at)


def _segments(c: np.ndarray):
    """[t0, t1) runs of constant value in the 1-D array ``c``"""
    cuts = [0] + [t for t in range(1, len(c)) if c[t] != c[t - 1]] + [len(c)]
    return list(zip(cuts[:-1], cuts[1:]))


def step_response(c: float, y0: float, y: np.ndarray, floor: float, dt: float, wrap: bool = False) -> Optional[dict]:
    """The figures of one commanded step: command ``c`` held over the rows ``y`` (the actual values of the
    segment's steps, in order), ``y0`` the actual value before it.  None when |delta| does not exceed ``floor``.  Row j of the
    segment is (j + 1) dt after the command took effect."""
    y = np.asarray(y, dtype=np.float64)
    e = c - y
    delta = c - y0
    if wrap:
        e, delta = _wrap(e), float(_wrap(delta))
    if not abs(delta) > floor:
        return None
    ae, ad = np.abs(e), abs(delta)
    L = len(y)
    hit = np.nonzero(ae <= 0.1 * ad)[0]
    t90 = (hit[0] + 1) * dt if len(hit) else math.nan
    overshoot = max(0.0, float(np.max(-math.copysign(1.0, delta) * e))) / ad
    band = max(0.05 * ad, floor)
    out = np.nonzero(ae > band)[0]
    if len(out) == 0:
        settling = dt
    elif out[-1] == L - 1:
        settling = math.nan
    else:
        settling = (out[-1] + 2) * dt
    m = max(1, L // 10)
    return {"delta": float(delta), "t90": float(t90), "overshoot": float(overshoot), "settling": float(settling),
            "ss_error": float(np.mean(ae[L - m:])), "steps": int(L)}


def _median(xs):
    xs = [x for x in xs if math.isfinite(x)]
    return float(np.median(xs)) if xs else math.nan


def response_figures(ct: CommandTrace) -> dict:
    """Step-response and tracking figures of a :class:`CommandTrace` ("Commanding the controller").

    Returns ``{"summary": {...}, "steps": [...]}``.  ``steps``: one record per commanded step (env, axis, t0, t1 and the figures of
    :func:`step_response`).  ``summary``: per axis the number of steps, the fraction that reached 90 %, the medians of t90,
    overshoot, settling time and steady-state error over the steps where they are finite (NaN when none is), the MAE / RMSE of
    the tracking error over every traced step up to each env's first episode end, and ``survival_rate``."""
    tr = np.asarray(ct.trace, dtype=np.float64)
    start = np.asarray(ct.start, dtype=np.float64)
    T, N = tr.shape[0], tr.shape[1]
    ended = np.asarray(ct.ended_at, dtype=np.int64)
    steps = []
    err_abs, err_sq, n_err = np.zeros(3), np.zeros(3), 0
    for i in range(N):
        end = T if ended[i] < 0 else int(ended[i]) + 1          # the ending step's row (its terminal observation) still counts
        n_err += end
        for a in range(3):
            c, y = tr[:end, i, 2 * a], tr[:end, i, 2 * a + 1]
            e = c - y
            if a == 0:
                e = _wrap(e)
            err_abs[a] += float(np.sum(np.abs(e)))
            err_sq[a] += float(np.sum(e * e))
            for t0, t1 in _segments(c):
                y0 = start[i, 2 * a + 1] if t0 == 0 else tr[t0 - 1, i, 2 * a + 1]
                r = step_response(float(c[t0]), float(y0), y[t0:t1], FLOORS[a], ct.dt, wrap=(a == 0))
                if r is not None:
                    steps.append({"env": i, "axis": AXES[a], "t0": t0, "t1": t1, **r})
    summary = {}
    for a, name in enumerate(AXES):
        mine = [s for s in steps if s["axis"] == name]
        summary[f"{name}_steps"] = len(mine)
        summary[f"{name}_reached"] = float(np.mean([math.isfinite(s["t90"]) for s in mine])) if mine else math.nan
        for k in ("t90", "overshoot", "settling", "ss_error"):
            summary[f"{name}_{k}"] = _median([s[k] for s in mine])
        summary[f"{name}_mae"] = err_abs[a] / n_err if n_err else math.nan
        summary[f"{name}_rmse"] = math.sqrt(err_sq[a] / n_err) if n_err else math.nan
    survived = [(ended[i] < 0) or (tr[ended[i], i, 7] == FLAG_TRUNCATED) for i in range(N)]
    summary["survival_rate"] = float(np.mean(survived)) if N else math.nan
    return {"summary": summary, "steps": steps}
