"""Flight records and path figures of the waypoint and duck tasks: what ``command.fly`` / ``highlevel.fly`` and
their evaluation figures are to the two controller tasks, for Fixedwing-Waypoints, ObjLock, the combined waypoint -> duck task and
the direct-command waypoints task.

* :func:`fly` records a flight, one row per env and vec-step (``fw_trace_rows``, :class:`FlightTrace`): the post-step observation row
  as it is, the waypoints reached so far and the done flag.  The kernel copies; :class:`RowLayout` says which column is what.
* :func:`path_step` is the torch statement of one ``fw_eval_track_wp`` update -- twelve per-episode path sums (``PATH_SUMS``) carried on
  the device inside the replayed evaluation (``evaluate_policy(path_figures=True)``); :func:`path_figures` computes the same sums
  from a recorded trace in plain numpy, written independently of it.

The reference looks at the flight in ``utils/vis.py`` (the A -> B path against the straight line), in the HUD of ``envs/utils.py:21-45``
(altitude, airspeed, thrust, targets remaining, distance to target) and in ``train/train_ppo_ab.py:88`` ("success rate and arrival
time"); the figures here are build-owned definitions of those quantities.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import config as K
from ._lib import devptr as _devptr

# the per-episode path sums, in the column order of fw_eval_track_wp's cur_path / fin_path
PATH_SUMS = ("path_len", "speed_sum", "alt_sum", "alt_min", "ang_vel_sum", "act_delta_sum", "throttle_sum", "first_reach_step",
             "last_reach_step", "chord_len", "path_at_last_reach", "miss_dist")
(PS_PATH_LEN, PS_SPEED, PS_ALT, PS_ALT_MIN, PS_ANG_VEL, PS_ACT_DELTA, PS_THROTTLE, PS_FIRST_REACH, PS_LAST_REACH, PS_CHORD,
 PS_PATH_AT_REACH, PS_MISS) = range(12)
CARRY_DIM = 13            # p_prev[3], p_leg[3], a_prev[6], reached_prev
FLAG_RUNNING, FLAG_TERMINATED, FLAG_TRUNCATED = 0, 1, 2
_PATH_TASKS = (K.FW_TASK_WAYPOINTS, K.FW_TASK_OBJLOCK, K.FW_TASK_WAYPOINT_OBJLOCK, K.FW_TASK_WAYPOINTS_DIRECT)


@dataclass(frozen=True)
class RowLayout:
    """Where things sit in a flattened observation row (the oracle's ``flatten_obs``; envs/flatten_waypoint_env.py:52-72): angular velocity, attitude (three Euler
    angles, or the quaternion in the observation's own order x, y, z, w), body-frame velocity, position, the action block, the six
    actuator states (the last is the throttle) and, when the row is long enough, the first target row -- the current waypoint, the
    duck for ObjLock (``target_vector``), the duck once the waypoints are done for the combined task."""
    obs_dim: int
    att_dim: int          # 12 (euler) | 13 (quaternion): the columns up to and including the position
    act_dim: int          # 4 | 6

    @classmethod
    def of(cls, cfg) -> "RowLayout":
        task = int(cfg.task)
        if task not in _PATH_TASKS:
            raise ValueError("RowLayout.of: the waypoint, ObjLock, combined and direct-command waypoints tasks only (the low-level "
                             "task's 21-value row has its own figures)")
        return cls(obs_dim=int(K.obs_dim(cfg)), att_dim=12 if int(cfg.angle_representation) == 0 else 13, act_dim=int(K.act_dim(cfg)))

    def __post_init__(self):
        if self.att_dim not in (12, 13) or self.act_dim not in (4, 6) or self.obs_dim < self.att_dim + self.act_dim + 6:
            raise ValueError(f"RowLayout: att_dim 12 | 13, act_dim 4 | 6 and obs_dim >= att_dim + act_dim + 6, got {self}")

    ang_vel = property(lambda self: slice(0, 3))
    attitude = property(lambda self: slice(3, self.att_dim - 6))
    velocity = property(lambda self: slice(self.att_dim - 6, self.att_dim - 3))
    position = property(lambda self: slice(self.att_dim - 3, self.att_dim))
    action = property(lambda self: slice(self.att_dim, self.att_dim + self.act_dim))
    actuators = property(lambda self: slice(self.att_dim + self.act_dim, self.att_dim + self.act_dim + 6))
    throttle = property(lambda self: self.att_dim + self.act_dim + 5)
    has_target = property(lambda self: self.obs_dim >= self.att_dim + self.act_dim + 9)
    target = property(lambda self: slice(self.att_dim + self.act_dim + 6, self.att_dim + self.act_dim + 9) if self.has_target else None)
    quaternion = property(lambda self: self.att_dim == 13)

    def columns(self) -> dict:
        """name -> (first, one past last) column, for a saved trace"""
        out = {"ang_vel": (0, 3), "attitude": (3, self.att_dim - 6), "velocity": (self.att_dim - 6, self.att_dim - 3),
               "position": (self.att_dim - 3, self.att_dim), "action": (self.att_dim, self.att_dim + self.act_dim),
               "actuators": (self.att_dim + self.act_dim, self.att_dim + self.act_dim + 6),
               "targets_reached": (self.obs_dim, self.obs_dim + 1), "flag": (self.obs_dim + 1, self.obs_dim + 2)}
        if self.has_target:
            out["target"] = (self.att_dim + self.act_dim + 6, self.att_dim + self.act_dim + 9)
        return out


def _norm3(x: torch.Tensor) -> torch.Tensor:
    return torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])      # the kernel's plain sum of squares


def path_init(n: int, device=None) -> torch.Tensor:
    """[n, 12] sums of episodes that have not begun: zeros, ``alt_min`` and ``miss_dist`` +inf (what fw_eval_track_wp leaves behind a
    finished episode)"""
    cur = torch.zeros((n, len(PATH_SUMS)), dtype=torch.float64, device=device)
    cur[:, PS_ALT_MIN] = math.inf
    cur[:, PS_MISS] = math.inf
    return cur


def seed_carry(obs: torch.Tensor, layout: RowLayout) -> torch.Tensor:
    """The ``[N, 13]`` carry (p_prev, p_leg, a_prev[6], reached_prev) of episodes whose first observation is ``obs``: both positions
    the row's, a_prev its action block (zero-padded to six), nothing reached.  In double."""
    o = obs.to(torch.float64)
    c = torch.zeros((o.shape[0], CARRY_DIM), dtype=torch.float64, device=o.device)
    c[:, 0:3] = o[:, layout.position]
    c[:, 3:6] = o[:, layout.position]
    c[:, 6:6 + layout.act_dim] = o[:, layout.action]
    return c


def path_step(row: torch.Tensor, reached: Optional[torch.Tensor], first: torch.Tensor, cur: torch.Tensor, carry: torch.Tensor,
              layout: RowLayout, length: Optional[torch.Tensor] = None):
    """The torch statement of one ``fw_eval_track_wp`` update, in double, on any device.  ``row`` [N, obs_dim]: the post-step rows
    (the terminal observation where the episode ended; float32 rows are widened first), ``reached`` [N]: ``info[:, 0]`` as the step
    left it (None: 0), ``first`` [N] bool: the step opens an episode (``cur_len == 0`` before it: the sums restart),
    ``cur`` [N, 12], ``carry`` [N, 13], ``length`` [N]: L, the number of the step inside its episode (``cur_len + 1``), what the two
    reach-step columns record -- without it ``first`` must be the integer ``cur_len`` before the step itself, and both are derived.
    Returns ``(sums, carry)`` after the step, the carry as for an episode that goes on; where one ended the caller records the sums
    and re-seeds the carry from the live row (:func:`seed_carry`)."""
    o, cur, carry = row.to(torch.float64), cur.to(torch.float64), carry.to(torch.float64)
    n, dev = o.shape[0], o.device
    if length is None:
        if first.dtype == torch.bool:
            raise ValueError("path_step: give length (cur_len + 1), or pass cur_len itself as first")
        first, length = first == 0, first + 1
    L = length.to(device=dev, dtype=torch.float64)
    r = torch.zeros(n, dtype=torch.float64, device=dev) if reached is None else reached.to(device=dev, dtype=torch.float64)
    s = torch.where(first.to(dev)[:, None], path_init(n, dev), cur).clone()
    p, a = o[:, layout.position], o[:, layout.action]
    reach = r > carry[:, 12]
    s[:, PS_PATH_LEN] = s[:, PS_PATH_LEN] + _norm3(p - carry[:, 0:3])
    s[:, PS_SPEED] = s[:, PS_SPEED] + _norm3(o[:, layout.velocity])
    s[:, PS_ALT] = s[:, PS_ALT] + p[:, 2]
    s[:, PS_ALT_MIN] = torch.where(p[:, 2] < s[:, PS_ALT_MIN], p[:, 2], s[:, PS_ALT_MIN])
    s[:, PS_ANG_VEL] = s[:, PS_ANG_VEL] + _norm3(o[:, layout.ang_vel])
    da = torch.zeros(n, dtype=torch.float64, device=dev)
    for j in range(layout.act_dim):
        da = da + (a[:, j] - carry[:, 6 + j]).abs()
    s[:, PS_ACT_DELTA] = s[:, PS_ACT_DELTA] + da
    s[:, PS_THROTTLE] = s[:, PS_THROTTLE] + o[:, layout.throttle]
    s[:, PS_FIRST_REACH] = torch.where(reach & (s[:, PS_FIRST_REACH] == 0.0), L, s[:, PS_FIRST_REACH])
    s[:, PS_LAST_REACH] = torch.where(reach, L, s[:, PS_LAST_REACH])
    s[:, PS_CHORD] = torch.where(reach, s[:, PS_CHORD] + _norm3(p - carry[:, 3:6]), s[:, PS_CHORD])
    s[:, PS_PATH_AT_REACH] = torch.where(reach, s[:, PS_PATH_LEN], s[:, PS_PATH_AT_REACH])
    miss = s[:, PS_MISS]
    if layout.has_target:
        d = _norm3(o[:, layout.target])
        miss = torch.where(d < miss, d, miss)
    s[:, PS_MISS] = torch.where(reach, torch.full_like(miss, math.inf), miss)
    c = carry.clone()
    c[:, 0:3] = p
    c[:, 3:6] = torch.where(reach[:, None], p, carry[:, 3:6])
    c[:, 6:6 + layout.act_dim] = a
    c[:, 12] = r
    return s, c


# ---------------------------------------------------------------------- the flight record (fw_trace_rows)
def trace_rows(obs: torch.Tensor, info: Optional[torch.Tensor] = None, flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N, D + 2] trace rows of observation rows ``obs`` [N, D], in double: the torch statement of one fw_trace_rows row.  ``info``
    [N, >= 1] int rows (None: 0 waypoints reached), ``flag`` [N] (None: 0)."""
    o = obs.to(torch.float64)
    z = torch.zeros(o.shape[0], dtype=torch.float64, device=o.device)
    r = z if info is None else info[:, K.INFO_NUM_TARGETS_REACHED].to(torch.float64)
    f = z if flag is None else flag.to(torch.float64)
    return torch.cat([o, r[:, None], f[:, None]], dim=1)


def _euler_from_quat(q: np.ndarray) -> np.ndarray:
    """(roll, pitch, yaw) of quaternions ``q[..., 4]`` in the observation's order (x, y, z, w): Bullet's getEulerFromQuaternion, with
    its branches at the poles, in numpy"""
    x, y, z, w = (q[..., k] for k in range(4))
    sarg = -2.0 * (x * z - w * y)
    roll = np.arctan2(2.0 * (y * z + w * x), w * w - x * x - y * y + z * z)
    pitch = np.arcsin(np.clip(sarg, -1.0, 1.0))
    yaw = np.arctan2(2.0 * (x * y + w * z), w * w + x * x - y * y - z * z)
    lo, hi = sarg <= -0.99999, sarg >= 0.99999
    roll = np.where(lo | hi, 0.0, roll)
    pitch = np.where(lo, -0.5 * math.pi, np.where(hi, 0.5 * math.pi, pitch))
    yaw = np.where(lo, 2.0 * np.arctan2(x, -y), np.where(hi, 2.0 * np.arctan2(-x, y), yaw))
    return np.stack([roll, pitch, yaw], axis=-1)


@dataclass
class FlightTrace:
    """What :func:`fly` recorded.  ``trace [T, N, D + 2]`` (host, float64): per vec-step and env the post-step observation row -- on
    the step that ends an episode the terminal observation -- then the waypoints reached so far and the done flag (0 running,
    1 terminated, 2 truncated).  ``start [N, D + 2]``: the rows after ``env.reset()``.  ``dt``: seconds per vec-step.
    ``ended_at [N]``: the first step whose row carries a done flag, -1 if the env flew all T steps in one episode (the rows behind it
    belong to the env's next episodes).  ``layout``: which column is what.  The accessors take ``rows`` -- the whole trace by default,
    or any array whose last axis is a trace row (``start``, an :meth:`episode`)."""
    trace: np.ndarray
    start: np.ndarray
    dt: float
    ended_at: np.ndarray
    layout: RowLayout

    def _rows(self, rows):
        return self.trace if rows is None else np.asarray(rows)

    def position(self, rows=None) -> np.ndarray:
        return self._rows(rows)[..., self.layout.position]

    def airspeed(self, rows=None) -> np.ndarray:
        return np.linalg.norm(self._rows(rows)[..., self.layout.velocity], axis=-1)

    def attitude_euler(self, rows=None) -> np.ndarray:
        a = self._rows(rows)[..., self.layout.attitude]
        return _euler_from_quat(a) if self.layout.quaternion else a

    def throttle(self, rows=None) -> np.ndarray:
        return self._rows(rows)[..., self.layout.throttle]

    def actions(self, rows=None) -> np.ndarray:
        return self._rows(rows)[..., self.layout.action]

    def target_distance(self, rows=None) -> np.ndarray:
        """the norm of the first target row (the current waypoint / the duck); NaN where the layout has none"""
        r = self._rows(rows)
        if not self.layout.has_target:
            return np.full(r.shape[:-1], np.nan)
        return np.linalg.norm(r[..., self.layout.target], axis=-1)

    def targets_reached(self, rows=None) -> np.ndarray:
        return self._rows(rows)[..., self.layout.obs_dim].astype(np.int64)

    def flag(self, rows=None) -> np.ndarray:
        return self._rows(rows)[..., self.layout.obs_dim + 1].astype(np.int64)

    def episode(self, i: int) -> np.ndarray:
        """env i's rows up to and including ``ended_at[i]`` (all T rows if its first episode did not end inside the trace)"""
        e = int(self.ended_at[i])
        return self.trace[:(e + 1 if e >= 0 else self.trace.shape[0]), i]


def _flight_env(env, who: str):
    """the wrapped env of a normaliser that ``who`` can serve, or ValueError"""
    venv = getattr(env, "venv", None)
    task = getattr(getattr(venv, "cfg", None), "task", None)
    if venv is None or task is None or hasattr(venv, "step_low") or not hasattr(venv, "terminal_obs"):
        if venv is not None and hasattr(venv, "step_low"):
            raise ValueError(f"{who}: the high-level command task has its own flight record and figures (highlevel.fly, command_scalars)")
        raise ValueError(f"{who} needs a VecNormalizeDevice around a waypoints, ObjLock, combined or direct-command waypoints env")
    if task == K.FW_TASK_LOWLEVEL:
        raise ValueError(f"{who}: the low-level task has its own flight record and figures (command.fly, tracking_scalars)")
    if task not in _PATH_TASKS:
        raise ValueError(f"{who} needs a waypoints, ObjLock, combined or direct-command waypoints env")
    return venv


def fly(policy, env, n_steps: int, use_fused: Optional[bool] = None, graph_steps: int = 8) -> FlightTrace:
    """Fly ``policy`` (deterministic, frozen normaliser statistics) for ``n_steps`` vec-steps on ``env``, a
    ``VecNormalizeDevice(training=False)`` around a waypoints, ObjLock, combined or direct-command waypoints env.  ``env.reset()``
    first; then per vec-step k: act -> step -> ``fw_trace_rows`` (row k of the trace).  The act and the step are the torch forward
    followed by ``step_tensor`` (``use_fused`` None / False) or the one ``fw_collect_step`` launch of ``evalstep.CollectStep``
    (``use_fused=True``, where ``evalstep.select`` finds that it applies).  With ``graph_steps > 0`` the body is
    captured as a hipGraph of that many vec-steps and replayed (the trace row is picked on the device); the steps that do not fill a
    whole graph run eagerly after it.  ``graph_steps <= 0`` runs every step eagerly; both give the same trace bit for bit.  A policy
    with a CNN front end (``uses_image``) flies eagerly: MIOpen stays out of captures, as in ``evaluate_policy``."""
    from . import evalstep
    venv = _flight_env(env, "fly")
    if getattr(env, "training", True):
        raise ValueError("fly needs an evaluation normaliser (training=False): the statistics stay frozen")
    T = int(n_steps)
    if T <= 0:
        raise ValueError(f"n_steps must be positive, got {n_steps}")
    n, dev = env.num_envs, env.device
    layout = RowLayout.of(venv.cfg)
    kind = evalstep.select(policy, env, use_fused, ("collect_step",), "use_fused=True needs the four-action MlpPolicy, a device env on "
                           "the 8-lane mapping and an evaluation normaliser (training=False) on the GPU")
    step = evalstep.make(kind, policy, env)
    if getattr(policy, "uses_image", False):
        graph_steps = 0
    L = _lib.lib()
    D = int(venv.obs.shape[1])
    step_idx = torch.zeros((), dtype=torch.int64, device=dev)
    trace = torch.zeros((T, n, D + 2), dtype=torch.float64, device=dev)
    is_f64 = int(venv.obs.dtype == torch.float64)

    def body():
        step()
        _lib.check(L.fw_trace_rows(_devptr(venv.obs), _devptr(venv.terminal_obs), _devptr(venv.terminated), _devptr(venv.truncated),
                                   _devptr(venv.info), int(venv.info.shape[1]), is_f64, n, D, _devptr(trace), T, _devptr(step_idx),
                                   _lib.stream(dev)))

    def finish():                            # the status word is read once the stream has drained
        torch.cuda.current_stream(dev).synchronize()
        step.check()

    tr, start, ended_at = evalstep.replay_flight(env, trace, graph_steps, body, step.prepare, lambda: trace_rows(venv.obs), D + 1, finish)
    return FlightTrace(trace=tr, start=start, dt=1.0 / float(venv.cfg.agent_hz), ended_at=ended_at, layout=layout)


def path_figures(trace: FlightTrace) -> dict:
    """The twelve sums of ``PATH_SUMS`` of every env's first episode, where it ended inside the trace, in plain numpy from the
    recorded rows: ``{env index: array [12]}``.  Written from the definitions, not from :func:`path_step`."""
    lay, out = trace.layout, {}
    D = lay.obs_dim
    for i in range(trace.trace.shape[1]):
        if trace.ended_at[i] < 0:
            continue
        rows = trace.episode(i)
        pos = np.concatenate([trace.start[i:i + 1, lay.position], rows[:, lay.position]], axis=0)      # positions 0 .. L
        act = np.concatenate([trace.start[i:i + 1, lay.action], rows[:, lay.action]], axis=0)
        seg = np.sqrt((np.diff(pos, axis=0) ** 2).sum(axis=1))
        cum = np.cumsum(seg)
        reached = np.concatenate([[0.0], rows[:, D]])
        hit = np.nonzero(np.diff(reached) > 0)[0]                       # 0-based rows on which the count rose
        vel, w = rows[:, lay.velocity], rows[:, lay.ang_vel]
        legs = np.concatenate([pos[0:1], pos[hit + 1]], axis=0)         # start, then the aircraft at each reach
        chord = np.sqrt((np.diff(legs, axis=0) ** 2).sum(axis=1)).sum() if len(hit) else 0.0
        miss = math.inf
        if lay.has_target:
            since = rows[(hit[-1] + 1 if len(hit) else 0):, lay.target]  # the rows behind the last reach step
            if len(since):
                miss = float(np.sqrt((since ** 2).sum(axis=1)).min())
        out[i] = np.array([cum[-1], np.sqrt((vel ** 2).sum(axis=1)).sum(), rows[:, lay.position][:, 2].sum(),
                           rows[:, lay.position][:, 2].min(), np.sqrt((w ** 2).sum(axis=1)).sum(), np.abs(np.diff(act, axis=0)).sum(),
                           rows[:, lay.throttle].sum(), float(hit[0] + 1) if len(hit) else 0.0, float(hit[-1] + 1) if len(hit) else 0.0,
                           chord, cum[hit[-1]] if len(hit) else 0.0, miss], dtype=np.float64)
    return out
