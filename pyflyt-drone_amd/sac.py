"""Soft actor-critic for the low-level control task (the reference's ``examples/lowlevel.py``: SB3 ``SAC("MlpPolicy")`` with
``net_arch=[256, 256]``, a 200 000-row buffer, batches of 256, ``gamma=0.99``, ``tau=0.02``, one gradient step per env step, an
automatic entropy coefficient and no ``VecNormalize``).

Everything between two env steps runs on the device (csrc/fwsim_sac.hpp, include/fwsim.h):

* ``fw_sac_act``       the actor on the env's observations, the squashed-Gaussian sample (or SB3's uniform ``learning_starts``
                       actions), the fp32 staging copy of the observation the step is about to overwrite;
* ``fw_replay_store``  appends the N transitions to a flat fp32 ring at a device-resident cursor;
* ``fw_replay_sample`` draws a batch from the ring by a counter-based generator;
* ``fw_replay_mark_ends`` / ``fw_replay_sample_nstep``  (``SACConfig.n_steps > 1`` only) one flag byte per row for the episode ends,
                       and the same draw gathered as an n-step transition (:func:`nstep_rows_reference` restates its contract);
* ``fw_replay_sample_her``  (``SACConfig.her_goals > 0`` only) the same draw with hindsight goals: some rows get a goal their episode
                       achieved at or after them and the reward that goal earns (:func:`her_rows_reference` restates its contract);
* ``fw_replay_per_mark_new`` / ``fw_replay_per_rebuild`` / ``fw_replay_sample_per`` / ``fw_replay_per_update``
                       (``SACConfig.prioritized`` only) prioritized replay, Schaul et al. 2016, proportional variant: one priority leaf
                       per ring row under a three-level sum structure, the proportional draw with its importance weights, and the
                       write-back of the new priorities (:func:`per_sums_reference`, :func:`per_draw_reference` and
                       :func:`per_update_reference` restate their contracts);
* ``fw_sac_act_norm`` / ``fw_replay_normalize`` / ``fw_collect_stats``  (``SACConfig.normalize_obs`` / ``normalize_reward`` only) SB3's
                       ``VecNormalize`` with an off-policy buffer: the ring keeps raw rows, the actor reads observations normalised as
                       they are loaded, a sampled batch is normalised in place with the statistics of that moment, and one statistics
                       launch behind every env step moves them (:func:`normalize_rows_reference` and :func:`stats_step_reference`
                       restate their contracts);
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

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
MAX_OBS_DIM, MAX_ACT_DIM, HIDDEN_WIDTHS, MAX_BATCH = 64, 8, (64, 256), 512
MAX_BATCH_WIDE, WIDE_BATCH_MULTIPLE = 8192, 64                  # above MAX_BATCH: the wide form of the gradient step
MAX_N_STEPS = 16                                                # fw_replay_sample_nstep
END_TERMINATED, END_TRUNCATED = 1, 2                            # bits of the `ends` side ring
MAX_HER_HORIZON, HER_OBS_DIM, HER_ROW_FLOATS = 64, 21, 50       # fw_replay_sample_her: the low-level task with Euler attitude
HER_TAG = 0x5AC0E000                                            # the Philox tag of its second draw (kSacTagHer)
CTR_CURSOR, CTR_SIZE, CTR_STEPS, CTR_GRAD = 0, 1, 2, 3          # the device counters (int64[4])
PER_GROUP, PER_MAX_CAPACITY = 256, 1 << 22                      # prioritized replay: entries per group of a level; rows at most
PER_MAX, PER_TOTAL, PER_MIN = 0, 1, 2                           # per_state (float32[4]): running max leaf, total, smallest positive leaf


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


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
        self.prioritized = bool(self.prioritized)
        if not (0.0 <= float(self.per_alpha) <= 1.0 and 0.0 <= float(self.per_beta) <= 1.0):
            raise ValueError(f"per_alpha and per_beta must lie in [0, 1], got {self.per_alpha!r} and {self.per_beta!r}")
        if isinstance(self.per_beta_steps, bool) or int(self.per_beta_steps) != self.per_beta_steps or int(self.per_beta_steps) < 0:
            raise ValueError(f"per_beta_steps must be a non-negative integer, got {self.per_beta_steps!r}")
        if not (float(self.per_eps) > 0.0 and math.isfinite(float(self.per_eps))):
            raise ValueError(f"per_eps must be positive, got {self.per_eps!r}")
        self.per_alpha, self.per_beta, self.per_beta_steps, self.per_eps = (float(self.per_alpha), float(self.per_beta),
                                                                            int(self.per_beta_steps), float(self.per_eps))
        if isinstance(self.her_goals, bool) or int(self.her_goals) != self.her_goals or int(self.her_goals) < 0:
            raise ValueError(f"her_goals must be a non-negative integer, got {self.her_goals!r}")
        if (isinstance(self.her_horizon, bool) or int(self.her_horizon) != self.her_horizon
                or not 1 <= int(self.her_horizon) <= MAX_HER_HORIZON):
            raise ValueError(f"her_horizon must be an integer in [1, {MAX_HER_HORIZON}], got {self.her_horizon!r}")
        self.her_goals, self.her_horizon = int(self.her_goals), int(self.her_horizon)
        if isinstance(self.n_steps, bool) or int(self.n_steps) != self.n_steps or not 1 <= int(self.n_steps) <= MAX_N_STEPS:
            raise ValueError(f"n_steps must be an integer in [1, {MAX_N_STEPS}], got {self.n_steps!r}")
        self.n_steps = int(self.n_steps)
        if self.her_goals > 0 and self.n_steps > 1:
            raise ValueError("her_goals > 0 together with n_steps > 1 is not built: the relabelled gather forms 1-step transitions only")
        if self.prioritized and (self.n_steps > 1 or self.her_goals > 0):
            raise ValueError("prioritized together with n_steps > 1 or her_goals > 0 is not built: those gathers draw their own indices")
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


def ring_capacity(buffer_size: int, num_envs: int) -> int:
    """Rows of the ring: whole vec-steps only, so a store never wraps inside itself."""
    cap = (int(buffer_size) // int(num_envs)) * int(num_envs)
    if cap <= 0:
        raise ValueError(f"buffer_size {buffer_size} holds no vec-step of {num_envs} envs")
    return cap


def row_floats(obs_dim: int, act_dim: int) -> int:
    return 2 * obs_dim + act_dim + 2


def split_rows(rows: torch.Tensor, obs_dim: int, act_dim: int):
    """(s, a, r, s', done) views of ring / batch rows ``[obs | action | reward | next_obs | done]``."""
    d, a = obs_dim, act_dim
    return rows[:, :d], rows[:, d:d + a], rows[:, d + a], rows[:, d + a + 1:2 * d + a + 1], rows[:, 2 * d + a + 1]


def nstep_rows_reference(ring, ends, cursor, size, N, idx, n_steps, gamma, obs_dim):
    """``fw_replay_sample_nstep`` in plain numpy on CPU arrays: ``(rows [B, R] float32, k [B] int32)`` of the start rows ``idx``.

    ``ring`` ``[capacity, R]`` float32, ``ends`` ``[capacity]`` uint8, ``cursor`` / ``size`` the first two device counters, ``N`` the env
    count (env e's consecutive steps are N rows apart), ``obs_dim`` locates the reward column of a row (R = 2 obs_dim + act_dim + 2).
    Walk ``row_j = (i + j N) mod capacity``: row_j is used, then the walk stops if ``j + 1 == n_steps``, or ``ends[row_j] != 0``, or
    row_j lies in the newest vec-step stored (``row_j - row_j mod N == (cursor - N) mod capacity``, the cursor normalised as
    ``fw_replay_store`` does).  With k rows used, ``g_0 = 1`` and ``g_j = g_(j-1) gamma`` in float32 (gamma itself rounded to float32,
    as the entry point receives it): obs | action from row_0, reward ``r_0 + g_1 r_1 + ... + g_(k-1) r_(k-1)`` in float32 in ascending j,
    next_obs from row_(k-1), last column ``1 - (1 - done_(k-1)) g_(k-1)``.  The kernel adds each term with one fused multiply-add, this
    function with a rounded product and a rounded sum: the two rewards differ by roundings only (tests/test_sac_nstep_gpu.py)."""
    import numpy as np
    ring, ends = np.asarray(ring, dtype=np.float32), np.asarray(ends, dtype=np.uint8)
    capacity, R = ring.shape
    N, n_steps, d = int(N), int(n_steps), int(obs_dim)
    if not 1 <= n_steps <= MAX_N_STEPS:
        raise ValueError(f"n_steps must be in [1, {MAX_N_STEPS}]")
    if N <= 0 or capacity % N or ends.shape != (capacity,) or R < 2 * d + 3:
        raise ValueError("capacity must be a multiple of N, ends one byte per row and a row 2 obs_dim + act_dim + 2 floats")
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= max(int(size), 1)):
        raise ValueError("idx must lie in [0, size)")
    cursor = int(cursor)
    if cursor < 0 or cursor + N > capacity:
        cursor = 0
    newest = (cursor - N + capacity) % capacity
    rcol, one, gam = R - d - 2, np.float32(1.0), np.float32(gamma)
    rows, ks = np.empty((idx.size, R), dtype=np.float32), np.empty(idx.size, dtype=np.int32)
    for b, i in enumerate(idx):
        j, g, ret = 0, one, np.float32(0.0)
        while True:
            row = (int(i) + j * N) % capacity
            g = one if j == 0 else np.float32(g * gam)
            ret = ring[row, rcol] if j == 0 else np.float32(ret + np.float32(g * ring[row, rcol]))
            if j + 1 == n_steps or ends[row] != 0 or row - row % N == newest:
                break
            j += 1
        rows[b, :rcol] = ring[i, :rcol]
        rows[b, rcol] = ret
        rows[b, rcol + 1:R - 1] = ring[row, rcol + 1:R - 1]
        rows[b, R - 1] = np.float32(one - np.float32(np.float32(one - ring[row, R - 1]) * g))
        ks[b] = j + 1
    return rows, ks


class HerTask(C.Structure):
    """``fw_her_task``: which of the low-level task's two rewards a relabelled row earns, and the two env settings the second reads."""
    _fields_ = [("variant", C.c_int32), ("dome", C.c_float), ("min_speed", C.c_float)]


def her_task_of(cfg) -> HerTask:
    """The ``fw_her_task`` of an env's ``fw_config``.  ``ValueError`` unless it is the low-level task with Euler attitude (21
    observations, the goal in columns 18:21)."""
    from . import config as K
    if cfg is None or cfg.task != K.FW_TASK_LOWLEVEL or int(cfg.angle_representation) != 0 or K.obs_dim(cfg) != HER_OBS_DIM:
        raise ValueError("hindsight relabelling (her_goals > 0) needs the low-level task (FW_TASK_LOWLEVEL) with Euler attitude: "
                         f"{HER_OBS_DIM} observations, the goal in columns 18:21")
    return HerTask(int(cfg.lowlevel_variant), float(cfg.flight_dome_size), float(cfg.lowlevel_min_speed))


def her_achieved_goal(next_obs):
    """The goal ``(psi, z, |v|)`` a post-step observation achieved, float32 ``[..., 3]``: the norm in float64 from the float32
    components, rounded to float32."""
    import numpy as np
    no = np.asarray(next_obs, dtype=np.float32)
    v = no[..., 6:9].astype(np.float64)
    speed = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    return np.stack([no[..., 5], no[..., 11], speed.astype(np.float32)], axis=-1)


def her_reward_reference(next_obs, goal, done, task):
    """The low-level task's reward for (post-step observation, goal, ``terminated``) in float64, not rounded: what ``fw_her_reward`` and
    ``fw_replay_sample_her`` round once to float32.  ``next_obs`` ``[..., >= 18]`` and ``goal`` ``[..., 3]`` float32 values.  The
    airspeed it reads is the achieved goal's (:func:`her_achieved_goal`, rounded to float32), so a goal the observation itself achieved
    has tracking errors of exactly 0.  Variant 0 (fixedwing_lowlevel_env.py): ``-(|wrap(psi_ref - psi)| + |h_ref - z| + 0.5 |V_ref - V|)
    + 0.1``, and 100 less where done.  Variant 1 (the SAC script's env): ``-(1.5, 1.2, 0.8) . errors``, 0.3 per radian of roll beyond
    35 deg and of pitch beyond 20 deg, 0.05 |next_obs[12:18]|, the distance beyond the dome, and 2 below ``min_speed``."""
    import numpy as np
    no = np.asarray(next_obs, dtype=np.float32).astype(np.float64)
    g = np.asarray(goal, dtype=np.float32).astype(np.float64)
    done = np.asarray(done) != 0
    roll, pitch, psi, z = no[..., 3], no[..., 4], no[..., 5], no[..., 11]
    speed = her_achieved_goal(next_obs)[..., 2].astype(np.float64)
    psi_err = np.abs((g[..., 0] - psi + np.pi) % (2.0 * np.pi) - np.pi)
    h_err, v_err = np.abs(g[..., 1] - z), np.abs(g[..., 2] - speed)
    if int(task.variant) == 1:
        rho = np.sqrt(no[..., 9] * no[..., 9] + no[..., 10] * no[..., 10])
        aa = np.zeros_like(psi)
        for k in range(12, 18):
            aa = aa + no[..., k] * no[..., k]
        rew = -(1.5 * psi_err + 1.2 * h_err + 0.8 * v_err)
        rew = rew - 0.3 * np.maximum(np.abs(roll) - 35.0 * np.pi / 180.0, 0.0)
        rew = rew - 0.3 * np.maximum(np.abs(pitch) - 20.0 * np.pi / 180.0, 0.0)
        rew = rew - 0.05 * np.sqrt(aa)
        rew = rew - np.maximum(rho - float(np.float32(task.dome)), 0.0)
        return np.where(speed < float(np.float32(task.min_speed)), rew - 2.0, rew)
    if int(task.variant) != 0:
        raise ValueError("task.variant must be 0 or 1")
    rew = -(psi_err + h_err + 0.5 * v_err) + 0.1
    return np.where(done, rew - 100.0, rew)


def her_rows_reference(ring, ends, cursor, size, N, idx, relabel, j_star_draw, horizon, task):
    """``fw_replay_sample_her`` in plain numpy on CPU arrays: ``(rows [B, 50] float32, j [B] int32)`` of the start rows ``idx``.

    ``ring`` ``[capacity, 50]`` float32 (21 observations, 6 actions), ``ends`` ``[capacity]`` uint8, ``cursor`` / ``size`` the first two
    device counters, ``N`` the env count.  ``relabel`` ``[B]`` says which rows are relabelled and ``j_star_draw`` ``[B]`` is the uint32
    word that picks the future row: the kernel takes both from its second Philox block (``o[0] < relabel_prob 2^32``, ``o[1]``; counter
    words ``(b, 0, gs, gs >> 32 ^ HER_TAG)``).  A row that is not relabelled is the ring row and its ``j`` is -1.  Otherwise walk ``row_j =
    (i + j N) mod capacity`` by :func:`nstep_rows_reference`'s rule with ``horizon`` in the place of ``n_steps``; with k rows used,
    ``j* = (j_star_draw k) >> 32``, the goal ``g'`` is :func:`her_achieved_goal` of ``row_j*``'s next_obs, it replaces columns 18:21 of
    obs and of next_obs, and the reward column is :func:`her_reward_reference` of (row_0's next_obs, ``g'``, row_0's done) rounded to
    float32.  Everything else is row_0."""
    import numpy as np
    ring, ends = np.asarray(ring, dtype=np.float32), np.asarray(ends, dtype=np.uint8)
    capacity, R = ring.shape
    N, horizon, d = int(N), int(horizon), HER_OBS_DIM
    if not 1 <= horizon <= MAX_HER_HORIZON:
        raise ValueError(f"horizon must be in [1, {MAX_HER_HORIZON}]")
    if N <= 0 or capacity % N or ends.shape != (capacity,) or R != HER_ROW_FLOATS:
        raise ValueError(f"capacity must be a multiple of N, ends one byte per row and a row {HER_ROW_FLOATS} floats")
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    relabel, draw = np.asarray(relabel).reshape(-1) != 0, np.asarray(j_star_draw).reshape(-1)
    if relabel.shape != idx.shape or draw.shape != idx.shape:
        raise ValueError("relabel and j_star_draw must have one entry per row of idx")
    if idx.size and (idx.min() < 0 or idx.max() >= max(int(size), 1)):
        raise ValueError("idx must lie in [0, size)")
    cursor = int(cursor)
    if cursor < 0 or cursor + N > capacity:
        cursor = 0
    newest = (cursor - N + capacity) % capacity
    rcol, nobs = R - d - 2, R - d - 1
    rows, js = ring[idx].copy(), np.full(idx.size, -1, dtype=np.int32)
    for b, i in enumerate(idx):
        if not relabel[b]:
            continue
        k = 0
        while True:
            row = (int(i) + k * N) % capacity
            k += 1
            if k == horizon or ends[row] != 0 or row - row % N == newest:
                break
        j = (int(draw[b]) * k) >> 32
        goal = her_achieved_goal(ring[(int(i) + j * N) % capacity, nobs:nobs + d])
        rows[b, d - 3:d] = goal
        rows[b, nobs + d - 3:nobs + d] = goal
        rows[b, rcol] = np.float32(her_reward_reference(ring[i, nobs:nobs + d], goal, ring[i, R - 1], task))
        js[b] = j
    return rows, js


# ---------------------------------------------------------------------------------------------
# prioritized replay in plain numpy (the contract of csrc/fwsim_per.hpp)
# ---------------------------------------------------------------------------------------------
def per_group_sums(x):
    """THE order of a group, in float32: ``x`` ``[..., 256]`` -> ``(S, F, total)``.  Entry ``4l + j`` belongs to chain ``l``:
    ``p(4l) = x(4l)``, ``p(4l + j) = p(4l + j - 1) + x(4l + j)``; ``E_0 = 0``, ``E_(l+1) = E_l + p(4l + 3)``.  ``S(4l + j) = E_l +
    p(4l + j)`` is the running sum up to and including the entry, ``F`` the running sum in front of it (``S`` of the entry before,
    0 in front of entry 0) and ``total = E_64`` the group's sum."""
    import numpy as np
    x = np.asarray(x, dtype=np.float32)
    assert x.shape[-1] == PER_GROUP
    q = x.reshape(x.shape[:-1] + (PER_GROUP // 4, 4))
    p = np.empty_like(q)
    p[..., 0] = q[..., 0]
    for j in range(1, 4):
        p[..., j] = p[..., j - 1] + q[..., j]
    E, run = np.empty(q.shape[:-1], dtype=np.float32), np.zeros(q.shape[:-2], dtype=np.float32)
    for l in range(PER_GROUP // 4):
        E[..., l] = run
        run = (run + p[..., l, 3]).astype(np.float32)
    S = (E[..., None] + p).astype(np.float32)
    F = np.concatenate([E[..., None], S[..., :3]], axis=-1)
    return S.reshape(x.shape), F.reshape(x.shape), run


def _per_groups(v, pad):
    """``v`` [n] as groups ``[ceil(n / 256), 256]``, the missing entries ``pad``."""
    import numpy as np
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    n = -(-v.size // PER_GROUP)
    out = np.full(n * PER_GROUP, pad, dtype=np.float32)
    out[:v.size] = v
    return out.reshape(n, PER_GROUP)


def per_sums_reference(prio):
    """``fw_replay_per_rebuild`` in plain numpy: ``dict(sum1, min1, sum2, min2, total, pmin)`` of the leaves ``prio`` [capacity]
    (float32, non-negative).  A sum is :func:`per_group_sums`' total of its 256 entries (missing ones 0), a min the smallest positive
    entry below it (+inf where there is none); ``total`` is the group sum of ``sum2`` (at most 64 entries: the capacity limit) and
    ``pmin`` the smallest positive leaf."""
    import numpy as np
    prio = np.asarray(prio, dtype=np.float32).reshape(-1)
    if not 0 < prio.size <= PER_MAX_CAPACITY:
        raise ValueError(f"capacity must lie in [1, {PER_MAX_CAPACITY}]")
    inf = np.float32(np.inf)
    g0 = _per_groups(prio, 0.0)
    sum1 = per_group_sums(g0)[2]
    min1 = np.where(g0 > 0, g0, inf).min(axis=1)
    sum2 = per_group_sums(_per_groups(sum1, 0.0))[2]
    min2 = _per_groups(min1, inf).min(axis=1)
    total = per_group_sums(_per_groups(sum2, 0.0))[2][0]
    return dict(sum1=sum1, min1=min1, sum2=sum2, min2=min2, total=np.float32(total), pmin=np.float32(min2.min()))


def _per_pick(values, group, t):
    """One level of the descent for a batch: in group ``group[b]`` of ``values`` the first positive entry whose running sum exceeds
    ``t[b]``, else the last positive entry, else entry 0 with t = 0 -> (entry index inside the group, t - front)."""
    import numpy as np
    x = _per_groups(values, 0.0)[group]
    S, F, _ = per_group_sums(x)
    pos = x > 0
    hit = pos & (S > t[:, None])
    k = np.where(hit.any(1), hit.argmax(1), PER_GROUP - 1 - pos[:, ::-1].argmax(1))
    none = ~pos.any(1)
    k = np.where(none, 0, k)
    left = (t - F[np.arange(len(t)), k]).astype(np.float32)
    return k.astype(np.int64), np.where(none, np.float32(0.0), left).astype(np.float32)


def per_draw_reference(prio, sums, o0, t=None):
    """The draw of ``fw_replay_sample_per`` in plain numpy: the row index [B] (int64) of each batch row.  ``prio`` [capacity] the
    leaves, ``sums`` what :func:`per_sums_reference` made of them, ``o0`` [B] the first word (uint32) of each row's Philox block
    (``fw_replay_sample``'s: counter words ``(b, 0, gs, gs >> 32 ^ 0x5AC0C000)``, key the seed).  ``u = (o0 + 0.5) 2^-32`` in float64,
    ``t = float32(u float64(total))`` (``t`` [B] float32 overrides it: the clamp rule can then be driven directly).  Three levels --
    ``sum2``, the chosen group of ``sum1``, the chosen group of ``prio`` -- each takes the FIRST positive entry whose running sum
    (:func:`per_group_sums`) exceeds t, or, where rounding leaves none, the LAST positive entry, and carries ``t - front`` down."""
    import numpy as np
    prio = np.asarray(prio, dtype=np.float32).reshape(-1)
    if t is None:
        u = (np.asarray(o0).astype(np.float64) + 0.5) * 2.0 ** -32
        t = (u * np.float64(sums["total"])).astype(np.float32)
    t = np.asarray(t, dtype=np.float32).reshape(-1).copy()
    k2, t = _per_pick(sums["sum2"], np.zeros(len(t), dtype=np.int64), t)
    k1, t = _per_pick(sums["sum1"], k2, t)
    g = k2 * PER_GROUP + k1
    k0, t = _per_pick(prio, g, t)
    return g * PER_GROUP + k0


def per_beta_reference(beta0, beta_steps, grad_step):
    """The exponent ``fw_replay_sample_per`` uses at gradient step ``grad_step`` (``counters[3]``), in float32 as the device forms it."""
    import numpy as np
    b0 = np.float32(beta0)
    if int(beta_steps) <= 0:
        return b0
    frac = np.float32(np.float32(grad_step) / np.float32(beta_steps))
    return np.float32(min(np.float32(1.0), np.float32(b0 + np.float32(np.float32(1.0) - b0) * frac)))


def per_weights_reference(prio, idx, pmin, beta):
    """The importance weights ``(p_min / p_row)^beta`` of the rows ``idx`` in float64 (the kernel: ``exp(beta log x)`` in float32).
    With ``P(row) = p_row / total`` this is ``(n P(row))^-beta`` divided by its maximum over the ring, which the row of ``p_min`` has."""
    import numpy as np
    p = np.asarray(prio, dtype=np.float32)[np.asarray(idx, dtype=np.int64)].astype(np.float64)
    return (np.float64(np.float32(pmin)) / p) ** np.float64(np.float32(beta))


def per_update_reference(prio, idx, td, alpha, eps, pmax):
    """``fw_replay_per_update`` in plain numpy: ``(prio', pmax')``.  The leaf of batch row b is ``(|td[b]| + eps)^alpha``, the sum in
    float32, the power in float64 rounded to float32 (the kernel: ``exp(alpha log x)`` in float32); a row that occurs more than once
    receives the largest of its leaves, and ``pmax'`` is the max of ``pmax`` and the batch's leaves.  An index outside the ring and a
    td that is not finite are skipped (a skipped row that is in the batch only this way keeps a leaf of 0)."""
    import numpy as np
    out = np.asarray(prio, dtype=np.float32).copy()
    idx, td = np.asarray(idx, dtype=np.int64).reshape(-1), np.asarray(td, dtype=np.float32).reshape(-1)
    x = (np.abs(td) + np.float32(eps)).astype(np.float32)
    with np.errstate(all="ignore"):
        leaf = (x.astype(np.float64) ** np.float64(np.float32(alpha))).astype(np.float32)
    inside = (idx >= 0) & (idx < out.size)
    out[idx[inside]] = 0.0
    ok = inside & np.isfinite(leaf) & (leaf > 0)
    np.maximum.at(out, idx[ok], leaf[ok])
    return out, np.float32(max([np.float32(pmax)] + list(leaf[ok])))


# ---------------------------------------------------------------------------------------------
# running normalisation in plain torch (the contracts of fw_sac_act_norm's load, fw_replay_normalize and fw_collect_stats)
# ---------------------------------------------------------------------------------------------
def _eps64(eps: float) -> float:
    """An epsilon as the entry points receive it: a C float, widened to double on the device."""
    return float(torch.tensor(float(eps), dtype=torch.float32).double())


def normalize_obs_reference(obs, mean, var, clip: float = 10.0, eps: float = 1e-8):
    """``clip((float32)((x - mean) / sqrt(var + eps)), +-clip)`` with the arithmetic in float64 and one division per element: what
    ``fw_normalize_obs(update=0)``, ``fw_sac_act_norm``'s load and ``fw_replay_normalize`` compute.  CPU tensors too."""
    mean, var = torch.as_tensor(mean, dtype=torch.float64), torch.as_tensor(var, dtype=torch.float64)
    z = (obs.to(torch.float64) - mean.to(obs.device)) / torch.sqrt(var.to(obs.device) + _eps64(eps))
    return z.to(torch.float32).clamp_(-float(clip), float(clip))


def normalize_rows_reference(rows, obs_dim: int, act_dim: int, obs_mean=None, obs_var=None, clip_obs: float = 10.0, eps_obs: float = 1e-8,
                             ret_var=None, clip_reward: float = 10.0, eps_reward: float = 1e-8):
    """``fw_replay_normalize`` in plain torch (CPU tensors too): a copy of ``rows`` ``[B, 2d + A + 2]`` float32 with both observation
    blocks replaced by :func:`normalize_obs_reference` (``obs_mean`` / ``obs_var`` ``[d]`` float64; ``None``: left alone) and the reward
    column by ``clip((float32)(r / sqrt(ret_var + eps_reward)), +-clip_reward)`` in float64 (``ret_var`` a float64 scalar; ``None``:
    left alone).  The action and done columns are the input's."""
    d, A = int(obs_dim), int(act_dim)
    if rows.dim() != 2 or rows.shape[1] != row_floats(d, A) or rows.dtype != torch.float32:
        raise ValueError(f"rows must be float32 [B, {row_floats(d, A)}]")
    if obs_mean is None and ret_var is None:
        raise ValueError("one of obs_mean and ret_var must be given")
    if (obs_mean is None) != (obs_var is None):
        raise ValueError("obs_mean and obs_var come together")
    out = rows.clone()
    if obs_mean is not None:
        for lo in (0, d + A + 1):
            out[:, lo:lo + d] = normalize_obs_reference(rows[:, lo:lo + d], obs_mean, obs_var, clip_obs, eps_obs)
    if ret_var is not None:
        rv = torch.as_tensor(ret_var, dtype=torch.float64).reshape(()).to(rows.device)
        r = rows[:, d + A].to(torch.float64) / torch.sqrt(rv + _eps64(eps_reward))
        out[:, d + A] = r.to(torch.float32).clamp_(-float(clip_reward), float(clip_reward))
    return out


def running_moments_reference(mean, var, count, x):
    """One update of SB3's ``RunningMeanStd`` in float64, as ``fw_collect_stats`` merges a batch: ``(mean', var', count')`` from the
    column sums and sums of squares of ``x`` ``[n, ...]`` -- batch mean ``s / n``, population variance ``max(s2 / n - bm^2, 0)``, then
    the merge of Chan et al.  Nothing is written in place."""
    mean, var = torch.as_tensor(mean, dtype=torch.float64), torch.as_tensor(var, dtype=torch.float64)
    cnt = torch.as_tensor(count, dtype=torch.float64).reshape(-1)[0]
    x = x.to(torch.float64).reshape(x.shape[0], -1)
    n = float(x.shape[0])
    bm = x.sum(0) / n
    bv = ((x * x).sum(0) / n - bm * bm).clamp_min(0.0)
    bm, bv = bm.reshape(mean.shape), bv.reshape(var.shape)
    delta, tot = bm - mean, cnt + n
    m2 = var * cnt + bv * n + delta * delta * cnt * n / tot
    return mean + delta * n / tot, m2 / tot, tot.reshape(1)


def stats_step_reference(obs_stats, ret_stats, returns, obs, reward, ended, gamma: float, update_obs: bool = True, update_ret: bool = True):
    """What the statistics launch behind an env step does (``VecNormalize.step_wait``'s bookkeeping), in plain torch on any device:
    ``(obs_stats', ret_stats', returns')``, each ``*_stats`` a ``(mean, var, count)`` triple.  The new observations ``obs`` ``[N, d]``
    (the reset rows of the envs that ended, never a terminal observation) go into ``obs_stats``; ``returns gamma + reward`` goes into
    ``ret_stats``; then ``returns`` is zeroed where ``ended``."""
    returns = torch.as_tensor(returns, dtype=torch.float64).clone()
    if update_obs:
        obs_stats = running_moments_reference(*obs_stats, obs)
    if update_ret:
        returns = returns * float(gamma) + reward.to(torch.float64)
        ret_stats = running_moments_reference(*ret_stats, returns)
    returns = torch.where(ended.bool(), torch.zeros_like(returns), returns)
    return tuple(obs_stats), tuple(ret_stats), returns


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
        if weights is not None:
            assert weights.dtype == torch.float32 and weights.is_contiguous() and weights.numel() == B
            assert td_out is None or (td_out.dtype == torch.float32 and td_out.is_contiguous() and td_out.numel() == B)
            _lib.check(_lib.lib().fw_sac_update_weighted(_p(self.image), _p(rows), self.d, self.A, self.H, B, C.byref(H), _p(counters),
                                                         _p(self.out), _p(ws), ws.numel(), _p(weights), _p(td_out), _stream(rows.device)))
            return
        if td_out is not None:
            raise ValueError("td_out is written by the weighted step: pass weights (ones for an unweighted one)")
        _lib.check(_lib.lib().fw_sac_update(_p(self.image), _p(rows), self.d, self.A, self.H, B, C.byref(H), _p(counters), _p(self.out),
                                            _p(ws), ws.numel(), _stream(rows.device)))

    def scalars(self) -> Dict[str, float]:
        return dict(zip(SCALARS, self.out[:5].tolist()))


# ---------------------------------------------------------------------------------------------
# the replay ring
# ---------------------------------------------------------------------------------------------
class ReplayBufferDevice:
    """Flat fp32 ring ``[capacity, 2d + A + 2]`` and the device counters (cursor, rows filled, vec-steps stored, gradient steps):
    the host reads none of them on the training path.  ``n_steps > 1`` adds the episode-end side ring ``ends`` (uint8 per row:
    ``END_TERMINATED`` | ``END_TRUNCATED``), marked in front of every store, and ``sample`` gathers n-step transitions.
    ``her_goals > 0`` (with ``her_task``, :func:`her_task_of`) owns the same side ring and ``sample`` relabels goals in hindsight.
    ``prioritized`` owns one priority leaf per row (``prio``), the two levels of sums and mins above them and ``per_state``: a store
    gives its rows the running max leaf and rebuilds the sums, ``sample`` draws in proportion to the leaves and reports the importance
    weights, ``update_priorities`` writes the new leaves back and rebuilds."""

    def __init__(self, buffer_size: int, num_envs: int, obs_dim: int, act_dim: int, device, n_steps: int = 1, her_goals: int = 0,
                 her_horizon: int = MAX_HER_HORIZON, her_task: Optional[HerTask] = None, prioritized: bool = False,
                 per_alpha: float = 0.6, per_beta: float = 0.4, per_beta_steps: int = 0, per_eps: float = 1e-6):
        if not 1 <= int(n_steps) <= MAX_N_STEPS:
            raise ValueError(f"n_steps must be in [1, {MAX_N_STEPS}], got {n_steps}")
        self.n_steps = int(n_steps)
        self.her_goals, self.her_horizon, self.her_task = int(her_goals), int(her_horizon), her_task
        if self.her_goals < 0 or not 1 <= self.her_horizon <= MAX_HER_HORIZON:
            raise ValueError(f"her_goals must be non-negative and her_horizon in [1, {MAX_HER_HORIZON}], got {her_goals} and {her_horizon}")
        if self.her_goals > 0 and (self.n_steps > 1 or her_task is None or int(obs_dim) != HER_OBS_DIM
                                   or row_floats(obs_dim, act_dim) != HER_ROW_FLOATS):
            raise ValueError("her_goals > 0 needs her_task, n_steps 1 and the low-level task's rows "
                             f"({HER_OBS_DIM} observations, {HER_ROW_FLOATS} floats)")
        self.her_prob = self.her_goals / (self.her_goals + 1.0)
        self.num_envs, self.obs_dim, self.act_dim = int(num_envs), int(obs_dim), int(act_dim)
        self.capacity = ring_capacity(buffer_size, num_envs)
        self.row = row_floats(obs_dim, act_dim)
        self.ring = torch.zeros((self.capacity, self.row), dtype=torch.float32, device=device)
        self.counters = torch.zeros(4, dtype=torch.int64, device=device)
        self.ends = torch.zeros(self.capacity, dtype=torch.uint8, device=device) if self.n_steps > 1 or self.her_goals > 0 else None
        self.prioritized = bool(prioritized)
        self.per_alpha, self.per_beta, self.per_beta_steps, self.per_eps = float(per_alpha), float(per_beta), int(per_beta_steps), float(per_eps)
        self.prio = self.sum1 = self.min1 = self.sum2 = self.min2 = self.per_state = None
        if self.prioritized:
            if self.n_steps > 1 or self.her_goals > 0:
                raise ValueError("prioritized together with n_steps > 1 or her_goals > 0 is not built: those gathers draw their own indices")
            if not (0.0 <= self.per_alpha <= 1.0 and 0.0 <= self.per_beta <= 1.0 and self.per_beta_steps >= 0 and self.per_eps > 0.0):
                raise ValueError("per_alpha and per_beta must lie in [0, 1], per_beta_steps must not be negative and per_eps must be positive")
            if self.capacity > PER_MAX_CAPACITY:
                raise ValueError(f"a prioritized ring holds at most 2^22 = {PER_MAX_CAPACITY} rows (above that a float32 sum stops resolving "
                                 f"one leaf), got {self.capacity}")
            n1 = -(-self.capacity // PER_GROUP)
            n2 = -(-n1 // PER_GROUP)
            kw = dict(dtype=torch.float32, device=device)
            self.prio = torch.zeros(self.capacity, **kw)
            self.sum1, self.min1 = torch.zeros(n1, **kw), torch.full((n1,), math.inf, **kw)
            self.sum2, self.min2 = torch.zeros(n2, **kw), torch.full((n2,), math.inf, **kw)
            self.per_state = torch.tensor([1.0, 0.0, math.inf, 0.0], **kw)

    def rebuild(self) -> None:
        """Both levels of sums and mins, the total and the smallest positive leaf from the leaves (``fw_replay_per_rebuild``; for a
        ring of CPU tensors -- checkpoints are inspected there -- :func:`per_sums_reference`)."""
        if not self.prio.is_cuda:
            r = per_sums_reference(self.prio.numpy())
            for name in ("sum1", "min1", "sum2", "min2"):
                getattr(self, name).copy_(torch.from_numpy(r[name]))
            self.per_state[PER_TOTAL], self.per_state[PER_MIN] = float(r["total"]), float(r["pmin"])
            return
        _lib.check(_lib.lib().fw_replay_per_rebuild(_p(self.prio), self.capacity, _p(self.sum1), _p(self.min1), _p(self.sum2), _p(self.min2),
                                                    _p(self.per_state), _stream(self.ring.device)))

    def update_priorities(self, idx: torch.Tensor, td: torch.Tensor) -> None:
        """The leaves of the batch's rows ``idx`` [B] int32 become ``(|td| + per_eps)^per_alpha`` (the largest one where a row was
        drawn more than once), the running max follows, and the sums are rebuilt."""
        assert idx.dtype == torch.int32 and td.dtype == torch.float32 and idx.is_contiguous() and td.is_contiguous() and idx.numel() == td.numel()
        _lib.check(_lib.lib().fw_replay_per_update(_p(self.prio), self.capacity, _p(idx), _p(td), idx.numel(), self.per_alpha, self.per_eps,
                                                   _p(self.per_state), _stream(self.ring.device)))
        self.rebuild()

    def store(self, obs_stage, act_f32, reward, next_obs, terminal_obs, terminated, truncated) -> None:
        if self.ends is not None:        # the rows this store is about to write: the mark reads the cursor the store advances
            _lib.check(_lib.lib().fw_replay_mark_ends(_p(self.ends), self.capacity, _p(self.counters), _p(terminated), _p(truncated),
                                                      self.num_envs, _stream(self.ring.device)))
        if self.prioritized:             # new rows enter with the running max leaf, so every one of them is drawn at least once soon
            _lib.check(_lib.lib().fw_replay_per_mark_new(_p(self.prio), self.capacity, _p(self.counters), _p(self.per_state), self.num_envs,
                                                         _stream(self.ring.device)))
        _lib.check(_lib.lib().fw_replay_store(_p(self.ring), self.capacity, _p(self.counters), _p(obs_stage), _p(act_f32), _p(reward),
                                              _p(next_obs), _p(terminal_obs), _p(terminated), _p(truncated),
                                              int(reward.dtype == torch.float64), self.num_envs, self.obs_dim, self.act_dim,
                                              _stream(self.ring.device)))
        if self.prioritized:
            self.rebuild()

    def sample(self, seed: int, out: torch.Tensor, idx_out: Optional[torch.Tensor] = None, gamma: Optional[float] = None,
               k_out: Optional[torch.Tensor] = None, j_out: Optional[torch.Tensor] = None, w_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A batch into ``out``.  With ``n_steps > 1``: n-step transitions, which need ``gamma`` (``k_out`` [B] int32 receives the
        rows each one spans).  With ``her_goals > 0``: 1-step transitions, relabelled with probability ``her_prob`` (``j_out`` [B] int32
        receives -1, or how many steps ahead the goal was achieved).  With ``prioritized``: rows drawn in proportion to their leaves
        (``w_out`` [B] float32 receives the importance weights)."""
        if self.prioritized:
            _lib.check(_lib.lib().fw_replay_sample_per(_p(self.ring), self.capacity, _p(self.counters), int(seed) & (2**64 - 1), self.row,
                                                       out.shape[0], _p(out), _p(idx_out), _p(w_out), _p(self.prio), _p(self.sum1), _p(self.sum2),
                                                       _p(self.per_state), self.per_beta, self.per_beta_steps, _stream(self.ring.device)))
            return out
        if w_out is not None:
            raise ValueError("w_out is written by a prioritized buffer's sample")
        if self.her_goals > 0:
            _lib.check(_lib.lib().fw_replay_sample_her(_p(self.ring), self.capacity, _p(self.counters), int(seed) & (2**64 - 1), self.row,
                                                       out.shape[0], _p(out), _p(idx_out), _p(self.ends), self.obs_dim, self.num_envs,
                                                       self.her_horizon, float(self.her_prob), C.byref(self.her_task), _p(j_out),
                                                       _stream(self.ring.device)))
            return out
        if self.ends is not None:
            if gamma is None:
                raise ValueError("an n-step sample needs gamma")
            _lib.check(_lib.lib().fw_replay_sample_nstep(_p(self.ring), self.capacity, _p(self.counters), int(seed) & (2**64 - 1), self.row,
                                                         out.shape[0], _p(out), _p(idx_out), _p(self.ends), self.obs_dim, self.num_envs,
                                                         self.n_steps, float(gamma), _p(k_out), _stream(self.ring.device)))
            return out
        _lib.check(_lib.lib().fw_replay_sample(_p(self.ring), self.capacity, _p(self.counters), int(seed) & (2**64 - 1), self.row,
                                               out.shape[0], _p(out), _p(idx_out), _stream(self.ring.device)))
        return out

    @property
    def size(self) -> int:
        return int(self.counters[CTR_SIZE].item())

    @property
    def cursor(self) -> int:
        return int(self.counters[CTR_CURSOR].item())

    def state_dict(self, include_buffer: bool = False):
        sd = {"counters": self.counters.cpu().clone(), "capacity": self.capacity}
        if include_buffer:
            sd["ring"] = self.ring.cpu().clone()
            if self.ends is not None:
                sd["ends"] = self.ends.cpu().clone()
            if self.prioritized:
                sd["prio"], sd["per_state"] = self.prio.cpu().clone(), self.per_state.cpu().clone()
        return sd

    def load_state_dict(self, sd) -> None:
        if int(sd["capacity"]) != self.capacity:
            raise ValueError(f"the checkpoint's ring has {sd['capacity']} rows, this one {self.capacity}")
        if self.ends is not None and "ring" in sd and "ends" not in sd:
            raise ValueError("the checkpoint carries the ring's rows but not their episode ends (it was written with n_steps 1 and "
                             "without her_goals): neither n-step returns nor hindsight goals can be formed from them")
        self.counters.copy_(sd["counters"])
        if "ring" in sd:
            self.ring.copy_(sd["ring"])
            if self.ends is not None:
                self.ends.copy_(sd["ends"])
        else:                            # no rows came along: the ring starts empty, the step and gradient counters go on
            self.ring.zero_()
            if self.ends is not None:
                self.ends.zero_()
            self.counters[CTR_CURSOR] = 0; self.counters[CTR_SIZE] = 0
        if self.prioritized:             # rows that come without priorities enter as new rows do, with a leaf of 1.0; no rows: no leaves
            if "ring" in sd and "prio" in sd:
                self.prio.copy_(sd["prio"]); self.per_state.copy_(sd["per_state"])
            else:
                filled = min(max(int(sd["counters"][CTR_SIZE]), 0), self.capacity) if "ring" in sd else 0
                self.prio.zero_()
                self.prio[:filled] = 1.0
                self.per_state.copy_(torch.tensor([1.0, 0.0, math.inf, 0.0]))
            self.rebuild()


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
        self.buffer = ReplayBufferDevice(cfg.buffer_size, self.N, self.d, self.A, self.device, n_steps=cfg.n_steps, her_goals=cfg.her_goals,
                                         her_horizon=cfg.her_horizon, her_task=her_task, prioritized=cfg.prioritized, per_alpha=cfg.per_alpha,
                                         per_beta=cfg.per_beta, per_beta_steps=cfg.per_beta_steps, per_eps=cfg.per_eps)
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
        env = self.env
        if self.cfg.normalize_obs:       # the same launch with the observation normalised on load; obs_stage stays raw
            rms = self.normalizer.obs_rms
            _lib.check(_lib.lib().fw_sac_act_norm(_p(self._image_for_act()), _p(env.obs), int(env.torch_dtype == torch.float64), self.N, self.d,
                                                  self.A, self.cfg.hidden, int(mode), int(self.cfg.seed) & (2**64 - 1), self.env_offset,
                                                  _p(self.buffer.counters), _p(self.act_f32), _p(self.act_env), _p(self.obs_stage), _p(logp),
                                                  _p(eps), _p(rms.mean), _p(rms.var), self.cfg.clip_obs, self.cfg.norm_epsilon,
                                                  _stream(self.device)))
            return self.act_env
        _lib.check(_lib.lib().fw_sac_act(_p(self._image_for_act()), _p(env.obs), int(env.torch_dtype == torch.float64), self.N, self.d,
                                         self.A, self.cfg.hidden, int(mode), int(self.cfg.seed) & (2**64 - 1), self.env_offset,
                                         _p(self.buffer.counters), _p(self.act_f32), _p(self.act_env), _p(self.obs_stage), _p(logp), _p(eps),
                                         _stream(self.device)))
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
        if self.cfg.prioritized:         # sample -> weighted update -> priorities -> rebuild, all stream-ordered: one graph still
            self.buffer.sample(self.cfg.seed, self.batch, self.batch_idx, w_out=self.batch_w)
            self.normalize_batch(self.batch)
            self.fused.run(self.batch, self.buffer.counters, weights=self.batch_w, td_out=self.batch_td)
            self.buffer.update_priorities(self.batch_idx, self.batch_td)
            return
        self.buffer.sample(self.cfg.seed, self.batch, self.batch_idx, gamma=self.cfg.gamma)
        self.normalize_batch(self.batch)     # (behind the gather: hindsight rewards and n-step sums are formed on raw values)
        self.fused.run(self.batch, self.buffer.counters)

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
