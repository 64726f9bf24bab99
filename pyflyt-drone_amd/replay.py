"""The SAC replay ring (csrc/fwsim_replay.hpp, csrc/fwsim_per.hpp, include/fwsim.h): :class:`ReplayBufferDevice` and the contract of
every ring kernel restated in plain numpy / torch, which the GPU tests hold the kernels to bit for bit.  On the device:

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
                       restate their contracts).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib

MAX_N_STEPS = 16                                                # fw_replay_sample_nstep
END_TERMINATED, END_TRUNCATED = 1, 2                            # bits of the `ends` side ring
MAX_HER_HORIZON, HER_OBS_DIM, HER_ROW_FLOATS = 64, 21, 50       # fw_replay_sample_her: the low-level task with Euler attitude
HER_TAG = 0x5AC0E000                                            # the Philox tag of its second draw (kSacTagHer)
CTR_CURSOR, CTR_SIZE, CTR_STEPS, CTR_GRAD = 0, 1, 2, 3          # the device counters (int64[4])
PER_GROUP, PER_MAX_CAPACITY = 256, 1 << 22                      # prioritized replay: entries per group of a level; rows at most
PER_MAX, PER_TOTAL, PER_MIN = 0, 1, 2                           # per_state (float32[4]): running max leaf, total, smallest positive leaf

_p, _stream = _lib.devptr, _lib.stream


def _whole(name: str, v, lo: int, hi: Optional[int] = None) -> int:          # v as an int: a whole number (no bool) in [lo, hi]
    if isinstance(v, bool) or int(v) != v or int(v) < lo or (hi is not None and int(v) > hi):
        raise ValueError(f"{name} must be " + ("a non-negative integer" if hi is None else f"an integer in [{lo}, {hi}]") + f", got {v!r}")
    return int(v)


def check_sampler_options(n_steps, her_goals, her_horizon, prioritized, per_alpha, per_beta, per_beta_steps, per_eps):
    """The ring's sampler options, validated once for ``SACConfig`` and :class:`ReplayBufferDevice` alike: the same eight values with
    their types settled, or ``ValueError``.  At most one of n-step returns, hindsight goals and prioritized replay is built at a time."""
    if not (0.0 <= float(per_alpha) <= 1.0 and 0.0 <= float(per_beta) <= 1.0):
        raise ValueError(f"per_alpha and per_beta must lie in [0, 1], got {per_alpha!r} and {per_beta!r}")
    per_beta_steps = _whole("per_beta_steps", per_beta_steps, 0)
    if not (float(per_eps) > 0.0 and math.isfinite(float(per_eps))):
        raise ValueError(f"per_eps must be positive, got {per_eps!r}")
    her_goals = _whole("her_goals", her_goals, 0)
    her_horizon = _whole("her_horizon", her_horizon, 1, MAX_HER_HORIZON)
    n_steps = _whole("n_steps", n_steps, 1, MAX_N_STEPS)
    if her_goals > 0 and n_steps > 1:
        raise ValueError("her_goals > 0 together with n_steps > 1 is not built: the relabelled gather forms 1-step transitions only")
    if prioritized and (n_steps > 1 or her_goals > 0):
        raise ValueError("prioritized together with n_steps > 1 or her_goals > 0 is not built: those gathers draw their own indices")
    return n_steps, her_goals, her_horizon, bool(prioritized), float(per_alpha), float(per_beta), per_beta_steps, float(per_eps)


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


def _ring_args(ring, ends, cursor, size, N, idx, rows, limit):
    """What both row references take, as the kernels see it: ``(ring, ends, capacity, R, N, idx, newest)`` -- float32 / uint8 arrays,
    ``idx`` int64 [B] inside ``[0, size)``, and the first row of the newest vec-step stored, ``(cursor - N) mod capacity`` with the
    cursor normalised as ``fw_replay_store`` does.  ``rows``: (does the sampler take rows of R floats, in words); ``limit``: (name, value, max)."""
    import numpy as np
    if not 1 <= int(limit[1]) <= limit[2]:
        raise ValueError(f"{limit[0]} must be in [1, {limit[2]}]")
    ring, ends = np.asarray(ring, dtype=np.float32), np.asarray(ends, dtype=np.uint8)
    capacity, R = ring.shape
    N = int(N)
    if N <= 0 or capacity % N or ends.shape != (capacity,) or not rows[0](R):
        raise ValueError(f"capacity must be a multiple of N, ends one byte per row and a row {rows[1]} floats")
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= max(int(size), 1)):
        raise ValueError("idx must lie in [0, size)")
    cursor = int(cursor)
    if cursor < 0 or cursor + N > capacity:
        cursor = 0
    return ring, ends, capacity, R, N, idx, (cursor - N + capacity) % capacity


def _walk(i, limit, ends, N, capacity, newest):
    """``replay_walk`` (csrc/fwsim_replay.hpp): k, how many rows ``row_j = (i + j N) mod capacity`` a gather that starts at row ``i`` may use.
    row_j is used, then the walk stops if ``j + 1 == limit``, ``ends[row_j] != 0`` or row_j lies in the newest vec-step stored."""
    k = 0
    while True:
        row = (int(i) + k * N) % capacity
        k += 1
        if k == limit or ends[row] != 0 or row - row % N == newest:
            return k


def nstep_rows_reference(ring, ends, cursor, size, N, idx, n_steps, gamma, obs_dim):
    """``fw_replay_sample_nstep`` in plain numpy on CPU arrays: ``(rows [B, R] float32, k [B] int32)`` of the start rows ``idx``.

    ``ring`` ``[capacity, R]`` float32, ``ends`` ``[capacity]`` uint8, ``cursor`` / ``size`` the first two device counters, ``N`` the env
    count (env e's consecutive steps are N rows apart), ``obs_dim`` locates the reward column of a row (R = 2 obs_dim + act_dim + 2).
    :func:`_walk` with ``n_steps`` as its limit gives k, the rows used.  ``g_0 = 1`` and ``g_j = g_(j-1) gamma`` in float32 (gamma
    itself rounded to float32, as the entry point receives it): obs | action from row_0, reward ``r_0 + g_1 r_1 + ... + g_(k-1) r_(k-1)``
    in float32 in ascending j, next_obs from row_(k-1), last column ``1 - (1 - done_(k-1)) g_(k-1)``.  The kernel adds each term with
    one fused multiply-add, this function with a rounded product and a rounded sum: the two rewards differ by roundings only
    (tests/test_sac_nstep_gpu.py)."""
    import numpy as np
    n_steps, d = int(n_steps), int(obs_dim)
    ring, ends, capacity, R, N, idx, newest = _ring_args(ring, ends, cursor, size, N, idx, (lambda R: R >= 2 * d + 3, "2 obs_dim + act_dim + 2"),
                                                         ("n_steps", n_steps, MAX_N_STEPS))
    rcol, one, gam = R - d - 2, np.float32(1.0), np.float32(gamma)
    rows, ks = np.empty((idx.size, R), dtype=np.float32), np.empty(idx.size, dtype=np.int32)
    for b, i in enumerate(idx):
        k = _walk(i, n_steps, ends, N, capacity, newest)
        g, ret = one, ring[i, rcol]
        for j in range(1, k):
            g = np.float32(g * gam)
            ret = np.float32(ret + np.float32(g * ring[(int(i) + j * N) % capacity, rcol]))
        last = (int(i) + (k - 1) * N) % capacity
        rows[b, :rcol] = ring[i, :rcol]
        rows[b, rcol] = ret
        rows[b, rcol + 1:R - 1] = ring[last, rcol + 1:R - 1]
        rows[b, R - 1] = np.float32(one - np.float32(np.float32(one - ring[last, R - 1]) * g))
        ks[b] = k
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
    words ``(b, 0, gs, gs >> 32 ^ HER_TAG)``).  A row that is not relabelled is the ring row and its ``j`` is -1.  Otherwise :func:`_walk`
    with ``horizon`` as its limit gives k, the candidate rows; ``j* = (j_star_draw k) >> 32``, the goal ``g'`` is
    :func:`her_achieved_goal` of ``row_j*``'s next_obs, it replaces columns 18:21 of obs and of next_obs, and the reward column is
    :func:`her_reward_reference` of (row_0's next_obs, ``g'``, row_0's done) rounded to float32.  Everything else is row_0."""
    import numpy as np
    horizon, d = int(horizon), HER_OBS_DIM
    ring, ends, capacity, R, N, idx, newest = _ring_args(ring, ends, cursor, size, N, idx, (lambda R: R == HER_ROW_FLOATS, HER_ROW_FLOATS),
                                                         ("horizon", horizon, MAX_HER_HORIZON))
    relabel, draw = np.asarray(relabel).reshape(-1) != 0, np.asarray(j_star_draw).reshape(-1)
    if relabel.shape != idx.shape or draw.shape != idx.shape:
        raise ValueError("relabel and j_star_draw must have one entry per row of idx")
    rcol, nobs = R - d - 2, R - d - 1
    rows, js = ring[idx].copy(), np.full(idx.size, -1, dtype=np.int32)
    for b, i in enumerate(idx):
        if not relabel[b]:
            continue
        j = (int(draw[b]) * _walk(i, horizon, ends, N, capacity, newest)) >> 32
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
        (self.n_steps, self.her_goals, self.her_horizon, self.prioritized, self.per_alpha, self.per_beta, self.per_beta_steps,
         self.per_eps) = check_sampler_options(n_steps, her_goals, her_horizon, prioritized, per_alpha, per_beta, per_beta_steps, per_eps)
        self.her_task, self.her_prob = her_task, self.her_goals / (self.her_goals + 1.0)
        if self.her_goals > 0 and (her_task is None or int(obs_dim) != HER_OBS_DIM or row_floats(obs_dim, act_dim) != HER_ROW_FLOATS):
            raise ValueError(f"her_goals > 0 needs her_task and the low-level task's rows ({HER_OBS_DIM} observations, {HER_ROW_FLOATS} floats)")
        self.num_envs, self.obs_dim, self.act_dim = int(num_envs), int(obs_dim), int(act_dim)
        self.capacity, self.row = ring_capacity(buffer_size, num_envs), row_floats(obs_dim, act_dim)
        self.ring = torch.zeros((self.capacity, self.row), dtype=torch.float32, device=device)
        self.counters = torch.zeros(4, dtype=torch.int64, device=device)
        self.ends = torch.zeros(self.capacity, dtype=torch.uint8, device=device) if self.n_steps > 1 or self.her_goals > 0 else None
        self.prio = self.sum1 = self.min1 = self.sum2 = self.min2 = self.per_state = None
        self._sampler = (self._sample_per if self.prioritized else self._sample_her if self.her_goals > 0
                         else self._sample_nstep if self.n_steps > 1 else self._sample_uniform)
        if self.prioritized:
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

    @classmethod
    def from_config(cls, cfg, num_envs: int, obs_dim: int, act_dim: int, device, her_task: Optional[HerTask] = None):
        """The ring a ``SACConfig`` asks for."""
        return cls(cfg.buffer_size, num_envs, obs_dim, act_dim, device, n_steps=cfg.n_steps, her_goals=cfg.her_goals,
                   her_horizon=cfg.her_horizon, her_task=her_task, prioritized=cfg.prioritized, per_alpha=cfg.per_alpha,
                   per_beta=cfg.per_beta, per_beta_steps=cfg.per_beta_steps, per_eps=cfg.per_eps)

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
        _lib.check(_lib.lib().fw_replay_store(_p(self.ring), self.capacity, _p(self.counters), _p(obs_stage), _p(act_f32), _p(reward), _p(next_obs),
                                              _p(terminal_obs), _p(terminated), _p(truncated), int(reward.dtype == torch.float64), self.num_envs,
                                              self.obs_dim, self.act_dim, _stream(self.ring.device)))
        if self.prioritized:
            self.rebuild()

    def _sample_uniform(self, gamma, k_out, j_out, w_out):          # per mode: the entry point, and its arguments behind the common ones
        return _lib.lib().fw_replay_sample, ()

    def _sample_nstep(self, gamma, k_out, j_out, w_out):
        if gamma is None:
            raise ValueError("an n-step sample needs gamma")
        return _lib.lib().fw_replay_sample_nstep, (_p(self.ends), self.obs_dim, self.num_envs, self.n_steps, float(gamma), _p(k_out))

    def _sample_her(self, gamma, k_out, j_out, w_out):
        return _lib.lib().fw_replay_sample_her, (_p(self.ends), self.obs_dim, self.num_envs, self.her_horizon, float(self.her_prob),
                                                 C.byref(self.her_task), _p(j_out))

    def _sample_per(self, gamma, k_out, j_out, w_out):
        return _lib.lib().fw_replay_sample_per, (_p(w_out), _p(self.prio), _p(self.sum1), _p(self.sum2), _p(self.per_state), self.per_beta,
                                                 self.per_beta_steps)

    def sample(self, seed: int, out: torch.Tensor, idx_out: Optional[torch.Tensor] = None, gamma: Optional[float] = None,
               k_out: Optional[torch.Tensor] = None, j_out: Optional[torch.Tensor] = None, w_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A batch into ``out``.  With ``n_steps > 1``: n-step transitions, which need ``gamma`` (``k_out`` [B] int32 receives the
        rows each one spans).  With ``her_goals > 0``: 1-step transitions, relabelled with probability ``her_prob`` (``j_out`` [B] int32
        receives -1, or how many steps ahead the goal was achieved).  With ``prioritized``: rows drawn in proportion to their leaves
        (``w_out`` [B] float32 receives the importance weights)."""
        if w_out is not None and not self.prioritized:
            raise ValueError("w_out is written by a prioritized buffer's sample")
        entry, tail = self._sampler(gamma, k_out, j_out, w_out)
        _lib.check(entry(_p(self.ring), self.capacity, _p(self.counters), int(seed) & (2**64 - 1), self.row, out.shape[0], _p(out), _p(idx_out),
                         *tail, _stream(self.ring.device)))
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
