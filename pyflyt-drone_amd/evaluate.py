"""Evaluation harness: the reference's acceptance metrics on the device envs.

Mirrors, for the device-resident envs:

* SB3 ``evaluate_policy(model, eval_env, n_eval_episodes, deterministic=True,
  return_episode_rewards=True, callback=...)`` as the reference calls it
  (train/train_Fixedwing_Waypoints_v3.py:161-170): episodes are counted per env with the
  targets ``(n_eval_episodes + i) // n_envs`` so that short episodes of fast envs do not bias
  the sample, rewards are the *un-normalised* env rewards, observations are normalised with
  frozen statistics (``training=False, norm_reward=False`` eval wrapper, ``:264-270``);
* ``sync_envs_normalization`` before every evaluation (``:146-150``);
* the logged scalars of ``WaypointEvalCallback._on_step`` (``:196-214``): ``eval/mean_reward``,
  ``eval/mean_ep_length``, ``eval/wp{i}_reach_rate`` = mean(num_targets_reached >= i),
  ``eval/success_rate`` = mean(is_success); the ObjLock scripts add ``duck_strike_rate``
  (train/train_objlock.py:163-167, eval/eval_objlock.py:260-325);
* ``evaluations.npz`` (timesteps / results / ep_lengths / successes) and ``best_model`` on a
  new best mean reward (``:172-190, 216-222``);
* for the low-level control task, the figures of eval/eval_lowlevel.py: heading / altitude / airspeed
  tracking error (MAE, RMSE, pooled over every evaluated step), mean angular-rate norm, survival rate
  (:meth:`EvalResult.tracking_scalars`, definitions in DESIGN.md section 2d);
* for the high-level command task, figures the reference has no script for (build-owned, DESIGN.md section 2e "Evaluation"): how
  the frozen controller follows the commander's commands, how much the commands jump from step to step, how often they sit on a
  bound of the action Box and how many actions were rejected as non-finite (:meth:`EvalResult.command_scalars`);
* for the waypoint, ObjLock and combined tasks, on request (``path_figures=True``), figures of the flight itself (build-owned,
  DESIGN.md section 2f): path length, airspeed, altitude, control activity, time to the targets, path efficiency and the closest
  approach to a target that was not reached (:meth:`EvalResult.path_scalars`).

Everything per step stays on the device; the host reads one small ``dones`` mask per
vec-step (the episode bookkeeping is host-side like SB3's).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from . import _lib, evalstep
from . import config as K
from ._lib import devptr as _p, stream as _stream
from .rollout import clip_actions, policy_inputs


def sync_envs_normalization(train_env, eval_env) -> None:
    """Copy the running statistics of the training wrapper into the eval wrapper
    (SB3 ``sync_envs_normalization``)."""
    eval_env.obs_rms.load_state_dict(train_env.obs_rms.state_dict())
    eval_env.ret_rms.load_state_dict(train_env.ret_rms.state_dict())


# FW_TASK_LOWLEVEL's per-episode tracking sums, in the column order of fw_eval_track_ll's cur_track / fin_track
TRACK_SUMS = ("heading_abs", "heading_sq", "altitude_abs", "altitude_sq", "airspeed_abs", "airspeed_sq", "ang_vel")


# the keys of EvalResult.path_scalars (without "eval/"), in the order the evaluation log keeps them
PATH_SCALARS = ("airspeed_mean", "altitude_mean", "ang_vel_mean", "throttle_mean", "action_delta_mean", "path_length_mean", "altitude_min",
                "time_to_first_target_s", "time_per_target_s", "path_efficiency", "miss_distance_mean")


def _track_terms(o: torch.Tensor) -> torch.Tensor:
    """[N, 7] per-step terms of TRACK_SUMS from post-step observation rows ``o`` [N, 21], in double: the
    torch statement of what fw_eval_track_ll adds up."""
    o = o.to(torch.float64)
    e_psi = torch.remainder(o[:, 18] - o[:, 5] + math.pi, 2 * math.pi) - math.pi      # Python's (a + pi) % (2 pi) - pi
    e_h = o[:, 19] - o[:, 11]
    e_v = o[:, 20] - torch.sqrt(o[:, 6] * o[:, 6] + o[:, 7] * o[:, 7] + o[:, 8] * o[:, 8])
    w = torch.sqrt(o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] + o[:, 2] * o[:, 2])
    return torch.stack([e_psi.abs(), e_psi * e_psi, e_h.abs(), e_h * e_h, e_v.abs(), e_v * e_v, w], dim=1)


# the high-level command task's per-episode sums, in the column order of fw_eval_track_hl's cur_track / fin_track: the seven of
# TRACK_SUMS taken against the commander's command, the step-to-step command changes and the steps with a command on a Box bound
HL_TRACK_SUMS = TRACK_SUMS + ("dcmd_heading", "dcmd_altitude", "dcmd_airspeed", "saturated")


def _wrap_pi(a: torch.Tensor) -> torch.Tensor:
    return torch.remainder(a + math.pi, 2 * math.pi) - math.pi          # Python's (a + pi) % (2 pi) - pi


def _track_terms_hl(o: torch.Tensor, c: torch.Tensor, p: torch.Tensor, first: torch.Tensor, alt_high: float,
                    speed_high: float) -> torch.Tensor:
    """[N, 11] per-step terms of HL_TRACK_SUMS (DESIGN.md section 2e "Evaluation"), in double: the torch statement of what
    fw_eval_track_hl adds up.  ``o`` [N, 30] post-step observation rows, ``c`` [N, 3] the conditioned commands in force during the
    step, ``p`` [N, 3] the commands of the step before, ``first`` [N] bool: the step opens an episode (no previous command: the
    three changes are 0).  ``alt_high`` / ``speed_high``: the upper bounds of the action Box.  Works on CPU tensors."""
    o, c, p = o.to(torch.float64), c.to(torch.float64), p.to(torch.float64)
    e_psi = _wrap_pi(c[:, 0] - o[:, 5])
    e_h = c[:, 1] - o[:, 11]
    e_v = c[:, 2] - torch.sqrt(o[:, 6] * o[:, 6] + o[:, 7] * o[:, 7] + o[:, 8] * o[:, 8])
    w = torch.sqrt(o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] + o[:, 2] * o[:, 2])
    zero = torch.zeros_like(w)
    d_psi = torch.where(first, zero, _wrap_pi(c[:, 0] - p[:, 0]).abs())
    d_h = torch.where(first, zero, (c[:, 1] - p[:, 1]).abs())
    d_v = torch.where(first, zero, (c[:, 2] - p[:, 2]).abs())
    sat = ((c[:, 1] <= 0.0) | (c[:, 1] >= alt_high) | (c[:, 2] <= 0.0) | (c[:, 2] >= speed_high)).to(torch.float64)
    return torch.stack([e_psi.abs(), e_psi * e_psi, e_h.abs(), e_h * e_h, e_v.abs(), e_v * e_v, w, d_psi, d_h, d_v, sat], dim=1)


def _hl_bounds(venv):
    """(alt_high, speed_high) of a HighLevelCmdVecEnv's action Box when the command figures apply to ``venv`` (its 30-value
    observation), else None"""
    if not evalstep.is_highlevel(venv):
        return None
    from .highlevel import AIRSPEED_HIGH
    return float(venv.cfg.flight_dome_size), float(AIRSPEED_HIGH)


def _path_layout(venv):
    """the row layout of ``venv`` for ``path_figures=True``, or ValueError for an env it is not meant for"""
    from .flight import RowLayout
    if _hl_bounds(venv) is not None or hasattr(venv, "step_low"):
        raise ValueError("path_figures: the high-level command task has its own figures (command_scalars)")
    cfg = getattr(venv, "cfg", None)
    if cfg is None or not hasattr(venv, "terminal_obs"):
        raise ValueError("path_figures needs a waypoints, ObjLock, combined or direct-command waypoints device env")
    if cfg.task == K.FW_TASK_LOWLEVEL:
        raise ValueError("path_figures: the low-level task has its own figures (tracking_scalars)")
    return RowLayout.of(cfg)


def _path_complete(info_row) -> bool:
    return info_row is not None and bool(info_row[K.INFO_ENV_COMPLETE] or info_row[K.INFO_DUCK_STRIKE])


@dataclass
class EvalResult:
    episode_rewards: List[float]
    episode_lengths: List[int]
    num_targets_reached: List[int] = field(default_factory=list)
    is_success: List[bool] = field(default_factory=list)
    duck_strike: List[bool] = field(default_factory=list)
    # FW_TASK_LOWLEVEL only: per episode, the sums over its steps of |e_psi|, e_psi^2, |e_h|, e_h^2, |e_V|, e_V^2 and the
    # angular-rate norm (TRACK_SUMS), and survived = not terminated (a truncated episode survived)
    heading_abs: List[float] = field(default_factory=list)
    heading_sq: List[float] = field(default_factory=list)
    altitude_abs: List[float] = field(default_factory=list)
    altitude_sq: List[float] = field(default_factory=list)
    airspeed_abs: List[float] = field(default_factory=list)
    airspeed_sq: List[float] = field(default_factory=list)
    ang_vel: List[float] = field(default_factory=list)
    survived: List[bool] = field(default_factory=list)
    # the high-level command task only (HL_TRACK_SUMS): the seven lists above hold the sums against the commander's commands
    # (survived stays empty); per episode the summed |command change| of each component, the number of steps with the altitude or
    # airspeed command on a bound of the action Box; and, for the whole evaluation, the actions rejected as non-finite
    dcmd_heading: List[float] = field(default_factory=list)
    dcmd_altitude: List[float] = field(default_factory=list)
    dcmd_airspeed: List[float] = field(default_factory=list)
    saturated: List[float] = field(default_factory=list)
    rejected_actions: int = 0
    # path_figures=True only (flight.PATH_SUMS): per episode the twelve path sums, and whether the episode ended
    # with env_complete or a duck strike (its closest approach then says nothing about a miss)
    path_len: List[float] = field(default_factory=list)
    speed_sum: List[float] = field(default_factory=list)
    alt_sum: List[float] = field(default_factory=list)
    alt_min: List[float] = field(default_factory=list)
    ang_vel_sum: List[float] = field(default_factory=list)
    act_delta_sum: List[float] = field(default_factory=list)
    throttle_sum: List[float] = field(default_factory=list)
    first_reach_step: List[float] = field(default_factory=list)
    last_reach_step: List[float] = field(default_factory=list)
    chord_len: List[float] = field(default_factory=list)
    path_at_last_reach: List[float] = field(default_factory=list)
    miss_dist: List[float] = field(default_factory=list)
    path_complete: List[bool] = field(default_factory=list)

    def add_path(self, sums, complete: bool = False) -> None:
        from .flight import PATH_SUMS
        for name, v in zip(PATH_SUMS, sums):
            getattr(self, name).append(float(v))
        self.path_complete.append(bool(complete))

    def add_command(self, sums) -> None:
        for name, v in zip(HL_TRACK_SUMS, sums):
            getattr(self, name).append(float(v))

    def add_tracking(self, sums, survived: bool) -> None:
        for name, v in zip(TRACK_SUMS, sums):
            getattr(self, name).append(float(v))
        self.survived.append(bool(survived))

    @property
    def mean_reward(self) -> float: return float(np.mean(self.episode_rewards))
    @property
    def std_reward(self) -> float: return float(np.std(self.episode_rewards))
    @property
    def mean_ep_length(self) -> float: return float(np.mean(self.episode_lengths))
    @property
    def std_ep_length(self) -> float: return float(np.std(self.episode_lengths))

    def scalars(self, num_targets_total: int = 0, has_duck: bool = False) -> Dict[str, float]:
        """The ``eval/*`` scalars the reference's callbacks record."""
        out = {"eval/mean_reward": self.mean_reward, "eval/mean_ep_length": self.mean_ep_length}
        if self.num_targets_reached and num_targets_total > 0:
            reached = np.asarray(self.num_targets_reached, dtype=np.float64)
            for i in range(1, num_targets_total + 1):
                out[f"eval/wp{i}_reach_rate"] = float(np.mean(reached >= i))
        if self.is_success:
            out["eval/success_rate"] = float(np.mean(self.is_success))
        if has_duck and self.duck_strike:
            out["eval/duck_strike_rate"] = float(np.mean(self.duck_strike))
        return out

    def tracking_scalars(self) -> Dict[str, float]:
        """The low-level controller's figures (eval/eval_lowlevel.py): MAE = sum |e| / sum L and RMSE = sqrt(sum e^2 / sum L), pooled
        over every evaluated step as the reference's ``extend`` does, the mean angular-rate norm likewise, and the survival rate
        over episodes.  Empty for the other tasks."""
        if not self.survived:
            return {}
        steps = float(np.sum(self.episode_lengths))
        out = {}
        for q in ("heading", "altitude", "airspeed"):
            out[f"eval/{q}_mae"] = float(np.sum(getattr(self, q + "_abs"))) / steps
            out[f"eval/{q}_rmse"] = math.sqrt(float(np.sum(getattr(self, q + "_sq"))) / steps)
        out["eval/ang_vel_mean"] = float(np.sum(self.ang_vel)) / steps
        out["eval/survival_rate"] = float(np.mean(self.survived))
        return out

    def command_scalars(self) -> Dict[str, float]:
        """The high-level command task's figures (build-owned, DESIGN.md section 2e "Evaluation"), pooled over every evaluated step
        as :meth:`tracking_scalars` pools: ``cmd_*_mae`` / ``cmd_*_rmse`` = how far the flight was from the commander's command,
        ``ang_vel_mean``, ``cmd_*_delta`` = sum |command change| / (sum L - episodes) (0.0 when no episode has a second step),
        ``cmd_saturation_rate`` = steps with the altitude or airspeed command on a Box bound / sum L, ``rejected_actions``.  Empty for
        the other tasks."""
        if not self.saturated:
            return {}
        steps = float(np.sum(self.episode_lengths))
        pairs = steps - float(len(self.episode_lengths))
        out = {}
        for q in ("heading", "altitude", "airspeed"):
            out[f"eval/cmd_{q}_mae"] = float(np.sum(getattr(self, q + "_abs"))) / steps
            out[f"eval/cmd_{q}_rmse"] = math.sqrt(float(np.sum(getattr(self, q + "_sq"))) / steps)
        out["eval/ang_vel_mean"] = float(np.sum(self.ang_vel)) / steps
        for q in ("heading", "altitude", "airspeed"):
            out[f"eval/cmd_{q}_delta"] = float(np.sum(getattr(self, "dcmd_" + q))) / pairs if pairs > 0 else 0.0
        out["eval/cmd_saturation_rate"] = float(np.sum(self.saturated)) / steps
        out["eval/rejected_actions"] = float(self.rejected_actions)
        return out

    def path_scalars(self, agent_hz: float, complete=None) -> Dict[str, float]:
        """The flight's figures (build-owned) from the path sums of ``path_figures=True``; empty without them.
        Pooled over every evaluated step, as :meth:`tracking_scalars` pools: ``airspeed_mean``, ``altitude_mean``, ``ang_vel_mean``,
        ``throttle_mean``, ``action_delta_mean`` = sum of the per-step sum / sum L.  Over episodes: ``path_length_mean``;
        ``altitude_min``, the minimum over episodes; over the episodes that reached a target (absent when none did)
        ``time_to_first_target_s`` = mean first_reach_step / agent_hz, ``time_per_target_s`` = sum last_reach_step / sum targets reached
        / agent_hz, ``path_efficiency`` = sum chord_len / sum path_at_last_reach; ``miss_distance_mean`` over the episodes that ended
        neither with env_complete nor with a duck strike (``complete``: one bool per episode, default what ``add_path`` was told) and
        whose closest approach is finite (absent when there is none)."""
        if not self.path_len:
            return {}
        hz = float(agent_hz)
        steps = float(np.sum(self.episode_lengths))
        out = {"eval/airspeed_mean": float(np.sum(self.speed_sum)) / steps, "eval/altitude_mean": float(np.sum(self.alt_sum)) / steps,
               "eval/ang_vel_mean": float(np.sum(self.ang_vel_sum)) / steps, "eval/throttle_mean": float(np.sum(self.throttle_sum)) / steps,
               "eval/action_delta_mean": float(np.sum(self.act_delta_sum)) / steps,
               "eval/path_length_mean": float(np.mean(self.path_len)), "eval/altitude_min": float(np.min(self.alt_min))}
        first, last = np.asarray(self.first_reach_step, dtype=np.float64), np.asarray(self.last_reach_step, dtype=np.float64)
        hit = first > 0
        if hit.any():
            out["eval/time_to_first_target_s"] = float(np.mean(first[hit] / hz))
            if len(self.num_targets_reached) == len(first):
                n_reached = float(np.asarray(self.num_targets_reached, dtype=np.float64)[hit].sum())
                if n_reached > 0:
                    out["eval/time_per_target_s"] = float(last[hit].sum()) / n_reached / hz
            at = float(np.asarray(self.path_at_last_reach, dtype=np.float64)[hit].sum())
            if at > 0:
                out["eval/path_efficiency"] = float(np.asarray(self.chord_len, dtype=np.float64)[hit].sum()) / at
        comp = np.asarray(self.path_complete if complete is None else complete, dtype=bool)
        miss = np.asarray(self.miss_dist, dtype=np.float64)
        keep = ~comp & np.isfinite(miss)
        if keep.any():
            out["eval/miss_distance_mean"] = float(np.mean(miss[keep]))
        return out


def _targets(n_eval_episodes: int, n: int) -> np.ndarray:
    """episodes wanted of each of ``n`` envs: SB3's ``(n_eval_episodes + i) // n_envs``"""
    return np.array([(n_eval_episodes + i) // n for i in range(n)], dtype=np.int64)


@torch.no_grad()
def evaluate_policy(policy, env, n_eval_episodes: int = 10, deterministic: bool = True,
                    callback: Optional[Callable[[dict], None]] = None, max_vec_steps: Optional[int] = None,
                    generator: Optional[torch.Generator] = None, use_graph: Optional[bool] = None,
                    use_fused: Optional[bool] = None, path_figures: bool = False) -> EvalResult:
    """Run ``policy`` on ``env`` (a :class:`~.rollout.VecNormalizeDevice` over a device env,
    normally with ``training=False, norm_reward=False``) until ``n_eval_episodes`` episodes are
    complete.  ``callback(info_dict)`` is called for every finished episode with the keys the
    reference's callbacks read (``num_targets_reached``, ``is_success``, ``duck_strike``, ...).

    Deterministic evaluations on the GPU run as replays of a captured hipGraph of 8 vec-steps with the episode bookkeeping
    on the device (``use_graph``; default: whenever possible): an evaluation of 16 envs flying 1800-step episodes is ~30
    framework ops per step, and read back after every step it cost as much wall clock as 0.4 M training steps.  Both paths
    return the same episodes in the same order; ``callback`` is then called once the evaluation is over.

    ``use_fused`` (default: whenever possible -- the reference's MlpPolicy on a device env with the 8-lane mapping, an
    evaluation normaliser with frozen statistics): a vec-step of the replayed evaluation is ONE ``fw_collect_step`` launch in
    its deterministic, statistics-frozen form (normalisation, policy forward on the matrix cores, clip, env step) instead of
    ~20 framework ops; the policy's actions then agree with the torch forward to fp32 rounding, not to the bit.  The low-level task's
    six-action MlpPolicy (either lane mapping) keeps the torch forward by default; ``use_fused=True`` makes its vec-step three launches
    (``fw_collect_act_a`` -> ``fw_step`` -> ``fw_eval_track_ll``).

    For the low-level control task the result also carries the per-episode tracking sums and survival
    (:meth:`EvalResult.tracking_scalars`): from torch ops in the step-by-step loop, from ``fw_eval_track_ll`` in the replayed one.

    For the high-level command task (``HighLevelCmdVecEnv``) it carries the command figures (:meth:`EvalResult.command_scalars`):
    from torch ops (``_track_terms_hl``) in the step-by-step loop, from ``fw_eval_track_hl`` in the replayed one.  Its three-action
    MlpPolicy keeps the torch forward by default; ``use_fused=True`` makes a vec-step ``fw_collect_act_hl`` -> ``fw_step`` ->
    ``fw_eval_track_hl``.  ``venv.rejected`` is zeroed when the evaluation begins and read once at its end
    (``EvalResult.rejected_actions``: every env-step the evaluation ran counts, the ones past an env's last wanted episode too).

    ``path_figures=True`` (the waypoint, ObjLock, combined and direct-command waypoints tasks; ``ValueError`` for the low- and
    high-level tasks): the result also carries the twelve path sums of every episode (:meth:`EvalResult.path_scalars`, DESIGN.md
    section 2f): from torch ops (``flight.path_step``) in the step-by-step loop, from ``fw_eval_track_wp`` -- in place of
    ``fw_eval_track`` / the framework ops -- in the replayed one, on its torch-forward and on its ``fw_collect_step`` body."""
    venv = env.venv
    n = env.num_envs
    path_layout = _path_layout(venv) if path_figures else None
    targets = _targets(n_eval_episodes, n)
    if use_graph is None:
        use_graph = (deterministic and generator is None and torch.device(env.device).type == "cuda" and hasattr(venv, "step_tensor")
                     and not getattr(policy, "uses_image", False))        # (a CNN front end keeps MIOpen out of captures)
    if use_graph:
        return ReplayedEvaluation(policy, env, targets, callback, use_fused=use_fused, path_figures=path_figures).run(max_vec_steps)
    counts = np.zeros(n, dtype=np.int64)
    cur_rew = torch.zeros(n, dtype=torch.float64, device=env.device)
    cur_len = torch.zeros(n, dtype=torch.int64, device=env.device)
    res = EvalResult([], [])
    has_info = hasattr(venv, "info")
    is_objlock = getattr(getattr(venv, "cfg", None), "task", K.FW_TASK_WAYPOINTS) in (K.FW_TASK_OBJLOCK, K.FW_TASK_WAYPOINT_OBJLOCK)
    track = getattr(getattr(venv, "cfg", None), "task", K.FW_TASK_WAYPOINTS) == K.FW_TASK_LOWLEVEL
    cur_trk = torch.zeros((n, len(TRACK_SUMS)), dtype=torch.float64, device=env.device) if track else None
    hl = _hl_bounds(venv)
    if hl is not None:
        cur_hl = torch.zeros((n, len(HL_TRACK_SUMS)), dtype=torch.float64, device=env.device)
        prev_cmd = torch.zeros((n, 3), dtype=torch.float64, device=env.device)
        venv.rejected.zero_()
    obs = env.reset()
    if path_layout is not None:
        from . import flight
        cur_path, carry = flight.path_init(n, env.device), flight.seed_carry(venv.obs, path_layout)
    steps = 0
    while (counts < targets).any():
        actions, _, _ = policy(obs, deterministic=deterministic, generator=generator, **policy_inputs(policy, env))
        clipped = clip_actions(actions, venv).to(venv.torch_dtype)
        obs, _, dones, _, _ = env.step(clipped)
        cur_rew += venv.rewards.to(torch.float64)        # un-normalised reward of the wrapped env
        if hl is not None:                               # venv.command: the triple that was in force during the step
            cur_hl += _track_terms_hl(torch.where(dones[:, None], venv.terminal_obs, venv.obs), venv.command, prev_cmd, cur_len == 0, *hl)
            prev_cmd = venv.command.to(torch.float64).clone()
        if path_layout is not None:                      # the post-step row; where the episode ended the live row seeds the next one
            cur_path, carry = flight.path_step(torch.where(dones[:, None], venv.terminal_obs, venv.obs),
                                               venv.info[:, K.INFO_NUM_TARGETS_REACHED] if has_info else None, cur_len == 0, cur_path,
                                               carry, path_layout, cur_len + 1)
            carry = torch.where(dones[:, None], flight.seed_carry(venv.obs, path_layout), carry)
        cur_len += 1
        if track:                                        # the post-step row: the terminal observation where the episode ended
            cur_trk += _track_terms(torch.where(dones[:, None], venv.terminal_obs, venv.obs))
        d = dones.cpu().numpy()
        if d.any():
            idx = np.nonzero(d)[0]
            rew_h, len_h = cur_rew.cpu().numpy(), cur_len.cpu().numpy()
            info_h = venv.info.cpu().numpy() if has_info else None
            trk_h, term_h = (cur_trk.cpu().numpy(), venv.terminated.cpu().numpy()) if track else (None, None)
            hl_h = cur_hl.cpu().numpy() if hl is not None else None
            path_h = cur_path.cpu().numpy() if path_layout is not None else None
            for i in idx:
                if counts[i] < targets[i]:
                    counts[i] += 1
                    res.episode_rewards.append(float(rew_h[i])); res.episode_lengths.append(int(len_h[i]))
                    if track:
                        res.add_tracking(trk_h[i], not term_h[i])
                    if hl_h is not None:
                        res.add_command(hl_h[i])
                    if path_h is not None:
                        res.add_path(path_h[i], _path_complete(info_h[i] if info_h is not None else None))
                    info = _episode_info(res, float(rew_h[i]), int(len_h[i]), info_h[i] if info_h is not None else None, is_objlock)
                    if callback is not None:
                        callback(info)
            m = torch.as_tensor(d, device=env.device)
            cur_rew.masked_fill_(m, 0.0); cur_len.masked_fill_(m, 0)
            if track:
                cur_trk.masked_fill_(m[:, None], 0.0)
            if hl is not None:
                cur_hl.masked_fill_(m[:, None], 0.0)
            if path_layout is not None:
                cur_path = torch.where(m[:, None], flight.path_init(n, env.device), cur_path)
        steps += 1
        if max_vec_steps is not None and steps >= max_vec_steps:
            break
    if hl is not None:
        res.rejected_actions = int(venv.rejected.item())
    return res


def _episode_info(res: "EvalResult", rew: float, length: int, info_row, is_objlock: bool) -> dict:
    info = {"episode": {"r": rew, "l": length}}
    if info_row is not None:
        info["num_targets_reached"] = int(info_row[K.INFO_NUM_TARGETS_REACHED])
        info["collision"] = bool(info_row[K.INFO_COLLISION])
        info["out_of_bounds"] = bool(info_row[K.INFO_OUT_OF_BOUNDS])
        info["env_complete"] = bool(info_row[K.INFO_ENV_COMPLETE])
        res.num_targets_reached.append(info["num_targets_reached"])
        if is_objlock:
            info["duck_strike"] = bool(info_row[K.INFO_DUCK_STRIKE])
            info["is_success"] = bool(info_row[K.INFO_IS_SUCCESS])
            res.duck_strike.append(info["duck_strike"])
        else:
            info["is_success"] = info["env_complete"]
        res.is_success.append(info["is_success"])
    return info


REPLAY_STEPS = 8


class ReplayedEvaluation:
    """evaluate_policy with the loop body captured: policy forward, env step, normalisation and the per-episode bookkeeping
    (reward / length accumulators, the slot of the episode that just ended, its info row) are device ops on fixed buffers.

    ``run()`` drives it from the host (one look at the episode counters per replay of ``REPLAY_STEPS`` steps).
    ``launch()`` enqueues the WHOLE evaluation on a side stream -- as many replays as the longest possible episodes need,
    ``episodes per env x (max_steps + 2)`` vec-steps -- and returns at once: the evaluation (a few envs) then runs beside the
    training that continues on the main stream (the PPO update keeps eight of the 256 CUs busy); ``ready()`` / ``result()``
    collect it.  The policy handed in must not change while it runs (EvalCallback evaluates a copy of the weights).

    The low-level control task's bookkeeping is one ``fw_eval_track_ll`` launch per vec-step, which also sums its tracking figures.
    ``use_fused=True`` with its six-action MlpPolicy: a vec-step is ``fw_collect_act_a`` (policy only, deterministic, frozen
    statistics) -> ``fw_step`` -> ``fw_eval_track_ll``, in sequence.

    The high-level command task's bookkeeping is one ``fw_eval_track_hl`` launch per vec-step, which also sums its command figures.
    ``use_fused=True`` with its three-action MlpPolicy (``step.kind == "act_hl"``): a vec-step is ``fw_collect_act_hl`` (commander and
    controller, policy nets only, deterministic, frozen statistics) -> ``fw_step`` (``step_low``) -> ``fw_eval_track_hl``, in sequence.

    ``path_figures=True`` (the waypoint, ObjLock, combined and direct-command waypoints tasks): the bookkeeping of a vec-step is one
    ``fw_eval_track_wp`` launch -- in place of the framework ops behind the torch forward, and of ``fw_eval_track`` behind
    ``fw_collect_step`` -- which also carries the twelve path sums of ``flight.PATH_SUMS``.  Off, nothing is launched that was not.

    ``step`` is the act and the env step (an :mod:`evalstep` object; ``step.kind`` names it, ``fused`` says it is not the torch forward)."""

    def __init__(self, policy, env, targets: np.ndarray, callback=None, use_fused: Optional[bool] = None, path_figures: bool = False):
        self.policy, self.env, self.callback = policy, env, callback
        venv, n, dev = env.venv, env.num_envs, env.device
        self.path_layout = _path_layout(venv) if path_figures else None
        # fw_collect_step by default where it applies; the six- and three-action policies get their fused act only on request
        kind = evalstep.select(policy, env, use_fused, evalstep.FUSED_KINDS, default="collect_step", refusal=(
            "use_fused=True needs the MlpPolicy, a device env on the 8-lane mapping (any mapping for the low-level task's six actions and "
            "for the high-level command task's three actions on its 30-value observation) and an evaluation normaliser (training=False)"))
        self.venv, self.n, self.dev, self.targets = venv, n, dev, targets
        self.E = E = max(int(targets.max()), 1)
        self.has_info = hasattr(venv, "info")
        task = getattr(getattr(venv, "cfg", None), "task", K.FW_TASK_WAYPOINTS)
        self.is_objlock = task in (K.FW_TASK_OBJLOCK, K.FW_TASK_WAYPOINT_OBJLOCK)
        self.track = task == K.FW_TASK_LOWLEVEL and hasattr(venv, "terminal_obs")
        self.tg = torch.as_tensor(targets, device=dev)
        self.ar = torch.arange(n, device=dev)
        self.counts = torch.zeros(n, dtype=torch.int64, device=dev)
        self.cur_rew = torch.zeros(n, dtype=torch.float64, device=dev)
        self.cur_len = torch.zeros(n, dtype=torch.int64, device=dev)
        self.step_ctr = torch.zeros((), dtype=torch.int64, device=dev)
        self.fin_rew = torch.zeros((n, E), dtype=torch.float64, device=dev)
        self.fin_len = torch.zeros((n, E), dtype=torch.int64, device=dev)
        self.fin_step = torch.zeros((n, E), dtype=torch.int64, device=dev)
        self.fin_info = torch.zeros((n, E, venv.info.shape[1]), dtype=venv.info.dtype, device=dev) if self.has_info else None
        if self.track:
            self.cur_track = torch.zeros((n, len(TRACK_SUMS)), dtype=torch.float64, device=dev)
            self.fin_track = torch.zeros((n, E, len(TRACK_SUMS) + 1), dtype=torch.float64, device=dev)      # + survived
        self.hl = _hl_bounds(venv)
        if self.hl is not None:
            self.cur_track = torch.zeros((n, len(HL_TRACK_SUMS)), dtype=torch.float64, device=dev)
            self.fin_track = torch.zeros((n, E, len(HL_TRACK_SUMS)), dtype=torch.float64, device=dev)
            self.prev_cmd = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        if self.path_layout is not None:
            from . import flight
            self.cur_path = flight.path_init(n, dev)
            self.carry = torch.zeros((n, flight.CARRY_DIM), dtype=torch.float64, device=dev)      # seeded behind the reset (begin)
            self.fin_path = torch.zeros((n, E, len(flight.PATH_SUMS)), dtype=torch.float64, device=dev)
        self.obs = None
        self.side = torch.cuda.Stream(device=dev)
        self.done_event = None
        self.steps = 0
        # a vec-step is the act and the env step (self.step, chosen above) and then the episode bookkeeping of the task
        self.step = evalstep.make(kind, policy, env, through_wrapper=True)
        # (kept as the plain function: a bound method stored on the object would make it a reference cycle, and its graph and
        # buffers would then be freed by the cycle collector at a moment of its choosing, inside somebody's capture for one)
        cls = type(self)
        self._books = (cls._track_step if self.track else cls._track_hl_step if self.hl is not None
                       else cls._track_wp_step if self.path_layout is not None
                       else cls._track_plain_step if kind == "collect_step" else cls._track_torch)

    fused = property(lambda self: self.step.kind != "torch")
    books = property(lambda self: self._books.__get__(self), doc="the bookkeeping of a vec-step, as a callable")

    def _track_hl_step(self) -> None:
        """the high-level command task's bookkeeping of a vec-step, command sums included: one fw_eval_track_hl launch"""
        venv, fi = self.venv, self.fin_info
        _lib.check(_lib.lib().fw_eval_track_hl(
            _p(venv.rewards), int(venv.rewards.dtype == torch.float64), _p(venv.terminated), _p(venv.truncated),
            _p(venv.info) if fi is not None else None, int(venv.info.shape[1]) if fi is not None else 0,
            _p(venv.obs), _p(venv.terminal_obs), _p(venv.command), int(venv.obs.dtype == torch.float64), int(venv.obs.shape[1]),
            self.hl[0], self.hl[1], _p(self.tg), _p(self.counts), _p(self.cur_rew), _p(self.cur_len), _p(self.step_ctr),
            _p(self.cur_track), _p(self.prev_cmd), _p(self.fin_rew), _p(self.fin_len), _p(self.fin_step),
            _p(fi), _p(self.fin_track), self.n, self.E, _stream(self.dev)))

    def _track_step(self) -> None:
        """the low-level task's bookkeeping of a vec-step, tracking sums included: one fw_eval_track_ll launch"""
        venv, fi = self.venv, self.fin_info
        _lib.check(_lib.lib().fw_eval_track_ll(
            _p(venv.rewards), int(venv.rewards.dtype == torch.float64), _p(venv.terminated), _p(venv.truncated),
            _p(venv.info) if fi is not None else None, int(venv.info.shape[1]) if fi is not None else 0,
            _p(venv.obs), _p(venv.terminal_obs), int(venv.obs.dtype == torch.float64), int(venv.obs.shape[1]),
            _p(self.tg), _p(self.counts), _p(self.cur_rew), _p(self.cur_len), _p(self.step_ctr), _p(self.cur_track),
            _p(self.fin_rew), _p(self.fin_len), _p(self.fin_step), _p(fi), _p(self.fin_track),
            self.n, self.E, _stream(self.dev)))

    def _track_wp_step(self) -> None:
        """the bookkeeping of a vec-step with the path sums: one fw_eval_track_wp launch (path_figures=True)"""
        venv, fi, lay = self.venv, self.fin_info, self.path_layout
        _lib.check(_lib.lib().fw_eval_track_wp(
            _p(venv.rewards), int(venv.rewards.dtype == torch.float64), _p(venv.terminated), _p(venv.truncated),
            _p(venv.info) if fi is not None else None, int(venv.info.shape[1]) if fi is not None else 0,
            _p(venv.obs), _p(venv.terminal_obs), int(venv.obs.dtype == torch.float64), int(venv.obs.shape[1]), lay.att_dim, lay.act_dim,
            _p(self.tg), _p(self.counts), _p(self.cur_rew), _p(self.cur_len), _p(self.step_ctr), _p(self.cur_path), _p(self.carry),
            _p(self.fin_rew), _p(self.fin_len), _p(self.fin_step), _p(fi), _p(self.fin_path),
            self.n, self.E, _stream(self.dev)))

    def _track_plain_step(self) -> None:
        """the bookkeeping of a vec-step behind fw_collect_step: one fw_eval_track launch"""
        venv, fi = self.venv, self.fin_info
        _lib.check(_lib.lib().fw_eval_track(
            _p(venv.rewards), int(venv.rewards.dtype == torch.float64), _p(venv.terminated), _p(venv.truncated),
            _p(venv.info) if fi is not None else None, int(venv.info.shape[1]) if fi is not None else 0,
            _p(self.tg), _p(self.counts), _p(self.cur_rew), _p(self.cur_len), _p(self.step_ctr), _p(self.fin_rew), _p(self.fin_len),
            _p(self.fin_step), _p(fi), self.n, self.E, _stream(self.dev)))

    def _track_torch(self) -> None:
        """the bookkeeping of a vec-step behind the torch forward, in framework ops"""
        venv, ar, tg, E, counts, dones = self.venv, self.ar, self.tg, self.E, self.counts, self.step.dones
        self.cur_rew.add_(venv.rewards.to(torch.float64))            # un-normalised reward of the wrapped env
        self.cur_len.add_(1); self.step_ctr.add_(1)
        take = dones & (counts < tg)
        slot = counts.clamp(max=E - 1)
        self.fin_rew[ar, slot] = torch.where(take, self.cur_rew, self.fin_rew[ar, slot])
        self.fin_len[ar, slot] = torch.where(take, self.cur_len, self.fin_len[ar, slot])
        self.fin_step[ar, slot] = torch.where(take, self.step_ctr.expand(self.n), self.fin_step[ar, slot])
        if self.has_info:
            self.fin_info[ar, slot] = torch.where(take[:, None], venv.info, self.fin_info[ar, slot])
        counts.add_(take.to(torch.int64))
        self.cur_rew.masked_fill_(dones, 0.0); self.cur_len.masked_fill_(dones, 0)

    def _body(self) -> None:
        self.step()
        self._books(self)

    def begin(self):
        """reset, two eager steps (they are evaluation steps like any other), capture: on the side stream"""
        self.side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.side):
            if self.hl is not None:
                self.venv.rejected.zero_()
            self.obs = self.step.obs = self.env.reset().clone()      # (the torch forward's fixed input buffer)
            if self.path_layout is not None:
                from . import flight
                self.carry.copy_(flight.seed_carry(self.venv.obs, self.path_layout))
            for _ in range(2):
                self._body(); self.steps += 1
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.side):
                for _ in range(REPLAY_STEPS):
                    self._body()

    def run(self, max_vec_steps: Optional[int] = None) -> "EvalResult":
        self.begin()
        with torch.cuda.stream(self.side):
            while True:
                self.graph.replay(); self.steps += REPLAY_STEPS
                if not bool((self.counts < self.tg).any().item()) or (max_vec_steps is not None and self.steps >= max_vec_steps):
                    break
        torch.cuda.current_stream(self.dev).wait_stream(self.side)
        return self.result()

    def launch(self, bound_vec_steps: int) -> "ReplayedEvaluation":
        self.begin()
        with torch.cuda.stream(self.side):
            for _ in range(-(-max(bound_vec_steps - 2, 1) // REPLAY_STEPS)):
                self.graph.replay(); self.steps += REPLAY_STEPS
            self.done_event = torch.cuda.Event()
            self.done_event.record(self.side)
        return self

    def ready(self) -> bool:
        return self.done_event is None or self.done_event.query()

    def result(self) -> "EvalResult":
        if self.done_event is not None:
            self.done_event.synchronize()
        else:
            self.side.synchronize()
        self.step.check()
        n, has_info = self.n, self.has_info
        res = EvalResult([], [])
        c_h = torch.minimum(self.counts, self.tg).cpu().numpy()
        rew_h, len_h, step_h = self.fin_rew.cpu().numpy(), self.fin_len.cpu().numpy(), self.fin_step.cpu().numpy()
        info_h = self.fin_info.cpu().numpy() if has_info else None
        trk_h = self.fin_track.cpu().numpy() if self.track else None
        hl_h = self.fin_track.cpu().numpy() if self.hl is not None else None
        path_h = self.fin_path.cpu().numpy() if self.path_layout is not None else None
        if self.hl is not None:
            res.rejected_actions = int(self.venv.rejected.item())
        order = sorted((int(step_h[i, k]), i, k) for i in range(n) for k in range(int(c_h[i])))    # as they ended: by step, then env
        for _, i, k in order:
            res.episode_rewards.append(float(rew_h[i, k])); res.episode_lengths.append(int(len_h[i, k]))
            if trk_h is not None:
                res.add_tracking(trk_h[i, k, :len(TRACK_SUMS)], trk_h[i, k, len(TRACK_SUMS)] != 0.0)
            if hl_h is not None:
                res.add_command(hl_h[i, k])
            if path_h is not None:
                res.add_path(path_h[i, k], _path_complete(info_h[i, k] if has_info else None))
            info = _episode_info(res, float(rew_h[i, k]), int(len_h[i, k]), info_h[i, k] if has_info else None, self.is_objlock)
            if self.callback is not None:
                self.callback(info)
        return res


def start_evaluation(policy, env, n_eval_episodes: int = 10, callback=None, use_fused: Optional[bool] = None,
                     path_figures: bool = False) -> ReplayedEvaluation:
    """Asynchronous :func:`evaluate_policy` (deterministic, device envs whose config bounds the episode length): returns a
    running :class:`ReplayedEvaluation`; ``.result()`` waits for it."""
    targets = _targets(n_eval_episodes, env.num_envs)
    bound = int(targets.max()) * (K.max_steps(env.venv.cfg) + 2)
    return ReplayedEvaluation(policy, env, targets, callback, use_fused=use_fused, path_figures=path_figures).launch(bound)


class EvalCallback:
    """``WaypointEvalCallback`` / SB3 ``EvalCallback`` for :meth:`rollout.PPO.learn`: every
    ``eval_freq`` vec-steps of training (the reference passes ``10000 // num_envs``) sync the
    normaliser, evaluate, append to ``evaluations.npz``, keep ``best_model``.

    ``overlap=True`` (single-process jobs on the GPU; off by default): the evaluation is *launched* -- a copy of the
    weights, the normaliser statistics, then :func:`start_evaluation` on a side stream -- and the training goes on; its
    figures are logged (under the timestep count at which it was launched) when a later callback finds it finished, at the
    latest before the next evaluation starts and when training ends.  ``best_model`` is written from the snapshot taken at
    launch, so it holds the evaluated weights, not the ones trained since.  Same figures as the synchronous form
    (tests/test_eval_checkpoint_gpu.py) -- but measured SLOWER on the training examples (combined 208 k -> 186 k,
    waypoints 209 k -> 202 k env-steps/s over whole runs): without a host in the loop every env is stepped for the longest
    possible episodes, and those ~1800 small launches on a second queue cost the training stream more than the 0.1 s of
    waiting they replace.  The default is therefore the synchronous evaluation, replayed as hipGraphs of 8 vec-steps."""

    def __init__(self, eval_env, n_eval_episodes: int = 5, eval_freq: int = 10000, log_path: Optional[str] = None,
                 best_model_save_path: Optional[str] = None, deterministic: bool = True, num_targets_total: int = 0,
                 verbose: int = 0, overlap: Optional[bool] = None, use_fused: Optional[bool] = None,
                 path_figures: bool = False):
        self.eval_env, self.n_eval_episodes, self.eval_freq = eval_env, n_eval_episodes, max(int(eval_freq), 1)
        self.log_path = os.path.join(log_path, "evaluations") if log_path else None
        self.best_model_save_path, self.deterministic = best_model_save_path, deterministic
        self.num_targets_total, self.verbose = num_targets_total, verbose
        self.best_mean_reward, self.last_mean_reward = -np.inf, -np.inf
        self.evaluations_timesteps: List[int] = []
        self.evaluations_results: List[List[float]] = []
        self.evaluations_length: List[List[int]] = []
        self.evaluations_successes: List[List[bool]] = []
        self.evaluations_tracking: Dict[str, List[float]] = {}      # the low-level task: figure name -> one value per evaluation
        self.last_scalars: Dict[str, float] = {}
        self._next_eval_calls = self.eval_freq
        self.n_evals = 0
        self.overlap = overlap
        self.path_figures = bool(path_figures)      # the flight's figures as well (EvalResult.path_scalars; not for the low- / high-level tasks)
        if self.path_figures:
            _path_layout(eval_env.venv)
        self.use_fused = use_fused        # handed to evaluate_policy / start_evaluation (None: fused whenever it is the default there)
        self._pending = None              # (job, num_timesteps at launch, checkpoint snapshot or None)
        self._policy_copy = None
        self._seed0, self._n_launched = None, 0

    def _agent_hz(self) -> float:
        return float(self.eval_env.venv.cfg.agent_hz)

    def _can_overlap(self, ppo) -> bool:
        if not self.overlap:
            return False
        venv = self.eval_env.venv
        return (self.deterministic and ppo.world_size == 1 and torch.device(self.eval_env.device).type == "cuda"
                and hasattr(venv, "step_tensor") and hasattr(venv, "cfg"))

    def on_rollout_end(self, ppo) -> bool:
        if self._pending is not None and self._pending[0].ready():
            self._finish(ppo)
        n_calls = ppo.num_timesteps // max(ppo.env.num_envs * ppo.world_size, 1)      # vec-steps so far (SB3 n_calls)
        if n_calls < self._next_eval_calls:
            return True
        while self._next_eval_calls <= n_calls:
            self._next_eval_calls += self.eval_freq
        from . import checkpoint
        if self._pending is not None:
            self._finish(ppo)                                    # one evaluation at a time: its env and weight copy are reused
        sync_envs_normalization(ppo.env, self.eval_env)
        # the k-th evaluation draws its scenarios from (seed of the eval env + k): its episodes then do not depend on how many
        # steps the earlier evaluations happened to run past their last episode (the overlapped form runs every env for the
        # longest possible episodes), and two runs of the same training evaluate on the same scenarios
        venv = self.eval_env.venv
        if hasattr(venv, "seed") and hasattr(venv, "seed_value"):
            if self._seed0 is None:
                self._seed0 = int(venv.seed_value)
            venv.seed(self._seed0 + self._n_launched)
        self._n_launched += 1
        writer = ppo.rank == 0
        snap = checkpoint.snapshot(ppo, include_env_state=False) if (self.best_model_save_path is not None and writer) else None
        if self._can_overlap(ppo):
            import copy
            if self._policy_copy is None:
                self._policy_copy = copy.deepcopy(ppo.policy)
            else:
                self._policy_copy.load_state_dict(ppo.policy.state_dict())
            job = start_evaluation(self._policy_copy, self.eval_env, self.n_eval_episodes, use_fused=self.use_fused,
                                   path_figures=self.path_figures)
            self._pending = (job, ppo.num_timesteps, snap)
        else:
            r = evaluate_policy(ppo.policy, self.eval_env, self.n_eval_episodes, deterministic=self.deterministic, use_fused=self.use_fused,
                                path_figures=self.path_figures)
            self._record(ppo, r, ppo.num_timesteps, snap)
        return True

    def on_training_end(self, ppo) -> None:
        if self._pending is not None:
            self._finish(ppo)

    def _finish(self, ppo) -> None:
        job, timesteps, snap = self._pending
        self._pending = None
        self._record(ppo, job.result(), timesteps, snap)

    def _record(self, ppo, r: EvalResult, timesteps: int, snap) -> None:
        from . import checkpoint
        self.n_evals += 1
        self.evaluations_timesteps.append(timesteps)
        self.evaluations_results.append(r.episode_rewards); self.evaluations_length.append(r.episode_lengths)
        writer = ppo.rank == 0               # multi-process job: every rank evaluates (identical weights), ONE rank writes files
        from .rollout import _dist
        if _dist() is not None:              # ... and every rank keeps rank 0's figure, so best_mean_reward agrees everywhere
            import torch.distributed as td
            t = torch.tensor([r.mean_reward], dtype=torch.float64, device=ppo.device if td.get_backend() == "nccl" else "cpu")
            td.broadcast(t, src=0)
            r.mean_reward_override = float(t.item())
        if self.log_path is not None and writer:
            os.makedirs(os.path.dirname(self.log_path), exist_ok=True)
            kw = {}
            if r.is_success:
                self.evaluations_successes.append(r.is_success); kw = dict(successes=np.array(self.evaluations_successes, dtype=object))
            for k, v in r.tracking_scalars().items():              # heading_mae, ..., survival_rate: (n_evals,)
                self.evaluations_tracking.setdefault(k.split("/", 1)[1], []).append(v)
            for k, v in r.command_scalars().items():               # the high-level command task: cmd_heading_mae, ...: (n_evals,)
                self.evaluations_tracking.setdefault(k.split("/", 1)[1], []).append(v)
            if self.path_figures:                                  # path_length_mean, ...: (n_evals,), NaN where a key was absent
                ps = r.path_scalars(self._agent_hz())
                for name in PATH_SCALARS:
                    self.evaluations_tracking.setdefault(name, []).append(ps.get("eval/" + name, float("nan")))
            kw.update({k: np.array(v, dtype=np.float64) for k, v in self.evaluations_tracking.items()})
            np.savez(self.log_path, timesteps=self.evaluations_timesteps, results=np.array(self.evaluations_results, dtype=object),
                     ep_lengths=np.array(self.evaluations_length, dtype=object), **kw)
        mean_reward = getattr(r, "mean_reward_override", r.mean_reward)
        self.last_mean_reward = mean_reward
        is_objlock = getattr(getattr(self.eval_env.venv, "cfg", None), "task", 0) in (K.FW_TASK_OBJLOCK, K.FW_TASK_WAYPOINT_OBJLOCK)
        self.last_scalars = r.scalars(self.num_targets_total, has_duck=is_objlock)
        self.last_scalars.update(r.tracking_scalars())             # (the low-level task's; nothing for the others)
        self.last_scalars.update(r.command_scalars())              # (the high-level command task's; nothing for the others)
        if self.path_figures:
            self.last_scalars.update(r.path_scalars(self._agent_hz()))
        self.last_scalars["time/total_timesteps"] = timesteps
        if self.verbose and writer:
            print(f"Eval num_timesteps={timesteps}, episode_reward={r.mean_reward:.2f} +/- {r.std_reward:.2f}")
            print(f"Episode length: {r.mean_ep_length:.2f} +/- {r.std_ep_length:.2f}")
        if mean_reward > self.best_mean_reward:
            self.best_mean_reward = mean_reward
            if snap is not None:
                checkpoint.write(snap, os.path.join(self.best_model_save_path, "best_model.pt"))
