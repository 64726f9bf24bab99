"""Rollout episode statistics -- SB3's ``rollout/ep_rew_mean``, ``ep_len_mean`` and ``success_rate`` for a device env.

SB3 gets these from ``Monitor`` (a per-env running return and length, an ``info["episode"]`` dict when the episode ends) and
``OnPolicyAlgorithm._update_info_buffer`` (``ep_info_buffer.extend(...)`` over the step's finished envs in env order, a
``deque(maxlen=stats_window_size)``).  Here one launch per vec-step (``fw_episode_fold``) does both, from the env's output buffers
(``venv.rewards`` / ``terminated`` / ``truncated`` / ``info`` hold the step until the next launch overwrites them): per-env
accumulators, a ring of the last W finished episodes in SB3's order, and running totals since creation, all in one caller-owned
state block on the device (layout: include/fwsim.h).  No step, collector or update kernel knows about it; ``PPOConfig.episode_stats``
puts the launch behind every vec-step of every collector, inside the captured rollout graph.  One workgroup walks all envs in that
launch; for large env counts ``fold="wide"`` runs the same fold over one workgroup per span of envs instead (``fw_episode_fold_wide``,
three launches, the same block).

With thousands of envs a 100-episode window is a sliver of one vec-step (every env meets the time limit in the same step), so
``scalars()`` also reports the means over ALL episodes finished since the previous call under ``rollout/interval/*`` -- the figures to
watch at that scale.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from . import config as K

# the state block in 8-byte words (include/fwsim.h, fw_episode_fold)
H_EPISODES, H_STEPS, H_TRUNCATED, H_SUM_LEN, H_SUM_INFO, H_SUM_RET, H_SUM_RET2, HEADER_WORDS = 0, 1, 2, 3, 4, 10, 11, 16
INFO_SUMS = ("targets_reached", "collision", "out_of_bounds", "env_complete", "duck_strike", "is_success")      # info columns 0..5
RING_WORDS = 5 + K.FW_INFO_DIM // 2         # per slot: return, length, step, env, truncated, the info row (int32 x 8)

# the figures a sharded job sums over ranks (one all-reduce): the totals, then the sums over the rank's window
_TOTALS = ("episodes", "steps", "truncated", "sum_len") + tuple("sum_" + k for k in INFO_SUMS) + ("sum_ret", "sum_ret2")
_WINDOW = ("n", "ret", "len", "truncated") + INFO_SUMS


FOLD_FORMS = ("one", "wide", "auto")        # fw_episode_fold (one workgroup), fw_episode_fold_wide (one per span of envs), or by env count
# fold="auto": the wide form from this env count on -- the smallest measured env count from which it is not slower than the
# one-workgroup form (profiles/r25_episode_fold_wide.jsonl, "what": "wide")
WIDE_FROM_ENVS = 4096


def resolve_fold(fold: str, num_envs: int) -> str:
    """``"one"`` or ``"wide"`` for a ``fold`` option; ``ValueError`` for anything but :data:`FOLD_FORMS`."""
    if fold not in FOLD_FORMS:
        raise ValueError(f"fold must be one of {FOLD_FORMS}, got {fold!r}")
    if fold == "auto":
        return "wide" if int(num_envs) >= WIDE_FROM_ENVS else "one"
    return fold


def state_words(num_envs: int, window: int) -> int:
    """Words of the documented layout (what ``fw_episode_state_bytes`` must at least return, in bytes / 8)."""
    return HEADER_WORDS + RING_WORDS * int(window) + 2 * int(num_envs)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _mean(s: float, n: float) -> float:
    return float(s) / float(n) if n > 0 else float("nan")


class EpisodeMonitor:
    """The state block of ``fw_episode_fold`` and its host-side readers.

    ``fold(rewards, terminated, truncated, info)`` books one vec-step: the kernel on device tensors, a plain torch statement of the
    same semantics on CPU tensors (the reference the kernel is tested against).  The truncated flag of an episode is the env's
    ``truncated`` output of its last step.

    ``fold``: the device form -- ``"one"`` (``fw_episode_fold``: one workgroup walks all envs), ``"wide"`` (``fw_episode_fold_wide``:
    one workgroup per ``fw_episode_fold_span()`` envs, three launches, for large env counts) or ``"auto"`` (``"wide"`` from
    :data:`WIDE_FROM_ENVS` envs on).  Both work on the same block; only the two double totals may differ in their last bits."""

    def __init__(self, num_envs: int, window: int = 100, device="cpu", fold: str = "one"):
        self.num_envs, self.window_size = int(num_envs), int(window)
        if self.num_envs <= 0 or self.window_size <= 0:
            raise ValueError(f"EpisodeMonitor needs num_envs > 0 and window > 0, got {num_envs} and {window}")
        self.fold_form = resolve_fold(fold, self.num_envs)      # "one" or "wide"; not part of a checkpoint (the block is form-agnostic)
        self.device = torch.device(device)
        words = state_words(self.num_envs, self.window_size)
        if self.device.type == "cuda":
            nbytes = int(_lib.lib().fw_episode_state_bytes(self.num_envs, self.window_size))
            if nbytes < 0:
                _lib.check(nbytes)
            words = max(words, (nbytes + 7) // 8)
        self.state = torch.zeros(words, dtype=torch.int64, device=self.device)       # zeroed once; the kernel owns it from here on
        self.workspace = None              # fw_episode_fold_wide's scratch: allocated once (a captured graph holds its address)
        if self.device.type == "cuda" and self.fold_form == "wide":
            nbytes = int(_lib.lib().fw_episode_fold_workspace_bytes(self.num_envs))
            if nbytes < 0:
                _lib.check(nbytes)
            self.workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=self.device)
        self._saved = None                 # snapshot(): a device copy of the block
        self._last = None                  # the totals at the previous scalars() call (the base of rollout/interval/*)

    # ---- views of the block ---------------------------------------------------------------------
    def _views(self, state: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        s = self.state if state is None else state
        W, N, o = self.window_size, self.num_envs, HEADER_WORDS
        v = {"header": s[:o], "ring_ret": s[o:o + W].view(torch.float64), "ring_len": s[o + W:o + 2 * W],
             "ring_step": s[o + 2 * W:o + 3 * W], "ring_env": s[o + 3 * W:o + 4 * W], "ring_trunc": s[o + 4 * W:o + 5 * W],
             "ring_info": s[o + 5 * W:o + RING_WORDS * W].view(torch.int32).view(W, K.FW_INFO_DIM)}
        o += RING_WORDS * W
        if s.numel() >= o + 2 * N:
            v["cur_ret"], v["cur_len"] = s[o:o + N].view(torch.float64), s[o + N:o + 2 * N]
        return v

    @property
    def head_words(self) -> int:
        """Header + ring: what the host readers need (the per-env accumulators stay on the device)."""
        return HEADER_WORDS + RING_WORDS * self.window_size

    # ---- one vec-step ---------------------------------------------------------------------------
    def fold(self, rewards: torch.Tensor, terminated: torch.Tensor, truncated: torch.Tensor, info: Optional[torch.Tensor] = None,
             stream=None) -> None:
        N = self.num_envs
        if rewards.shape != (N,) or terminated.shape != (N,) or truncated.shape != (N,):
            raise ValueError(f"fold() takes [N] = [{N}] rewards / terminated / truncated")
        if info is not None and (info.dim() != 2 or info.shape[0] != N or info.dtype != torch.int32):
            raise ValueError(f"info must be an int32 [{N}, info_dim] tensor")
        if rewards.device.type != self.device.type:
            raise ValueError(f"the monitor lives on {self.device}, the step on {rewards.device}")
        if self.device.type != "cuda":
            return self._fold_torch(rewards, terminated, truncated, info)
        if rewards.dtype not in (torch.float32, torch.float64) or terminated.dtype != torch.uint8 or truncated.dtype != torch.uint8:
            raise ValueError("the kernel takes float32 / float64 rewards and uint8 flags (the env's output buffers)")
        if not (rewards.is_contiguous() and terminated.is_contiguous() and truncated.is_contiguous() and (info is None or info.is_contiguous())):
            raise ValueError("fold() takes contiguous tensors")
        if stream is None:
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        if self.workspace is not None:
            _lib.check(_lib.lib().fw_episode_fold_wide(_ptr(rewards), int(rewards.dtype == torch.float64), _ptr(terminated),
                                                       _ptr(truncated), _ptr(info), int(info.shape[1]) if info is not None else 0,
                                                       _ptr(self.state), _ptr(self.workspace), N, self.window_size, stream))
            return
        _lib.check(_lib.lib().fw_episode_fold(_ptr(rewards), int(rewards.dtype == torch.float64), _ptr(terminated), _ptr(truncated),
                                              _ptr(info), int(info.shape[1]) if info is not None else 0, _ptr(self.state), N,
                                              self.window_size, stream))

    def _fold_torch(self, rewards, terminated, truncated, info) -> None:
        """The semantics of fw_episode_fold in torch (CPU tensors; reads the cursor on the host)."""
        v, W = self._views(), self.window_size
        h = v["header"]
        v["cur_ret"] += rewards.to(torch.float64)
        v["cur_len"] += 1
        trunc = truncated != 0
        idx = torch.nonzero((terminated != 0) | trunc).flatten()          # the step's finished envs, ascending
        step, pushed, D = int(h[H_STEPS]) + 1, int(h[H_EPISODES]), int(idx.numel())
        if D:
            ret, length, tr = v["cur_ret"][idx], v["cur_len"][idx], trunc[idx].to(torch.int64)
            rows = torch.zeros((D, K.FW_INFO_DIM), dtype=torch.int32)
            if info is not None:
                k = min(int(info.shape[1]), K.FW_INFO_DIM)
                rows[:, :k] = info[idx, :k]
            keep = slice(max(D - W, 0), D)                                 # what deque(maxlen=W).extend() leaves of this step
            slots = (pushed + torch.arange(D)[keep]) % W
            v["ring_ret"][slots] = ret[keep]; v["ring_len"][slots] = length[keep]; v["ring_step"][slots] = step
            v["ring_env"][slots] = idx[keep]; v["ring_trunc"][slots] = tr[keep]; v["ring_info"][slots] = rows[keep]
            h[H_TRUNCATED] += tr.sum(); h[H_SUM_LEN] += length.sum()
            h[H_SUM_INFO:H_SUM_INFO + len(INFO_SUMS)] += rows[:, :len(INFO_SUMS)].to(torch.int64).sum(0)
            hd = h.view(torch.float64)
            hd[H_SUM_RET] += ret.sum(); hd[H_SUM_RET2] += (ret * ret).sum()
            v["cur_ret"][idx] = 0.0; v["cur_len"][idx] = 0
        h[H_EPISODES] = pushed + D
        h[H_STEPS] = step

    # ---- host-side readers ------------------------------------------------------------------------
    def head(self) -> np.ndarray:
        """Header + ring as int64 words on the host: one small copy (it synchronises with the stream that folded)."""
        return self.state[:self.head_words].cpu().numpy().copy()

    def window(self, head: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
        """The ring in push order (oldest first), as ``deque(maxlen=W)`` would iterate: ``r`` (float64), ``l``, ``step`` (1-based
        vec-step index), ``env``, ``truncated`` (int64) and ``info`` (int32 ``[n, FW_INFO_DIM]``)."""
        h = self.head() if head is None else np.asarray(head)
        W, o = self.window_size, HEADER_WORDS
        pushed = int(h[H_EPISODES])
        n = min(pushed, W)
        order = (np.arange(pushed - n, pushed) % W).astype(np.int64)
        ring = h[o:o + RING_WORDS * W]
        return {"r": ring[:W].view(np.float64)[order], "l": ring[W:2 * W][order], "step": ring[2 * W:3 * W][order],
                "env": ring[3 * W:4 * W][order], "truncated": ring[4 * W:5 * W][order],
                "info": ring[5 * W:].view(np.int32).reshape(W, K.FW_INFO_DIM)[order]}

    def totals(self, head: Optional[np.ndarray] = None) -> Dict[str, float]:
        """Running totals since creation: ``episodes``, ``steps`` (vec-steps folded), ``truncated``, ``sum_len`` and ``sum_<info
        column>`` (exact integers), ``sum_ret`` and ``sum_ret2`` (float64)."""
        h = (self.state[:HEADER_WORDS].cpu().numpy() if head is None else np.asarray(head))[:HEADER_WORDS]
        out = {"episodes": int(h[H_EPISODES]), "steps": int(h[H_STEPS]), "truncated": int(h[H_TRUNCATED]), "sum_len": int(h[H_SUM_LEN])}
        out.update({"sum_" + k: int(h[H_SUM_INFO + i]) for i, k in enumerate(INFO_SUMS)})
        hd = h.view(np.float64)
        out.update(sum_ret=float(hd[H_SUM_RET]), sum_ret2=float(hd[H_SUM_RET2]))
        return out

    def figures(self, head: Optional[np.ndarray] = None) -> np.ndarray:
        """What ranks exchange: float64 ``[len(_TOTALS) + len(_WINDOW)]`` -- the totals, then entry count and column sums of the
        window.  Sums over ranks of these vectors are the figures of the job (the window's: of the union of the ranks' windows)."""
        h = self.head() if head is None else head
        t, w = self.totals(h), self.window(h)
        win = [float(w["r"].size), float(np.sum(w["r"])) if w["r"].size else 0.0, float(w["l"].sum()), float(w["truncated"].sum())]
        win += [float(w["info"][:, i].sum()) for i in range(len(INFO_SUMS))]
        return np.array([float(t[k]) for k in _TOTALS] + win, dtype=np.float64)

    def reduced_figures(self, reduce, figures: Optional[np.ndarray] = None) -> np.ndarray:
        """``figures()`` summed over the ranks of a sharded job: ONE small collective (a point every rank must reach)."""
        f = self.figures() if figures is None else figures
        return reduce(torch.as_tensor(f, dtype=torch.float64, device=self.device)).cpu().numpy()

    def scalars(self, head: Optional[np.ndarray] = None, reduce=None, figures: Optional[np.ndarray] = None) -> Dict[str, float]:
        """SB3's rollout figures over the window, the build-owned window rates, the total, and the same means over the episodes
        finished since the previous call (``rollout/interval/*``).  No finished episode: NaN means, zero counts.  ``reduce``: a
        function summing a float64 tensor over the ranks of a sharded job in place (``rollout.all_reduce_sum_``); ``figures``: a
        vector of ``figures()`` taken (and summed over ranks) earlier."""
        f = self.figures(head) if figures is None else np.asarray(figures, dtype=np.float64)
        if reduce is not None:
            f = self.reduced_figures(reduce, f)
        tot = {k: float(x) for k, x in zip(_TOTALS, f[:len(_TOTALS)])}
        win = {k: float(x) for k, x in zip(_WINDOW, f[len(_TOTALS):])}
        last = self._last if self._last is not None else {k: 0.0 for k in _TOTALS}
        d = {k: tot[k] - last[k] for k in _TOTALS}
        self._last = tot
        n, m = win["n"], d["episodes"]
        return {
            "rollout/ep_rew_mean": _mean(win["ret"], n), "rollout/ep_len_mean": _mean(win["len"], n),
            "rollout/success_rate": _mean(win["is_success"], n),
            "rollout/targets_reached_mean": _mean(win["targets_reached"], n), "rollout/collision_rate": _mean(win["collision"], n),
            "rollout/out_of_bounds_rate": _mean(win["out_of_bounds"], n), "rollout/duck_strike_rate": _mean(win["duck_strike"], n),
            "rollout/timeout_rate": _mean(win["truncated"], n),
            "rollout/episodes": float(tot["episodes"]),
            "rollout/interval/episodes": float(m),
            "rollout/interval/ep_rew_mean": _mean(d["sum_ret"], m), "rollout/interval/ep_len_mean": _mean(d["sum_len"], m),
            "rollout/interval/success_rate": _mean(d["sum_is_success"], m),
            "rollout/interval/targets_reached_mean": _mean(d["sum_targets_reached"], m),
            "rollout/interval/collision_rate": _mean(d["sum_collision"], m),
            "rollout/interval/out_of_bounds_rate": _mean(d["sum_out_of_bounds"], m),
            "rollout/interval/duck_strike_rate": _mean(d["sum_duck_strike"], m),
            "rollout/interval/timeout_rate": _mean(d["truncated"], m),
        }

    # ---- what a rollout moves, kept so that a void rollout can be taken back ------------------------------------------------
    def snapshot(self) -> None:
        """A device copy of the block into a persistent buffer (the shape of ``VecNormalizeDevice.save_statistics``)."""
        if self._saved is None:
            self._saved = torch.zeros_like(self.state)
        self._saved.copy_(self.state)
        self._saved_last = None if self._last is None else dict(self._last)

    def restore(self) -> bool:
        """Back to what ``snapshot()`` kept (in place: a captured graph holds the block's address).  False if nothing was saved."""
        if self._saved is None:
            return False
        self.state.copy_(self._saved)
        self._last = None if self._saved_last is None else dict(self._saved_last)
        return True

    # ---- checkpoint ---------------------------------------------------------------------------------
    def state_dict(self):
        return {"num_envs": self.num_envs, "window": self.window_size, "state": self.state.cpu().clone(),
                "interval_base": None if self._last is None else dict(self._last)}

    def load_state_dict(self, sd) -> None:
        if int(sd["num_envs"]) != self.num_envs or int(sd["window"]) != self.window_size:
            raise ValueError(f"episode statistics of {sd['num_envs']} envs / window {sd['window']} do not fit a monitor of "
                             f"{self.num_envs} envs / window {self.window_size}")
        src = sd["state"]
        n = state_words(self.num_envs, self.window_size)
        self.state.zero_()
        self.state[:n].copy_(src[:n])
        self._last = None if sd.get("interval_base") is None else dict(sd["interval_base"])


class VecMonitorDevice:
    """Pass-through wrapper of a device env for callers that run their own loop: folds after every ``step`` / ``step_tensor``
    (SB3's ``VecMonitor``).  Everything else is the wrapped env's; ``.monitor`` is the :class:`EpisodeMonitor`."""

    def __init__(self, venv, window: int = 100, fold: str = "one"):
        self.venv = venv
        self.monitor = EpisodeMonitor(venv.num_envs, window, venv.device, fold)

    def _fold(self) -> None:
        v = self.venv
        self.monitor.fold(v.rewards, v.terminated, v.truncated, getattr(v, "info", None))

    def step_tensor(self, actions):
        out = self.venv.step_tensor(actions)
        self._fold()
        return out

    def step(self, actions):
        out = self.venv.step(actions)
        self._fold()
        return out

    def step_wait(self):
        out = self.venv.step_wait()
        self._fold()
        return out

    def __getattr__(self, name):
        if name in ("venv", "monitor"):
            raise AttributeError(name)
        return getattr(self.venv, name)
