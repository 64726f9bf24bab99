"""The multi-workgroup episode fold (fw_episode_fold_wide) and its options without a device: the exported symbols, the span and the
workspace size, the argument errors through the C ABI, the ``fold`` option of monitor.EpisodeMonitor / VecMonitorDevice,
PPOConfig.episode_fold and SACConfig.episode_stats / episode_fold, and a PPO on the CPU toy env under either form."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_stats_jobs as J  # noqa: E402

from pyflyt_drone_amd import _lib  # noqa: E402
from pyflyt_drone_amd import config as K  # noqa: E402
from pyflyt_drone_amd import monitor as M  # noqa: E402
from pyflyt_drone_amd import rollout as R  # noqa: E402
from pyflyt_drone_amd import sac as S  # noqa: E402

NAMES = ("fw_episode_fold_span", "fw_episode_fold_workspace_bytes", "fw_episode_fold_wide")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fwsim.h")


def test_the_three_symbols_are_exported_and_declared():
    L = _lib.lib()                              # (loads without a device; a missing or stale library is a failure, not a skip)
    text = open(HEADER).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"^int(32|64)_t " + name + r"\(", text, re.M), name
    assert L.fw_episode_fold_wide.argtypes is not None and len(L.fw_episode_fold_wide.argtypes) == 11


def test_span_and_workspace_size():
    L = _lib.lib()
    span = L.fw_episode_fold_span()
    assert span > 0 and span % 64 == 0
    sizes = [L.fw_episode_fold_workspace_bytes(n) for n in (1, span, span + 1, 2 ** 20)]
    assert all(s > 0 for s in sizes)
    assert sizes[0] == sizes[1] < sizes[2] < sizes[3]          # B = ceil(N / span) is fixed by N: one block, one block, two, many
    for n in (0, -1, -(2 ** 31)):
        assert L.fw_episode_fold_workspace_bytes(n) == K.FW_EINVAL and "must be positive" in L.fw_last_error(None).decode()


def test_argument_errors_through_the_c_abi():
    L = _lib.lib()
    one = C.c_void_p(16)                        # (a non-NULL address: the checks below return before anything is read or launched)

    def call(reward=one, term=one, trunc=one, info=None, info_dim=0, state=one, ws=one, n=8, w=4):
        return L.fw_episode_fold_wide(reward, 1, term, trunc, info, info_dim, state, ws, n, w, None)
    for kw in (dict(reward=None), dict(term=None), dict(trunc=None), dict(state=None), dict(ws=None)):
        assert call(**kw) == K.FW_EINVAL and "must be non-NULL" in L.fw_last_error(None).decode()
    assert "workspace" in L.fw_last_error(None).decode()
    for kw in (dict(n=0), dict(n=-5), dict(w=0), dict(w=-1)):
        assert call(**kw) == K.FW_EINVAL and "must be positive" in L.fw_last_error(None).decode()
    for d in (0, -8):
        assert call(info=one, info_dim=d) == K.FW_EINVAL and "info_dim" in L.fw_last_error(None).decode()


def test_fold_option_of_the_monitor():
    assert M.FOLD_FORMS == ("one", "wide", "auto")
    for bad in ("bogus", "", "Wide", None):
        with pytest.raises(ValueError):
            M.EpisodeMonitor(8, 4, fold=bad)
    with pytest.raises(ValueError):
        M.VecMonitorDevice(J.ToyVenv(n=4), fold="bogus")
    assert M.EpisodeMonitor(8, 4).fold_form == "one"                           # the default stays the one-workgroup form
    assert M.VecMonitorDevice(J.ToyVenv(n=4), window=3, fold="wide").monitor.fold_form == "wide"
    # "auto" resolves at construction, on either side of the measured threshold
    T = M.WIDE_FROM_ENVS
    assert isinstance(T, int) and T > 1
    assert M.EpisodeMonitor(T - 1, 4, fold="auto").fold_form == "one"
    assert M.EpisodeMonitor(T, 4, fold="auto").fold_form == "wide"
    assert M.EpisodeMonitor(T + 1, 4, fold="auto").fold_form == "wide"
    assert M.resolve_fold("auto", 1) == "one" and M.resolve_fold("wide", 1) == "wide" and M.resolve_fold("one", 10 ** 7) == "one"


@pytest.mark.parametrize("f64", [False, True])
def test_wide_on_cpu_folds_exactly_like_one(f64):
    N, W = 199, 7
    a, b = M.EpisodeMonitor(N, W, fold="one"), M.EpisodeMonitor(N, W, "cpu", "wide")
    assert b.workspace is None                                                  # no device, no scratch: the torch fold whatever the form
    for rew, te, tr, info in J.make_stream(N, W, f64, seed=6):
        for m in (a, b):
            m.fold(torch.from_numpy(rew), torch.from_numpy(te), torch.from_numpy(tr), torch.from_numpy(info))
    assert torch.equal(a.state, b.state)
    J.assert_window_equal(a.window(), b.window())
    # the form is not part of a checkpoint: a block written under one form loads under the other
    sd = b.state_dict()
    assert "fold" not in sd and set(sd) == set(a.state_dict())
    c = M.EpisodeMonitor(N, W, fold="one")
    c.load_state_dict(sd)
    assert torch.equal(c.state, a.state)


def test_config_options_validate():
    assert R.PPOConfig().episode_fold == "one" and R.PPOConfig().episode_stats is False
    for form in M.FOLD_FORMS:
        assert R.PPOConfig(episode_fold=form).episode_fold == form
        assert S.SACConfig(episode_stats=True, episode_fold=form).episode_fold == form
    with pytest.raises(ValueError):
        R.PPOConfig(episode_fold="bogus")
    d = S.SACConfig()
    assert d.episode_stats is False and d.stats_window_size == 100 and d.episode_fold == "one"
    with pytest.raises(ValueError):
        S.SACConfig(episode_fold="bogus")
    with pytest.raises(ValueError):
        S.SACConfig(episode_stats=True, stats_window_size=0)


def _toy_ppo(**cfg):
    venv = J.ToyVenv(n=16, d=6, seed=3)
    kw = dict(n_steps=8, batch_size=32, n_epochs=2, seed=9, use_graphs=False, episode_stats=True, stats_window_size=12)
    kw.update(cfg)
    return R.PPO(R.VecNormalizeDevice(venv), R.PPOConfig(**kw), gae_fn=R.gae_reference)


def test_ppo_on_the_toy_env_reports_the_same_figures_under_either_form():
    one, wide, auto = _toy_ppo(), _toy_ppo(episode_fold="wide"), _toy_ppo(episode_fold="auto")
    assert one.episode_monitor.fold_form == "one" and wide.episode_monitor.fold_form == "wide"
    assert auto.episode_monitor.fold_form == ("wide" if 16 >= M.WIDE_FROM_ENVS else "one")
    for _ in range(3):
        stats = []
        for p in (one, wide, auto):
            p.collect_rollouts(); p.train()
            stats.append(p.rollout_stats)
        assert stats[0]["rollout/episodes"] > 0
        assert J.same_scalars(stats[1], stats[0]) and J.same_scalars(stats[2], stats[0]) and set(stats[1]) == set(stats[0])
    assert torch.equal(one.episode_monitor.state, wide.episode_monitor.state)
    for p, q in zip(one.policy.parameters(), wide.policy.parameters()):
        assert torch.equal(p, q)
