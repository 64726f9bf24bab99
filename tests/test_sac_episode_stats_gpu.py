"""Rollout episode statistics behind the off-policy learner (SACConfig.episode_stats): the figures of an eager run against SB3's
statement fed with the env's own output buffers, graph replay (both graph forms, warm-up and training) against the eager run,
either fold form, the flag-off twin and the state_dict round trip."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_stats_jobs as J  # noqa: E402

import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import config as K  # noqa: E402
from pyflyt_drone_amd import monitor as M  # noqa: E402
from pyflyt_drone_amd import sac as S  # noqa: E402

pytestmark = pytest.mark.gpu

N, WINDOW, STEPS = 16, 20, 8       # learning_starts = 32: two warm-up vec-steps, six trained ones; max_episode_steps = 4: episodes end inside


def _env(seed=3):
    return P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=4), N, seed=seed)


def _sac(graphs=False, stats=True, **kw):
    cfg = S.SACConfig(batch_size=32, net_arch=(64, 64), learning_starts=32, gradient_steps=2, seed=7, use_graphs=graphs,
                      buffer_size=N * 40, episode_stats=stats, stats_window_size=WINDOW, **kw)
    return S.SAC(_env(), cfg)


def _run(sac, n, record=None):
    for _ in range(n):
        sac.collect_step()
        if record is not None:
            e = sac.env
            record.append(tuple(x.cpu().numpy().copy() for x in (e.rewards, e.terminated, e.truncated, e.info)))
    torch.cuda.synchronize()
    return sac


@pytest.fixture(scope="module")
def eager():
    record = []
    sac = _run(_sac(), STEPS, record)
    return sac, record


def test_eager_run_reports_what_the_sb3_statement_reports(eager):
    sac, record = eager
    assert sac.episode_monitor is not None and sac.episode_monitor.fold_form == "one" and len(record) == STEPS
    ref = J.Sb3Statement(N, WINDOW)
    for step in record:
        ref.step(*step)
    m = sac.episode_monitor
    assert len(ref.all) >= N                                                  # every env met the time limit at least once
    J.assert_window_equal(m.window(), ref.window())                           # exactly
    t = m.totals()
    assert {k: t[k] for k in ref.int_totals()} == ref.int_totals()
    ref.check_double_totals(t["sum_ret"], t["sum_ret2"])
    s = sac.rollout_stats
    assert J.same_scalars(s, ref.window_scalars()) and s["rollout/episodes"] == len(ref.all) == s["rollout/interval/episodes"]
    assert sac.num_timesteps == STEPS * N and sac.n_updates == 2 * (STEPS - 2)


@pytest.mark.parametrize("form", ["one", "wide"])
def test_graph_replay_gives_the_eager_block_bit_for_bit(eager, form):
    a = eager[0]
    b = _run(_sac(graphs=True, episode_fold=form), STEPS)
    assert len(b._graphs) == 2 and all(isinstance(g, torch.cuda.CUDAGraph) for g in b._graphs.values())     # warm-up and training
    assert b.episode_monitor.fold_form == form
    n = M.state_words(N, WINDOW)
    # (16 envs are one workgroup of either form: lane tree of one wave, then zeros -- the two double totals come out the same bits too)
    assert torch.equal(a.episode_monitor.state[:n], b.episode_monitor.state[:n])
    assert torch.equal(a.fused.image, b.fused.image) and torch.equal(a.buffer.ring, b.buffer.ring)


def test_flag_off_twin(eager):
    on, off = eager[0], _run(_sac(stats=False), STEPS)
    assert off.episode_monitor is None and off.rollout_stats == {} and "episode_stats" not in off.state_dict()
    assert torch.equal(on.fused.image, off.fused.image) and torch.equal(on.buffer.ring, off.buffer.ring)
    assert torch.equal(on.buffer.counters, off.buffer.counters) and torch.equal(on.env.obs, off.env.obs)


def test_state_dict_round_trip_keeps_the_figures():
    a = _run(_sac(), 5)
    sd = a.state_dict(include_buffer=True)
    assert "episode_stats" in sd
    b = _sac(episode_fold="wide")                                             # the form is not part of a checkpoint
    b.env.reset_tensor(); b._started = True
    b.env.set_state(a.env.get_state()); b.env.obs.copy_(a.env.obs)
    b.load_state_dict(sd)
    n = M.state_words(N, WINDOW)
    assert torch.equal(a.episode_monitor.state[:n], b.episode_monitor.state[:n])
    assert J.same_scalars(b.episode_monitor.scalars(), a.episode_monitor.scalars())
    _run(a, 3); _run(b, 3)
    J.assert_window_equal(a.episode_monitor.window(), b.episode_monitor.window())
    ta, tb = a.episode_monitor.totals(), b.episode_monitor.totals()
    assert {k: v for k, v in ta.items() if not k.startswith("sum_ret")} == {k: v for k, v in tb.items() if not k.startswith("sum_ret")}
    assert ta["episodes"] > sd["episode_stats"]["state"][M.H_EPISODES].item()
    # a checkpoint written with the flag off leaves the monitor as it is
    off = _run(_sac(stats=False), 2)
    b.load_state_dict(off.state_dict(include_buffer=True))
    assert b.episode_monitor.totals()["episodes"] == tb["episodes"]
