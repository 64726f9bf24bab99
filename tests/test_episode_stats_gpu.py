"""Rollout episode statistics on the device: fw_episode_fold against the torch fold of monitor.EpisodeMonitor (itself held to SB3's
statement in tests/test_episode_stats_cpu.py), under graph replay, and behind every collector of rollout.PPO
(PPOConfig.episode_stats): figures, exact invariants, take-back, checkpoint resume and the flag-off twin."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_stats_jobs as J  # noqa: E402

import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import checkpoint  # noqa: E402
from pyflyt_drone_amd import config as K  # noqa: E402
from pyflyt_drone_amd import monitor as M  # noqa: E402
from pyflyt_drone_amd import rollout as R  # noqa: E402

pytestmark = pytest.mark.gpu

DOUBLES = (M.H_SUM_RET, M.H_SUM_RET2)          # the two header words whose summation order is the kernel's own


def _dev(step):
    return tuple(torch.from_numpy(x).cuda() for x in step)


def _assert_blocks_equal(dev: M.EpisodeMonitor, ref: M.EpisodeMonitor, ref_eps):
    """Ring, cursor, per-env accumulators and integer totals bit for bit; the double totals to the reordered-sum bound."""
    got, want = dev.state.cpu(), ref.state
    n = M.state_words(ref.num_envs, ref.window_size)
    mask = torch.ones(n, dtype=torch.bool)
    mask[list(DOUBLES)] = False
    assert torch.equal(got[:n][mask], want[:n][mask])
    t = dev.totals()
    ref_eps.check_double_totals(t["sum_ret"], t["sum_ret2"])


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("N,W", J.SHAPES + [(129, 64)])
def test_kernel_equals_the_torch_fold(N, W, f64):
    stream = J.make_stream(N, W, f64)
    dev, ref, eps = M.EpisodeMonitor(N, W, "cuda"), M.EpisodeMonitor(N, W), J.Sb3Statement(N, W)
    for k, step in enumerate(stream):
        dev.fold(*_dev(step))
        ref.fold(*(torch.from_numpy(x) for x in step))
        eps.step(*step)
        if k in (2, 4, 6):                       # behind the all-done, the exactly-W and the tail-only step, and at the end
            _assert_blocks_equal(dev, ref, eps)
    _assert_blocks_equal(dev, ref, eps)
    J.assert_window_equal(dev.window(), eps.window())
    s = dev.scalars()
    assert J.same_scalars(s, eps.window_scalars())
    # the kernel's double sums have a fixed order: a second run gives the same bits
    again = M.EpisodeMonitor(N, W, "cuda")
    for step in stream:
        again.fold(*_dev(step))
    assert torch.equal(again.state, dev.state)


def test_kernel_without_info_and_with_short_info_rows():
    N, W = 199, 7
    stream = J.make_stream(N, W, True, seed=3)
    for cols in (None, 3):
        dev, ref = M.EpisodeMonitor(N, W, "cuda"), M.EpisodeMonitor(N, W)
        for rew, te, tr, info in stream:
            i = None if cols is None else np.ascontiguousarray(info[:, :cols])
            dev.fold(*_dev((rew, te, tr)), None if i is None else torch.from_numpy(i).cuda())
            ref.fold(torch.from_numpy(rew), torch.from_numpy(te), torch.from_numpy(tr), None if i is None else torch.from_numpy(i))
        J.assert_window_equal(dev.window(), ref.window())
        assert {k: v for k, v in dev.totals().items() if not k.startswith("sum_ret")} == \
               {k: v for k, v in ref.totals().items() if not k.startswith("sum_ret")}


def test_eight_folds_in_one_graph_replayed_three_times_equal_24_eager_folds():
    N, W = 199, 7
    streams = [J.make_stream(N, W, True, seed=20 + r)[:8] for r in range(3)]
    dev, eager = M.EpisodeMonitor(N, W, "cuda"), M.EpisodeMonitor(N, W, "cuda")
    rew = torch.zeros((8, N), dtype=torch.float64, device="cuda")
    te, tr = torch.zeros((8, N), dtype=torch.uint8, device="cuda"), torch.zeros((8, N), dtype=torch.uint8, device="cuda")
    info = torch.zeros((8, N, J.INFO_DIM), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for t in range(8):
            dev.fold(rew[t], te[t], tr[t], info[t])
    assert int(dev.state.abs().sum()) == 0                                     # capturing ran nothing
    for stream in streams:
        for t, step in enumerate(stream):
            for dst, src in zip((rew, te, tr, info), _dev(step)):
                dst[t].copy_(src)
            eager.fold(*_dev(step))
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(dev.state, eager.state)
    assert dev.totals()["steps"] == 24 and dev.totals()["episodes"] > 3 * N


# ------------------------------------------------------------------------------------------------------------ collectors
SHORT = 0.25           # max_duration_seconds: 7 agent steps at 30 Hz (episodes of about 9), so every env ends at least four in 3 rollouts of 16 steps


def _waypoints(n, stats=True, window=100, seed=11, **cfg):
    env = R.VecNormalizeDevice(P.FixedwingWaypointsVecEnv(n, angle_representation="euler", max_duration_seconds=SHORT, seed=seed))
    kw = dict(n_steps=16, batch_size=64, n_epochs=2, seed=seed, episode_stats=stats, stats_window_size=window)
    kw.update(cfg)
    return R.PPO(env, R.PPOConfig(**kw))


def _six_actions(n, **cfg):
    env = R.VecNormalizeDevice(P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=8), n, device=0, seed=12))
    return R.PPO(env, R.PPOConfig(n_steps=16, batch_size=64, n_epochs=2, seed=12, fused_six_actions=True, episode_stats=True, **cfg))


def _three_actions(n, **cfg):
    # a low-level controller the way tests/test_highlevel_learner_gpu.py and tests/test_learner_diag_gpu.py make one
    from pyflyt_drone_amd.highlevel import HighLevelCmdVecEnv
    torch.manual_seed(21)
    pol = R.MlpPolicy(21, 6)
    with torch.no_grad():
        for q in pol.parameters():
            q.add_(0.1 * torch.randn_like(q))
    g = np.random.default_rng(21)
    mean = g.normal(0.0, 1.0, 21) * np.array([1] * 6 + [10] * 6 + [0.3] * 6 + [1, 50, 10], dtype=np.float64)
    var = g.uniform(0.2, 4.0, 21) * np.array([1] * 6 + [100] * 6 + [0.1] * 6 + [3, 2500, 80], dtype=np.float64)
    env = R.VecNormalizeDevice(HighLevelCmdVecEnv(n, pol, (mean, var), seed=13, max_duration_seconds=SHORT), gamma=0.995)
    return R.PPO(env, R.PPOConfig(n_steps=16, batch_size=64, n_epochs=2, gamma=0.995, seed=13, fused_three_actions=True,
                                  episode_stats=True, **cfg))


def test_torch_collector_reports_what_the_sb3_statement_reports():
    ppo = _waypoints(16, use_graphs=False, fused_collect=False)
    assert not ppo._collect_fused and ppo.episode_monitor is not None
    venv, record = ppo.env.venv, []
    step_tensor = venv.step_tensor

    def recording(actions):
        out = step_tensor(actions)
        record.append(tuple(x.cpu().numpy().copy() for x in (venv.rewards, venv.terminated, venv.truncated, venv.info)))
        return out
    venv.step_tensor = recording
    ref, fed = J.Sb3Statement(16, 100), 0
    for it in range(3):
        ppo.collect_rollouts()
        for step in record[fed:]:
            ref.step(*step)
        fed = len(record)
        assert fed == 16 * (it + 1)
        s = ppo.rollout_stats
        assert J.same_scalars(s, ref.window_scalars())
        J.assert_window_equal(ppo.episode_monitor.window(), ref.window())
    assert len(ref.all) >= 4 * 16 and s["rollout/episodes"] == len(ref.all)
    assert s["rollout/interval/episodes"] > 0 and s["rollout/timeout_rate"] > 0
    venv.close()


@pytest.mark.parametrize("make,kind", [(lambda: _waypoints(16, one_launch_collect=False), "three-launch"),
                                       (lambda: _waypoints(64), "one-launch"),
                                       (lambda: _six_actions(16), "six-action"),
                                       (lambda: _three_actions(16), "three-action")],
                         ids=["three-launch", "one-launch", "six-action", "three-action"])
def test_fused_collectors_keep_the_exact_invariants(make, kind):
    ppo = make()
    m, venv, N = ppo.episode_monitor, ppo.env.venv, ppo.env.num_envs
    assert ppo._collect_fused and ppo._graphs and bool(ppo._one_launch) == (kind == "one-launch")
    assert ppo.act_dim == {"three-launch": 4, "one-launch": 4, "six-action": 6, "three-action": 3}[kind]
    episodes = 0
    for it in range(3):                                      # eager, captured, replayed
        ppo.collect_rollouts()
        s = ppo.rollout_stats
        torch.cuda.synchronize()
        # every episode start the rollout buffer saw is an episode the monitor finished
        starts = int((ppo.buf_start[1:] == 1).sum().item()) + int((ppo.last_starts == 1).sum().item())
        assert s["rollout/episodes"] - episodes == starts == s["rollout/interval/episodes"]
        episodes = s["rollout/episodes"]
        t, v = m.totals(), m._views()
        assert t["steps"] == 16 * (it + 1)
        assert t["sum_len"] + int(v["cur_len"].sum().item()) == t["steps"] * N
        w = m.window()
        assert np.array_equal(w["l"], w["info"][:, K.INFO_EP_LEN])             # the env's own count of the episode's agent steps
        key = w["step"] * N + w["env"]
        assert (np.diff(key) > 0).all() and (w["env"] >= 0).all() and (w["env"] < N).all() and (w["step"] <= t["steps"]).all()
        # FW_S_EP_RETURN: the step kernels add the very reward they write out, in the env dtype (`ep_return += rew`, cleared by the
        # auto-reset; csrc/fwsim.hip, fwsim_direct.hpp).  These envs are float64, so the env and the monitor add the same doubles in
        # the same order from the same zero: the bound is 0.
        assert venv.torch_dtype == torch.float64
        state = venv.get_state()
        assert np.array_equal(v["cur_ret"].cpu().numpy(), state[:, K.S_EP_RETURN])
    assert ppo._g_rollout is not None and episodes >= 4 * N
    ppo.train()                                              # the figures do not get in the update's way
    assert all(torch.isfinite(p).all() for p in ppo.policy.parameters())
    venv.close()


def test_take_back_restores_the_block_of_before_the_rollout():
    ppo = _waypoints(64)
    assert ppo._one_launch
    m = ppo.episode_monitor
    for step in J.make_stream(64, 100, True, seed=9)[:4]:    # a block that is not the fresh one: some history in front of the rollout
        m.fold(*_dev(step))
    m.scalars()
    torch.cuda.synchronize()
    before, base = m.state.clone(), dict(m._last)
    ppo.collect_rollouts()
    torch.cuda.synchronize()
    assert torch.equal(m._saved, before)                     # snapshotted where the normaliser's statistics are saved
    assert not torch.equal(m.state, before) and ppo.rollout_stats["rollout/episodes"] > base["episodes"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ppo._take_back_void_rollout(1, 1)                    # (called directly: no wait is made to run out)
    assert torch.equal(m.state, before) and m._last == base  # byte for byte, and the interval base with it
    assert ppo.rollout_stats == {}
    ppo.collect_rollouts()                                   # the same rollout again, on the three-launch collector
    assert not ppo._one_launch and ppo.collect_fallbacks == 1
    assert ppo.rollout_stats["rollout/episodes"] > base["episodes"]
    ppo.env.venv.close()


def test_checkpoint_resume_continues_window_and_totals(tmp_path):
    a = _waypoints(16, window=20, one_launch_collect=False)
    a.collect_rollouts(); a.train()
    a.collect_rollouts()
    torch.cuda.synchronize()
    assert int(a.episode_monitor._views()["cur_len"].max().item()) > 0           # mid-episode
    path = checkpoint.save(str(tmp_path / "stats.pt"), a)
    a.collect_rollouts()
    b = _waypoints(16, window=20, one_launch_collect=False)
    sd = checkpoint.load(path, b, reset_num_timesteps=False, restore_env_state=True)
    assert "episode_stats" in sd
    b.collect_rollouts()
    torch.cuda.synchronize()
    assert torch.equal(a.episode_monitor.state, b.episode_monitor.state)
    J.assert_window_equal(a.episode_monitor.window(), b.episode_monitor.window())
    assert a.episode_monitor.totals() == b.episode_monitor.totals()
    # a checkpoint written with the flag off leaves a fresh monitor
    off = _waypoints(16, stats=False, one_launch_collect=False)
    off.collect_rollouts()
    assert "episode_stats" not in off.state_dict()
    b.load_state_dict(off.state_dict())
    assert int(b.episode_monitor.state.abs().sum().item()) == 0
    for p in (a, b, off):
        p.env.venv.close()


def test_flag_off_twin_on_the_one_launch_collector_and_the_fused_update():
    on, off = _waypoints(64, stats=True), _waypoints(64, stats=False)
    assert on._one_launch and off._one_launch and off.episode_monitor is None
    for _ in range(2):
        for p in (on, off):
            p.collect_rollouts(); p.train()
    torch.cuda.synchronize()
    assert on._fused is not None and on._fused.synced
    for p, q in zip(on.policy.parameters(), off.policy.parameters()):
        assert torch.equal(p, q)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(on.optimizer.state[p][k], off.optimizer.state[q][k])
    assert on.logs == off.logs and off.rollout_stats == {} and on.rollout_stats["rollout/episodes"] > 0
    assert torch.equal(on.buf_rew, off.buf_rew) and torch.equal(on.env.obs_rms.mean, off.env.obs_rms.mean)
    for p in (on, off):
        p.env.venv.close()
