"""The multi-workgroup episode fold on the device: fw_episode_fold_wide against the torch fold of monitor.EpisodeMonitor and SB3's
statement at the block edges of its span, on directed steps, run twice, mixed with fw_episode_fold on one block, under graph
replay, and behind rollout.PPO (PPOConfig.episode_fold) against a one-workgroup twin.

The comparison rule is the one of tests/test_episode_stats_gpu.py: every word of the documented layout bit-equal to the torch fold,
except the two double totals, which are held to Sb3Statement.check_double_totals (|sum - fsum| <= n 2^-52 sum |x|)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_stats_jobs as J  # noqa: E402

import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import _lib  # noqa: E402
from pyflyt_drone_amd import checkpoint  # noqa: E402
from pyflyt_drone_amd import monitor as M  # noqa: E402
from pyflyt_drone_amd import rollout as R  # noqa: E402

pytestmark = pytest.mark.gpu

DOUBLES = (M.H_SUM_RET, M.H_SUM_RET2)          # the two header words whose summation order is the kernel's own
S = _lib.lib().fw_episode_fold_span()          # envs per workgroup (loads without a device)
# one block; a one-env last block; a ragged last wave; a window smaller than, larger than and straddling a block; W > N
SHAPES = [(1, 1), (5, 100), (S, 7), (S + 1, 7), (2 * S + 71, 7), (2 * S + 71, 100), (2 * S + 71, S + 300), (3 * S, 3 * S + 5)]


def _dev(step):
    return tuple(None if x is None else torch.from_numpy(x).cuda() for x in step)


def _cpu(step):
    return tuple(None if x is None else torch.from_numpy(x) for x in step)


def _masked(state, n):
    mask = torch.ones(n, dtype=torch.bool)
    mask[list(DOUBLES)] = False
    return state.cpu()[:n][mask]


def _assert_blocks_equal(dev: M.EpisodeMonitor, ref: M.EpisodeMonitor, ref_eps):
    """Ring, cursor, per-env accumulators and integer totals bit for bit; the double totals to the reordered-sum bound."""
    n = M.state_words(ref.num_envs, ref.window_size)
    assert torch.equal(_masked(dev.state, n), _masked(ref.state, n))
    t = dev.totals()
    ref_eps.check_double_totals(t["sum_ret"], t["sum_ret2"])


def _wide(N, W):
    m = M.EpisodeMonitor(N, W, "cuda", fold="wide")
    assert m.fold_form == "wide" and m.workspace is not None
    m.workspace.fill_(-0x0123456789ABCDEF)       # the workspace needs no initialisation: every call writes every word it reads
    return m


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("N,W", SHAPES)
def test_wide_kernel_equals_the_torch_fold_and_the_sb3_statement(N, W, f64):
    stream = J.make_stream(N, W, f64)
    dev, ref, eps = _wide(N, W), M.EpisodeMonitor(N, W), J.Sb3Statement(N, W)
    for k, step in enumerate(stream):
        dev.fold(*_dev(step))
        ref.fold(*_cpu(step))
        eps.step(*step)
        if k in (2, 4, 6):                       # behind the all-done, the exactly-W and the tail-only step, and at the end
            _assert_blocks_equal(dev, ref, eps)
    _assert_blocks_equal(dev, ref, eps)
    J.assert_window_equal(dev.window(), eps.window())
    assert J.same_scalars(dev.scalars(), eps.window_scalars())
    assert dev.totals()["episodes"] == len(eps.all) and {k: dev.totals()[k] for k in eps.int_totals()} == eps.int_totals()


def _directed(N, rng, done_at):
    rew = rng.normal(size=N) * 3.0 + 0.5
    done = np.zeros(N, dtype=bool)
    done[list(done_at)] = True
    trunc = done & (rng.random(N) < 0.5)
    info = rng.integers(0, 5, (N, J.INFO_DIM)).astype(np.int32)
    return rew, (done & ~trunc).astype(np.uint8), trunc.astype(np.uint8), info


DIRECTED = {
    "block-0-only": lambda: [3, 64, S - 1],
    "last-block-only": lambda: [2 * S, 2 * S + 65, 3 * S - 1],
    "one-per-block": lambda: [S - 1, S, 3 * S - 1],
    # D = W + 1: the dropped one in block 0, the kept five in block 2, block 1 empty (a base that must skip an empty block)
    "dropped-in-block-0-kept-in-block-2": lambda: [7, 2 * S, 2 * S + 1, 2 * S + 63, 2 * S + 64, 3 * S - 1],
}


@pytest.mark.parametrize("case", list(DIRECTED))
def test_directed_steps_on_three_blocks(case):
    N, W = 3 * S, 5
    rng = np.random.default_rng(len(case))
    at = DIRECTED[case]()
    steps = [_directed(N, rng, []), _directed(N, rng, at), _directed(N, rng, []), _directed(N, rng, at), _directed(N, rng, at)]
    dev, ref, eps = _wide(N, W), M.EpisodeMonitor(N, W), J.Sb3Statement(N, W)
    for step in steps:
        dev.fold(*_dev(step))
        ref.fold(*_cpu(step))
        eps.step(*step)
        _assert_blocks_equal(dev, ref, eps)
    J.assert_window_equal(dev.window(), eps.window())
    assert dev.totals()["episodes"] == 3 * len(at)
    if case.startswith("dropped"):
        assert 7 not in dev.window()["env"] and sorted(dev.window()["env"]) == sorted(at[1:])


@pytest.mark.parametrize("cols", [None, 3])
def test_without_info_and_with_three_column_info_rows(cols):
    N, W = 3 * S, 5
    dev, ref, eps = _wide(N, W), M.EpisodeMonitor(N, W), J.Sb3Statement(N, W)
    for rew, te, tr, info in J.make_stream(N, W, True, seed=3):
        i = None if cols is None else np.ascontiguousarray(info[:, :cols])
        dev.fold(*_dev((rew, te, tr, i)))
        ref.fold(*_cpu((rew, te, tr, i)))
        padded = None
        if i is not None:
            padded = np.zeros((N, J.INFO_DIM), dtype=np.int32); padded[:, :cols] = i
        eps.step(rew, te, tr, padded)
    _assert_blocks_equal(dev, ref, eps)
    J.assert_window_equal(dev.window(), eps.window())


def test_the_same_bits_twice():
    N, W = 2 * S + 71, 100
    stream = J.make_stream(N, W, True, seed=8)
    a, b = _wide(N, W), _wide(N, W)
    b.workspace.zero_()                          # (and whatever the workspace held before)
    for step in stream:
        a.fold(*_dev(step))
    for step in stream:
        b.fold(*_dev(step))
    assert torch.equal(a.state, b.state)         # the two double words included


def test_the_two_forms_mix_on_one_block():
    N, W = 2 * S + 71, 100
    stream = J.make_stream(N, W, False, seed=9)
    wide, one = _wide(N, W), M.EpisodeMonitor(N, W, "cuda", fold="one")
    assert one.workspace is None
    one.state = wide.state                       # one block, two forms
    ref, eps = M.EpisodeMonitor(N, W), J.Sb3Statement(N, W)
    for k, step in enumerate(stream):
        (wide if k % 2 == 0 else one).fold(*_dev(step))
        ref.fold(*_cpu(step))
        eps.step(*step)
        _assert_blocks_equal(wide, ref, eps)
    J.assert_window_equal(one.window(), eps.window())


def test_eight_wide_folds_in_one_graph_replayed_three_times_equal_24_eager_folds():
    N, W = 2 * S + 71, 7
    streams = [J.make_stream(N, W, True, seed=20 + r)[:8] for r in range(3)]
    dev, eager = _wide(N, W), _wide(N, W)
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


# ------------------------------------------------------------------------------------------------------------ behind PPO
SHORT = 0.25           # max_duration_seconds: 7 agent steps at 30 Hz, so episodes end inside a rollout of 16 steps


def _waypoints(n, fold, window=100, seed=11, **cfg):
    env = R.VecNormalizeDevice(P.FixedwingWaypointsVecEnv(n, angle_representation="euler", max_duration_seconds=SHORT, seed=seed))
    kw = dict(n_steps=16, batch_size=64, n_epochs=1, seed=seed, episode_stats=True, stats_window_size=window, episode_fold=fold)
    kw.update(cfg)
    return R.PPO(env, R.PPOConfig(**kw))


def _assert_same_figures(wide: R.PPO, one: R.PPO):
    """Window figures, integer totals and rollout/episodes equal; the two double totals within 2 n 2^-52 sqrt(n sum_ret2): the
    reordered-sum bound n 2^-52 sum |x| for each of the two orders, with sum |x| <= sqrt(n sum x^2)."""
    torch.cuda.synchronize()
    mw, mo = wide.episode_monitor, one.episode_monitor
    n = M.state_words(mo.num_envs, mo.window_size)
    assert torch.equal(_masked(mw.state, n), _masked(mo.state, n))
    J.assert_window_equal(mw.window(), mo.window())
    tw, to = mw.totals(), mo.totals()
    assert {k: v for k, v in tw.items() if not k.startswith("sum_ret")} == {k: v for k, v in to.items() if not k.startswith("sum_ret")}
    eps = to["episodes"]
    assert eps > 0
    bound = 2 * eps * 2.0 ** -52 * math.sqrt(eps * to["sum_ret2"])
    assert abs(tw["sum_ret"] - to["sum_ret"]) <= bound, (tw["sum_ret"], to["sum_ret"], bound)
    # (the squared returns: the same bound with x^2 in place of x, sum x^2 itself in place of sum |x|)
    assert abs(tw["sum_ret2"] - to["sum_ret2"]) <= 2 * eps * 2.0 ** -52 * to["sum_ret2"]
    sw, so = wide.rollout_stats, one.rollout_stats
    window_keys = [k for k in so if "/interval/" not in k]
    assert J.same_scalars(sw, so, window_keys) and sw["rollout/episodes"] == so["rollout/episodes"] == eps
    assert sw["rollout/interval/episodes"] == so["rollout/interval/episodes"]


@pytest.mark.parametrize("n,one_launch", [(2 * S + 8, False), (16, True)], ids=["three-launch", "one-launch"])
def test_wide_behind_ppo_equals_a_one_workgroup_twin(n, one_launch):
    wide, one = _waypoints(n, "wide", one_launch_collect=one_launch), _waypoints(n, "one", one_launch_collect=one_launch)
    assert wide.episode_monitor.fold_form == "wide" and one.episode_monitor.fold_form == "one"
    for p in (wide, one):
        assert p._collect_fused and p._graphs and bool(p._one_launch) == one_launch
    for _ in range(2):
        for p in (wide, one):
            p.collect_rollouts(); p.train()
        _assert_same_figures(wide, one)
    assert wide.episode_monitor.totals()["episodes"] >= 2 * n
    for p, q in zip(wide.policy.parameters(), one.policy.parameters()):
        assert torch.equal(p, q)
    for p in (wide, one):
        p.env.venv.close()


def test_checkpoint_written_under_wide_resumes_under_one(tmp_path):
    a = _waypoints(16, "wide", window=20, one_launch_collect=False)
    a.collect_rollouts(); a.train()
    a.collect_rollouts()
    torch.cuda.synchronize()
    assert int(a.episode_monitor._views()["cur_len"].max().item()) > 0           # mid-episode
    path = checkpoint.save(str(tmp_path / "wide.pt"), a)
    a.collect_rollouts()
    b = _waypoints(16, "one", window=20, one_launch_collect=False)
    sd = checkpoint.load(path, b, reset_num_timesteps=False, restore_env_state=True)
    assert "episode_stats" in sd and b.episode_monitor.fold_form == "one"
    b.collect_rollouts()
    _assert_same_figures(a, b)
    for p in (a, b):
        p.env.venv.close()
