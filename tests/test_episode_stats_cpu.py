"""Rollout episode statistics (monitor.EpisodeMonitor, PPOConfig.episode_stats) without a device: the torch fold against SB3's
Monitor + ep_info_buffer written out, the empty window, the interval figures, checkpoint and snapshot round trips, the argument
errors of fw_episode_fold / fw_episode_state_bytes through the C ABI, the flag-off twin on a CPU toy env, and the world_size-2 sum."""
import ctypes as C
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_stats_jobs as J  # noqa: E402

from pyflyt_drone_amd import config as K  # noqa: E402
from pyflyt_drone_amd import monitor as M  # noqa: E402
from pyflyt_drone_amd import rollout as R  # noqa: E402

WINDOW_KEYS = ("rollout/ep_rew_mean", "rollout/ep_len_mean", "rollout/success_rate", "rollout/targets_reached_mean",
               "rollout/collision_rate", "rollout/out_of_bounds_rate", "rollout/duck_strike_rate", "rollout/timeout_rate",
               "rollout/episodes")
INTERVAL_KEYS = ("rollout/interval/episodes", "rollout/interval/ep_rew_mean", "rollout/interval/ep_len_mean",
                 "rollout/interval/success_rate", "rollout/interval/targets_reached_mean", "rollout/interval/collision_rate",
                 "rollout/interval/out_of_bounds_rate", "rollout/interval/duck_strike_rate", "rollout/interval/timeout_rate")


def _feed(m, stream, ref=None):
    for rew, te, tr, info in stream:
        m.fold(torch.from_numpy(rew), torch.from_numpy(te), torch.from_numpy(tr), torch.from_numpy(info))
        if ref is not None:
            ref.step(rew, te, tr, info)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("N,W", J.SHAPES)
def test_torch_fold_equals_the_sb3_statement(N, W, f64):
    stream = J.make_stream(N, W, f64)
    dones = [int(((te | tr) != 0).sum()) for _, te, tr, _ in stream]
    assert N in dones and 0 in dones and min(W, N) in dones                   # every env, none, exactly W (or all there are)
    tail = [i for i, (_, te, tr, _) in enumerate(stream) if ((te | tr)[N - N % 64:] != 0).all() and not ((te | tr)[:N - N % 64] != 0).any()]
    assert tail or N % 64 == 0
    m, ref = M.EpisodeMonitor(N, W), J.Sb3Statement(N, W)
    for k, step in enumerate(stream):
        _feed(m, [step], ref)
        J.assert_window_equal(m.window(), ref.window())                        # after every step, not only at the end
    t = m.totals()
    for k, v in ref.int_totals().items():
        assert t[k] == v and isinstance(t[k], int), k
    ref.check_double_totals(t["sum_ret"], t["sum_ret2"])
    s = m.scalars()
    assert set(s) == set(WINDOW_KEYS) | set(INTERVAL_KEYS)
    assert J.same_scalars(s, ref.window_scalars())
    # the running episodes: what the statement still holds
    v = m._views()
    assert np.array_equal(v["cur_ret"].numpy(), np.array(ref.cur_r)) and np.array_equal(v["cur_len"].numpy(), np.array(ref.cur_l))
    # the first interval is everything so far
    n = len(ref.all)
    assert s["rollout/interval/episodes"] == n
    assert s["rollout/interval/ep_len_mean"] == sum(e["l"] for e in ref.all) / n
    assert s["rollout/interval/success_rate"] == sum(int(e["info"][5]) for e in ref.all) / n
    assert s["rollout/interval/timeout_rate"] == sum(e["truncated"] for e in ref.all) / n
    exact = math.fsum(e["r"] for e in ref.all)
    assert abs(s["rollout/interval/ep_rew_mean"] * n - exact) <= n * 2.0 ** -52 * math.fsum(abs(e["r"]) for e in ref.all) + abs(exact) * 2.0 ** -52


def test_no_info_pushes_zero_rows_and_short_info_rows_are_padded():
    N, W = 9, 4
    stream = J.make_stream(N, W, True, seed=3)
    m, ref = M.EpisodeMonitor(N, W), J.Sb3Statement(N, W)
    for rew, te, tr, info in stream:
        m.fold(torch.from_numpy(rew), torch.from_numpy(te), torch.from_numpy(tr), None)
        ref.step(rew, te, tr, None)
    J.assert_window_equal(m.window(), ref.window())
    assert m.totals()["sum_is_success"] == 0
    m2, ref2 = M.EpisodeMonitor(N, W), J.Sb3Statement(N, W)
    for rew, te, tr, info in stream:
        m2.fold(torch.from_numpy(rew), torch.from_numpy(te), torch.from_numpy(tr), torch.from_numpy(info[:, :3].copy()))
        padded = info.copy(); padded[:, 3:] = 0
        ref2.step(rew, te, tr, padded)
    J.assert_window_equal(m2.window(), ref2.window())
    assert m2.totals()["sum_collision"] == ref2.int_totals()["sum_collision"] > 0


def test_empty_window_gives_nan_means_and_zero_counts():
    m = M.EpisodeMonitor(6, 3)
    for _ in range(2):
        m.fold(torch.ones(6), torch.zeros(6, dtype=torch.uint8), torch.zeros(6, dtype=torch.uint8), None)
    s = m.scalars()
    for k, v in s.items():
        if k in ("rollout/episodes", "rollout/interval/episodes"):
            assert v == 0.0
        else:
            assert math.isnan(v), k
    w = m.window()
    assert all(a.shape[0] == 0 for a in w.values())
    t = m.totals()
    assert t["steps"] == 2 and t["episodes"] == 0 and t["sum_ret"] == 0.0
    with pytest.raises(ValueError):
        M.EpisodeMonitor(0, 3)
    with pytest.raises(ValueError):
        M.EpisodeMonitor(3, 0)
    with pytest.raises(ValueError):
        m.fold(torch.ones(5), torch.zeros(6, dtype=torch.uint8), torch.zeros(6, dtype=torch.uint8), None)


def test_interval_figures_cover_the_episodes_since_the_previous_read():
    N, W = 199, 7
    stream = J.make_stream(N, W, True, seed=2)
    m, ref = M.EpisodeMonitor(N, W), J.Sb3Statement(N, W)
    seen = 0
    for part in (stream[:3], stream[3:5], stream[5:6], stream[6:]):           # (the third part is the step without a done)
        _feed(m, part, ref)
        s = m.scalars()
        new = ref.all[seen:]
        seen = len(ref.all)
        assert s["rollout/interval/episodes"] == len(new) and s["rollout/episodes"] == seen
        if not new:
            assert all(math.isnan(s[k]) for k in INTERVAL_KEYS if k != "rollout/interval/episodes")
            continue
        assert s["rollout/interval/ep_len_mean"] == sum(e["l"] for e in new) / len(new)
        assert s["rollout/interval/targets_reached_mean"] == sum(int(e["info"][0]) for e in new) / len(new)
        assert s["rollout/interval/collision_rate"] == sum(int(e["info"][1]) for e in new) / len(new)
        # (a difference of two running sums: the rounding of both, each bounded as the totals are)
        bound = 2 * seen * 2.0 ** -52 * math.fsum(abs(e["r"]) for e in ref.all) / len(new)
        assert abs(s["rollout/interval/ep_rew_mean"] - math.fsum(e["r"] for e in new) / len(new)) <= bound
        assert J.same_scalars(s, ref.window_scalars())
    again = m.scalars()                                                        # nothing finished in between
    assert again["rollout/interval/episodes"] == 0 and math.isnan(again["rollout/interval/ep_rew_mean"])
    assert J.same_scalars(again, ref.window_scalars())


def test_state_dict_round_trip_continues_like_the_original(tmp_path):
    N, W = 199, 7
    stream = J.make_stream(N, W, False, seed=4)
    a = M.EpisodeMonitor(N, W)
    _feed(a, stream[:5])
    a.scalars()
    sd = a.state_dict()
    path = str(tmp_path / "episode_stats.pt")
    torch.save(sd, path)
    sd = torch.load(path, map_location="cpu", weights_only=True)               # (what checkpoint.load does)
    b = M.EpisodeMonitor(N, W)
    b.load_state_dict(sd)
    assert torch.equal(a.state, b.state)
    _feed(a, stream[5:]); _feed(b, stream[5:])
    assert torch.equal(a.state, b.state)
    assert J.same_scalars(a.scalars(), b.scalars())                            # the interval base travelled too
    with pytest.raises(ValueError):
        M.EpisodeMonitor(N, W + 1).load_state_dict(sd)
    with pytest.raises(ValueError):
        M.EpisodeMonitor(N + 1, W).load_state_dict(sd)


def test_snapshot_and_restore_take_a_rollout_back():
    N, W = 199, 7
    stream = J.make_stream(N, W, True, seed=5)
    m = M.EpisodeMonitor(N, W)
    assert m.restore() is False
    _feed(m, stream[:4])
    first = m.scalars()
    before = m.state.clone()
    addr = m.state.data_ptr()
    m.snapshot()
    _feed(m, stream[4:])
    m.scalars()
    assert not torch.equal(m.state, before)
    assert m.restore() is True
    assert torch.equal(m.state, before) and m.state.data_ptr() == addr         # in place: a captured graph keeps the address
    _feed(m, stream[4:])
    twin = M.EpisodeMonitor(N, W)
    _feed(twin, stream[:4]); twin.scalars(); _feed(twin, stream[4:])
    assert torch.equal(m.state, twin.state)
    assert J.same_scalars(m.scalars(), twin.scalars()) and first["rollout/episodes"] > 0


def test_argument_errors_and_state_size_through_the_c_abi():
    from pyflyt_drone_amd import _lib
    L = _lib.lib()                              # (loads without a device; a missing or stale library is a failure, not a skip)
    for n, w in ((16, 100), (1, 1), (65536, 100), (199, 7)):
        assert L.fw_episode_state_bytes(n, w) >= 8 * M.state_words(n, w)
        assert M.state_words(n, w) == 16 + 9 * w + 2 * n                       # header, ring (5 words + 8 int32 per slot), accumulators
    for n, w in ((0, 4), (-1, 4), (4, 0), (4, -2)):
        assert L.fw_episode_state_bytes(n, w) == K.FW_EINVAL
    one = C.c_void_p(16)                        # (a non-NULL address: the checks below return before anything is read)

    def call(reward=one, term=one, trunc=one, info=None, info_dim=0, state=one, n=8, w=4):
        return L.fw_episode_fold(reward, 1, term, trunc, info, info_dim, state, n, w, None)
    for kw in (dict(reward=None), dict(term=None), dict(trunc=None), dict(state=None)):
        assert call(**kw) == K.FW_EINVAL and "must be non-NULL" in L.fw_last_error(None).decode()
    for kw in (dict(n=0), dict(n=-5), dict(w=0), dict(w=-1)):
        assert call(**kw) == K.FW_EINVAL and "must be positive" in L.fw_last_error(None).decode()
    for d in (0, -8):
        assert call(info=one, info_dim=d) == K.FW_EINVAL and "info_dim" in L.fw_last_error(None).decode()
    assert "fw_episode_fold" in _lib.EXPORTS and "fw_episode_state_bytes" in _lib.EXPORTS


def _train_state(ppo):
    out = [p.detach().clone() for p in ppo.policy.parameters()]
    for p in ppo.policy.parameters():
        st = ppo.optimizer.state[p]
        out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone(), torch.as_tensor(float(st["step"]))]
    return out


def _toy_ppo(**cfg):
    venv = J.ToyVenv(n=16, d=6, seed=3)
    kw = dict(n_steps=8, batch_size=32, n_epochs=2, seed=9, use_graphs=False)
    kw.update(cfg)
    return R.PPO(R.VecNormalizeDevice(venv), R.PPOConfig(**kw), gae_fn=R.gae_reference), venv


def test_flag_off_twin_on_the_toy_env_and_the_figures_of_the_torch_collector():
    assert R.PPOConfig().episode_stats is False and R.PPOConfig().stats_window_size == 100
    never, _ = _toy_ppo()
    off, _ = _toy_ppo(episode_stats=False)
    on, venv = _toy_ppo(episode_stats=True, stats_window_size=10)
    ref = J.Sb3Statement(16, 10)
    fed = 0
    for it in range(2):
        for p in (never, off, on):
            p.collect_rollouts(); p.train()
        assert never.logs == off.logs == on.logs
        assert off.rollout_stats == {} and off.episode_monitor is None and never.episode_monitor is None
        for step in venv.record[fed:]:
            ref.step(*step)
        fed = len(venv.record)
        assert fed == 8 * (it + 1)
        s = on.rollout_stats
        assert J.same_scalars(s, ref.window_scalars()) and s["rollout/episodes"] > 16
        J.assert_window_equal(on.episode_monitor.window(), ref.window())
        w = on.episode_monitor.window()
        assert np.array_equal(w["l"], w["info"][:, K.INFO_EP_LEN])             # the env's own episode length
    for x, y, z in zip(_train_state(never), _train_state(off), _train_state(on)):
        assert torch.equal(x, y) and torch.equal(x, z)
    keys = {"policy", "optimizer", "vecnormalize", "num_timesteps"}
    assert set(off.state_dict()) == keys == set(never.state_dict())
    assert set(on.state_dict()) == keys | {"episode_stats"}
    # a checkpoint of the flag-on learner resumes window and totals; one written with the flag off leaves a fresh monitor
    fresh, _ = _toy_ppo(episode_stats=True, stats_window_size=10)
    fresh.load_state_dict(on.state_dict())
    assert torch.equal(fresh.episode_monitor.state, on.episode_monitor.state)
    fresh.load_state_dict(off.state_dict())
    assert int(fresh.episode_monitor.state.abs().sum()) == 0
    # an env without the output buffers cannot be monitored: an error, not silence
    class Bare:
        device, num_envs, obs_dim = torch.device("cpu"), 4, 3
    with pytest.raises(ValueError, match="episode_stats"):
        bare = Bare(); bare.venv = Bare()
        R.PPO(bare, R.PPOConfig(episode_stats=True, use_graphs=False))


def test_vec_monitor_device_folds_behind_every_step_of_a_callers_own_loop():
    venv = J.ToyVenv(n=16, d=6, seed=5)
    mon = M.VecMonitorDevice(venv, window=12)
    assert mon.num_envs == 16 and mon.monitor.window_size == 12               # everything else is the wrapped env's
    mon.reset_tensor()
    ref = J.Sb3Statement(16, 12)
    g = torch.Generator().manual_seed(1)
    for _ in range(20):
        mon.step_tensor(torch.randn((16, 4), generator=g))
        ref.step(*venv.record[-1])
    J.assert_window_equal(mon.monitor.window(), ref.window())
    assert J.same_scalars(mon.monitor.scalars(), ref.window_scalars())


def test_world_size_2_sums_equal_one_monitor_fed_both_streams():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = [ctx.Process(target=J.monitor_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60); assert p.exitcode == 0
    a, b = res[0][1], res[1][1]
    assert a["reduces"] == b["reduces"] == 2                                   # one all-reduce per read
    N, W = 37, 5
    streams = [J.make_stream(N, W, True, seed=11 + r) for r in range(2)]
    both = M.EpisodeMonitor(2 * N, W)
    ref = J.Sb3Statement(2 * N, W)
    want = []
    for lo, hi in ((0, 6), (6, len(streams[0]))):
        for x, y in zip(streams[0][lo:hi], streams[1][lo:hi]):
            step = tuple(np.concatenate([u, v]) for u, v in zip(x, y))
            _feed(both, [step], ref)
        want.append(both.scalars())
    for k in range(2):
        assert J.same_scalars(a["scalars"][k], b["scalars"][k])                # every rank reports the job's figures
        got = a["scalars"][k]
        exact = [key for key in INTERVAL_KEYS if key != "rollout/interval/ep_rew_mean"] + ["rollout/episodes"]
        assert J.same_scalars(got, want[k], exact)
        n = want[k]["rollout/interval/episodes"]
        bound = 2 * len(ref.all) * 2.0 ** -52 * math.fsum(abs(e["r"]) for e in ref.all) / n
        assert abs(got["rollout/interval/ep_rew_mean"] - want[k]["rollout/interval/ep_rew_mean"]) <= bound
    t = both.totals()
    for key in ("episodes", "truncated", "sum_len", "sum_is_success", "sum_targets_reached"):
        assert a["local"][key] + b["local"][key] == t[key], key
    assert a["local"]["steps"] == b["local"]["steps"] == t["steps"]
    # the window figures: over the union of the ranks' windows (2 W entries)
    union_r = np.concatenate([a["window"]["r"], b["window"]["r"]])
    union_l = np.concatenate([a["window"]["l"], b["window"]["l"]])
    assert a["scalars"][1]["rollout/ep_len_mean"] == union_l.sum() / union_l.size
    assert a["scalars"][1]["rollout/ep_rew_mean"] == pytest.approx(union_r.mean(), rel=1e-14)
