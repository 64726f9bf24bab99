"""Flight records and path figures on the host: flight.path_step (the torch statement of fw_eval_track_wp) against a
plain-Python loop, flight.path_figures (numpy, from recorded rows) against the sums path_step accumulates, EvalResult.path_scalars on
hand-filled results, the FlightTrace accessors, RowLayout.of against config.obs_dim, and the ValueErrors of fly and path_figures=True."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import evaluate, flight
from pyflyt_drone_amd.flight import RowLayout

INF = math.inf


def _norm(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def _python_step(o, r, L, first, cur, carry, att, act, has_delta):
    """one env, one step, from the definitions of DESIGN.md section 2f, in Python floats"""
    s = [0.0] * 12 if first else list(cur)
    if first:
        s[3] = s[11] = INF
    p, v, w = o[att - 3:att], o[att - 6:att - 3], o[0:3]
    a = o[att:att + act]
    p_prev, p_leg, a_prev, r_prev = carry[0:3], carry[3:6], carry[6:12], carry[12]
    s[0] += _norm([p[k] - p_prev[k] for k in range(3)])
    s[1] += _norm(v)
    s[2] += p[2]
    s[3] = min(s[3], p[2])
    s[4] += _norm(w)
    s[5] += sum(abs(a[j] - a_prev[j]) for j in range(act))
    s[6] += o[att + act + 5]
    c = list(carry)
    if r > r_prev:
        if s[7] == 0:
            s[7] = float(L)
        s[8] = float(L)
        s[9] += _norm([p[k] - p_leg[k] for k in range(3)])
        s[10] = s[0]
        s[11] = INF
        c[3:6] = p
    elif has_delta:
        s[11] = min(s[11], _norm(o[att + act + 6:att + act + 9]))
    c[0:3] = p
    c[6:6 + act] = a
    c[12] = float(r)
    return s, c


def _case(att, act, with_delta, seed):
    """64 random rows, then hand-made ones: a reach on an episode's first step, a count that rises by two, ..."""
    rng = np.random.default_rng(seed)
    n = 70
    D = att + act + 6 + (3 if with_delta else 0) + (3 if with_delta and seed % 2 else 0)
    o = rng.normal(0.0, 5.0, size=(n, D))
    o[:, att - 1] = rng.uniform(1.0, 80.0, n)                               # altitudes positive
    cur = np.abs(rng.normal(0.0, 20.0, size=(n, 12)))
    cur[:, 7] = rng.integers(0, 2, n) * rng.integers(1, 9, n)               # some already reached a target
    cur[:, 8] = np.where(cur[:, 7] > 0, cur[:, 7] + rng.integers(0, 5, n), 0)
    carry = rng.normal(0.0, 5.0, size=(n, 13))
    carry[:, 6 + act:12] = 0.0
    carry[:, 12] = rng.integers(0, 4, n)
    reached = carry[:, 12] + (rng.random(n) < 0.3)
    L = rng.integers(2, 40, n)
    first = np.zeros(n, dtype=bool)
    # 64: a reach on an episode's first step; 65: a count that rises by two in one step; 66: a first step, nothing reached;
    # 67: no reach, the closest approach so far is nearer than this row; 68: no reach, this row is nearer; 69: first step after leftovers
    first[64], L[64], carry[64, 12], reached[64] = True, 1, 0, 1
    first[65], carry[65, 12], reached[65] = False, 1, 3
    first[66], L[66], carry[66, 12], reached[66] = True, 1, 0, 0
    carry[67, 12] = reached[67] = 2
    cur[67, 11] = 1e-3
    carry[68, 12] = reached[68] = 2
    cur[68, 11] = 1e6
    first[69], L[69], carry[69, 12], reached[69] = True, 1, 0, 0
    cur[69] = 1e3                                                         # whatever the buffer holds: the sums restart
    return o, reached, L, first, cur, carry, D


@pytest.mark.parametrize("att", [12, 13])
@pytest.mark.parametrize("act", [4, 6])
@pytest.mark.parametrize("with_delta", [True, False], ids=["delta", "no_delta"])
def test_path_step_follows_the_definitions(att, act, with_delta):
    o, reached, L, first, cur, carry, D = _case(att, act, with_delta, seed=att + act)
    lay = RowLayout(D, att, act)
    assert lay.has_target == with_delta and (D == att + act + 6) == (not with_delta)
    s, c = flight.path_step(torch.as_tensor(o), torch.as_tensor(reached), torch.as_tensor(first), torch.as_tensor(cur),
                            torch.as_tensor(carry), lay, torch.as_tensor(L))
    assert s.dtype == torch.float64 and c.dtype == torch.float64 and tuple(s.shape) == (70, 12) and tuple(c.shape) == (70, 13)
    s, c = s.numpy(), c.numpy()
    for i in range(len(o)):
        ws, wc = _python_step(o[i].tolist(), reached[i], int(L[i]), bool(first[i]), cur[i].tolist(), carry[i].tolist(), att, act, with_delta)
        np.testing.assert_allclose(s[i], ws, rtol=1e-13, atol=0, err_msg=str(i))
        np.testing.assert_array_equal(c[i], wc, err_msg=str(i))
    # the hand-made rows say what they were made to say
    p = o[:, att - 3:att]
    assert s[64, 7] == 1 and s[64, 8] == 1 and s[64, 10] == s[64, 0] and s[64, 11] == INF
    assert s[64, 9] == pytest.approx(np.linalg.norm(p[64] - carry[64, 3:6]), rel=1e-13)
    assert s[65, 8] == L[65] and c[65, 12] == 3 and (c[65, 3:6] == p[65]).all()       # one reach step, whatever the count's rise
    assert s[66, 7] == 0 and s[66, 8] == 0 and s[66, 9] == 0 and s[66, 10] == 0 and s[66, 3] == p[66, 2]
    assert s[66, 0] == pytest.approx(np.linalg.norm(p[66] - carry[66, 0:3]), rel=1e-13)  # a one-step episode: |p - p_seed|
    if with_delta:
        d = np.linalg.norm(o[:, att + act + 6:att + act + 9], axis=1)
        assert s[67, 11] == 1e-3 and s[68, 11] == pytest.approx(d[68], rel=1e-13) and s[66, 11] == pytest.approx(d[66], rel=1e-13)
    else:
        assert s[67, 11] == 1e-3 and s[68, 11] == 1e6 and s[66, 11] == INF            # a row without a target: never measured
    assert (s[69] < 1e3).all() or s[69, 11] == INF
    # cur_len itself in place of (first, length)
    s2, c2 = flight.path_step(torch.as_tensor(o), torch.as_tensor(reached), torch.as_tensor(L - 1), torch.as_tensor(cur),
                              torch.as_tensor(carry), lay)
    first_from_len = (L - 1) == 0
    same = first_from_len == first
    np.testing.assert_array_equal(s2.numpy()[same], s[same])
    with pytest.raises(ValueError, match="length"):
        flight.path_step(torch.as_tensor(o), None, torch.as_tensor(first), torch.as_tensor(cur), torch.as_tensor(carry), lay)


def test_path_step_takes_float32_rows_in_double():
    o, reached, L, first, cur, carry, D = _case(12, 4, True, seed=3)
    lay = RowLayout(D, 12, 4)
    o32 = o.astype(np.float32)
    args = (torch.as_tensor(reached), torch.as_tensor(first), torch.as_tensor(cur), torch.as_tensor(carry), lay, torch.as_tensor(L))
    a = flight.path_step(torch.as_tensor(o32), *args)
    b = flight.path_step(torch.as_tensor(o32.astype(np.float64)), *args)
    assert a[0].dtype == torch.float64 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    sa, sb = flight.seed_carry(torch.as_tensor(o32), lay), flight.seed_carry(torch.as_tensor(o32.astype(np.float64)), lay)
    assert sa.dtype == torch.float64 and torch.equal(sa, sb)
    assert torch.equal(sa[:, 0:3], sa[:, 3:6]) and bool((sa[:, 10:13] == 0).all())


def _synthetic_flight(att=12, act=4, T=40, n=8, seed=2):
    """a 40-step sequence for 8 envs: env 0 reaches two targets and ends, env 1 ends at step 1, env 2 is still running at the end,
    env 3 reaches one target on its first step, the others end somewhere without a reach; after an end the env goes on (next episode)"""
    rng = np.random.default_rng(seed)
    D = att + act + 6 + 6
    obs = rng.normal(0.0, 3.0, size=(T + 1, n, D))                          # obs[0]: after the reset; obs[k + 1]: the live row of step k
    obs[:, :, att - 3:att] = np.cumsum(rng.normal(0.0, 1.0, size=(T + 1, n, 3)), axis=0) + [0.0, 0.0, 50.0]
    tobs = obs[1:] + rng.normal(0.0, 0.1, size=(T, n, D))
    tobs[:, :, att - 1] = np.abs(tobs[:, :, att - 1]) + 1.0
    obs[:, :, att - 1] = np.abs(obs[:, :, att - 1]) + 1.0
    end = {0: 30, 1: 0, 3: 12, 4: 5, 5: 17, 6: 39, 7: 8}                    # 0-based step of the first episode's end; env 2: none
    flag = np.zeros((T, n), dtype=np.int64)
    for i, k in end.items():
        flag[k, i] = 1 + (i % 2)
    flag[20, 4] = 1                                                        # a second episode of env 4 (not in the figures)
    reached = np.zeros((T, n), dtype=np.int64)
    reached[10:, 0] = 1
    reached[22:31, 0] = 2
    reached[31:, 0] = 0
    reached[0:13, 3] = 1
    reached[5:, 2] = 1
    return obs, tobs, flag, reached, end, D


def test_path_figures_from_a_trace_equal_the_sums_path_step_accumulates():
    att, act = 12, 4
    obs, tobs, flag, reached, end, D = _synthetic_flight(att, act)
    T, n = flag.shape
    lay = RowLayout(D, att, act)
    # the recorder's rows, as fw_trace_rows writes them
    trace = np.zeros((T, n, D + 2))
    for k in range(T):
        done = flag[k] != 0
        row = np.where(done[:, None], tobs[k], obs[k + 1])
        trace[k] = flight.trace_rows(torch.as_tensor(row), torch.as_tensor(reached[k][:, None].astype(np.int32)), torch.as_tensor(flag[k])).numpy()
    done_any = (flag != 0)
    ended_at = np.where(done_any.any(axis=0), done_any.argmax(axis=0), -1)
    tr = flight.FlightTrace(trace=trace, start=flight.trace_rows(torch.as_tensor(obs[0])).numpy(), dt=1 / 30, ended_at=ended_at, layout=lay)
    got = flight.path_figures(tr)
    # the evaluation's accumulation, step by step
    cur, carry = flight.path_init(n), flight.seed_carry(torch.as_tensor(obs[0]), lay)
    cur_len = torch.zeros(n, dtype=torch.int64)
    want = {}
    for k in range(T):
        done = torch.as_tensor(flag[k] != 0)
        row = torch.where(done[:, None], torch.as_tensor(tobs[k]), torch.as_tensor(obs[k + 1]))
        cur, carry = flight.path_step(row, torch.as_tensor(reached[k]), cur_len == 0, cur, carry, lay, cur_len + 1)
        carry = torch.where(done[:, None], flight.seed_carry(torch.as_tensor(obs[k + 1]), lay), carry)
        cur_len = cur_len + 1
        for i in torch.nonzero(done)[:, 0].tolist():
            want.setdefault(i, (cur[i].numpy().copy(), int(cur_len[i])))
        cur = torch.where(done[:, None], flight.path_init(n), cur)
        cur_len[done] = 0
    assert set(got) == set(want) == set(end) and 2 not in got                # the env still running at the end is in neither
    for i in got:
        assert want[i][1] == end[i] + 1 == len(tr.episode(i))
        np.testing.assert_allclose(got[i], want[i][0], rtol=1e-12, atol=0, err_msg=str(i))
    assert got[0][7] == 11 and got[0][8] == 23 and got[0][10] < got[0][0] and got[0][9] > 0      # two reaches
    assert want[1][1] == 1 and got[1][7] == 0                                                     # the episode that ends at step 1
    assert got[3][7] == 1 and got[3][8] == 1                                                      # a reach on the first step
    assert got[4][7] == 0 and math.isfinite(got[4][11]) and got[0][11] != got[4][11]
    assert len(tr.episode(2)) == T


def test_path_scalars_pool_over_steps_and_skip_what_they_must():
    r = evaluate.EvalResult([-50.0, -20.0, 5.0], [10, 90, 100])
    r.num_targets_reached = [0, 2, 1]
    #           path  speed   alt    min  ang   dact  thr   first last chord  at    miss
    r.add_path([50.0, 200.0, 300.0, 12.0, 5.0, 4.0, 6.0, 0.0, 0.0, 0.0, 0.0, 7.5], complete=False)
    r.add_path([900.0, 1800.0, 4500.0, 3.0, 45.0, 9.0, 45.0, 30.0, 60.0, 400.0, 500.0, INF], complete=False)
    r.add_path([700.0, 2000.0, 2000.0, 8.0, 10.0, 7.0, 50.0, 90.0, 90.0, 300.0, 650.0, 2.5], complete=True)
    sc = r.path_scalars(30.0)
    assert set(sc) == {"eval/" + k for k in evaluate.PATH_SCALARS}
    assert sc["eval/airspeed_mean"] == pytest.approx(4000.0 / 200)
    assert sc["eval/altitude_mean"] == pytest.approx(6800.0 / 200)
    assert sc["eval/ang_vel_mean"] == pytest.approx(60.0 / 200)
    assert sc["eval/throttle_mean"] == pytest.approx(101.0 / 200)
    assert sc["eval/action_delta_mean"] == pytest.approx(20.0 / 200)
    assert sc["eval/path_length_mean"] == pytest.approx(1650.0 / 3)
    assert sc["eval/altitude_min"] == 3.0
    assert sc["eval/time_to_first_target_s"] == pytest.approx((30.0 / 30 + 90.0 / 30) / 2)
    assert sc["eval/time_per_target_s"] == pytest.approx((60.0 + 90.0) / 3 / 30)
    assert sc["eval/path_efficiency"] == pytest.approx(700.0 / 1150.0)
    assert sc["eval/miss_distance_mean"] == 7.5                              # the infinite and the complete episode are skipped
    assert r.path_scalars(30.0, complete=[False, False, False])["eval/miss_distance_mean"] == pytest.approx(5.0)
    # pooled, not the mean of the episodes' means
    assert abs((200.0 / 10 + 1800.0 / 90 + 2000.0 / 100) / 3 - sc["eval/airspeed_mean"]) < 1e-9
    assert abs((300.0 / 10 + 4500.0 / 90 + 2000.0 / 100) / 3 - sc["eval/altitude_mean"]) > 0.5
    # nothing reached, everything complete: the keys are absent
    q = evaluate.EvalResult([1.0], [5])
    q.add_path([5.0, 100.0, 50.0, 9.0, 1.0, 1.0, 2.5, 0.0, 0.0, 0.0, 0.0, 3.0], complete=True)
    sq = q.path_scalars(30.0)
    assert set(sq) == {"eval/airspeed_mean", "eval/altitude_mean", "eval/ang_vel_mean", "eval/throttle_mean", "eval/action_delta_mean",
                       "eval/path_length_mean", "eval/altitude_min"}
    # without the sums: empty; and the other tasks' figures stay away
    plain = evaluate.EvalResult([1.0], [5])
    assert plain.path_scalars(30.0) == {} and plain.path_len == [] and plain.path_complete == []
    assert r.tracking_scalars() == {} and r.command_scalars() == {}


def _quat(e):
    hr, hp, hy = 0.5 * e[0], 0.5 * e[1], 0.5 * e[2]
    cr, sr, cp, sp, cy, sy = math.cos(hr), math.sin(hr), math.cos(hp), math.sin(hp), math.cos(hy), math.sin(hy)
    return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]


def test_flight_trace_accessors_against_numpy():
    rng = np.random.default_rng(8)
    T, n = 5, 3
    for att, act in ((12, 4), (13, 6)):
        D = att + act + 6 + 6
        lay = RowLayout(D, att, act)
        tr = rng.normal(0.0, 2.0, size=(T, n, D + 2))
        eul = rng.uniform(-1.2, 1.2, size=(T, n, 3))
        if att == 13:
            tr[:, :, 3:7] = np.array([[_quat(eul[k, i]) for i in range(n)] for k in range(T)])
        else:
            tr[:, :, 3:6] = eul
        tr[:, :, D] = rng.integers(0, 3, size=(T, n))
        tr[:, :, D + 1] = 0
        tr[3, 1, D + 1], tr[4, 1, D + 1], tr[1, 2, D + 1] = 2, 1, 1
        t = flight.FlightTrace(trace=tr, start=tr[0], dt=1 / 30, ended_at=np.array([-1, 3, 1]), layout=lay)
        np.testing.assert_array_equal(t.position(), tr[:, :, att - 3:att])
        np.testing.assert_allclose(t.airspeed(), np.sqrt((tr[:, :, att - 6:att - 3] ** 2).sum(-1)), rtol=1e-15)
        np.testing.assert_allclose(t.attitude_euler(), eul, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(t.throttle(), tr[:, :, att + act + 5])
        np.testing.assert_array_equal(t.actions(), tr[:, :, att:att + act])
        np.testing.assert_allclose(t.target_distance(), np.sqrt((tr[:, :, att + act + 6:att + act + 9] ** 2).sum(-1)), rtol=1e-15)
        np.testing.assert_array_equal(t.targets_reached(), tr[:, :, D].astype(np.int64))
        np.testing.assert_array_equal(t.flag(), tr[:, :, D + 1].astype(np.int64))
        assert t.episode(0).shape == (T, D + 2) and t.episode(1).shape == (4, D + 2) and t.episode(2).shape == (2, D + 2)
        assert t.position(t.start).shape == (n, 3) and t.flag(t.episode(1))[-1] == 2
        assert t.attitude_euler().shape == (T, n, 3)
        cols = lay.columns()
        assert cols["position"] == (att - 3, att) and cols["flag"] == (D + 1, D + 2) and cols["target"][1] - cols["target"][0] == 3
    bare = flight.FlightTrace(trace=np.zeros((2, 1, 24)), start=np.zeros((1, 24)), dt=1 / 30, ended_at=np.array([-1]), layout=RowLayout(22, 12, 4))
    assert np.isnan(bare.target_distance()).all() and "target" not in bare.layout.columns()
    # the poles of the Euler conversion take Bullet's branch
    q = np.array(_quat([0.0, 0.5 * math.pi, 0.3]))
    e = flight._euler_from_quat(q)
    assert e[0] == 0.0 and e[1] == pytest.approx(0.5 * math.pi)


def test_trace_rows_against_numpy():
    rng = np.random.default_rng(5)
    o = rng.normal(0.0, 3.0, size=(37, 28))
    info = rng.integers(0, 5, size=(37, 8)).astype(np.int32)
    flag = rng.integers(0, 3, size=37)
    got = flight.trace_rows(torch.as_tensor(o), torch.as_tensor(info), torch.as_tensor(flag)).numpy()
    np.testing.assert_array_equal(got, np.concatenate([o, info[:, :1].astype(np.float64), flag[:, None].astype(np.float64)], axis=1))
    bare = flight.trace_rows(torch.as_tensor(o.astype(np.float32))).numpy()
    assert bare.dtype == np.float64 and (bare[:, 28:] == 0).all()
    np.testing.assert_array_equal(bare[:, :28], o.astype(np.float32).astype(np.float64))


def test_row_layout_of_the_four_and_six_action_configs():
    cfgs = {"waypoints_euler": (K.train_waypoints_v3_config(), 12, 4),
            "waypoints_quat_ctx1": (K.waypoints_config(angle_representation="quaternion", context_length=1), 13, 4),
            "objlock": (K.train_objlock_config(), 12, 4),
            "combined": (K.train_waypoint_objlock_config(), 12, 4),
            "direct": (K.highlevel_config(), 12, 6)}
    for name, (cfg, att, act) in cfgs.items():
        lay = RowLayout.of(cfg)
        assert (lay.obs_dim, lay.att_dim, lay.act_dim) == (K.obs_dim(cfg), att, act), name
        assert lay.position == slice(att - 3, att) and lay.velocity == slice(att - 6, att - 3) and lay.ang_vel == slice(0, 3), name
        assert lay.action == slice(att, att + act) and lay.throttle == att + act + 5 and lay.has_target, name
        assert lay.target == slice(att + act + 6, att + act + 9) and lay.target.stop <= lay.obs_dim, name
        assert lay.quaternion == (att == 13) and lay.attitude == slice(3, att - 6), name
    assert RowLayout.of(K.objlock_config_from_reference_kwargs(duck_vision_use_deltas=False, angle_representation="euler")).obs_dim == 52
    assert RowLayout.of(K.objlock_config(angle_representation="euler")).obs_dim == 56
    assert not RowLayout.of(K.waypoints_config(context_length=0)).has_target and RowLayout.of(K.waypoints_config(context_length=0)).target is None
    with pytest.raises(ValueError, match="low-level"):
        RowLayout.of(K.lowlevel_config())
    for bad in ((22, 11, 4), (22, 12, 5), (21, 12, 4)):
        with pytest.raises(ValueError):
            RowLayout(*bad)


def _fake_env(cfg, training=False, **extra):
    venv = SimpleNamespace(cfg=cfg, terminal_obs=None, obs=torch.zeros((2, K.obs_dim(cfg))), **extra)
    return SimpleNamespace(venv=venv, training=training, num_envs=2, device="cpu", norm_obs=True, obs_dim=K.obs_dim(cfg))


def test_fly_and_path_figures_refuse_what_they_are_not_for():
    wp = K.train_waypoints_v3_config()
    with pytest.raises(ValueError, match="training=False"):
        flight.fly(None, _fake_env(wp, training=True), 4)
    with pytest.raises(ValueError, match="command.fly"):
        flight.fly(None, _fake_env(K.lowlevel_config()), 4)
    with pytest.raises(ValueError, match="highlevel.fly"):
        flight.fly(None, _fake_env(K.highlevel_config(), step_low=lambda: None), 4)
    with pytest.raises(ValueError, match="VecNormalizeDevice"):
        flight.fly(None, SimpleNamespace(), 4)
    with pytest.raises(ValueError, match="n_steps"):
        flight.fly(None, _fake_env(wp), 0)
    with pytest.raises(ValueError, match="use_fused=True"):
        flight.fly(None, _fake_env(wp), 4, use_fused=True)                    # no device handle: fw_collect_step cannot apply
    for call in (lambda e: evaluate.evaluate_policy(None, e, path_figures=True),
                 lambda e: evaluate.start_evaluation(None, e, path_figures=True),
                 lambda e: evaluate.ReplayedEvaluation(None, e, np.ones(2, dtype=np.int64), path_figures=True),
                 lambda e: evaluate.EvalCallback(e, path_figures=True)):
        with pytest.raises(ValueError, match="tracking_scalars"):
            call(_fake_env(K.lowlevel_config()))
        with pytest.raises(ValueError, match="command_scalars"):
            call(_fake_env(K.highlevel_config(), step_low=lambda: None))
    cb = evaluate.EvalCallback(_fake_env(wp), path_figures=True)
    assert cb.path_figures is True and evaluate.EvalCallback(None).path_figures is False
