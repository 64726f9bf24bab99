"""Flight records and path figures on the GPU: fw_eval_track_wp and fw_trace_rows against their torch statements
on synthetic buffers; on a real waypoints env with targets put on the path of a zero-action flight, the three evaluation paths -- the
step-by-step loop (flight.path_step), the replayed torch-forward body and the replayed fw_collect_step body (both fw_eval_track_wp) --
against each other; the flight record against the evaluation; and the asynchronous and EvalCallback forms."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from pyflyt_drone_amd import _lib, evalstep, evaluate, flight
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R
from pyflyt_drone_amd.flight import RowLayout
from pyflyt_drone_amd.vec_env import FixedwingObjLockVecEnv, FixedwingWaypointsVecEnv

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _p(t):
    return t.data_ptr() if t is not None else None


def _sums(r):
    return np.array([getattr(r, k) for k in flight.PATH_SUMS]).T              # [episodes, 12]


# ------------------------------------------------------------------------------------------------------------------ the kernels alone
def _synthetic_step(g, n, D, att, td, reached_prev):
    """one vec-step's worth of random env outputs: positive altitudes, both ways of ending and both at once, a count that stays,
    rises by one or by two"""
    obs = (torch.randn((n, D), generator=g, dtype=torch.float64) * 4)
    tobs = (torch.randn((n, D), generator=g, dtype=torch.float64) * 4)
    obs[:, att - 1] = torch.rand(n, generator=g, dtype=torch.float64) * 90 + 1
    tobs[:, att - 1] = torch.rand(n, generator=g, dtype=torch.float64) * 90 + 1
    term = (torch.rand(n, generator=g) < 0.25).to(torch.uint8)
    trunc = (torch.rand(n, generator=g) < 0.2).to(torch.uint8)
    info = torch.randint(0, 5, (n, 4), generator=g, dtype=torch.int32)
    info[:, 0] = (reached_prev + torch.randint(0, 3, (n,), generator=g) * (torch.rand(n, generator=g) < 0.4)).to(torch.int32)
    rew = (torch.randn(n, generator=g, dtype=torch.float64) * 20)
    return obs.to(td), tobs.to(td), term, trunc, info, rew.to(td)


@pytest.mark.parametrize("n", [300, 1030])
@pytest.mark.parametrize("dtype,att,act,ctx", [(torch.float64, 12, 4, 2), (torch.float32, 13, 6, 1), (torch.float64, 13, 4, 0)],
                         ids=["f64_euler_4", "f32_quat_6", "f64_quat_4_no_delta"])
def test_fw_eval_track_wp_against_its_torch_statement(n, dtype, att, act, ctx):
    """six steps on random buffers, N = 300 and N = 1030 (the 256 threads stride four times and more), E = 2, uneven targets that some
    envs outrun: the kernel against flight.path_step plus the host loop of the fw_eval_track_hl test.  Counts, lengths, steps, info rows
    and carry equal, sums to 1e-12, the two selections (alt_min, miss_dist) bit for bit.

    The statement runs twice: on host tensors (IEEE arithmetic: every column to 1e-12) and on device tensors, where torch.sqrt is
    the square root the kernel itself calls.  miss_dist selects among computed norms, and the device's double-precision sqrt is
    not correctly rounded (measured on one MI355X: 27 605 of 2 000 000 random arguments differ from the host's by one ulp), so bit
    equality of the selections is asserted against the device evaluation; against the host one miss_dist agrees to 1e-12."""
    L, E = _lib.lib(), 2
    D = att + act + 6 + 3 * ctx
    lay = RowLayout(D, att, act)
    g = torch.Generator().manual_seed(17 + n)
    tg = torch.randint(1, 3, (n,), generator=g, dtype=torch.int64)
    assert set(tg.tolist()) == {1, 2}
    seed_obs = (torch.randn((n, D), generator=g, dtype=torch.float64) * 4).to(dtype)
    # host state
    counts, cur_len, cur_rew = torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.float64)
    cur, carry = flight.path_init(n), flight.seed_carry(seed_obs, lay)
    cur_d, carry_d = cur.to(DEV), carry.to(DEV)                             # the same statement on device tensors
    fin_sel_d = torch.zeros((n, E, 2), dtype=torch.float64)
    fin_rew, fin_len, fin_step = torch.zeros((n, E), dtype=torch.float64), torch.zeros((n, E), dtype=torch.int64), torch.zeros((n, E), dtype=torch.int64)
    fin_info, fin_path = torch.zeros((n, E, 4), dtype=torch.int32), torch.zeros((n, E, 12), dtype=torch.float64)
    d = {k: v.clone().to(DEV) for k, v in dict(tg=tg, counts=counts, cur_len=cur_len, cur_rew=cur_rew, cur=cur, carry=carry, fin_rew=fin_rew,
                                               fin_len=fin_len, fin_step=fin_step, fin_info=fin_info, fin_path=fin_path).items()}
    d["cur"].fill_(123.0)                                                   # whatever the buffer holds: a first step restarts the sums
    ctr = torch.zeros((), dtype=torch.int64, device=DEV)
    ar = torch.arange(n)
    outran = torch.zeros(n, dtype=torch.bool)
    sel = [flight.PS_ALT_MIN, flight.PS_MISS]
    for step in range(1, 7):
        obs, tobs, term, trunc, info, rew = _synthetic_step(g, n, D, att, dtype, carry[:, 12])
        dv = [x.to(DEV) for x in (obs, tobs, term, trunc, info, rew)]
        rc = L.fw_eval_track_wp(_p(dv[5]), int(dtype == torch.float64), _p(dv[2]), _p(dv[3]), _p(dv[4]), 4, _p(dv[0]), _p(dv[1]),
                                int(dtype == torch.float64), D, att, act, _p(d["tg"]), _p(d["counts"]), _p(d["cur_rew"]), _p(d["cur_len"]),
                                _p(ctr), _p(d["cur"]), _p(d["carry"]), _p(d["fin_rew"]), _p(d["fin_len"]), _p(d["fin_step"]),
                                _p(d["fin_info"]), _p(d["fin_path"]), n, E, None)
        assert rc == K.FW_OK, L.fw_last_error(None)
        torch.cuda.synchronize()
        done = (term | trunc).bool()
        if step == 1:
            row1 = torch.where(done[:, None], tobs, obs).to(torch.float64)
        cur, carry = flight.path_step(torch.where(done[:, None], tobs, obs), info[:, 0], cur_len == 0, cur, carry, lay, cur_len + 1)
        carry = torch.where(done[:, None], flight.seed_carry(obs, lay), carry)
        cur_d, carry_d = flight.path_step(torch.where(done[:, None], tobs, obs).to(DEV), info[:, 0].to(DEV), (cur_len == 0).to(DEV), cur_d,
                                          carry_d, lay, (cur_len + 1).to(DEV))
        carry_d = torch.where(done[:, None].to(DEV), flight.seed_carry(dv[0], lay), carry_d)
        sel_d = cur_d[:, sel].cpu()
        cur_rew = cur_rew + rew.to(torch.float64)
        cur_len = cur_len + 1
        take = done & (counts < tg)
        outran |= done & (counts >= tg)
        slot = counts.clamp(max=E - 1)
        for i in ar[take].tolist():
            s = int(slot[i])
            fin_rew[i, s], fin_len[i, s], fin_step[i, s], fin_info[i, s], fin_path[i, s] = cur_rew[i], cur_len[i], step, info[i], cur[i]
            fin_sel_d[i, s] = sel_d[i]
        counts = counts + take.to(torch.int64)
        cur_rew[done], cur_len[done] = 0.0, 0
        cur = torch.where(done[:, None], flight.path_init(n), cur)
        cur_d = torch.where(done[:, None].to(DEV), flight.path_init(n, DEV), cur_d)
        # after every step: the running state
        assert int(ctr.item()) == step
        assert torch.equal(d["counts"].cpu(), counts) and torch.equal(d["cur_len"].cpu(), cur_len)
        assert torch.equal(d["carry"].cpu().view(torch.int64), carry.view(torch.int64))
        assert torch.equal(d["carry"].view(torch.int64), carry_d.view(torch.int64))
        got = d["cur"].cpu()
        torch.testing.assert_close(got, cur, rtol=1e-12, atol=0)
        torch.testing.assert_close(got, cur_d.cpu(), rtol=1e-12, atol=0)
        assert torch.equal(got[:, sel].view(torch.int64), cur_d[:, sel].cpu().view(torch.int64))
        assert torch.equal(got[:, flight.PS_ALT_MIN].view(torch.int64), cur[:, flight.PS_ALT_MIN].view(torch.int64))      # (copies: the host's too)
        torch.testing.assert_close(d["cur_rew"].cpu(), cur_rew, rtol=1e-12, atol=0)
    assert bool(outran.any()) and bool((counts <= tg).all()) and bool((counts == tg).any())
    assert torch.equal(d["fin_len"].cpu(), fin_len) and torch.equal(d["fin_step"].cpu(), fin_step) and torch.equal(d["fin_info"].cpu(), fin_info)
    torch.testing.assert_close(d["fin_rew"].cpu(), fin_rew, rtol=1e-12, atol=0)
    got = d["fin_path"].cpu()
    torch.testing.assert_close(got, fin_path, rtol=1e-12, atol=0)
    assert torch.equal(got[:, :, sel].view(torch.int64), fin_sel_d.view(torch.int64))
    assert torch.equal(got[:, :, flight.PS_ALT_MIN].view(torch.int64), fin_path[:, :, flight.PS_ALT_MIN].view(torch.int64))
    assert torch.equal(got[:, :, 7:9], fin_path[:, :, 7:9])                   # the reach steps: integers
    rec = fin_len > 0
    assert float(fin_path[:, :, 9].sum()) > 0 and bool((fin_path[:, :, 8] > fin_path[:, :, 7]).any())      # chords, and episodes with two reach steps
    assert bool(torch.isinf(fin_path[:, :, 11][rec]).any()) and (ctx == 0 or bool(torch.isfinite(fin_path[:, :, 11][rec]).any()))
    if ctx == 0:
        assert bool(torch.isinf(fin_path[:, :, 11][rec]).all())               # a row without a target: never measured
    one = fin_len == 1                                                      # one-step episodes: |p - p_seed|, a reach on step 0 or 1
    assert bool(one.any())
    assert bool(((got[:, :, 7][one] == 0) | (got[:, :, 7][one] == 1)).all())
    first_ep_one = one[:, 0] & (fin_step[:, 0] == 1)                        # ... those of the very first step started from seed_obs
    assert bool(first_ep_one.any())
    dp = (row1[:, lay.position] - seed_obs.to(torch.float64)[:, lay.position])[first_ep_one]
    torch.testing.assert_close(got[:, 0, 0][first_ep_one], torch.sqrt(dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1] + dp[:, 2] * dp[:, 2]), rtol=1e-12, atol=0)


@pytest.mark.parametrize("dtype,D", [(torch.float64, 28), (torch.float32, 56)], ids=["f64_28", "f32_56"])
def test_fw_trace_rows_against_its_torch_statement(dtype, D):
    """N = 1100 (the 1024 threads stride), T = 4: four rows against flight.trace_rows, bit for bit, then two calls past the end"""
    L, n, T = _lib.lib(), 1100, 4
    g = torch.Generator().manual_seed(23)
    trace = torch.full((T, n, D + 2), -7.0, dtype=torch.float64, device=DEV)
    idx = torch.zeros((), dtype=torch.int64, device=DEV)
    keep = None
    for k in range(T + 2):
        obs, tobs, term, trunc, info, _ = _synthetic_step(g, n, D, 12, dtype, torch.zeros(n))
        dv = [x.to(DEV) for x in (obs, tobs, term, trunc, info)]
        rc = L.fw_trace_rows(_p(dv[0]), _p(dv[1]), _p(dv[2]), _p(dv[3]), _p(dv[4]), 4, int(dtype == torch.float64), n, D, _p(trace), T,
                             _p(idx), None)
        assert rc == K.FW_OK, L.fw_last_error(None)
        torch.cuda.synchronize()
        assert int(idx.item()) == k + 1
        if k < T:
            done = (term | trunc).bool()
            flag = torch.where(term.bool(), 1, torch.where(trunc.bool(), 2, 0))
            assert set(flag.tolist()) == {0, 1, 2} and bool((term.bool() & trunc.bool()).any())      # terminated wins where both are set
            want = flight.trace_rows(torch.where(done[:, None], tobs, obs), info, flag)
            assert torch.equal(trace[k].cpu().view(torch.int64), want.view(torch.int64))
            if k + 1 < T:
                assert bool((trace[k + 1:] == -7.0).all())
        if k == T - 1:
            keep = trace.clone()
    assert torch.equal(trace, keep)                                          # the calls behind row T - 1 wrote nothing
    # without info and without done flags: zeros in their columns, the live observation
    idx.zero_()
    rc = L.fw_trace_rows(_p(dv[0]), None, None, None, None, 0, int(dtype == torch.float64), n, D, _p(trace), T, _p(idx), None)
    assert rc == K.FW_OK
    torch.cuda.synchronize()
    assert torch.equal(trace[0].cpu(), flight.trace_rows(obs)) and torch.equal(trace[1:], keep[1:])


def test_fw_eval_track_wp_and_fw_trace_rows_reject_bad_arguments():
    L = _lib.lib()
    n, E, D = 8, 2, 28
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)          # noqa: E731
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64, device=DEV)            # noqa: E731
    u8 = torch.zeros(n, dtype=torch.uint8, device=DEV)
    rew, obs, tobs = f64(n), f64(n, D), f64(n, D)
    tg, cnt, cl, ctr, fl, fs = i64(n), i64(n), i64(n), i64(1), i64(n, E), i64(n, E)
    cr, cp, cy, fr, fp = f64(n), f64(n, 12), f64(n, 13), f64(n, E), f64(n, E, 12)

    def call(obs_dim=D, att=12, act=4, N=n, E_=E, obs_=obs, cp_=cp, cy_=cy, fp_=fp):
        return L.fw_eval_track_wp(_p(rew), 1, _p(u8), _p(u8), None, 0, _p(obs_), _p(tobs), 1, obs_dim, att, act, _p(tg), _p(cnt), _p(cr),
                                  _p(cl), _p(ctr), _p(cp_), _p(cy_), _p(fr), _p(fl), _p(fs), None, _p(fp_), N, E_, None)

    def err():
        return L.fw_last_error(None).decode()
    assert call(att=11) == K.FW_EINVAL and "att_dim" in err()
    assert call(act=5) == K.FW_EINVAL and "act_dim" in err()
    assert call(obs_dim=21) == K.FW_EINVAL and "obs_dim" in err()
    assert call(att=13, act=6, obs_dim=24) == K.FW_EINVAL and "obs_dim" in err()
    assert call(obs_=None) == K.FW_EINVAL and "obs" in err()
    assert call(cp_=None) == K.FW_EINVAL and "cur_path" in err()
    assert call(cy_=None) == K.FW_EINVAL and "carry" in err()
    assert call(fp_=None) == K.FW_EINVAL and "fin_path" in err()
    assert call(N=0) == K.FW_EINVAL and "N" in err() and "fw_eval_track_wp" in err()
    assert call(E_=0) == K.FW_EINVAL and "E" in err()
    torch.cuda.synchronize()
    assert int(ctr.item()) == 0 and int(cl.sum().item()) == 0                  # nothing was launched
    assert call() == K.FW_OK                                                 # the same buffers, well formed: one launch
    assert call(obs_dim=22) == K.FW_OK                                       # the shortest row: no target columns
    torch.cuda.synchronize()
    assert int(ctr.item()) == 2 and torch.equal(cl, torch.full_like(cl, 2))
    # fw_trace_rows
    trace, idx = f64(2, n, D + 2), i64(1)
    i32 = torch.zeros((n, 4), dtype=torch.int32, device=DEV)
    assert L.fw_trace_rows(None, None, None, None, None, 0, 1, n, D, _p(trace), 2, _p(idx), None) == K.FW_EINVAL and "obs" in err()
    assert L.fw_trace_rows(_p(obs), None, None, None, None, 0, 1, n, D, None, 2, _p(idx), None) == K.FW_EINVAL
    assert L.fw_trace_rows(_p(obs), None, None, None, None, 0, 1, n, D, _p(trace), 2, None, None) == K.FW_EINVAL
    assert L.fw_trace_rows(_p(obs), None, None, None, None, 0, 1, 0, D, _p(trace), 2, _p(idx), None) == K.FW_EINVAL and "N and T" in err()
    assert L.fw_trace_rows(_p(obs), None, None, None, None, 0, 1, n, D, _p(trace), 0, _p(idx), None) == K.FW_EINVAL
    assert L.fw_trace_rows(_p(obs), None, None, None, None, 0, 1, n, 0, _p(trace), 2, _p(idx), None) == K.FW_EINVAL and "obs_dim" in err()
    assert L.fw_trace_rows(_p(obs), None, None, None, _p(i32), 0, 1, n, D, _p(trace), 2, _p(idx), None) == K.FW_EINVAL and "info_dim" in err()
    torch.cuda.synchronize()
    assert int(idx.item()) == 0
    assert L.fw_trace_rows(_p(obs), None, None, None, None, 0, 1, n, D, _p(trace), 2, _p(idx), None) == K.FW_OK
    torch.cuda.synchronize()
    assert int(idx.item()) == 1


# ------------------------------------------------------------------------------------------------------------------ a real env
N_ENVS, SECONDS = 16, 2.0
FAR = (-80.0, 0.0, 50.0)                    # a waypoint the 2 s flight never comes near


def _zero_policy(obs_dim, act_dim=4):
    torch.manual_seed(5)
    p = R.MlpPolicy(obs_dim, act_dim).to(DEV)
    with torch.no_grad():
        p.action_net.weight.zero_()
        p.action_net.bias.zero_()
    return p


def _waypoints_env(targets=None, seed=9, **kw):
    """16 waypoint envs (quaternion, context 2: 29 columns), f64, motor noise off, 2 s episodes, two targets; every reset of the
    wrapper starts the episodes on ``targets`` [N, 2, 3] (fw_scenario)"""
    venv = FixedwingWaypointsVecEnv(N_ENVS, num_targets=2, max_duration_seconds=SECONDS, motor_noise=False, seed=seed, **kw)
    if targets is not None:
        venv.reset_tensor = functools.partial(venv.reset_tensor, scenario=dict(targets=targets))
    env = R.VecNormalizeDevice(venv, training=False, norm_reward=False)
    with torch.no_grad():                                                  # statistics as after some training
        env.obs_rms.mean.copy_(torch.linspace(-0.2, 0.3, env.obs_dim, dtype=torch.float64, device=DEV))
        env.obs_rms.var.copy_(torch.linspace(0.5, 2.0, env.obs_dim, dtype=torch.float64, device=DEV))
    return env


_PATH = {}


def _zero_action_path():
    """the positions of a zero-action flight, one per agent step, read from a plain step_tensor loop (no new code): without motor noise
    or wind every env flies it.  Computed once."""
    if "p" not in _PATH:
        far = np.tile(np.array(FAR), (N_ENVS, 2, 1))
        venv = FixedwingWaypointsVecEnv(N_ENVS, num_targets=2, max_duration_seconds=SECONDS, motor_noise=False, seed=9)
        venv.reset_tensor(scenario=dict(targets=far))
        a = torch.zeros((N_ENVS, 4), dtype=torch.float64, device=DEV)
        pos = []
        for _ in range(K.max_steps(venv.cfg) + 2):
            venv.step_tensor(a)
            done = bool((venv.terminated | venv.truncated)[0].item())
            pos.append((venv.terminal_obs if done else venv.obs)[0, 10:13].cpu().numpy().copy())
            if done:
                break
        venv.close()
        _PATH["p"] = np.array(pos)
        assert len(pos) == K.max_steps(venv.cfg) + 2, "the zero-action flight must last until the time limit"
    return _PATH["p"]


def _targets_on_the_path():
    """env i mod 4: 0 -- two targets on the path, well apart (two reach steps, env_complete); 1 -- one on the path, one far (one reach,
    then the time limit); 2 -- both far (the time limit, nothing reached); 3 -- two at the very start of the path (a reach on the
    first step).  The positions along the path differ from env to env."""
    p = _zero_action_path()
    tg = np.tile(np.array(FAR), (N_ENVS, 2, 1))
    for i in range(N_ENVS):
        j = i // 4
        if i % 4 == 0:
            tg[i] = [p[8 + 2 * j], p[24 + 5 * j]]
        elif i % 4 == 1:
            tg[i, 0] = p[12 + 3 * j]
        elif i % 4 == 3:
            tg[i] = [p[0], p[3 + j]]
    return tg


@pytest.fixture(params=[1, 8], ids=["lane_per_env", "8_lanes_per_env"])
def lanes(request, monkeypatch):
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", str(request.param))
    return request.param


def test_the_three_evaluation_paths_record_the_same_flights(lanes):
    """evaluate_policy(path_figures=True) with a zero-action policy on targets put on the zero-action path: the step-by-step loop, the
    replayed torch-forward body and -- where fw_collect_step applies (the 8-lane mapping) -- the replayed fused body give the same
    episodes and the same twelve sums to 1e-12; path_figures=False gives today's EvalResult."""
    tg = _targets_on_the_path()
    runs = [dict(use_graph=False), dict(use_graph=True, use_fused=False)]
    out = []
    for kw in runs + [dict(use_graph=True, use_fused=True)]:
        env = _waypoints_env(tg)
        assert env.venv.lanes_per_env == lanes
        pol = _zero_policy(env.obs_dim)
        if kw.get("use_fused") and not evalstep.applies("collect_step", pol, env):
            assert lanes == 1
            with pytest.raises(ValueError, match="use_fused=True"):
                evaluate.evaluate_policy(pol, env, n_eval_episodes=N_ENVS, path_figures=True, **kw)
            env.venv.close()
            continue
        out.append(evaluate.evaluate_policy(pol, env, n_eval_episodes=N_ENVS, deterministic=True, path_figures=True, **kw))
        env.venv.close()
    assert len(out) == (3 if lanes == 8 else 2)
    a = out[0]
    full = K.max_steps(K.waypoints_config(max_duration_seconds=SECONDS)) + 2
    assert len(a.episode_lengths) == N_ENVS == len(a.path_len) == len(a.path_complete)
    sa = _sums(a)
    print("lengths", a.episode_lengths, "\nreached", a.num_targets_reached, "\nfirst / last reach step", sa[:, 7].tolist(), sa[:, 8].tolist())
    assert bool(((sa[:, 7] > 0) & (sa[:, 8] > sa[:, 7])).any()), "an episode with two reach steps"
    assert any(L == full and not ok for L, ok in zip(a.episode_lengths, a.is_success)), "an episode that met the time limit"
    assert bool((sa[:, 7] == 1).any()), "a reach on the first step"
    for b in out[1:]:
        assert b.episode_lengths == a.episode_lengths and b.episode_rewards == a.episode_rewards
        assert b.num_targets_reached == a.num_targets_reached and b.is_success == a.is_success and b.path_complete == a.path_complete
        np.testing.assert_allclose(_sums(b), sa, rtol=1e-12, atol=0)
        assert a.path_scalars(30.0) == pytest.approx(b.path_scalars(30.0), rel=1e-12, abs=0)
    sc = a.path_scalars(30.0)
    assert set(sc) == {"eval/" + k for k in evaluate.PATH_SCALARS}
    assert 0 < sc["eval/path_efficiency"] <= 1 + 1e-12 and 15 < sc["eval/airspeed_mean"] < 25 and 5 < sc["eval/altitude_min"] < 11
    assert sc["eval/action_delta_mean"] == 0.0 and sc["eval/miss_distance_mean"] > 10
    # a straight flight: what was flown between the reaches is (almost) the chord
    two = (sa[:, 8] > sa[:, 7]) & (sa[:, 7] > 0)
    assert bool((sa[two, 9] <= sa[two, 10] * (1 + 1e-12)).all()) and bool((sa[two, 9] > 0.99 * sa[two, 10]).all())
    # off: the EvalResult of today, from the launches of today
    for kw in runs + ([dict(use_graph=True, use_fused=True)] if lanes == 8 else []):
        env = _waypoints_env(tg)
        r = evaluate.evaluate_policy(_zero_policy(env.obs_dim), env, n_eval_episodes=N_ENVS, deterministic=True, **kw)
        env.venv.close()
        assert r.episode_lengths == a.episode_lengths and r.episode_rewards == a.episode_rewards
        assert r.num_targets_reached == a.num_targets_reached and r.is_success == a.is_success
        assert r.path_len == [] and r.miss_dist == [] and r.path_complete == [] and r.path_scalars(30.0) == {}


def test_flight_record_and_evaluation_agree(lanes):
    """two kernels, one flight: path_figures(trace) of each env's first episode equals that episode's fw_eval_track_wp sums from the
    same seed; graphs of 8 steps and no graphs record the same trace bit for bit."""
    tg = _targets_on_the_path()
    fused = lanes == 8
    env = _waypoints_env(tg)
    pol = _zero_policy(env.obs_dim)
    job = evaluate.ReplayedEvaluation(pol, env, np.ones(N_ENVS, dtype=np.int64), use_fused=fused, path_figures=True)
    job.run(None)
    fin_path, fin_len = job.fin_path[:, 0].cpu().numpy(), job.fin_len[:, 0].cpu().numpy()
    env.venv.close()
    T = K.max_steps(env.venv.cfg) + 4
    env = _waypoints_env(tg)
    tr = flight.fly(pol, env, T, use_fused=fused, graph_steps=8)
    env.venv.close()
    D = env.obs_dim
    assert tr.trace.shape == (T, N_ENVS, D + 2) and tr.start.shape == (N_ENVS, D + 2) and tr.dt == pytest.approx(1.0 / 30.0)
    assert (tr.ended_at >= 0).all() and tr.layout == RowLayout(D, 13, 4)
    np.testing.assert_array_equal(tr.ended_at + 1, fin_len)
    figs = flight.path_figures(tr)
    assert set(figs) == set(range(N_ENVS))
    for i in range(N_ENVS):
        np.testing.assert_allclose(figs[i], fin_path[i], rtol=1e-12, atol=0, err_msg=str(i))
        ep = tr.episode(i)
        assert (tr.flag(ep)[:-1] == 0).all() and tr.flag(ep)[-1] in (1, 2)
        assert tr.targets_reached(ep)[-1] == (2 if i % 4 in (0, 3) else 1 if i % 4 == 1 else 0), i
    assert (tr.flag(tr.start) == 0).all() and (tr.targets_reached(tr.start) == 0).all()
    p0 = tr.position(tr.start)                                               # the start pose behind the env's warm-up ticks: the same for all
    assert (p0 == p0[0]).all() and 0.0 < p0[0, 0] < 3.0 and p0[0, 1] == 0.0 and abs(p0[0, 2] - 10.0) < 0.01
    env = _waypoints_env(tg)
    eager = flight.fly(pol, env, T, use_fused=fused, graph_steps=0)
    env.venv.close()
    np.testing.assert_array_equal(eager.trace, tr.trace)
    np.testing.assert_array_equal(eager.start, tr.start)
    np.testing.assert_array_equal(eager.ended_at, tr.ended_at)


def test_flight_record_of_a_quaternion_and_of_an_objlock_env():
    """what the accessors return is what the env holds: positions match get_state() at the last step, target_distance() is the
    distance to the current waypoint (quaternion rows, f64) and the norm of target_vector (ObjLock, float32 rows, 8 envs)"""
    T = 6
    # waypoints, quaternion attitude
    env = _waypoints_env(None)
    tr = flight.fly(_zero_policy(env.obs_dim), env, T, graph_steps=4)
    st = env.venv.get_state()
    assert (tr.flag() == 0).all() and (tr.ended_at == -1).all() and tr.layout.quaternion
    np.testing.assert_allclose(tr.position()[-1], st[:, K.S_POS:K.S_POS + 3], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(tr.target_distance()[-1], np.linalg.norm(st[:, K.S_TARGETS:K.S_TARGETS + 3] - st[:, K.S_POS:K.S_POS + 3], axis=1),
                               rtol=1e-9, atol=1e-9)
    eul = tr.attitude_euler()
    assert eul.shape == (T, N_ENVS, 3) and np.abs(eul[-1, :, 0]).max() < 0.5 and np.abs(eul[-1, :, 2]).max() < 0.5
    np.testing.assert_allclose(tr.airspeed()[0], 20.0, atol=1.0)
    env.venv.close()
    # ObjLock: float32 rows.  (The env starts at [0, 0, 100]: under the constructor's 100 m dome every step would end out of bounds,
    # so the dome is the training configuration's 200 m.)
    venv = FixedwingObjLockVecEnv(8, dtype="float32", motor_noise=False, seed=4, angle_representation="euler", flight_dome_size=200.0)
    env = R.VecNormalizeDevice(venv, training=False, norm_reward=False)
    assert venv.obs.dtype == torch.float32 and env.obs_dim == 56
    tr = flight.fly(_zero_policy(56), env, T, graph_steps=4)
    assert tr.trace.shape == (T, 8, 58) and (tr.flag() == 0).all() and tr.layout == RowLayout(56, 12, 4)
    last = venv.obs.double().cpu().numpy()
    np.testing.assert_array_equal(tr.trace[-1, :, :56], last)                 # the float32 row, widened
    np.testing.assert_array_equal(tr.target_distance()[-1], np.linalg.norm(last[:, 22:25], axis=1))
    np.testing.assert_allclose(tr.position()[-1], venv.get_state()[:, K.S_POS:K.S_POS + 3], rtol=0, atol=1e-4)      # (float32 rows of ~100 m)
    assert (tr.targets_reached() == 0).all() and (tr.throttle() >= 0).all()
    venv.close()


def test_async_evaluation_and_eval_callback_carry_the_path_figures(tmp_path):
    tg = _targets_on_the_path()
    env = _waypoints_env(tg)
    pol = _zero_policy(env.obs_dim)
    sync = evaluate.evaluate_policy(pol, env, n_eval_episodes=N_ENVS, deterministic=True, path_figures=True)
    env.venv.close()
    env = _waypoints_env(tg)
    job = evaluate.start_evaluation(pol, env, n_eval_episodes=N_ENVS, path_figures=True)
    r = job.result()
    env.venv.close()
    assert r.episode_lengths == sync.episode_lengths and r.episode_rewards == sync.episode_rewards
    np.testing.assert_array_equal(_sums(r), _sums(sync))
    keys = {"eval/" + k for k in evaluate.PATH_SCALARS}
    assert set(r.path_scalars(30.0)) == keys

    train = R.VecNormalizeDevice(FixedwingWaypointsVecEnv(N_ENVS, num_targets=2, max_duration_seconds=SECONDS, seed=1), norm_obs=True,
                                 norm_reward=True, clip_obs=10.0, gamma=0.99)
    ppo = R.PPO(train, R.PPOConfig(n_steps=32, batch_size=256, n_epochs=1, seed=1))
    eval_env = _waypoints_env(tg, seed=2)
    ev = evaluate.EvalCallback(eval_env, n_eval_episodes=N_ENVS, eval_freq=32, log_path=str(tmp_path / "logs"), num_targets_total=2,
                               path_figures=True)
    ppo.learn(2 * 32 * N_ENVS, callbacks=[ev])
    assert ev.n_evals == 2
    always = {"eval/airspeed_mean", "eval/altitude_mean", "eval/ang_vel_mean", "eval/throttle_mean", "eval/action_delta_mean",
              "eval/path_length_mean", "eval/altitude_min"}
    assert always <= set(ev.last_scalars) and {"eval/mean_reward", "eval/mean_ep_length", "eval/wp1_reach_rate"} <= set(ev.last_scalars)
    z = np.load(os.path.join(tmp_path, "logs", "evaluations.npz"), allow_pickle=True)
    for name in evaluate.PATH_SCALARS:
        assert z[name].shape == (2,), name
        k = "eval/" + name
        assert (math.isnan(z[name][-1]) and k not in ev.last_scalars) or z[name][-1] == pytest.approx(ev.last_scalars[k])
    train.venv.close(); eval_env.venv.close()
