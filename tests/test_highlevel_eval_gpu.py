"""The high-level command task's evaluation on the GPU (DESIGN.md section 2e "Evaluation"): fw_eval_track_hl and fw_trace_hl against
their torch statements on synthetic buffers, the three evaluation paths -- the step-by-step loop (torch ops), the replayed loop
(fw_eval_track_hl) and the fused three-action loop (fw_collect_act_hl -> fw_step -> fw_eval_track_hl) -- against each other, what the
command figures mean, the flight record against the evaluation, and the asynchronous and EvalCallback forms."""
import math
import os

import numpy as np
import pytest
import torch

from pyflyt_drone_amd import _lib, evaluate, highlevel
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R
from pyflyt_drone_amd.highlevel import HighLevelCmdVecEnv

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALT_HIGH, SPEED_HIGH = 200.0, 30.0
# (controller, max_duration_seconds): the random controller (actions over the whole of [-1, 1]) flies most planes into the ground
# inside 4 s; the one with zeroed action weights (every surface near 0, throttle near 0.5) flies on until the truncation at 2 s
FLIGHTS = {"random": 4.0, "zeroed": 2.0}


def _full_length(env):
    """the length of a truncated episode: the base env truncates once its step count exceeds max_steps = 30 Hz x duration, which an
    episode's step max_steps + 2 is the first to see (start_evaluation bounds an episode by the same figure)"""
    return K.max_steps(env.venv.cfg) + 2


def _controller(seed=21, zeroed=False):
    """a controller with random (seeded) weights whose actions use the whole of [-1, 1], and non-trivial statistics"""
    torch.manual_seed(seed)
    p = R.MlpPolicy(21, 6)
    with torch.no_grad():
        for q in p.parameters():
            q.add_(0.1 * torch.randn_like(q))
        p.action_net.weight.mul_(1.5)
        if zeroed:
            p.action_net.weight.zero_()
    g = np.random.default_rng(seed)
    mean = g.normal(0.0, 1.0, 21) * np.array([1] * 6 + [10] * 6 + [0.3] * 6 + [1, 50, 10], dtype=np.float64)
    var = g.uniform(0.2, 4.0, 21) * np.array([1] * 6 + [100] * 6 + [0.1] * 6 + [3, 2500, 80], dtype=np.float64)
    return p, mean, var


def _commander(seed=31, bias=(0.0, 100.0, 15.0), constant=False, gain=(1.0, 1.0, 1.0)):
    """a three-action policy whose mean sits inside the Box; gain scales the rows of its head (how far each command moves)"""
    torch.manual_seed(seed)
    p = R.MlpPolicy(30, 3).cuda()
    with torch.no_grad():
        for q in p.parameters():
            q.add_(0.1 * torch.randn_like(q))
        p.action_net.weight.mul_(torch.tensor(gain, device=p.action_net.weight.device)[:, None])
        if constant:
            p.action_net.weight.zero_()
        p.action_net.bias.copy_(torch.tensor(bias))
    return p


def _env(n, kind="random", seed=9, dtype="float64", seconds=None, identity=True):
    pol, mean, var = _controller(zeroed=(kind == "zeroed"))
    venv = HighLevelCmdVecEnv(n, pol, (mean, var), max_duration_seconds=FLIGHTS[kind] if seconds is None else seconds, seed=seed, dtype=dtype)
    env = R.VecNormalizeDevice(venv, training=False, norm_reward=False)
    if not identity:                                               # statistics as after some training
        with torch.no_grad():
            env.obs_rms.mean.copy_(torch.linspace(-0.2, 0.3, env.obs_dim, dtype=torch.float64, device=DEV))
            env.obs_rms.var.copy_(torch.linspace(0.5, 2.0, env.obs_dim, dtype=torch.float64, device=DEV))
    return env


def _targets(n_episodes, n):
    return np.array([(n_episodes + i) // n for i in range(n)])


def _sums(r):
    return np.array([getattr(r, k) for k in evaluate.HL_TRACK_SUMS]).T        # [episodes, 11]


def _p(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------------------------------------------------------ the kernels alone
def _synthetic_step(g, n, td):
    """one vec-step's worth of random env outputs; commands on and off the Box bounds; both ways of ending and both at once"""
    obs = (torch.randn((n, 30), generator=g, dtype=torch.float64) * 4).to(td)
    tobs = (torch.randn((n, 30), generator=g, dtype=torch.float64) * 4).to(td)
    cmd = torch.stack([torch.rand(n, generator=g, dtype=torch.float64) * 2 * math.pi - math.pi,
                       torch.rand(n, generator=g, dtype=torch.float64) * ALT_HIGH,
                       torch.rand(n, generator=g, dtype=torch.float64) * SPEED_HIGH], dim=1)
    pick = torch.randint(0, 8, (n,), generator=g)
    cmd[pick == 0, 1], cmd[pick == 1, 1], cmd[pick == 2, 2], cmd[pick == 3, 2] = 0.0, ALT_HIGH, 0.0, SPEED_HIGH
    cmd = cmd.to(td)
    term = (torch.rand(n, generator=g) < 0.25).to(torch.uint8)
    trunc = (torch.rand(n, generator=g) < 0.2).to(torch.uint8)
    info = torch.randint(0, 5, (n, 4), generator=g, dtype=torch.int32)
    rew = (torch.randn(n, generator=g, dtype=torch.float64) * 20).to(td)
    return obs, tobs, cmd, term, trunc, info, rew


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_fw_eval_track_hl_against_its_torch_statement(dtype):
    """six steps on random buffers, N = 300 (the 256 threads stride), E = 2, uneven targets that some envs outrun: the kernel against
    evaluate._track_terms_hl plus a host loop.  Sums to 1e-12, everything else equal, prev_cmd bit for bit."""
    L, n, E = _lib.lib(), 300, 2
    g = torch.Generator().manual_seed(17)
    tg = torch.randint(1, 3, (n,), generator=g, dtype=torch.int64)
    assert set(tg.tolist()) == {1, 2}
    # host state
    counts, cur_len, cur_rew = torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.float64)
    cur_trk, prev = torch.zeros((n, 11), dtype=torch.float64), torch.zeros((n, 3), dtype=torch.float64)
    fin_rew, fin_len, fin_step = torch.zeros((n, E), dtype=torch.float64), torch.zeros((n, E), dtype=torch.int64), torch.zeros((n, E), dtype=torch.int64)
    fin_info, fin_trk = torch.zeros((n, E, 4), dtype=torch.int32), torch.zeros((n, E, 11), dtype=torch.float64)
    # device state
    d = {k: v.clone().to(DEV) for k, v in dict(tg=tg, counts=counts, cur_len=cur_len, cur_rew=cur_rew, cur_trk=cur_trk, prev=prev, fin_rew=fin_rew,
                                               fin_len=fin_len, fin_step=fin_step, fin_info=fin_info, fin_trk=fin_trk).items()}
    ctr = torch.zeros((), dtype=torch.int64, device=DEV)
    ar = torch.arange(n)
    outran = torch.zeros(n, dtype=torch.bool)
    for step in range(1, 7):
        obs, tobs, cmd, term, trunc, info, rew = _synthetic_step(g, n, dtype)
        dv = [x.to(DEV) for x in (obs, tobs, cmd, term, trunc, info, rew)]
        rc = L.fw_eval_track_hl(_p(dv[6]), int(dtype == torch.float64), _p(dv[3]), _p(dv[4]), _p(dv[5]), 4, _p(dv[0]), _p(dv[1]), _p(dv[2]),
                                int(dtype == torch.float64), 30, ALT_HIGH, SPEED_HIGH, _p(d["tg"]), _p(d["counts"]), _p(d["cur_rew"]),
                                _p(d["cur_len"]), _p(ctr), _p(d["cur_trk"]), _p(d["prev"]), _p(d["fin_rew"]), _p(d["fin_len"]),
                                _p(d["fin_step"]), _p(d["fin_info"]), _p(d["fin_trk"]), n, E, None)
        assert rc == K.FW_OK, L.fw_last_error(None)
        torch.cuda.synchronize()
        done = (term | trunc).bool()
        cur_trk = cur_trk + evaluate._track_terms_hl(torch.where(done[:, None], tobs, obs), cmd, prev, cur_len == 0, ALT_HIGH, SPEED_HIGH)
        prev = cmd.to(torch.float64)
        cur_rew = cur_rew + rew.to(torch.float64)
        cur_len = cur_len + 1
        take = done & (counts < tg)
        outran |= done & (counts >= tg)
        slot = counts.clamp(max=E - 1)
        for i in ar[take].tolist():
            s = int(slot[i])
            fin_rew[i, s], fin_len[i, s], fin_step[i, s], fin_info[i, s], fin_trk[i, s] = cur_rew[i], cur_len[i], step, info[i], cur_trk[i]
        counts = counts + take.to(torch.int64)
        cur_rew[done], cur_len[done], cur_trk[done] = 0.0, 0, 0.0
        # after every step: the running state
        assert int(ctr.item()) == step
        assert torch.equal(d["counts"].cpu(), counts) and torch.equal(d["cur_len"].cpu(), cur_len)
        assert torch.equal(d["prev"].cpu().view(torch.int64), prev.view(torch.int64))
        torch.testing.assert_close(d["cur_trk"].cpu(), cur_trk, rtol=1e-12, atol=0)
        torch.testing.assert_close(d["cur_rew"].cpu(), cur_rew, rtol=1e-12, atol=0)
    assert bool(outran.any()) and bool((counts <= tg).all()) and bool((counts == tg).any())      # some envs finished more episodes than wanted
    assert torch.equal(d["fin_len"].cpu(), fin_len) and torch.equal(d["fin_step"].cpu(), fin_step) and torch.equal(d["fin_info"].cpu(), fin_info)
    torch.testing.assert_close(d["fin_rew"].cpu(), fin_rew, rtol=1e-12, atol=0)
    torch.testing.assert_close(d["fin_trk"].cpu(), fin_trk, rtol=1e-12, atol=0)
    assert float(fin_trk[:, :, 7:10].sum()) > 0 and float(fin_trk[:, :, 10].sum()) > 0
    assert bool((fin_len == 1).any())                                    # one-step episodes: their command changes are exactly 0
    assert float(d["fin_trk"].cpu()[:, :, 7:10][fin_len == 1].abs().sum()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_fw_trace_hl_against_its_torch_statement(dtype):
    """N = 1100 (the 1024 threads stride), T = 4: four rows against highlevel.trace_rows_hl, then two calls past the end of the trace"""
    L, n, T = _lib.lib(), 1100, 4
    g = torch.Generator().manual_seed(23)
    trace = torch.full((T, n, 11), -7.0, dtype=torch.float64, device=DEV)
    idx = torch.zeros((), dtype=torch.int64, device=DEV)
    keep = None
    for k in range(T + 2):
        obs, tobs, cmd, term, trunc, info, _ = _synthetic_step(g, n, dtype)
        dv = [x.to(DEV) for x in (obs, tobs, cmd, term, trunc, info)]
        rc = L.fw_trace_hl(_p(dv[0]), _p(dv[1]), _p(dv[3]), _p(dv[4]), _p(dv[2]), _p(dv[5]), 4, int(dtype == torch.float64), n, _p(trace), T,
                           _p(idx), None)
        assert rc == K.FW_OK, L.fw_last_error(None)
        torch.cuda.synchronize()
        assert int(idx.item()) == k + 1
        if k < T:
            done = (term | trunc).bool()
            flag = torch.where(term.bool(), 1, torch.where(trunc.bool(), 2, 0))
            want = highlevel.trace_rows_hl(torch.where(done[:, None], tobs, obs), cmd, info, flag)
            got = trace[k].cpu()
            assert set(flag.tolist()) == {0, 1, 2}
            for col in (0, 1, 2, 3, 4, 7, 8, 9, 10):                      # copied values: bit for bit
                assert torch.equal(got[:, col], want[:, col]), col
            torch.testing.assert_close(got, want, rtol=1e-12, atol=0)
            if k + 1 < T:
                assert bool((trace[k + 1:] == -7.0).all())
        if k == T - 1:
            keep = trace.clone()
    assert torch.equal(trace, keep)                                      # the calls behind row T - 1 wrote nothing
    # without info and without done flags: zeros in their columns, the live observation
    idx.zero_()
    rc = L.fw_trace_hl(_p(dv[0]), None, None, None, _p(dv[2]), None, 0, int(dtype == torch.float64), n, _p(trace), T, _p(idx), None)
    assert rc == K.FW_OK
    torch.cuda.synchronize()
    torch.testing.assert_close(trace[0].cpu(), highlevel.trace_rows_hl(obs, cmd), rtol=1e-12, atol=0)


def test_fw_eval_track_hl_and_fw_trace_hl_reject_bad_arguments():
    L = _lib.lib()
    n, E = 8, 2
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)          # noqa: E731
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64, device=DEV)            # noqa: E731
    u8 = torch.zeros(n, dtype=torch.uint8, device=DEV)
    rew, obs, tobs, cmd, prev = f64(n), f64(n, 30), f64(n, 30), f64(n, 3), f64(n, 3)
    tg, cnt, cl, ctr, fl, fs = i64(n), i64(n), i64(n), i64(1), i64(n, E), i64(n, E)
    cr, ct, fr, ft = f64(n), f64(n, 11), f64(n, E), f64(n, E, 11)

    def call(obs_dim=30, N=n, E_=E, cmd_=cmd, ct_=ct, prev_=prev):
        return L.fw_eval_track_hl(_p(rew), 1, _p(u8), _p(u8), None, 0, _p(obs), _p(tobs), _p(cmd_), 1, obs_dim, ALT_HIGH, SPEED_HIGH, _p(tg),
                                  _p(cnt), _p(cr), _p(cl), _p(ctr), _p(ct_), _p(prev_), _p(fr), _p(fl), _p(fs), None, _p(ft), N, E_, None)

    def err():
        return L.fw_last_error(None).decode()
    assert call(obs_dim=29) == K.FW_EINVAL and "obs_dim must be 30" in err()
    assert call(cmd_=None) == K.FW_EINVAL and "command" in err()
    assert call(prev_=None) == K.FW_EINVAL and "prev_cmd" in err()
    assert call(ct_=None) == K.FW_EINVAL and "cur_track" in err()
    assert call(N=0) == K.FW_EINVAL and "N" in err() and "fw_eval_track_hl" in err()
    assert call(E_=0) == K.FW_EINVAL and "E" in err()
    with pytest.raises(ValueError, match="fw_eval_track_hl"):
        _lib.check(K.FW_EINVAL)
    assert call() == K.FW_OK                                  # the same buffers, well formed: one launch
    torch.cuda.synchronize()
    assert int(ctr.item()) == 1 and torch.equal(cl, torch.ones_like(cl))
    # fw_trace_hl
    trace, idx = f64(2, n, 11), i64(1)
    assert L.fw_trace_hl(_p(obs), None, None, None, None, None, 0, 1, n, _p(trace), 2, _p(idx), None) == K.FW_EINVAL and "command" in err()
    assert L.fw_trace_hl(_p(obs), None, None, None, _p(cmd), None, 0, 1, 0, _p(trace), 2, _p(idx), None) == K.FW_EINVAL and "N and T" in err()
    assert L.fw_trace_hl(_p(obs), None, None, None, _p(cmd), None, 0, 1, n, _p(trace), 0, _p(idx), None) == K.FW_EINVAL
    assert L.fw_trace_hl(_p(obs), None, None, None, _p(cmd), _p(tg), 0, 1, n, _p(trace), 2, _p(idx), None) == K.FW_EINVAL and "info_dim" in err()
    assert L.fw_trace_hl(_p(obs), None, None, None, _p(cmd), None, 0, 1, n, _p(trace), 2, _p(idx), None) == K.FW_OK
    torch.cuda.synchronize()
    assert int(idx.item()) == 1


# ------------------------------------------------------------------------------------------------------------------ the evaluation paths
def test_replayed_bookkeeping_kernel_matches_the_host_loop():
    """the step-by-step loop (torch ops, _track_terms_hl) against the replayed loop (fw_eval_track_hl), both with the torch forward: the
    same episodes in the same order, lengths, rewards and info equal, the eleven sums to 1e-12 -- with envs that finish several
    episodes, an uneven split, and truncated as well as terminated episodes."""
    ended = set()
    for kind in FLIGHTS:
        out = []
        for kw in (dict(use_graph=False), dict(use_graph=True, use_fused=False)):
            env = _env(24, kind)
            steps = _full_length(env)
            out.append(evaluate.evaluate_policy(_commander(), env, n_eval_episodes=61, deterministic=True, **kw))
            env.venv.close()
        a, b = out
        assert len(a.episode_lengths) == 61 == len(b.episode_lengths) == len(a.saturated) == len(b.saturated)
        assert a.episode_lengths == b.episode_lengths and a.episode_rewards == b.episode_rewards
        assert a.num_targets_reached == b.num_targets_reached and a.is_success == b.is_success
        assert a.survived == [] == b.survived and a.tracking_scalars() == {} == b.tracking_scalars()
        assert a.rejected_actions == 0 == b.rejected_actions
        np.testing.assert_allclose(_sums(b), _sums(a), rtol=1e-12, atol=0)
        assert a.command_scalars() == pytest.approx(b.command_scalars(), rel=1e-12, abs=1e-12)
        assert max(a.episode_lengths) <= steps
        ended |= {L == steps for L in a.episode_lengths}
        sc = a.command_scalars()
        for q in ("heading", "altitude", "airspeed"):
            assert sc[f"eval/cmd_{q}_rmse"] >= sc[f"eval/cmd_{q}_mae"] > 0 and sc[f"eval/cmd_{q}_delta"] > 0
    assert ended == {True, False}                            # truncations (full length) and terminations both compared


@pytest.fixture(params=[1, 8], ids=["lane_per_env", "8_lanes_per_env"])
def lanes(request, monkeypatch):
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", str(request.param))
    return request.param


def test_fused_three_action_evaluation_flies_the_episodes_of_the_torch_evaluation(lanes):
    """use_fused=True with the three-action policy: fw_collect_act_hl (fp32 MFMA forward) -> fw_step -> fw_eval_track_hl.  Same episodes
    as the torch path: same number and order, lengths equal but for a knife-edge ending (at most 3 of 61, the six-action test's cap),
    rewards and sums to ~1e-4.  use_fused=None keeps the torch path for three actions.
    The head's altitude row is scaled by 10: the altitude command is ~100 m, so the two forwards differ by ~1e-5 m in it (fp32), and
    the sum of its step-to-step changes is held to rtol 1e-4 only if a change is well above that -- ~0.4 m per step with the gain,
    ~0.04 m without (where the sums differed by 1.02e-4).  Heading and airspeed commands are of the size of their changes.
    Observed on one MI355X: 0 of the 61 lengths differ, on either lane mapping."""
    out = []
    for fused in (None, True):
        env = _env(24, "random", identity=False)
        assert env.venv.lanes_per_env == lanes
        job = evaluate.ReplayedEvaluation(_commander(gain=(1.0, 10.0, 1.0)), env, _targets(61, 24), use_fused=fused)
        assert job.fused == bool(fused) and job.step.kind == ("act_hl" if fused else "torch")
        out.append(job.run(None))
        env.venv.close()
    a, b = out
    assert len(a.episode_lengths) == 61 == len(b.episode_lengths)
    same = [x == y for x, y in zip(a.episode_lengths, b.episode_lengths)]
    print("episodes whose length differs between the fused and the torch forward:", 61 - sum(same))
    assert sum(same) >= 58, (a.episode_lengths, b.episode_lengths)      # observed: 61 of 61 the same
    sa, sb = _sums(a), _sums(b)
    for k, ok in enumerate(same):
        if ok:
            assert b.episode_rewards[k] == pytest.approx(a.episode_rewards[k], rel=1e-4, abs=1e-4), k
            np.testing.assert_allclose(sb[k], sa[k], rtol=1e-4, atol=1e-6, err_msg=str(k))
    assert a.rejected_actions == 0 == b.rejected_actions


def test_use_fused_names_the_three_action_case_when_it_cannot_apply():
    env = _env(8, "zeroed")
    env.training = True                                                   # not an evaluation normaliser
    with pytest.raises(ValueError, match="three actions"):
        evaluate.ReplayedEvaluation(_commander(), env, _targets(8, 8), use_fused=True)
    env.venv.close()


# ------------------------------------------------------------------------------------------------------------------ what the figures mean
@pytest.mark.parametrize("fused", [False, True], ids=["torch_forward", "fused"])
def test_command_figures_of_constant_saturated_and_rejected_commanders(fused):
    n = 8
    # a constant command inside the Box: no change from step to step, never on a bound
    env = _env(n, "zeroed")
    steps = _full_length(env)
    pol = _commander(bias=(0.5, 100.0, 15.0), constant=True)
    r = evaluate.ReplayedEvaluation(pol, env, _targets(12, n), use_fused=fused).run(None)
    assert len(r.episode_lengths) == 12 and min(r.episode_lengths) > 1
    assert r.dcmd_heading == [0.0] * 12 and r.dcmd_altitude == [0.0] * 12 and r.dcmd_airspeed == [0.0] * 12 and r.saturated == [0.0] * 12
    sc = r.command_scalars()
    assert sc["eval/cmd_saturation_rate"] == 0.0 and sc["eval/cmd_heading_delta"] == 0.0 and sc["eval/rejected_actions"] == 0
    tr = highlevel.fly(pol, env, 24, use_fused=fused)
    for col, v in ((0, 0.5), (2, 100.0), (4, 15.0)):                      # (the heading went through the wrap: 0.5 to rounding)
        assert (tr.trace[:, :, col] == tr.trace[0, 0, col]).all() and tr.trace[0, 0, col] == pytest.approx(v, abs=1e-12), col
    env.venv.close()
    # an altitude command above the dome clips to it: every step is saturated
    env = _env(n, "zeroed")
    r = evaluate.ReplayedEvaluation(_commander(bias=(0.5, 500.0, 15.0), constant=True), env, _targets(12, n), use_fused=fused).run(None)
    assert r.saturated == [float(L) for L in r.episode_lengths] and r.command_scalars()["eval/cmd_saturation_rate"] == 1.0
    assert r.dcmd_altitude == [0.0] * 12
    env.venv.close()
    # a NaN head bias: every action of every env-step is rejected, and the flight goes on under the command the env holds
    env = _env(n, "zeroed")
    job = evaluate.ReplayedEvaluation(_commander(bias=(0.5, float("nan"), 15.0), constant=True), env, _targets(12, n), use_fused=fused)
    r = job.run(None)
    assert r.rejected_actions == n * job.steps and r.command_scalars()["eval/rejected_actions"] == n * job.steps
    assert len(r.episode_lengths) == 12 and max(r.episode_lengths) == steps and all(math.isfinite(x) for x in r.episode_rewards)
    assert r.dcmd_heading == [0.0] * 12 and r.dcmd_altitude == [0.0] * 12 and r.dcmd_airspeed == [0.0] * 12
    cmd = env.venv.command.double().cpu().numpy()
    np.testing.assert_array_equal(cmd, env.venv.get_state()[:, K.S_TASK:K.S_TASK + 3])      # the stored command, finite
    assert np.isfinite(cmd).all() and (cmd[:, 0] == 0.0).all()
    env.venv.close()


def test_flight_record_and_evaluation_agree():
    """two kernels, one flight: each env's first episode summed from its fw_trace_hl rows (rebuilt in numpy from the trace columns)
    equals that episode's fw_eval_track_hl sums, both on the fused act path, from the same seed; graphs of 8 steps and of 1 step
    record the same trace bit for bit."""
    n, T = 24, 130                                                         # 4 s: 122 steps at the most, every first episode ends inside the trace
    env = _env(n, "random", identity=False)
    pol = _commander()
    job = evaluate.ReplayedEvaluation(pol, env, _targets(n, n), use_fused=True)
    job.run(None)
    fin_trk, fin_len = job.fin_track[:, 0].cpu().numpy(), job.fin_len[:, 0].cpu().numpy()
    env.venv.close()
    env = _env(n, "random", identity=False)
    tr = highlevel.fly(pol, env, T, use_fused=True, graph_steps=8)
    env.venv.close()
    assert tr.trace.shape == (T, n, 11) and tr.start.shape == (n, 11) and tr.dt == pytest.approx(1.0 / 30.0)
    assert (tr.ended_at >= 0).all()
    np.testing.assert_array_equal(tr.ended_at + 1, fin_len)
    wrap = lambda a: np.remainder(a + math.pi, 2 * math.pi) - math.pi      # noqa: E731
    for i in range(n):
        rows = tr.trace[:tr.ended_at[i] + 1, i]
        assert (rows[:-1, 10] == 0).all() and rows[-1, 10] in (1.0, 2.0)
        c = rows[:, [0, 2, 4]]
        e_psi, e_h, e_v = wrap(c[:, 0] - rows[:, 1]), c[:, 1] - rows[:, 3], c[:, 2] - rows[:, 5]
        dc = np.diff(c, axis=0)
        sat = (c[:, 1] <= 0) | (c[:, 1] >= ALT_HIGH) | (c[:, 2] <= 0) | (c[:, 2] >= SPEED_HIGH)
        want = [np.abs(e_psi).sum(), (e_psi * e_psi).sum(), np.abs(e_h).sum(), (e_h * e_h).sum(), np.abs(e_v).sum(), (e_v * e_v).sum(),
                rows[:, 6].sum(), np.abs(wrap(dc[:, 0])).sum(), np.abs(dc[:, 1]).sum(), np.abs(dc[:, 2]).sum(), float(sat.sum())]
        np.testing.assert_allclose(fin_trk[i], want, rtol=1e-12, atol=0, err_msg=str(i))
    # the rows after reset: the observation the first act saw, under the command the env held then
    assert (tr.start[:, 0] == 0.0).all() and (tr.start[:, 10] == 0).all() and (tr.start[:, 9] == 0).all()
    env = _env(n, "random", identity=False)
    one = highlevel.fly(pol, env, T, use_fused=True, graph_steps=1)
    env.venv.close()
    np.testing.assert_array_equal(one.trace, tr.trace)
    np.testing.assert_array_equal(one.start, tr.start)
    np.testing.assert_array_equal(one.ended_at, tr.ended_at)


def test_async_evaluation_and_eval_callback_carry_the_command_figures(tmp_path):
    pol = _commander()
    env = _env(16, "zeroed", seed=4)
    sync = evaluate.evaluate_policy(pol, env, n_eval_episodes=20, deterministic=True, use_fused=True)
    env.venv.close()
    env = _env(16, "zeroed", seed=4)
    job = evaluate.start_evaluation(pol, env, n_eval_episodes=20, use_fused=True)
    assert job.step.kind == "act_hl"
    r = job.result()
    env.venv.close()
    assert r.episode_lengths == sync.episode_lengths and r.episode_rewards == sync.episode_rewards
    np.testing.assert_array_equal(_sums(r), _sums(sync))
    keys = {"eval/cmd_heading_mae", "eval/cmd_heading_rmse", "eval/cmd_altitude_mae", "eval/cmd_altitude_rmse", "eval/cmd_airspeed_mae",
            "eval/cmd_airspeed_rmse", "eval/ang_vel_mean", "eval/cmd_heading_delta", "eval/cmd_altitude_delta", "eval/cmd_airspeed_delta",
            "eval/cmd_saturation_rate", "eval/rejected_actions"}
    assert set(r.command_scalars()) == keys

    ctl, mean, var = _controller()
    train = R.VecNormalizeDevice(HighLevelCmdVecEnv(16, ctl, (mean, var), seed=1), norm_obs=True, norm_reward=True, clip_obs=10.0, gamma=0.995)
    ppo = R.PPO(train, R.PPOConfig(n_steps=32, batch_size=256, n_epochs=1, gamma=0.995, seed=1, fused_three_actions=True))
    eval_env = _env(8, "zeroed", seed=2)
    ev = evaluate.EvalCallback(eval_env, n_eval_episodes=8, eval_freq=32, log_path=str(tmp_path / "logs"), use_fused=True)
    ppo.learn(2 * 32 * 16, callbacks=[ev])
    assert ev.n_evals == 2
    assert keys <= set(ev.last_scalars) and {"eval/mean_reward", "eval/mean_ep_length"} <= set(ev.last_scalars)
    z = np.load(os.path.join(tmp_path, "logs", "evaluations.npz"), allow_pickle=True)
    for k in keys:
        name = k.split("/", 1)[1]
        assert z[name].shape == (2,), name
        assert z[name][-1] == pytest.approx(ev.last_scalars[k])
    train.venv.close(); eval_env.venv.close()
