"""The low-level controller's evaluation on the GPU: tracking sums and survival on the three evaluation paths
-- the step-by-step loop (torch ops), the replayed loop (fw_eval_track_ll) and the fused six-action loop (fw_collect_act_a ->
fw_step -> fw_eval_track_ll) -- against the env's own reward, against each other, asynchronously and through EvalCallback."""
import os

import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib, evaluate
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R

pytestmark = pytest.mark.gpu

PATHS = {"host_loop": dict(use_graph=False), "replayed": dict(use_graph=True, use_fused=False),
         "fused": dict(use_graph=True, use_fused=True)}
# (policy, max_episode_steps): saturated actions that depend on the per-env target crash most planes within ~200 steps; zeroed
# action weights (every command 0, throttle 0.5) fly on until the truncation
POLICIES = {"saturated": 200, "zeroed": 60}


def _env(n, steps, seed=9, dtype="float64"):
    venv = P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=steps, dtype=dtype), n, seed=seed)
    return R.VecNormalizeDevice(venv, training=False, norm_reward=False)


def _policy(env, kind):
    torch.manual_seed(0)
    pol = R.MlpPolicy(env.obs_dim, env.act_dim).cuda()
    with torch.no_grad():
        if kind == "zeroed":
            pol.action_net.weight.zero_()
        else:
            pol.action_net.weight.mul_(300.0)
    return pol


def _targets(n_episodes, n):
    return np.array([(n_episodes + i) // n for i in range(n)])


def _sums(r):
    return np.array([getattr(r, k) for k in evaluate.TRACK_SUMS]).T        # [episodes, 7]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_tracking_sums_restate_the_episode_reward(dtype):
    """sum |e_psi| + sum |e_h| + 0.5 sum |e_V| == 0.1 L - R - 100 [terminated] for every episode, on every path: the env's reward
    (fixedwing_lowlevel_env.py:118-134) restated from the rows the sums were taken from.  It fails if the terminal step's row
    were the auto-reset observation.  Episodes of max_episode_steps steps survived; every shorter one was terminated."""
    rel = 1e-9 if dtype == "float64" else 1e-5
    seen = {True: 0, False: 0}
    for kind, steps in POLICIES.items():
        for name, kw in PATHS.items():
            env = _env(16, steps, dtype=dtype)
            pol = _policy(env, kind)
            r = evaluate.evaluate_policy(pol, env, n_eval_episodes=24, deterministic=True, **kw)
            assert len(r.episode_lengths) == 24 == len(r.survived) == len(r.heading_abs), (kind, name)
            for k, (L, R_, s) in enumerate(zip(r.episode_lengths, r.episode_rewards, r.survived)):
                lhs = r.heading_abs[k] + r.altitude_abs[k] + 0.5 * r.airspeed_abs[k]
                rhs = 0.1 * L - R_ - (0.0 if s else 100.0)
                assert lhs == pytest.approx(rhs, rel=rel), (kind, name, k, L, s)
                assert s == (L == steps), (kind, name, k, L, s)
                seen[s] += 1
            sc = r.tracking_scalars()
            assert sc["eval/survival_rate"] == pytest.approx(np.mean(r.survived))
            for q in ("heading", "altitude", "airspeed"):
                assert sc[f"eval/{q}_rmse"] >= sc[f"eval/{q}_mae"] > 0
            assert sc["eval/ang_vel_mean"] > 0
    assert seen[True] > 0 and seen[False] > 0, seen          # both endings were exercised


def test_replayed_bookkeeping_kernel_matches_the_host_loop():
    """fw_eval_track_ll (replayed path) against the torch restatement of the step-by-step loop: the same episodes in the same order,
    lengths, rewards and survival equal, the seven sums to 1e-12 -- with envs that finish several episodes and an uneven split."""
    ended = set()
    for kind, steps in POLICIES.items():
        out = []
        for kw in (PATHS["host_loop"], PATHS["replayed"]):
            env = _env(24, steps)
            out.append(evaluate.evaluate_policy(_policy(env, kind), env, n_eval_episodes=61, deterministic=True, **kw))
        a, b = out
        assert len(a.episode_lengths) == 61 == len(b.episode_lengths)
        assert a.episode_lengths == b.episode_lengths and a.episode_rewards == b.episode_rewards
        assert a.survived == b.survived
        np.testing.assert_allclose(_sums(b), _sums(a), rtol=1e-12, atol=0)
        assert a.tracking_scalars() == pytest.approx(b.tracking_scalars(), rel=1e-12)
        ended |= set(a.survived)
    assert ended == {True, False}                            # crashes and truncations both compared


@pytest.fixture(params=[1, 8], ids=["lane_per_env", "8_lanes_per_env"])
def lanes(request, monkeypatch):
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", str(request.param))
    return request.param


def test_fused_six_action_evaluation_flies_the_episodes_of_the_torch_evaluation(lanes):
    """use_fused=True with the six-action policy: fw_collect_act_a (fp32 MFMA forward) -> fw_step -> fw_eval_track_ll.  Same episodes
    as the torch path: same number and order, lengths and survival equal but for a knife-edge ending, rewards and sums to ~1e-4.
    use_fused=None keeps the torch path for six actions."""
    out = []
    for fused in (None, True):
        env = _env(24, 120)
        assert env.venv.lanes_per_env == lanes
        with torch.no_grad():                                      # statistics as after some training: not the identity
            env.obs_rms.mean.copy_(torch.linspace(-0.2, 0.3, env.obs_dim, dtype=torch.float64, device="cuda"))
            env.obs_rms.var.copy_(torch.linspace(0.5, 2.0, env.obs_dim, dtype=torch.float64, device="cuda"))
        torch.manual_seed(0)
        pol = R.MlpPolicy(env.obs_dim, env.act_dim).cuda()
        with torch.no_grad():
            pol.action_net.weight.mul_(30.0)
        job = evaluate.ReplayedEvaluation(pol, env, _targets(61, 24), use_fused=fused)
        assert job.fused == bool(fused) and job.step.kind == ("act_a" if fused else "torch")
        out.append(job.run(None))
    a, b = out
    assert len(a.episode_lengths) == 61 == len(b.episode_lengths)
    same = [x == y for x, y in zip(a.episode_lengths, b.episode_lengths)]
    assert sum(same) >= 58, (a.episode_lengths, b.episode_lengths)
    assert sum(x == y for x, y in zip(a.survived, b.survived)) >= 58
    sa, sb = _sums(a), _sums(b)
    for k, ok in enumerate(same):
        if ok:
            assert b.episode_rewards[k] == pytest.approx(a.episode_rewards[k], rel=1e-4, abs=1e-4), k
            np.testing.assert_allclose(sb[k], sa[k], rtol=1e-4, atol=1e-6, err_msg=str(k))


def test_async_evaluation_and_eval_callback_carry_the_tracking_figures(tmp_path):
    env = _env(16, 60, seed=4)
    pol = _policy(env, "saturated")
    sync = evaluate.evaluate_policy(pol, env, n_eval_episodes=20, deterministic=True)
    r = evaluate.start_evaluation(pol, _env(16, 60, seed=4), n_eval_episodes=20).result()
    assert r.episode_lengths == sync.episode_lengths and r.survived == sync.survived
    np.testing.assert_array_equal(_sums(r), _sums(sync))
    keys = {"eval/heading_mae", "eval/heading_rmse", "eval/altitude_mae", "eval/altitude_rmse", "eval/airspeed_mae",
            "eval/airspeed_rmse", "eval/ang_vel_mean", "eval/survival_rate"}
    assert set(r.tracking_scalars()) == keys

    train = R.VecNormalizeDevice(P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=60), 64, seed=1), norm_obs=True, norm_reward=True)
    ppo = R.PPO(train, R.PPOConfig(n_steps=16, batch_size=64, n_epochs=1, seed=1))
    ev = evaluate.EvalCallback(_env(8, 60, seed=2), n_eval_episodes=8, eval_freq=16, log_path=str(tmp_path / "logs"))
    ppo.learn(2 * 16 * 64, callbacks=[ev])
    assert ev.n_evals == 2
    assert keys <= set(ev.last_scalars) and {"eval/mean_reward", "eval/mean_ep_length"} <= set(ev.last_scalars)
    z = np.load(os.path.join(tmp_path, "logs", "evaluations.npz"), allow_pickle=True)
    for k in keys:
        name = k.split("/", 1)[1]
        assert z[name].shape == (2,), name
        assert z[name][-1] == pytest.approx(ev.last_scalars[k])


def test_fw_eval_track_ll_rejects_bad_arguments():
    L, dev = _lib.lib(), "cuda"
    n, E = 8, 2
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)          # noqa: E731
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)            # noqa: E731
    u8 = torch.zeros(n, dtype=torch.uint8, device=dev)
    rew, obs, tobs = f64(n), f64(n, 21), f64(n, 21)
    tg, cnt, cl, ctr, fl, fs = i64(n), i64(n), i64(n), i64(1), i64(n, E), i64(n, E)
    cr, ct, fr, ft = f64(n), f64(n, 7), f64(n, E), f64(n, E, 8)
    p = lambda t: t.data_ptr() if t is not None else None                     # noqa: E731

    def call(obs_=obs, obs_dim=21, N=n, E_=E):
        return L.fw_eval_track_ll(p(rew), 1, p(u8), p(u8), None, 0, p(obs_), p(tobs), 1, obs_dim, p(tg), p(cnt), p(cr), p(cl), p(ctr),
                                  p(ct), p(fr), p(fl), p(fs), None, p(ft), N, E_, None)
    assert call(obs_=None) == K.FW_EINVAL
    assert "non-NULL" in L.fw_last_error(None).decode()
    assert call(obs_dim=20) == K.FW_EINVAL
    assert "obs_dim must be 21" in L.fw_last_error(None).decode()
    assert call(E_=0) == K.FW_EINVAL and call(N=0) == K.FW_EINVAL
    assert call() == K.FW_OK                                  # the same buffers, well formed: one launch
    torch.cuda.synchronize()
    assert int(ctr.item()) == 1 and torch.equal(cl, torch.ones_like(cl))
