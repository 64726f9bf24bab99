"""Six-action fused learner (the low-level control task): fw_ppo_update_a / fw_policy_act_a / fw_collect_act_a against the torch
path, the four-action forms of the new entry points against the old ones, and PPO(fused_six_actions=True) end to end."""

import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib, checkpoint
from pyflyt_drone_amd import rollout as R

pytestmark = pytest.mark.gpu


class _BufEnv:
    """Just enough env for PPO.__init__ / train(): the update is tested on hand-filled rollout buffers."""
    def __init__(self, n, d, a):
        self.device, self.num_envs, self.obs_dim, self.act_dim = torch.device("cuda"), n, d, a


def _filled_ppo(fused, d, bs, n_epochs, a=6, T=4, n=256, seed=5):
    ppo = R.PPO(_BufEnv(n, d, a), R.PPOConfig(n_steps=T, batch_size=bs, n_epochs=n_epochs, seed=seed, use_graphs=False,
                                              fused_update=fused, fused_six_actions=True, ent_coef=0.01))
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    ppo.buf_obs.copy_(torch.randn(ppo.buf_obs.shape, device="cuda", generator=g).clamp(-10, 10))
    with torch.no_grad():
        act, _, _ = ppo.policy(ppo.buf_obs.reshape(-1, d), generator=g)
        ppo.buf_act.copy_((act + 0.3 * torch.randn(act.shape, device="cuda", generator=g)).reshape(ppo.buf_act.shape))
        _, lp2, _ = ppo.policy.evaluate_actions(ppo.buf_obs.reshape(-1, d), ppo.buf_act.reshape(-1, a))
        ppo.buf_logp.copy_((lp2 + 0.2 * torch.randn(lp2.shape, device="cuda", generator=g)).reshape(T, n))
    ppo.adv = torch.randn((T, n), device="cuda", generator=g) * 2.0 + 0.5
    ppo.ret = torch.randn((T, n), device="cuda", generator=g) * 3.0
    return ppo


# (d, batch, cut): every samples-per-pass form (16 / 32 / 64) and 1, 2, 4, 8 blocks per network, reduce-scatter and all-to-all
@pytest.mark.parametrize("d,bs,split", [(21, 64, None), (21, 128, None), (28, 64, None), (5, 64, None), (21, 16, None), (21, 32, None),
                                        (21, 128, "32x4"), (21, 256, "64x4"), (28, 128, "64x2"), (21, 64, "64x1"), (21, 256, "32x8"),
                                        (21, 512, "64x8"), (28, 128, "all-to-all"), (64, 128, None)])
def test_fused_six_action_update_matches_the_torch_path(d, bs, split, monkeypatch):
    if split == "all-to-all":
        monkeypatch.setenv("FWSIM_PPO_RS", "0")
    elif split is not None:
        monkeypatch.setenv("FWSIM_PPO_SPLIT", split)
    a, b = _filled_ppo(True, d, bs, 2), _filled_ppo(False, d, bs, 2)
    assert a.policy.action_net.out_features == 6
    for rnd in range(2):
        a.train(); b.train()
        assert a._fused is not None and a._fused.A == 6 and b._fused is None
        for (na, p), (_, q) in zip(a.policy.named_parameters(), b.policy.named_parameters()):
            torch.testing.assert_close(p, q, rtol=2e-3, atol=2e-5, msg=lambda m: f"{na} round {rnd}: {m}")
            sa, sb = a.optimizer.state[p], b.optimizer.state[q]
            assert float(sa["step"]) == float(sb["step"]) == (rnd + 1) * 2 * (4 * 256 // bs)
            torch.testing.assert_close(sa["exp_avg"], sb["exp_avg"], rtol=5e-3, atol=1e-6)
            torch.testing.assert_close(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=5e-3, atol=1e-9)
        for k in ("policy_loss", "value_loss", "entropy_loss"):
            assert a.logs[k] == pytest.approx(b.logs[k], rel=2e-3, abs=1e-5)
    assert all(torch.isfinite(p).all() for p in a.policy.parameters())


def test_six_action_update_without_the_shared_l2_is_bit_identical(monkeypatch):
    a = _filled_ppo(True, 21, 128, 2)
    b = _filled_ppo(True, 21, 128, 2)
    a.train()
    monkeypatch.setenv("FWSIM_PPO_NO_L2_SWAP", "1")
    b.train()
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a.optimizer.state[p][k], b.optimizer.state[q][k])


def _hyper():
    return R._PpoHyper(lr=3e-4, clip_range=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, beta1=0.9, beta2=0.999, eps=1e-5,
                       adv_mean=0.0, adv_std=1.0, norm_adv=1, step0=3)


@pytest.mark.parametrize("bs", [64, 128])
def test_four_actions_through_the_new_entry_points_equal_the_old_ones_bit_for_bit(bs):
    import ctypes as C
    L, d, S = _lib.lib(), 28, 1024
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    n = L.fw_ppo_param_count(d)
    assert L.fw_ppo_param_count_a(d, 4) == n
    flat = torch.randn(n, device="cuda", generator=g) * 0.1
    ns = L.fw_ppo_moment_count()
    m0, v0 = torch.randn(ns, device="cuda", generator=g) * 1e-3, torch.rand(ns, device="cuda", generator=g) * 1e-5
    obs, act = torch.randn((S, d), device="cuda", generator=g), torch.randn((S, 4), device="cuda", generator=g)
    lp, adv, ret = (torch.randn(S, device="cuda", generator=g) for _ in range(3))
    n_mb = 2 * S // bs
    perm = torch.cat([torch.randperm(S, device="cuda", generator=g) for _ in range(2)]).to(torch.int32)
    out = []
    for new in (False, True):
        p, m, v = flat.clone(), m0.clone(), v0.clone()
        loss = torch.zeros(16, device="cuda")
        ws = torch.zeros(int(L.fw_ppo_update_workspace_bytes(n_mb, bs, d)), dtype=torch.uint8, device="cuda")
        H = _hyper()
        args = [R._p(x) for x in (p, m, v, obs, act, lp, adv, ret, perm)]
        if new:
            rc = L.fw_ppo_update_a(*args, n_mb, bs, d, 4, C.byref(H), R._p(loss), R._p(ws), ws.numel(), None)
        else:
            rc = L.fw_ppo_update(*args, n_mb, bs, d, C.byref(H), R._p(loss), R._p(ws), ws.numel(), None)
        _lib.check(rc)
        torch.cuda.synchronize()
        out.append((p, m, v, loss))
    for x, y in zip(*out):
        assert torch.equal(x, y)
    # the act kernels: sampled actions, log-probs, values
    rng = torch.tensor([91, 4], dtype=torch.int64, device="cuda")
    res = []
    for new in (False, True):
        ar, ae, lpo, val = (torch.zeros((S, 4), device="cuda"), torch.zeros((S, 4), device="cuda", dtype=torch.float64),
                            torch.zeros(S, device="cuda"), torch.zeros(S, device="cuda"))
        if new:
            _lib.check(L.fw_policy_act_a(R._p(flat), R._p(obs), S, d, 4, 3, 0, R._p(rng), 0, None, R._p(ar), R._p(ae), 1, R._p(lpo), R._p(val), None))
        else:
            _lib.check(L.fw_policy_act(R._p(flat), R._p(obs), S, d, 3, 0, R._p(rng), 0, None, R._p(ar), R._p(ae), 1, R._p(lpo), R._p(val), None))
        res.append((ar, ae, lpo, val))
    for x, y in zip(*res):
        assert torch.equal(x, y)


def _policy_pair(d, seed=11):
    """A six-action policy and the four-action policy with the same trunk, value net and first four head rows; their flat images."""
    torch.manual_seed(seed)
    p6 = R.MlpPolicy(d, 6).cuda()
    with torch.no_grad():
        for q in p6.parameters():
            q.add_(0.1 * torch.randn_like(q))
    p4 = R.MlpPolicy(d, 4).cuda()
    sd = {k: (v[:4] if k.startswith(("action_net", "log_std")) else v) for k, v in p6.state_dict().items()}
    p4.load_state_dict(sd)
    f6 = R.FusedPpoUpdate(p6, torch.optim.Adam(p6.parameters()), d); f6.load_params_from_torch()
    f4 = R.FusedPpoUpdate(p4, torch.optim.Adam(p4.parameters()), d); f4.load_params_from_torch()
    return p6, p4, f6.flat, f4.flat


def _act(flat, obs, a, det, rng, env_offset=0, f64=False):
    L, (n, d) = _lib.lib(), obs.shape
    ar = torch.zeros((n, a), device="cuda")
    ae = torch.zeros((n, a), device="cuda", dtype=torch.float64 if f64 else torch.float32)
    lp, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    _lib.check(L.fw_policy_act_a(R._p(flat), R._p(obs), n, d, a, 3, int(det), R._p(rng), env_offset, None, R._p(ar), R._p(ae), int(f64),
                                 R._p(lp), R._p(v), None))
    return ar, ae, lp, v


@pytest.mark.parametrize("d", [21, 28, 5])
def test_policy_act_a6_against_the_torch_policy(d):
    n = 16384
    p6, p4, f6, f4 = _policy_pair(d)
    obs = torch.randn((n, d), device="cuda") * 2
    rng = torch.tensor([1234, 7], dtype=torch.int64, device="cuda")
    with torch.no_grad():
        mu = p6.action_net(p6.pi_net(obs))
        val = p6.predict_values(obs)
    ar, ae, lp, v = _act(f6, obs, 6, True, rng)
    torch.testing.assert_close(ar, mu, rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(v, val, rtol=1e-5, atol=2e-6)
    # sampling: the log-prob of the drawn action, the env copy clipped
    for f64 in (False, True):
        ar, ae, lp, v = _act(f6, obs, 6, False, rng, 512, f64)
        with torch.no_grad():
            _, lp_t, _ = p6.evaluate_actions(obs, ar)
        torch.testing.assert_close(lp, lp_t, rtol=1e-5, atol=2e-4)
        assert torch.equal(ae, ar.clamp(-1.0, 1.0).to(ae.dtype))
    # components 0-3: the four-action draw, bit for bit
    ar4, _, _, _ = _act(f4, obs, 4, False, rng, 512)
    assert torch.equal(ar[:, :4], ar4)
    # components 4, 5: N(0, 1), independent of 0-3
    z = ((ar - mu) / p6.log_std.detach().exp()).double().cpu().numpy()
    for k in (4, 5):
        assert abs(z[:, k].mean()) < 0.04 and abs(z[:, k].std() - 1.0) < 0.04
        for j in range(6):
            if j != k:
                assert abs(np.corrcoef(z[:, k], z[:, j])[0, 1]) < 0.04
    # same (seed, draw): the same noise; a new draw: new noise
    ar_again, _, _, _ = _act(f6, obs, 6, False, rng, 512)
    assert torch.equal(ar_again, ar)
    rng2 = torch.tensor([1234, 8], dtype=torch.int64, device="cuda")
    ar_next, _, _, _ = _act(f6, obs, 6, False, rng2, 512)
    assert not torch.equal(ar_next[:, 4:], ar[:, 4:]) and not torch.equal(ar_next[:, :4], ar[:, :4])


def test_collect_act_a6_normalises_on_load_and_finalises_the_previous_step():
    L, d, n = _lib.lib(), 21, 1000
    p6, _, f6, _ = _policy_pair(d, seed=4)
    raw = torch.randn((n, d), device="cuda", dtype=torch.float64) * 4 + 1
    mean, var = torch.randn(d, device="cuda", dtype=torch.float64), torch.rand(d, device="cuda", dtype=torch.float64) * 4 + 0.1
    cnt = torch.ones(1, device="cuda", dtype=torch.float64)
    rng = torch.tensor([77, 3], dtype=torch.int64, device="cuda")
    obs_n = torch.zeros((n, d), device="cuda")
    _lib.check(L.fw_normalize_obs(R._p(raw), 1, n, d, R._p(mean), R._p(var), R._p(cnt), 0, 10.0, 1e-8, R._p(obs_n), None, None, None))
    ar0, ae0, lp0, v0 = _act(f6, obs_n, 6, False, rng, 512, True)
    g = torch.Generator().manual_seed(2)
    rew = (torch.randn(n, generator=g, dtype=torch.float64) * 20).cuda()
    term = (torch.rand(n, generator=g) < 0.05).to(torch.uint8).cuda(); trunc = (torch.rand(n, generator=g) < 0.03).to(torch.uint8).cuda()
    trunc[64:128] = 0; term[64:128] = 0
    tobs = torch.randn((n, d), device="cuda", dtype=torch.float64) * 3
    ret_var = torch.tensor([7.5], dtype=torch.float64, device="cuda")
    oc1, ar1, ae1 = torch.zeros_like(obs_n), torch.zeros((n, 6), device="cuda"), torch.zeros((n, 6), device="cuda", dtype=torch.float64)
    lp1, v1 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    rew1, st1 = torch.full((n,), -9.0, device="cuda"), torch.full((n,), -9.0, device="cuda")
    _lib.check(L.fw_collect_act_a(R._p(f6), R._p(raw), 1, n, d, 6, R._p(mean), R._p(var), 10.0, 1e-8, 3, 0, R._p(rng), 512, R._p(oc1), R._p(ar1),
                                  R._p(ae1), 1, R._p(lp1), R._p(v1), R._p(rew), R._p(term), R._p(trunc), R._p(tobs), R._p(ret_var), 1, 10.0, 1e-8,
                                  0.99, R._p(rew1), R._p(st1), None))
    for x, y in ((oc1, obs_n), (ar1, ar0), (ae1, ae0), (lp1, lp0), (v1, v0)):
        assert torch.equal(x, y)
    # the previous step: VecNormalize's reward path + the bootstrap of truncated episodes with V(normalised terminal observation)
    tn = ((tobs - mean) / torch.sqrt(var + 1e-8)).clamp(-10, 10).float()
    with torch.no_grad():
        tv = p6.predict_values(tn)
    rn = (rew / torch.sqrt(ret_var + 1e-8)).clamp(-10, 10).float()
    boot = (trunc.bool() & ~term.bool())
    exp = rn + 0.99 * tv * boot.float()
    torch.testing.assert_close(rew1, exp, rtol=1e-5, atol=1e-5)
    assert torch.equal(st1, (term.bool() | trunc.bool()).float())


# ------------------------------------------------------------------------------------------------------------------ PPO
def _ll_ppo(seed=5, fused=True, n=256, graphs=True, n_steps=16):
    env = R.VecNormalizeDevice(P.FixedwingLowLevelVecEnv(num_envs=n, seed=seed, device=0), norm_obs=True, norm_reward=True, clip_obs=10.0)
    return R.PPO(env, R.PPOConfig(n_steps=n_steps, batch_size=64, n_epochs=2, seed=seed, use_graphs=graphs, fused_six_actions=fused))


def test_ppo_on_the_low_level_task_takes_the_fused_learner_when_asked():
    a, b = _ll_ppo(fused=True, graphs=False), _ll_ppo(fused=False, graphs=False)
    assert a._collect_fused and not a._one_launch and not a._close_gae
    assert a._act_env.shape == (256, 6)
    assert R.FusedPpoUpdate.applies(a.policy, a.cfg, a.env.obs_dim, a.cfg.batch_size, a.device)
    assert not b._collect_fused and not R.FusedPpoUpdate.applies(b.policy, b.cfg, b.env.obs_dim, b.cfg.batch_size, b.device)
    for _ in range(2):
        a.collect_rollouts(); b.collect_rollouts()
    with torch.no_grad():
        v, lp, _ = a.policy.evaluate_actions(a.buf_obs.reshape(-1, a.env.obs_dim), a.buf_act.reshape(-1, 6))
    torch.testing.assert_close(v, a.buf_val.reshape(-1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lp, a.buf_logp.reshape(-1), rtol=1e-5, atol=2e-4)
    assert torch.isfinite(a.buf_rew).all() and torch.isfinite(a.adv).all()
    assert float(a.env.obs_rms.count.item()) == float(b.env.obs_rms.count.item())
    assert float(a.env.ret_rms.count.item()) == float(b.env.ret_rms.count.item())


def test_graph_replayed_rollouts_accumulate_the_same_statistics_as_eager_ones():
    a, b = _ll_ppo(graphs=True), _ll_ppo(graphs=False)
    for _ in range(3):                                   # eager, capture, replay
        a.collect_rollouts(); b.collect_rollouts()
    assert a._g_rollout is not None and b._g_rollout is None
    for x, y in ((a.env.obs_rms, b.env.obs_rms), (a.env.ret_rms, b.env.ret_rms)):
        assert float(x.count.item()) == float(y.count.item())
        torch.testing.assert_close(x.mean, y.mean, rtol=0, atol=0)
        torch.testing.assert_close(x.var, y.var, rtol=0, atol=0)
    torch.testing.assert_close(a.buf_act, b.buf_act, rtol=0, atol=0)


def test_fused_six_action_training_and_checkpoints(tmp_path):
    a = _ll_ppo(fused=True)
    a.learn(3 * 16 * 256)
    assert a.num_timesteps == 3 * 16 * 256 and a._fused is not None and a._fused.A == 6
    assert all(torch.isfinite(p).all() for p in a.policy.parameters())
    assert all(np.isfinite(v) for v in a.logs.values())
    path = checkpoint.save(str(tmp_path / "ll.pt"), a)
    a.collect_rollouts()
    ref = [x.clone() for x in (a.buf_obs, a.buf_act, a.buf_rew, a.buf_logp, a.buf_val)]
    b = _ll_ppo(fused=True)
    checkpoint.load(path, b, reset_num_timesteps=False, restore_env_state=True)
    b.collect_rollouts()
    for x, y in zip(ref, (b.buf_obs, b.buf_act, b.buf_rew, b.buf_logp, b.buf_val)):
        torch.testing.assert_close(y, x, rtol=0, atol=0)


def _state(ppo):
    opt = ppo.optimizer
    mods = {k: v.detach().clone() for k, v in ppo.policy.state_dict().items()}
    mom = [(float(opt.state[p]["step"]), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ppo.policy.parameters()]
    rms = [t.clone() for r in (ppo.env.obs_rms, ppo.env.ret_rms) for t in (r.mean, r.var, r.count)]
    return mods, mom, rms


@pytest.mark.parametrize("saved_fused", [True, False])
def test_checkpoints_are_interchangeable_across_the_flag(tmp_path, saved_fused):
    a = _ll_ppo(fused=saved_fused, graphs=False)
    a.learn(2 * 16 * 256)
    path = checkpoint.save(str(tmp_path / "x.pt"), a)
    want = _state(a)
    b = _ll_ppo(fused=not saved_fused, graphs=False)
    checkpoint.load(path, b, reset_num_timesteps=False, restore_env_state=True)
    got = _state(b)
    for k in want[0]:
        assert torch.equal(want[0][k], got[0][k]), k
    for (s0, m0, v0), (s1, m1, v1) in zip(want[1], got[1]):
        assert s0 == s1 and torch.equal(m0, m1) and torch.equal(v0, v1)
    for x, y in zip(want[2], got[2]):
        assert torch.equal(x, y)
    b.learn(16 * 256, reset_num_timesteps=False)           # and the other path trains on from there
    assert all(torch.isfinite(p).all() for p in b.policy.parameters())
