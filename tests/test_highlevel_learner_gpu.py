"""Three-action fused learner and collector of the high-level command task: ``fw_ppo_update_a3`` against the torch path,
``fw_collect_act_hl`` against the chain of launches it replaces, and ``PPO(fused_three_actions=True)`` end to end."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib, checkpoint
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R
from pyflyt_drone_amd.highlevel import HighLevelCmdVecEnv

pytestmark = pytest.mark.gpu

TAIL = K.S_TASK
BASE_KW = dict(flight_dome_size=200.0, max_duration_seconds=120.0, agent_hz=30, context_length=2, angle_representation="euler")


# ------------------------------------------------------------------------------------------------------------------ update
class _BufEnv:
    """Just enough env for PPO.__init__ / train(): the update is tested on hand-filled rollout buffers."""
    def __init__(self, n, d, a):
        self.device, self.num_envs, self.obs_dim, self.act_dim = torch.device("cuda"), n, d, a


def _filled_ppo(fused, d, bs, n_epochs, T=4, n=256, seed=5):
    a = 3
    ppo = R.PPO(_BufEnv(n, d, a), R.PPOConfig(n_steps=T, batch_size=bs, n_epochs=n_epochs, seed=seed, use_graphs=False,
                                              fused_update=fused, fused_three_actions=True, ent_coef=0.01))
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


# (d, batch, cut): every samples-per-pass form (16 / 32 / 64) and 1, 2, 4, 8 blocks per network, reduce-scatter and all-to-all, once;
# plus the widest input.  Tolerances: the six-action kernel's (tests/test_wide_action_learner_gpu.py).
@pytest.mark.parametrize("d,bs,split", [(30, 64, None), (30, 256, None), (30, 16, None), (30, 32, None), (5, 64, None), (64, 128, None),
                                        (30, 128, "32x4"), (30, 256, "64x4"), (30, 128, "64x2"), (30, 64, "64x1"), (30, 256, "32x8"),
                                        (30, 512, "64x8"), (30, 128, "all-to-all")])
def test_fused_three_action_update_matches_the_torch_path(d, bs, split, monkeypatch):
    if split == "all-to-all":
        monkeypatch.setenv("FWSIM_PPO_RS", "0")
    elif split is not None:
        monkeypatch.setenv("FWSIM_PPO_SPLIT", split)
    a, b = _filled_ppo(True, d, bs, 2), _filled_ppo(False, d, bs, 2)
    assert a.policy.action_net.out_features == 3
    for rnd in range(2):
        a.train(); b.train()
        assert a._fused is not None and a._fused.A == 3 and b._fused is None
        for (na, p), (_, q) in zip(a.policy.named_parameters(), b.policy.named_parameters()):
            torch.testing.assert_close(p, q, rtol=2e-3, atol=2e-5, msg=lambda m: f"{na} round {rnd}: {m}")
            sa, sb = a.optimizer.state[p], b.optimizer.state[q]
            assert float(sa["step"]) == float(sb["step"]) == (rnd + 1) * 2 * (4 * 256 // bs)
            torch.testing.assert_close(sa["exp_avg"], sb["exp_avg"], rtol=5e-3, atol=1e-6)
            torch.testing.assert_close(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=5e-3, atol=1e-9)
        for k in ("policy_loss", "value_loss", "entropy_loss"):
            assert a.logs[k] == pytest.approx(b.logs[k], rel=2e-3, abs=1e-5)
    assert all(torch.isfinite(p).all() for p in a.policy.parameters())


def _same_bits(a, b):
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a.optimizer.state[p][k], b.optimizer.state[q][k])
    assert a.logs == b.logs


def test_three_action_update_without_the_shared_l2_is_bit_identical(monkeypatch):
    a = _filled_ppo(True, 30, 128, 2)
    b = _filled_ppo(True, 30, 128, 2)
    a.train()
    monkeypatch.setenv("FWSIM_PPO_NO_L2_SWAP", "1")
    b.train()
    _same_bits(a, b)


@pytest.mark.parametrize("bs", [64, 256])
def test_the_fourth_action_column_is_dead(bs):
    """What the implementation pads: the packed rows of the workspace keep the four-action width, the pre-pass writes their fourth
    action float as zero, and gout / sA rows in LDS are four floats wide with column 3 never read into a sum.  ``act`` itself is
    [S, 3] and is not padded.  So: the same update from the same state over workspaces whose packed-row region was filled with two
    different kinds of garbage (NaN bit patterns, a finite pattern) must give the same bits -- nothing of a previous call's fourth
    float, or of whatever the region held, reaches a parameter, a moment or a loss."""
    d, out = 30, []
    for fill in (0xFF, 0x41):
        ppo = _filled_ppo(True, d, bs, 2)
        ppo._fused = R.FusedPpoUpdate(ppo.policy, ppo.optimizer, d)
        n_mb = 2 * (4 * 256 // bs)
        ws = ppo._fused._workspace(n_mb, bs)
        packed_bytes = n_mb * bs * (((d + 3) & ~3) + 8) * 4
        assert 0 < packed_bytes < ws.numel()
        ws[ws.numel() - packed_bytes:].fill_(fill)
        ppo.train()
        assert ppo._fused._ws is ws
        out.append(ppo)
    _same_bits(*out)
    assert all(torch.isfinite(p).all() for p in out[0].policy.parameters())


# ------------------------------------------------------------------------------------------------------------------ fw_collect_act_hl
@pytest.fixture(params=[1, 8], ids=["lane_per_env", "8_lanes_per_env"])
def lanes(request, monkeypatch):
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", str(request.param))
    return request.param


def _controller(seed=21):
    """a controller with random (seeded) weights whose actions use the whole of [-1, 1], and non-trivial statistics"""
    torch.manual_seed(seed)
    p = R.MlpPolicy(21, 6)
    with torch.no_grad():
        for q in p.parameters():
            q.add_(0.1 * torch.randn_like(q))
        p.action_net.weight.mul_(1.5)
    g = np.random.default_rng(seed)
    mean = g.normal(0.0, 1.0, 21) * np.array([1] * 6 + [10] * 6 + [0.3] * 6 + [1, 50, 10], dtype=np.float64)
    var = g.uniform(0.2, 4.0, 21) * np.array([1] * 6 + [100] * 6 + [0.1] * 6 + [3, 2500, 80], dtype=np.float64)
    return p, mean, var


def _commander(seed=31):
    """a three-action policy whose mean sits inside the Box and whose log-std is wide enough for every Box bound to clip"""
    torch.manual_seed(seed)
    p = R.MlpPolicy(30, 3).cuda()
    with torch.no_grad():
        for q in p.parameters():
            q.add_(0.1 * torch.randn_like(q))
        p.action_net.bias.copy_(torch.tensor([0.0, 100.0, 15.0]))
        p.log_std.copy_(torch.tensor([1.5, 5.0, 3.5]))          # sigma 4.5 rad, 148 m, 33 m/s
    return p


def _flat(policy, d):
    f = R.FusedPpoUpdate(policy, None, d)
    f.load_params_from_torch()
    return f.flat


def _flown_env(n, dtype, seed=5):
    env = P.FixedwingWaypointsDirectVecEnv(n, **BASE_KW, dtype=dtype, seed=seed)
    env.reset_tensor()
    rng = np.random.default_rng(1)
    for _ in range(3):                                    # some flight: the shared observation columns are not the start pose
        env.step_tensor(torch.as_tensor(rng.uniform(-0.3, 0.3, (n, 6)), device=env.device, dtype=env.torch_dtype))
    return env


class _Hl:
    """The buffers of one fw_collect_act_hl call on `env`, and the call."""
    def __init__(self, env, low_flat, low_mean, low_var):
        n, dev, td = env.num_envs, env.device, env.torch_dtype
        self.env, self.low_flat = env, low_flat
        self.low_mean = torch.as_tensor(low_mean, dtype=torch.float64, device=dev)
        self.low_var = torch.as_tensor(low_var, dtype=torch.float64, device=dev)
        self.obs_copy, self.act_raw = torch.full((n, 30), -7.0, device=dev), torch.full((n, 3), -7.0, device=dev)
        self.logp, self.value = torch.full((n,), -7.0, device=dev), torch.full((n,), -7.0, device=dev)
        self.low_obs, self.cmd = torch.full((n, 21), -7.0, dtype=td, device=dev), torch.full((n, 3), -7.0, dtype=td, device=dev)
        self.act_env = torch.full((n, 6), -7.0, dtype=td, device=dev)
        self.rejected = torch.zeros(1, dtype=torch.int32, device=dev)
        self.rew_out, self.start_out = torch.full((n,), -9.0, device=dev), torch.full((n,), -9.0, device=dev)

    def args(self, flat, mean, var, rng, nets=3, det=0, env_offset=512, prev=None):
        a = K.FwCollectHlArgs()
        a.params, a.low_params, a.obs = flat.data_ptr(), self.low_flat.data_ptr(), self.env.obs.data_ptr()
        a.obs_mean, a.obs_var, a.low_mean, a.low_var = mean.data_ptr(), var.data_ptr(), self.low_mean.data_ptr(), self.low_var.data_ptr()
        a.rng, a.env_offset = rng.data_ptr(), env_offset
        a.obs_copy, a.act_raw, a.logp, a.value = self.obs_copy.data_ptr(), self.act_raw.data_ptr(), self.logp.data_ptr(), self.value.data_ptr()
        a.low_obs, a.cmd_out, a.act_env, a.rejected = self.low_obs.data_ptr(), self.cmd.data_ptr(), self.act_env.data_ptr(), self.rejected.data_ptr()
        a.clip_obs, a.eps_obs, a.low_clip, a.low_eps = 10.0, 1e-8, 10.0, 1e-8
        a.nets, a.deterministic = nets, det
        if prev is not None:
            rew, term, trunc, tobs, ret_var = prev
            a.prev_reward, a.prev_terminated, a.prev_truncated = rew.data_ptr(), term.data_ptr(), trunc.data_ptr()
            a.prev_terminal_obs, a.ret_var = tobs.data_ptr(), ret_var.data_ptr()
            a.norm_reward, a.clip_reward, a.eps_reward, a.gamma = 1, 10.0, 1e-8, 0.99
            a.rew_out, a.start_out = self.rew_out.data_ptr(), self.start_out.data_ptr()
        return a

    def run(self, a):
        _lib.check(_lib.lib().fw_collect_act_hl(self.env._h, C.byref(a), None), self.env._h)
        torch.cuda.synchronize()


def _same_words(x, y):
    """bit for bit, NaNs included"""
    w = torch.int32 if x.dtype == torch.float32 else torch.int64
    return torch.equal(x.view(w), y.view(w))


def _chain(env, act_raw, low_flat, low_mean, low_var):
    """what fw_collect_act_hl replaces behind the commander's forward: fw_command_hl on the float32 act_raw, then the controller"""
    L, n, td = _lib.lib(), env.num_envs, env.torch_dtype
    f64 = int(td == torch.float64)
    low_obs, cmd = torch.full((n, 21), -7.0, dtype=td, device=env.device), torch.full((n, 3), -7.0, dtype=td, device=env.device)
    rej = torch.zeros(1, dtype=torch.int32, device=env.device)
    _lib.check(L.fw_command_hl(env._h, R._p(act_raw), 0, None, R._p(env.obs), R._p(low_obs), R._p(cmd), R._p(rej), None), env._h)
    ar, lp = torch.zeros((n, 6), device=env.device), torch.zeros(n, device=env.device)
    act_env = torch.full((n, 6), -7.0, dtype=td, device=env.device)
    _lib.check(L.fw_collect_act_a(R._p(low_flat), R._p(low_obs), f64, n, 21, 6, R._p(low_mean), R._p(low_var), 10.0, 1e-8, 1, 1, None, 0,
                                  None, R._p(ar), R._p(act_env), f64, R._p(lp), None, None, None, None, None, None, 0, 0.0, 0.0, 0.0,
                                  None, None, None))
    torch.cuda.synchronize()
    return low_obs, cmd, act_env, int(rej.item())


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [16, 199])
def test_collect_act_hl_against_the_chain_it_replaces(n, dtype, lanes):
    L = _lib.lib()
    env = _flown_env(n, dtype)
    assert env.lanes_per_env == lanes
    dev, td = env.device, env.torch_dtype
    f64 = int(td == torch.float64)
    pol, ctl = _commander(), _controller()
    flat, low_flat = _flat(pol, 30), _flat(ctl[0].cuda(), 21)
    g = torch.Generator().manual_seed(2)
    mean = (torch.randn(30, generator=g, dtype=torch.float64) * 0.5).cuda()
    var = (torch.rand(30, generator=g, dtype=torch.float64) * 4 + 0.1).cuda()
    cnt = torch.ones(1, device=dev, dtype=torch.float64)
    rng = torch.tensor([77, 3], dtype=torch.int64, device=dev)
    # the previous step to finalise: the six-action test's recipe, a truncated-not-terminated row present
    rew = (torch.randn(n, generator=g, dtype=torch.float64) * 20).to(td).cuda()
    term = (torch.rand(n, generator=g) < 0.05).to(torch.uint8).cuda(); trunc = (torch.rand(n, generator=g) < 0.03).to(torch.uint8).cuda()
    trunc[3], term[3] = 1, 0
    trunc[5], term[5] = 1, 1
    tobs = (torch.randn((n, 30), generator=g, dtype=torch.float64) * 3).to(td).cuda()
    ret_var = torch.tensor([7.5], dtype=torch.float64, device=dev)
    h = _Hl(env, low_flat, ctl[1], ctl[2])
    state0 = env.get_state()

    # ---- sampled ----
    h.run(h.args(flat, mean, var, rng, prev=(rew, term, trunc, tobs, ret_var)))
    state1 = env.get_state()
    obs_n = torch.zeros((n, 30), device=dev)
    _lib.check(L.fw_normalize_obs(R._p(env.obs), f64, n, 30, R._p(mean), R._p(var), R._p(cnt), 0, 10.0, 1e-8, R._p(obs_n), None, None, None))
    torch.cuda.synchronize()
    assert torch.equal(h.obs_copy, obs_n)
    a64 = h.act_raw.double().cpu().numpy()
    lo, hi = np.array([-math.pi, 0.0, 0.0]), np.array([math.pi, 200.0, 30.0])
    assert (a64 < lo).any(axis=0).all() and (a64 > hi).any(axis=0).all(), "every Box bound must clip"
    assert ((a64 >= lo) & (a64 <= hi)).all(axis=1).any()
    env.set_state(state0)
    low_obs, cmd, act_env, rej = _chain(env, h.act_raw, low_flat, h.low_mean, h.low_var)
    assert torch.equal(h.cmd, cmd) and torch.equal(h.low_obs, low_obs) and torch.equal(h.act_env, act_env)
    assert int(h.rejected.item()) == rej == 0
    np.testing.assert_array_equal(state1, env.get_state())
    np.testing.assert_array_equal(state1[:, TAIL:TAIL + 3], h.cmd.double().cpu().numpy())
    assert (h.act_env.abs() <= 1.0).all() and (h.act_env.abs() == 1.0).any() and (h.act_env.abs() < 1.0).any()
    c = h.cmd.double().cpu().numpy()
    pi_t = float(env.np_dtype(math.pi))                   # (f32 handles: the double command rounded once, -pi to float32's -pi)
    assert (c[:, 0] >= -pi_t).all() and (c[:, 0] <= pi_t).all() and (c[:, 1:] >= 0).all() and (c[:, 1] <= 200.0).all() and (c[:, 2] <= 30.0).all()
    # log-prob and value against the torch policy on the normalised rows
    with torch.no_grad():
        v_t, lp_t, _ = pol.evaluate_actions(obs_n, h.act_raw)
        mu_t = pol.action_net(pol.pi_net(obs_n))
    torch.testing.assert_close(h.value, v_t, rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(h.logp, lp_t, rtol=1e-5, atol=2e-4)
    # the finalisation of the previous step
    tn = ((tobs.double() - mean) / torch.sqrt(var + 1e-8)).clamp(-10, 10).float()
    with torch.no_grad():
        tv = pol.predict_values(tn)
    rn = (rew.double() / torch.sqrt(ret_var + 1e-8)).clamp(-10, 10).float()
    boot = trunc.bool() & ~term.bool()
    assert bool(boot.any())
    torch.testing.assert_close(h.rew_out, rn + 0.99 * tv * boot.float(), rtol=1e-5, atol=1e-5)
    assert torch.equal(h.start_out, (term.bool() | trunc.bool()).float())
    sampled = h.act_raw.clone()

    # ---- deterministic: the mean ----
    env.set_state(state0)
    h.run(h.args(flat, mean, var, rng, det=1))
    torch.testing.assert_close(h.act_raw, mu_t, rtol=1e-5, atol=2e-6)
    mu = h.act_raw.clone()
    # the draw: components 0-2 of the four-action kernel's for the same (seed, counter, env) -- that kernel on zero weights returns
    # its z.  sampled = fl(mu + fl(z sigma')), sigma' = the kernel's expf(log_std); recomputed here as fl(fl(sampled - mu) / sigma),
    # sigma = torch's exp.  Relative to |z|: the two exponentials 2^-23 each, the product, the difference and the quotient 2^-24
    # each; the sum 2^-24 (|z| + |mu| / sigma).  Together |recomputed - z| <= 8 * 2^-24 (|z| + 1) where |mu| / sigma < 1.
    z4, ae4 = torch.zeros((n, 4), device=dev), torch.zeros((n, 4), device=dev)
    lp4 = torch.zeros(n, device=dev)
    zero = torch.zeros(L.fw_ppo_param_count_a(30, 4), device=dev)
    _lib.check(L.fw_policy_act_a(R._p(zero), R._p(obs_n), n, 30, 4, 1, 0, R._p(rng), 512, None, R._p(z4), R._p(ae4), 0, R._p(lp4), None, None))
    torch.cuda.synchronize()
    sigma = pol.log_std.detach().exp()
    assert float((mu.abs() / sigma).max()) < 1.0
    z = (sampled - mu) / sigma
    assert bool(((z - z4[:, :3]).abs() <= 8 * 2.0 ** -24 * (z4[:, :3].abs() + 1.0)).all())
    assert float(z4[:, :3].abs().max()) > 1.0

    # ---- a NaN head bias for one component: every row is rejected and keeps the command it holds ----
    env.set_state(state1)
    bad = pol
    with torch.no_grad():
        bad.action_net.bias[1] = float("nan")
    flat_bad = _flat(bad, 30)
    h.rejected.zero_()
    h.run(h.args(flat_bad, mean, var, rng))
    assert torch.isnan(h.act_raw[:, 1]).all() and torch.isfinite(h.act_raw[:, [0, 2]]).all()
    assert int(h.rejected.item()) == n
    state2 = env.get_state()
    np.testing.assert_array_equal(state2, state1)
    env.set_state(state1)
    low_obs, cmd, act_env, rej = _chain(env, h.act_raw, low_flat, h.low_mean, h.low_var)
    assert rej == n
    assert torch.equal(h.cmd, cmd) and torch.equal(h.low_obs, low_obs) and torch.equal(h.act_env, act_env)
    np.testing.assert_array_equal(h.cmd.double().cpu().numpy(), state1[:, TAIL:TAIL + 3])
    assert torch.isfinite(h.act_env).all()

    # ---- nets = 2: the closing call of a rollout touches nothing of the policy side ----
    before = [x.clone() for x in (h.act_raw, h.logp, h.low_obs, h.cmd, h.act_env, h.obs_copy)]
    h.value.fill_(-7.0)
    h.run(h.args(flat, mean, var, rng, nets=2, prev=(rew, term, trunc, tobs, ret_var)))
    torch.testing.assert_close(h.value, v_t, rtol=1e-5, atol=2e-6)
    for x, y in zip(before, (h.act_raw, h.logp, h.low_obs, h.cmd, h.act_env, h.obs_copy)):
        assert _same_words(x, y)
    np.testing.assert_array_equal(env.get_state(), state1)
    env.close()


def test_collect_act_hl_refuses_other_tasks_the_quaternion_attitude_and_missing_pointers():
    L = _lib.lib()
    for env in (P.FixedwingWaypointsVecEnv(8, angle_representation="euler"), P.FixedwingLowLevelVecEnv(8),
                P.FixedwingWaypointsDirectVecEnv(8, angle_representation="quaternion")):
        env.reset_tensor()
        a = K.FwCollectHlArgs()
        rc = L.fw_collect_act_hl(env._h, C.byref(a), None)
        assert rc == K.FW_EUNSUPPORTED
        with pytest.raises(RuntimeError, match="fw_collect_act_hl"):
            _lib.check(rc, env._h)
        env.close()
    env = _flown_env(16, "float64")
    pol, ctl = _commander(), _controller()
    h = _Hl(env, _flat(ctl[0].cuda(), 21), ctl[1], ctl[2])
    mean, var = torch.zeros(30, dtype=torch.float64, device="cuda"), torch.ones(30, dtype=torch.float64, device="cuda")
    rng = torch.tensor([1, 2], dtype=torch.int64, device="cuda")
    flat = _flat(pol, 30)
    for field in ("params", "low_params", "obs", "obs_mean", "low_var", "act_raw", "logp", "value", "low_obs", "cmd_out", "act_env", "rng"):
        a = h.args(flat, mean, var, rng)
        setattr(a, field, None)
        assert L.fw_collect_act_hl(env._h, C.byref(a), None) == K.FW_EINVAL, field
    a = h.args(flat, mean, var, rng)
    a.nets = 0
    assert L.fw_collect_act_hl(env._h, C.byref(a), None) == K.FW_EINVAL
    a = h.args(flat, mean, var, rng, nets=1)
    a.prev_reward = env.rewards.data_ptr()                 # a previous step without the value block and its buffers
    assert L.fw_collect_act_hl(env._h, C.byref(a), None) == K.FW_EINVAL
    with pytest.raises(ValueError, match="fw_collect_act_hl"):
        _lib.check(K.FW_EINVAL, env._h)
    a = h.args(flat, mean, var, rng)                       # rejected and obs_copy are optional
    a.rejected = a.obs_copy = None
    assert L.fw_collect_act_hl(env._h, C.byref(a), None) == K.FW_OK
    torch.cuda.synchronize()
    env.close()


# ------------------------------------------------------------------------------------------------------------------ PPO
def _hl_ppo(fused=True, graphs=False, seed=123, n_steps=64):
    pol, mean, var = _controller()
    venv = HighLevelCmdVecEnv(16, pol, (mean, var), seed=seed)
    env = R.VecNormalizeDevice(venv, norm_obs=True, norm_reward=True, clip_obs=10.0, gamma=0.995)
    return R.PPO(env, R.PPOConfig(n_steps=n_steps, batch_size=256, n_epochs=2, gamma=0.995, seed=seed, use_graphs=graphs,
                                  fused_three_actions=fused))


def test_ppo_collects_and_learns_on_the_fused_three_action_paths():
    a = _hl_ppo()
    venv = a.env.venv
    assert a.act_dim == 3 and a._collect_fused and not a._one_launch and not a._close_gae
    assert a._fused is not None and a._fused.A == 3
    assert R.FusedPpoUpdate.applies(a.policy, a.cfg, a.env.obs_dim, 256, a.device)
    a.collect_rollouts()                                 # (the first: it resets the env)
    counts = float(a.env.obs_rms.count.item()), float(a.env.ret_rms.count.item())
    a.collect_rollouts()
    torch.cuda.synchronize()
    with torch.no_grad():
        v, lp, _ = a.policy.evaluate_actions(a.buf_obs.reshape(-1, 30), a.buf_act.reshape(-1, 3))
    torch.testing.assert_close(v, a.buf_val.reshape(-1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lp, a.buf_logp.reshape(-1), rtol=1e-5, atol=2e-4)
    assert float(a.env.obs_rms.count.item()) - counts[0] == pytest.approx(64 * 16) == float(a.env.ret_rms.count.item()) - counts[1]      # a batch per vec-step
    a.train()
    a.learn(2 * 64 * 16)
    torch.cuda.synchronize()
    assert a.num_timesteps == 2 * 64 * 16
    assert all(math.isfinite(x) for x in a.logs.values()), a.logs
    for name in ("buf_obs", "buf_act", "buf_val", "buf_rew", "buf_logp", "adv", "ret"):
        assert torch.isfinite(getattr(a, name)).all(), name
    assert all(torch.isfinite(q).all() for q in a.policy.parameters())
    # the command the env holds is the conditioned one of the last sampled action, inside the conditioned Box
    c = venv.command.double().cpu().numpy()
    assert (c[:, 0] >= -math.pi).all() and (c[:, 0] < math.pi).all()
    assert (c[:, 1] >= 0.0).all() and (c[:, 1] <= 200.0).all() and (c[:, 2] >= 0.0).all() and (c[:, 2] <= 30.0).all()
    from pyflyt_drone_amd.highlevel import condition_command
    np.testing.assert_array_equal(c, condition_command(a.buf_act[-1].double().cpu().numpy(), 200.0))
    np.testing.assert_array_equal(venv.low_obs[:, 18:21].double().cpu().numpy(), c)
    assert (venv.low_action.abs() <= 1.0).all() and int(venv.rejected.item()) == 0
    venv.close()


def test_graph_replayed_rollouts_equal_eager_ones_bit_for_bit():
    a, b = _hl_ppo(graphs=True, n_steps=32), _hl_ppo(graphs=False, n_steps=32)
    for _ in range(3):                                   # eager, capture, replay
        a.collect_rollouts(); b.collect_rollouts()
    torch.cuda.synchronize()
    assert a._g_rollout is not None and b._g_rollout is None
    for x, y in ((a.env.obs_rms, b.env.obs_rms), (a.env.ret_rms, b.env.ret_rms)):
        assert float(x.count.item()) == float(y.count.item())
        assert torch.equal(x.mean, y.mean) and torch.equal(x.var, y.var)
    for name in ("buf_act", "buf_obs", "buf_logp", "buf_val", "buf_rew", "buf_start", "last_values", "last_obs"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    va, vb = a.env.venv, b.env.venv
    for name in ("obs", "rewards", "terminated", "truncated", "low_action", "command", "low_obs", "rejected"):
        assert torch.equal(getattr(va, name), getattr(vb, name)), name
    np.testing.assert_array_equal(va.get_state(), vb.get_state())
    va.close(); vb.close()


def _state(ppo):
    opt = ppo.optimizer
    mods = {k: v.detach().clone() for k, v in ppo.policy.state_dict().items()}
    mom = [(float(opt.state[p]["step"]), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ppo.policy.parameters()]
    rms = [t.clone() for r in (ppo.env.obs_rms, ppo.env.ret_rms) for t in (r.mean, r.var, r.count)]
    return mods, mom, rms


@pytest.mark.parametrize("saved_fused", [True, False])
def test_checkpoints_are_interchangeable_across_the_flag(tmp_path, saved_fused):
    a = _hl_ppo(fused=saved_fused, n_steps=32)
    a.learn(32 * 16)
    path = checkpoint.save(str(tmp_path / "x.pt"), a)
    want = _state(a)
    b = _hl_ppo(fused=not saved_fused, n_steps=32)
    checkpoint.load(path, b, reset_num_timesteps=False, restore_env_state=True)
    got = _state(b)
    for k in want[0]:
        assert torch.equal(want[0][k], got[0][k]), k
    for (s0, m0, v0), (s1, m1, v1) in zip(want[1], got[1]):
        assert s0 == s1 and torch.equal(m0, m1) and torch.equal(v0, v1)
    for x, y in zip(want[2], got[2]):
        assert torch.equal(x, y)
    np.testing.assert_array_equal(a.env.venv.get_state(), b.env.venv.get_state())
    b.learn(32 * 16, reset_num_timesteps=False)            # and the other path trains on from there
    assert all(torch.isfinite(p).all() for p in b.policy.parameters())
    a.env.venv.close(); b.env.venv.close()
