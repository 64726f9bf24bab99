"""Commanding the low-level controller on the GPU ("Commanding the controller"): fw_command_ll against the host
state round trip it replaces, its conditioning and refusals, the reward and infos that follow a command, what an auto-reset does to
it, fw_trace_ll against a torch restatement, and command.fly (graph-replayed against eager, fused against torch)."""
import math

import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import command as CMD
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R

pytestmark = pytest.mark.gpu

TGT = K.S_TASK + K.SL_TARGET          # the target's columns in a state record


@pytest.fixture(params=[1, 8], ids=["lane_per_env", "8_lanes_per_env"])
def lanes(request, monkeypatch):
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", str(request.param))
    return request.param


def _venv(n=16, dtype="float64", steps=2000, seed=5):
    return P.FixedwingVecEnv(K.lowlevel_config(dtype=dtype, max_episode_steps=steps, motor_noise=True), n, seed=seed)


def _condition(cmd, dome=100.0):
    """train/train_highlevel_cmd.py:164-166 in numpy: (psi + pi) % 2 pi - pi, clip(h, 0, dome), clip(V, 0, 100)"""
    c = np.array(cmd, dtype=np.float64)
    return np.stack([(c[:, 0] + np.pi) % (2 * np.pi) - np.pi, np.clip(c[:, 1], 0.0, dome), np.clip(c[:, 2], 0.0, 100.0)], axis=1)


def _commands(n, seed=0):
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-7.0, 7.0, n), rng.uniform(-10.0, 120.0, n), rng.uniform(-5.0, 130.0, n)], axis=1)
    c[0] = (4.0, 12.0, 15.0)
    return c


def _actions(n, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n, 6), generator=g, dtype=torch.float64) * 2 - 1).to(device="cuda", dtype=dtype)


def _np_dtype(venv):
    return np.float64 if venv.torch_dtype == torch.float64 else np.float32


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_command_equals_the_state_round_trip(dtype, lanes):
    """env A: fw_command_ll.  env B (same seed): get_state -> conditioned targets into the tail -> set_state -> observe.  Same obs;
    after the same action the same obs, reward, flags and state, bit for bit (motor noise on)."""
    n = 16
    a, b = _venv(n, dtype), _venv(n, dtype)
    assert a.lanes_per_env == lanes
    a.reset_tensor(); b.reset_tensor()
    for k in range(3):
        act = _actions(n, k, a.torch_dtype)
        a.step_tensor(act); b.step_tensor(act)
    # fw_step's observation row and fw_observe's can differ in the last bit of the yaw (a different inlining of the same Euler
    # conversion): refresh A's row with fw_observe too, so that the comparison below sees only what the command writes
    a.observe_tensor()
    cmd = _commands(n)
    assert a.command(cmd) == 0
    s = b.get_state()
    s[:, TGT:TGT + 3] = _condition(cmd).astype(_np_dtype(b))
    b.set_state(s)
    b.observe_tensor()
    assert torch.equal(a.obs, b.obs)
    np.testing.assert_array_equal(a.obs[:, 18:21].cpu().numpy(), _condition(cmd).astype(_np_dtype(a)))
    for k in range(3, 6):
        act = _actions(n, k, a.torch_dtype)
        a.step_tensor(act); b.step_tensor(act)
        for name in ("obs", "rewards", "terminated", "truncated", "terminal_obs"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (name, k)
        np.testing.assert_array_equal(a.get_state(), b.get_state())


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_conditioning_mask_and_rejected_rows(dtype, lanes):
    n = 8
    env = _venv(n, dtype)
    env.reset_tensor()
    before = env.obs.clone()
    s0 = env.get_state()
    cmd = np.array([[4.0, 10.0, 15.0], [0.5, -5.0, 12.0], [0.5, 500.0, 150.0], [math.nan, 10.0, 15.0],
                    [-4.0, 50.0, -3.0], [0.0, 10.0, math.inf], [1.0, 11.0, 16.0], [2.0, 12.0, 17.0]])
    mask = np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.uint8)
    assert env.command(cmd, mask=mask) == 2                     # the NaN row and the inf row
    o, s1 = env.obs.cpu().numpy(), env.get_state()
    dt = _np_dtype(env)
    assert o[0, 18] == pytest.approx(4.0 - 2 * math.pi, abs=1e-6)
    assert o[1, 19] == 0.0 and o[2, 19] == 100.0 and o[2, 20] == 100.0 and o[4, 20] == 0.0
    assert o[4, 18] == pytest.approx(2 * math.pi - 4.0, abs=1e-6)
    want = _condition(cmd[[0, 1, 2, 4, 7]]).astype(dt)
    np.testing.assert_array_equal(o[[0, 1, 2, 4, 7], 18:21], want)
    np.testing.assert_array_equal(s1[[0, 1, 2, 4, 7], TGT:TGT + 3], want.astype(np.float64))
    for i in (3, 5, 6):                                         # rejected and unmasked rows: untouched, bit for bit
        assert torch.equal(env.obs[i], before[i])
        np.testing.assert_array_equal(s1[i], s0[i])
    # everything but the target columns of the commanded rows is as it was
    keep = np.ones_like(s0, dtype=bool)
    keep[np.ix_([0, 1, 2, 4, 7], range(TGT, TGT + 3))] = False
    np.testing.assert_array_equal(s1[keep], s0[keep])
    assert torch.equal(env.obs[:, :18], before[:, :18])
    # [3] broadcasts to every env; without obs (command_tensor with a schedule row picked by step_idx) only the tail moves
    assert env.command((0.25, 20.0, 18.0)) == 0
    np.testing.assert_array_equal(env.obs[:, 18:21].cpu().numpy(), np.tile(np.array([0.25, 20.0, 18.0], dtype=dt), (n, 1)))
    sched = CMD.step_schedule([(1, (0.1, 11.0, 13.0)), (1, (0.2, 12.0, 14.0))], n, "cuda")
    idx = torch.full((), 7, dtype=torch.int64, device="cuda")              # past the end: the last row
    rc = _lib.lib().fw_command_ll(env._h, sched.data_ptr(), 2, idx.data_ptr(), None, None, None, None)
    assert rc == K.FW_OK
    torch.cuda.synchronize()
    assert int(idx.item()) == 7                                 # only read
    want = _condition(np.tile([0.2, 12.0, 14.0], (n, 1))).astype(dt).astype(np.float64)         # (the wrap moves 0.2 by an ulp)
    np.testing.assert_array_equal(env.get_state()[:, TGT:TGT + 3], want)
    np.testing.assert_array_equal(env.obs[:, 18:21].cpu().numpy(), np.tile(np.array([0.25, 20.0, 18.0], dtype=dt), (n, 1)))


def _reward(o, cmd, term):
    """fixedwing_lowlevel_env.py:118-134 restated from the post-step observation and the (conditioned) command"""
    psi, z = o[:, 5], o[:, 11]
    v = np.linalg.norm(o[:, 6:9], axis=1)
    e_psi = (cmd[:, 0] - psi + np.pi) % (2 * np.pi) - np.pi
    r = -(np.abs(e_psi) + np.abs(cmd[:, 1] - z) + 0.5 * np.abs(cmd[:, 2] - v)) + 0.1
    return r - 100.0 * term


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_the_next_reward_and_infos_use_the_command(dtype):
    n = 16
    env = P.FixedwingLowLevelVecEnv(num_envs=n, dtype=dtype, seed=3)
    env.reset()
    cmd = _commands(n, seed=1)
    env.command(cmd)
    c = _condition(cmd).astype(_np_dtype(env)).astype(np.float64)
    rng = np.random.default_rng(0)
    for k in range(4):
        obs, rew, dones, infos = env.step(rng.uniform(-1, 1, (n, 6)))
        assert not dones.any()
        tol = dict(rtol=1e-12, atol=1e-9) if dtype == "float64" else dict(rtol=1e-5, atol=1e-3)
        np.testing.assert_allclose(rew, _reward(obs.astype(np.float64), c, 0.0), **tol)
        for i in range(n):
            np.testing.assert_array_equal(infos[i]["target"], c[i])
    # against an uncommanded twin the reward moved, the dynamics did not
    twin = P.FixedwingLowLevelVecEnv(num_envs=n, dtype=dtype, seed=3)
    twin.reset()
    rng = np.random.default_rng(0)
    for k in range(4):
        o2, r2, _, _ = twin.step(rng.uniform(-1, 1, (n, 6)))
    np.testing.assert_array_equal(obs[:, :18], o2[:, :18])
    assert not np.array_equal(rew, r2)


def test_auto_reset_draws_the_random_target_and_the_next_command_replaces_it(lanes):
    """max_episode_steps 5: every env truncates at step 5.  The reset row carries the random draw (as an uncommanded twin's),
    the terminal row the command; the next fw_command_ll puts the command back before the act, so no trace row shows the draw."""
    n, T = 16, 12
    a, b = _venv(n, steps=5), _venv(n, steps=5)
    a.reset_tensor(); b.reset_tensor()
    sched = CMD.step_schedule([(T, _commands(n, seed=2))], n, "cuda")
    c = _condition(_commands(n, seed=2))
    idx = torch.zeros((), dtype=torch.int64, device="cuda")
    trace = torch.zeros((T, n, 8), dtype=torch.float64, device="cuda")
    for k in range(T):
        a.command_tensor(sched, T, idx)
        np.testing.assert_array_equal(a.obs[:, 18:21].cpu().numpy(), c)          # what the act sees
        act = _actions(n, k, a.torch_dtype)
        a.step_tensor(act); b.step_tensor(act)
        assert _lib.lib().fw_trace_ll(a.obs.data_ptr(), a.terminal_obs.data_ptr(), a.terminated.data_ptr(), a.truncated.data_ptr(), 1, n,
                                      trace.data_ptr(), T, idx.data_ptr(), None) == K.FW_OK
        done = (a.truncated | a.terminated).bool()
        if k in (4, 9):
            assert bool(a.truncated.all())
            assert torch.equal(a.obs, b.obs)                                      # the new episode: random draw, unchanged
            assert not np.array_equal(a.obs[:, 18:21].cpu().numpy(), c)
            np.testing.assert_array_equal(a.terminal_obs[:, 18:21].cpu().numpy(), c)
        else:
            assert not bool(done.any())
    tr = trace.cpu().numpy()
    for j in range(3):
        np.testing.assert_array_equal(tr[:, :, 2 * j], np.broadcast_to(c[:, j], (T, n)))
    ends = np.isin(np.arange(T), (4, 9))
    assert (tr[ends, :, 7] == CMD.FLAG_TRUNCATED).all() and (tr[~ends, :, 7] == 0).all()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_trace_kernel_against_a_torch_restatement(dtype):
    n, T = 40, 3
    env = _venv(n, dtype, steps=60)
    env.reset_tensor()
    L = _lib.lib()
    trace = torch.full((T + 2, n, 8), -7.0, dtype=torch.float64, device="cuda")      # two rows behind T: must stay untouched
    idx = torch.zeros((), dtype=torch.int64, device="cuda")
    is64 = int(env.obs.dtype == torch.float64)
    want = []
    torch.manual_seed(0)
    for k in range(T + 2):
        env.step_tensor(torch.rand((n, 6), device="cuda", dtype=env.torch_dtype) * 2 - 1)
        if k == 1:                                              # some terminated and some truncated rows
            env.terminated[::3] = 1
            env.truncated[1::3] = 1
            env.terminal_obs.copy_(env.obs * 1.5 + 0.25)
        assert L.fw_trace_ll(env.obs.data_ptr(), env.terminal_obs.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr(), is64, n,
                             trace.data_ptr(), T, idx.data_ptr(), None) == K.FW_OK
        te, tr = env.terminated.bool(), env.truncated.bool()
        o = torch.where((te | tr)[:, None], env.terminal_obs, env.obs).to(torch.float64)
        v = torch.sqrt(o[:, 6] * o[:, 6] + o[:, 7] * o[:, 7] + o[:, 8] * o[:, 8])
        w = torch.sqrt(o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] + o[:, 2] * o[:, 2])
        flag = torch.where(te, 1.0, torch.where(tr, 2.0, 0.0)).to(torch.float64)
        want.append(torch.stack([o[:, 18], o[:, 5], o[:, 19], o[:, 11], o[:, 20], v, w, flag], dim=1))
        torch.cuda.synchronize()
        assert int(idx.item()) == k + 1
    got = trace.cpu()
    for k in range(T):
        assert torch.equal(got[k], want[k].cpu()), k
    assert (got[T:] == -7.0).all()
    assert (got[1, ::3, 7] == 1).all() and (got[1, 1::3, 7] == 2).all() and (got[1, 2::3, 7] == 0).all()


class LinearPolicy(torch.nn.Module):
    """a six-action "policy" whose mean action is a fixed linear map of the normalised observation"""

    def __init__(self, obs_dim, scale):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.W = torch.nn.Parameter((torch.rand((6, obs_dim), generator=g) - 0.5) * scale)
        self.b = torch.nn.Parameter(torch.linspace(-0.2, 0.3, 6))

    def forward(self, obs, deterministic=True, generator=None):
        return obs @ self.W.t() + self.b, None, None


def _env(n, steps=300, seed=6, dtype="float64"):
    env = R.VecNormalizeDevice(_venv(n, dtype, steps=steps, seed=seed), training=False, norm_reward=False)
    with torch.no_grad():                                      # statistics as after some training: not the identity
        env.obs_rms.mean.copy_(torch.linspace(-0.2, 0.3, env.obs_dim, dtype=torch.float64, device="cuda"))
        env.obs_rms.var.copy_(torch.linspace(0.5, 2.0, env.obs_dim, dtype=torch.float64, device="cuda"))
    return env


SCHEDULE = [(13, (0.0, 10.0, 15.0)), (20, (1.2, 14.0, 17.0)), (14, (-1.0, 9.0, 13.0))]      # T = 47: not a multiple of 8


@pytest.mark.parametrize("kind", ["linear", "zero"])
def test_fly_replayed_equals_eager(kind, lanes):
    n = 24
    outs = []
    for gs in (0, 8):
        env = _env(n)
        pol = LinearPolicy(env.obs_dim, 2.0 if kind == "linear" else 0.0).cuda()
        sched = CMD.step_schedule(SCHEDULE, n)
        outs.append(CMD.fly(pol, env, sched, graph_steps=gs))
    a, b = outs
    assert a.trace.shape == (47, n, 8) and a.dt == 1.0 / 120.0
    np.testing.assert_array_equal(a.trace, b.trace)
    np.testing.assert_array_equal(a.start, b.start)
    np.testing.assert_array_equal(a.ended_at, b.ended_at)
    # every row, the ending one included, carries the commanded value, never an auto-reset's draw
    c = np.concatenate([np.broadcast_to(_condition(np.tile(v, (n, 1))), (s, n, 3)) for s, v in SCHEDULE])
    for j in range(3):
        np.testing.assert_array_equal(a.trace[:, :, 2 * j], c[:, :, j])
    assert np.isin(a.trace[:, :, 7], (0, 1)).all()
    fig = CMD.response_figures(a)
    assert set(fig["summary"]) >= {"heading_t90", "altitude_overshoot", "airspeed_settling", "heading_ss_error", "altitude_mae",
                                   "airspeed_rmse", "survival_rate"}
    assert fig["summary"]["survival_rate"] == np.mean(a.ended_at < 0)
    assert fig["summary"]["heading_steps"] > 0


def test_fly_fused_matches_torch(lanes):
    """use_fused=True (fw_collect_act_a, fp32 MFMA forward) against the torch forward: the same run to the tolerance of the
    six-action act tests -- the same envs end at the same steps, the traces agree to ~1e-4 before that"""
    n = 24
    outs = []
    for fused in (None, True):
        env = _env(n, steps=300)
        torch.manual_seed(0)
        pol = R.MlpPolicy(env.obs_dim, env.act_dim).cuda()
        with torch.no_grad():
            pol.action_net.weight.mul_(30.0)
        outs.append(CMD.fly(pol, env, CMD.step_schedule(SCHEDULE * 2, n), use_fused=fused))
    a, b = outs
    same = a.ended_at == b.ended_at
    assert same.sum() >= n - 2, (a.ended_at, b.ended_at)
    for i in np.nonzero(same)[0]:
        end = a.trace.shape[0] if a.ended_at[i] < 0 else a.ended_at[i] + 1
        np.testing.assert_allclose(b.trace[:end, i], a.trace[:end, i], rtol=1e-4, atol=1e-4, err_msg=str(i))
    with pytest.raises(ValueError):
        CMD.fly(LinearPolicy(21, 1.0).cuda(), _env(n), CMD.step_schedule(SCHEDULE, n), use_fused=True)


def test_refusals():
    L = _lib.lib()
    n = 8
    wp = P.FixedwingVecEnv(K.train_waypoints_v3_config(), n, seed=0)
    cmd = torch.zeros((1, n, 3), dtype=torch.float64, device="cuda")
    assert L.fw_command_ll(wp._h, cmd.data_ptr(), 1, None, None, None, None, None) == K.FW_EUNSUPPORTED
    assert "low-level" in L.fw_last_error(wp._h).decode()
    with pytest.raises(RuntimeError):
        _lib.check(L.fw_command_ll(wp._h, cmd.data_ptr(), 1, None, None, None, None, None), wp._h)
    ll = _venv(n)
    assert L.fw_command_ll(ll._h, None, 1, None, None, None, None, None) == K.FW_EINVAL
    assert L.fw_command_ll(ll._h, cmd.data_ptr(), 0, None, None, None, None, None) == K.FW_EINVAL
    assert "T must be positive" in L.fw_last_error(ll._h).decode()
    assert L.fw_command_ll(None, cmd.data_ptr(), 1, None, None, None, None, None) == K.FW_EINVAL
    assert L.fw_command_ll(ll._h, cmd.data_ptr(), 1, None, None, None, None, None) == K.FW_OK

    obs = torch.zeros((n, 21), dtype=torch.float64, device="cuda")
    trace = torch.zeros((2, n, 8), dtype=torch.float64, device="cuda")
    idx = torch.zeros((), dtype=torch.int64, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()            # noqa: E731

    def tr(obs_=obs, trace_=trace, idx_=idx, N=n, T=2):
        return L.fw_trace_ll(p(obs_), None, None, None, 1, N, p(trace_), T, p(idx_), None)
    assert tr(trace_=None) == K.FW_EINVAL and tr(idx_=None) == K.FW_EINVAL and tr(obs_=None) == K.FW_EINVAL
    assert tr(N=0) == K.FW_EINVAL and tr(T=0) == K.FW_EINVAL
    assert "must be positive" in L.fw_last_error(None).decode()
    assert tr() == K.FW_OK                                      # no flags / terminal rows: every row running, read from obs
    torch.cuda.synchronize()
    assert int(idx.item()) == 1 and not trace[0].any() and not trace[1].any()
    with pytest.raises(ValueError):
        ll.command(np.zeros((n, 4)))
