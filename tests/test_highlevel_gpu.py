"""The high-level command task on the GPU (train/train_highlevel_cmd.py:35-181), piece by piece:

1. the base env (the waypoints task under six direct actuator commands) against the CPU oracle's waypoints task behind a routing
   mixer: whole task, auto-resets included, in lockstep;
2. ``fw_command_hl`` against the numpy ``condition_command``, bit for bit;
3. the composed vec-step against a composition of independent pieces (numpy conditioning and normalisation, the torch forward of
   the controller, a second handle of the base env);
4. hipGraph replay of ``step_tensor`` against the eager loop;
5. the learner's plumbing (three-action policy on the torch path, the action Box; the six-action base env on the fused learner);
6. evaluation and checkpoints.
"""
import itertools
import math

import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib, checkpoint, evaluate
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R
from pyflyt_drone_amd.highlevel import HighLevelCmdVecEnv, condition_command
from helpers import as_oracle_obs as _as_oracle_obs, route as _route, seeded_actions, set_routing_mixer
from oracle import fw_oracle as O

pytestmark = pytest.mark.gpu

TAIL = K.S_TASK
CONST_RANDOM = dict(enabled=True, mode="constant", randomize_on_reset=True,
                    wind_enu_mps_range=[[-3.0, 3.0], [-3.0, 3.0], [-0.5, 0.5]])
GUST_RANDOM = dict(enabled=True, mode="gust_sine", randomize_on_reset=True, randomize_gust_phase=True, gust_freq_hz=0.7,
                   wind_enu_mps_range=[[-2.0, 2.0], [-2.0, 2.0], [0.0, 0.0]], gust_amp_enu_mps_range=[[0.0, 3.0], [0.0, 3.0], [0.0, 1.0]])
WINDS = {"no_wind": None, "constant": CONST_RANDOM, "gust": GUST_RANDOM}
BASE_KW = dict(flight_dome_size=200.0, max_duration_seconds=120.0, agent_hz=30, context_length=2, angle_representation="euler")
TRIPLES = list(itertools.combinations(range(5), 3))


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    O.build()


@pytest.fixture(params=[1, 8], ids=["lane_per_env", "8_lanes_per_env"])
def lanes(request, monkeypatch):
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", str(request.param))
    return request.param


def _routed_pair(triple, **kw):
    """(direct-command config, oracle config): the oracle's mode-0 mixer routes action components 0-2 to the three surfaces of
    `triple` and component 3 to the throttle, so it sees the actuator commands the direct kernel gets in those slots."""
    wd = K.waypoints_direct_config(**BASE_KW, **kw)
    kw.pop("dtype", None)
    wp = K.waypoints_config(**BASE_KW, **kw)
    return wd, set_routing_mixer(wp, triple)


# ------------------------------------------------------------------------------------------------ 1. the base env
@pytest.mark.parametrize("triple", TRIPLES, ids=["s" + "".join(map(str, t)) for t in TRIPLES])
def test_base_env_matches_the_oracle_through_a_routing_mixer(triple, lanes):
    wind = list(WINDS)[TRIPLES.index(triple) % 3]
    n, steps, seed = 199, 240, 11
    wd, wp = _routed_pair(triple, wind_config=WINDS[wind])
    assert wp.motor.noise_ratio > 0 and wd.motor.noise_ratio > 0
    env = P.FixedwingVecEnv(wd, n, seed=seed)
    assert env.lanes_per_env == lanes and env.obs_dim == 30 and env.act_dim == 6
    ora = O.OracleEnv(wp, n, seed=seed)
    tol = dict(rtol=0, atol=1e-7)
    oh, oo = env.reset_tensor().cpu().numpy(), ora.reset()
    np.testing.assert_allclose(_as_oracle_obs(oh), np.concatenate([oo[:, 0:12], oo[:, 16:28]], axis=1), **tol)
    assert not oh[:, 12:18].any()
    keep = np.ones(K.FW_STATE_DIM, dtype=bool)
    keep[K.S_ACTION:K.S_ACTION + 4] = False                # the oracle fills it with its four actions
    keep[TAIL:] = False                                    # the task tail: the oracle leaves it zero
    rng = np.random.default_rng(5)
    dones = 0
    worst = dict(obs=0.0, rew=0.0, state=0.0)
    for t in range(steps):
        a4 = rng.uniform(-1, 1, size=(n, 4))
        a6 = _route(a4, triple)
        o_obs, o_rew, o_term, o_trunc, o_tobs, o_info = ora.step(a4)
        env.step_tensor(torch.as_tensor(a6, device=env.device))
        tag = f"{wind}, step {t}"
        h_obs, h_tobs = env.obs.cpu().numpy(), env.terminal_obs.cpu().numpy()
        assert np.array_equal(env.terminated.cpu().numpy(), o_term), tag
        assert np.array_equal(env.truncated.cpu().numpy(), o_trunc), tag
        assert np.array_equal(env.info.cpu().numpy(), o_info), tag
        done = (o_term | o_trunc).astype(bool)
        o_map = np.concatenate([o_obs[:, 0:12], o_obs[:, 16:28]], axis=1)
        worst["obs"] = max(worst["obs"], float(np.abs(_as_oracle_obs(h_obs) - o_map).max()))
        worst["rew"] = max(worst["rew"], float(np.abs(env.rewards.cpu().numpy() - o_rew).max()))
        np.testing.assert_allclose(_as_oracle_obs(h_obs), o_map, err_msg=f"obs {tag}", **tol)
        np.testing.assert_allclose(env.rewards.cpu().numpy(), o_rew, err_msg=f"reward {tag}", **tol)
        np.testing.assert_array_equal(h_obs[~done, 12:18], a6[~done])          # the six commands just given ...
        assert not h_obs[done, 12:18].any()                                    # ... zeros after an auto-reset
        if done.any():
            t_map = np.concatenate([o_tobs[done][:, 0:12], o_tobs[done][:, 16:28]], axis=1)
            np.testing.assert_allclose(_as_oracle_obs(h_tobs[done]), t_map, err_msg=f"terminal obs {tag}", **tol)
            np.testing.assert_array_equal(h_tobs[done, 12:18], a6[done])
        sh, so = env.get_state(), ora.get_state()
        worst["state"] = max(worst["state"], float(np.abs(sh[:, keep] - so[:, keep]).max()))
        np.testing.assert_allclose(sh[:, keep], so[:, keep], err_msg=f"state {tag}", **tol)
        np.testing.assert_array_equal(sh[:, TAIL + K.SL_PREV_ACTION:TAIL + K.SL_PREV_ACTION + 6], np.where(done[:, None], 0.0, a6))
        dones += int(done.sum())
    print(f"triple {triple} {wind} lanes {lanes}: {dones} episode ends, worst |diff| {worst}")
    assert dones > 0
    c = env.get_counters()
    assert c["resets"] == dones == c["fallbacks"] and c["shadow_hits"] == 0 and c["scenario_hits"] == 0


@pytest.mark.parametrize("triple", [(0, 1, 2), (2, 3, 4)], ids=["s012", "s234"])
def test_base_env_f32_single_step_error(triple):
    """fp32 kernel vs the fp64 oracle from identical states: one agent step stays within 2e-3."""
    n = 512
    wd32, wp64 = _routed_pair(triple, motor_noise=False, dtype="float32")
    ora = O.OracleEnv(wp64, n, seed=3); ora.reset()
    rng = np.random.default_rng(4)
    for _ in range(20):
        _, _, te, tr, _, _ = ora.step(seeded_actions(rng, n, "gentle"))
    hip = P.FixedwingVecEnv(wd32, n, seed=3); hip.reset_tensor()
    hip.set_state(ora.get_state())
    ora.set_state(hip.get_state())                       # start both from the float32-rounded state
    a4 = seeded_actions(rng, n, "gentle").astype(np.float32)
    oo, ro, te, tr, _, _ = ora.step(a4.astype(np.float64))
    hip.step_tensor(torch.as_tensor(_route(a4, triple), device=hip.device))
    same = (hip.terminated.cpu().numpy() == te) & (hip.truncated.cpu().numpy() == tr) & ~(te | tr).astype(bool)
    print(f"triple {triple}: flags agree and the env did not end in {same.mean():.4f} of the envs")
    assert same.mean() > 0.97
    ho = hip.obs.cpu().numpy().astype(np.float64)
    err = np.abs(_as_oracle_obs(ho) - np.concatenate([oo[:, 0:12], oo[:, 16:28]], axis=1))[same]
    print(f"triple {triple}: worst observation error {err.max():.3e}")
    assert err.max() < 2e-3, err.max()
    q = hip.get_state()[:, K.S_QUAT:K.S_QUAT + 4]
    np.testing.assert_allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 2. fw_command_hl
def _command_hl(env, action, mask=None, low_obs=None, cmd_out=None, rejected=None):
    n = env.num_envs
    low_obs = torch.full((n, 21), -7.0, dtype=env.torch_dtype, device=env.device) if low_obs is None else low_obs
    cmd_out = torch.full((n, 3), -7.0, dtype=env.torch_dtype, device=env.device) if cmd_out is None else cmd_out
    rejected = torch.zeros(1, dtype=torch.int32, device=env.device) if rejected is None else rejected
    rc = _lib.lib().fw_command_hl(env._h, R._p(action), int(action.dtype == torch.float64), R._p(mask), R._p(env.obs), R._p(low_obs),
                                  R._p(cmd_out), R._p(rejected), None)
    _lib.check(rc, env._h)
    torch.cuda.synchronize()
    return low_obs.cpu().numpy(), cmd_out.cpu().numpy(), int(rejected.item())


def _raw_actions(n, rng):
    """wide enough to hit every clip: several times outside the Box on both sides, inside it, and exactly +-pi"""
    a = np.stack([rng.uniform(-4 * math.pi, 4 * math.pi, n), rng.uniform(-300.0, 700.0, n), rng.uniform(-60.0, 150.0, n)], axis=1)
    a[0] = [math.pi, 200.0, 30.0]
    a[1] = [-math.pi, 0.0, 0.0]
    a[2] = [math.pi, 10.0, 100.0]
    a[3:40] = np.stack([rng.uniform(-math.pi, math.pi, 37), rng.uniform(0.0, 200.0, 37), rng.uniform(0.0, 30.0, 37)], axis=1)
    a[40] = [1e30, -1e30, 1e300]
    return a


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_command_hl_against_the_numpy_statement(dtype, lanes):
    n, dome = 199, 200.0
    env = P.FixedwingWaypointsDirectVecEnv(n, **BASE_KW, dtype=dtype, seed=5)
    assert env.lanes_per_env == lanes
    env.reset_tensor()
    for _ in range(3):                                    # some flight: the shared observation columns are not the start pose
        env.step_tensor(torch.as_tensor(np.random.default_rng(1).uniform(-0.3, 0.3, (n, 6)), device=env.device, dtype=env.torch_dtype))
    obs = env.obs.cpu().numpy()
    st0 = env.get_state()
    np.testing.assert_array_equal(st0[:, TAIL:TAIL + 3], np.tile([0.0, 10.0, 20.0], (n, 1)))      # the command after a reset
    rng = np.random.default_rng(7)
    a = _raw_actions(n, rng)
    want = condition_command(a, dome)
    assert (want[:3, 0] == -math.pi).all() and (want[:, 0] >= -math.pi).all() and (want[:, 0] < math.pi).all()
    assert want[:, 1].min() == 0.0 and want[:, 1].max() == dome and want[:, 2].min() == 0.0 and want[:, 2].max() == 30.0
    want_t = want.astype(env.np_dtype)                    # f32: the double result, rounded once
    low, cmd, rej = _command_hl(env, torch.as_tensor(a, device=env.device))
    assert rej == 0
    np.testing.assert_array_equal(low[:, 0:18], obs[:, 0:18])
    np.testing.assert_array_equal(low[:, 18:21], want_t)
    np.testing.assert_array_equal(cmd, want_t)
    np.testing.assert_array_equal(env.get_state()[:, TAIL:TAIL + 3], want_t.astype(np.float64))
    np.testing.assert_array_equal(env.obs.cpu().numpy(), obs)                                      # only read
    if dtype == "float32":                                # the action as the policy hands it over (float32): conditioned in double
        a32 = a.astype(np.float32)
        low32, _, _ = _command_hl(env, torch.as_tensor(a32, device=env.device))
        np.testing.assert_array_equal(low32[:, 18:21], condition_command(a32.astype(np.float64), dome).astype(np.float32))
        _command_hl(env, torch.as_tensor(a, device=env.device))
    # masked rows are untouched (tail, low_obs, cmd_out); NaN / inf rows keep the previous command and are counted
    b = _raw_actions(n, np.random.default_rng(8))
    mask = (np.arange(n) % 3 != 0).astype(np.uint8)
    bad = np.zeros(n, dtype=bool)
    bad[[4, 5, 7, 100, 150]] = True
    b[4, 0], b[5, 1], b[7, 2], b[100], b[150, 0] = np.nan, np.inf, -np.inf, np.nan, np.inf
    low2, cmd2, rej2 = _command_hl(env, torch.as_tensor(b, device=env.device), mask=torch.as_tensor(mask, device=env.device))
    on = mask.astype(bool)
    assert rej2 == int((bad & on).sum()) > 0
    exp = np.where((on & ~bad)[:, None], condition_command(np.where(np.isfinite(b), b, 0.0), dome).astype(env.np_dtype), want_t)
    np.testing.assert_array_equal(env.get_state()[:, TAIL:TAIL + 3], exp.astype(np.float64))
    np.testing.assert_array_equal(low2[on, 18:21], exp[on])
    np.testing.assert_array_equal(low2[on, 0:18], obs[on, 0:18])
    np.testing.assert_array_equal(cmd2[on], exp[on])
    assert (low2[~on] == -7.0).all() and (cmd2[~on] == -7.0).all()
    # the six-wide action of the tail is not the command's business
    np.testing.assert_array_equal(env.get_state()[:, TAIL + 3:TAIL + 9], st0[:, TAIL + 3:TAIL + 9])
    env.close()


def test_command_hl_refuses_other_tasks_and_the_quaternion_attitude():
    a = torch.zeros((8, 3), dtype=torch.float64, device="cuda")
    for env in (P.FixedwingWaypointsVecEnv(8, angle_representation="euler"), P.FixedwingLowLevelVecEnv(8),
                P.FixedwingWaypointsDirectVecEnv(8, angle_representation="quaternion")):
        env.reset_tensor()
        low = torch.zeros((8, 21), dtype=torch.float64, device=env.device)
        rc = _lib.lib().fw_command_hl(env._h, R._p(a), 1, None, R._p(env.obs), R._p(low), None, None, None)
        assert rc == K.FW_EUNSUPPORTED
        with pytest.raises(RuntimeError, match="fw_command_hl"):
            _lib.check(rc, env._h)
        env.close()
    env = P.FixedwingWaypointsDirectVecEnv(8, angle_representation="euler")
    assert _lib.lib().fw_command_hl(env._h, None, 1, None, R._p(env.obs), R._p(env.obs), None, None, None) == K.FW_EINVAL
    env.close()


# ------------------------------------------------------------------------------------------------ 3. the composed step
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


def test_composed_step_against_independent_pieces(lanes):
    n, steps, seed = 199, 64, 13
    pol, mean, var = _controller()
    A = HighLevelCmdVecEnv(n, pol, (mean, var), seed=seed)
    B = P.FixedwingWaypointsDirectVecEnv(n, **BASE_KW, seed=seed)
    assert A.lanes_per_env == lanes == B.lanes_per_env and A.obs_dim == 30 and A.act_dim == 3
    assert torch.equal(A.reset_tensor(), B.reset_tensor())
    rng = np.random.default_rng(17)
    scale = np.array([2.0 * math.pi, 300.0, 40.0])
    worst, dones, clipped = 0.0, 0, 0
    for t in range(steps):
        raw = rng.normal(0.0, 1.0, (n, 3)) * scale + np.array([0.0, 60.0, 15.0])
        b_obs = B.obs.cpu().numpy()
        cmd = condition_command(raw, 200.0)
        low = np.concatenate([b_obs[:, 0:18], cmd], axis=1)
        norm = np.clip((low - mean) / np.sqrt(var + 1e-8), -10.0, 10.0).astype(np.float32)          # :134-143
        with torch.no_grad():
            x = torch.from_numpy(norm).to(A.device)
            want = A.low_policy.action_net(A.low_policy.pi_net(x)).clamp(-1.0, 1.0)
        A.step_tensor(torch.as_tensor(raw, device=A.device))
        # (a) the controller's action against the torch forward of the same MlpPolicy
        got = A.low_action.to(torch.float32)
        worst = max(worst, float((got - want).abs().max()))
        torch.testing.assert_close(got, want, rtol=1e-5, atol=2e-6, msg=lambda m: f"step {t}: {m}")
        clipped += int((want.abs() == 1.0).sum())
        np.testing.assert_array_equal(A.command.cpu().numpy(), cmd)
        np.testing.assert_array_equal(A.low_obs.cpu().numpy(), low)
        # (b) the base env by itself, given that action, stays bit for bit with the composed env
        B.step_tensor(A.low_action)
        for name in ("obs", "rewards", "terminated", "truncated", "info"):
            assert torch.equal(getattr(A, name), getattr(B, name)), (t, name)
        d = (B.terminated | B.truncated).bool()
        if d.any():
            assert torch.equal(A.terminal_obs[d], B.terminal_obs[d]), t
        dones += int(d.sum())
        sa, sb = A.get_state(), B.get_state()
        np.testing.assert_array_equal(sa[:, TAIL + 3:], sb[:, TAIL + 3:])
        np.testing.assert_array_equal(np.delete(sa, np.s_[TAIL:TAIL + 3], axis=1), np.delete(sb, np.s_[TAIL:TAIL + 3], axis=1))
        np.testing.assert_array_equal(sa[~d.cpu().numpy(), TAIL:TAIL + 3], cmd[~d.cpu().numpy()])     # A's tail holds the command
    print(f"lanes {lanes}: worst |low_action - torch| {worst:.3e}, {dones} episode ends, {clipped} clipped action components")
    assert clipped > 0
    assert int(A.rejected.item()) == 0
    A.close(); B.close()


def test_numpy_surface_and_infos():
    pol, mean, var = _controller()
    env = HighLevelCmdVecEnv(16, pol, {"mean": mean, "var": var}, seed=2)
    assert env.action_space.shape == (3,) and env.observation_space.shape == (30,)
    np.testing.assert_array_equal(env.action_space.low, np.array([-np.pi, 0.0, 0.0], dtype=np.float32))
    np.testing.assert_array_equal(env.action_space.high, np.array([np.pi, 200.0, 30.0], dtype=np.float32))
    assert torch.equal(env.action_low.cpu(), torch.from_numpy(env.action_space.low))
    obs = env.reset()
    assert obs.shape == (16, 30)
    a = np.tile(np.array([4.0, 250.0, 12.0]), (16, 1))
    obs, rew, dones, infos = env.step(a)
    assert obs.shape == (16, 30) and rew.shape == (16,) and len(infos) == 16
    for d in infos:
        np.testing.assert_array_equal(d["command"], [-math.pi, 200.0, 12.0])
        assert {"num_targets_reached", "collision", "out_of_bounds", "env_complete", "TimeLimit.truncated"} <= set(d)
        assert "duck_strike" not in d
    assert env.get_attr("flight_dome_size") == [200.0] * 16 and env.get_attr("act_dim", [0, 1]) == [3, 3]
    env.close()


# ------------------------------------------------------------------------------------------------ 4. hipGraph
def test_graph_replay_equals_the_eager_loop():
    n, seed, per, replays = 199, 9, 8, 8
    pol, mean, var = _controller()
    A = HighLevelCmdVecEnv(n, pol, (mean, var), seed=seed)
    E = HighLevelCmdVecEnv(n, pol, (mean, var), seed=seed)
    A.reset_tensor(); E.reset_tensor()
    g = torch.Generator(device="cpu").manual_seed(4)
    scale = torch.tensor([2.0 * math.pi, 300.0, 40.0], dtype=torch.float64)
    pool = [(torch.randn((n, 3), generator=g, dtype=torch.float64) * scale + torch.tensor([0.0, 60.0, 15.0], dtype=torch.float64)).to(A.device)
            for _ in range(per)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.step_tensor(pool[0]); E.step_tensor(pool[0])          # one eager vec-step on the capture stream first (lazy initialisation)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for a in pool:
            A.step_tensor(a)
    dones = 0
    for r in range(replays):
        graph.replay()
        for a in pool:
            E.step_tensor(a)
            dones += int((E.terminated | E.truncated).sum())
        torch.cuda.synchronize()
        for name in ("obs", "rewards", "terminated", "truncated", "info", "terminal_obs", "low_action", "command", "low_obs"):
            assert torch.equal(getattr(A, name), getattr(E, name)), (r, name)
        assert np.array_equal(A.get_state(), E.get_state()), r
    assert A.get_counters() == E.get_counters()
    assert dones > 0 and A.get_counters()["resets"] >= dones, (dones, A.get_counters())      # 64 replayed steps with auto-resets
    A.close(); E.close()


# ------------------------------------------------------------------------------------------------ 5. learner plumbing
def test_ppo_trains_the_three_action_policy_on_the_torch_path():
    pol, mean, var = _controller()
    venv = HighLevelCmdVecEnv(16, pol, (mean, var), seed=123)
    seen = []
    step_tensor = venv.step_tensor

    def spy(actions):
        seen.append(actions.detach().clone())
        return step_tensor(actions)
    venv.step_tensor = spy
    env = R.VecNormalizeDevice(venv, norm_obs=True, norm_reward=True, clip_obs=10.0, gamma=0.995)
    ppo = R.PPO(env, R.PPOConfig(n_steps=64, batch_size=256, n_epochs=2, gamma=0.995, ent_coef=0.0, seed=123, use_graphs=False))
    assert ppo.act_dim == 3 and ppo.buf_act.shape == (64, 16, 3) and ppo.policy.action_net.out_features == 3
    assert not ppo._collect_fused and not ppo._one_launch and not ppo._close_gae and ppo._fused is None      # the fused paths are off
    assert not R.FusedPpoUpdate.applies(ppo.policy, ppo.cfg, env.obs_dim, 256, ppo.device)
    ppo.learn(2 * 64 * 16)
    torch.cuda.synchronize()
    assert ppo.num_timesteps == 2 * 64 * 16 and len(seen) == 2 * 64
    for k in ("policy_loss", "value_loss"):
        assert any(k in name for name in ppo.logs), ppo.logs
    assert all(math.isfinite(v) for v in ppo.logs.values()), ppo.logs
    assert torch.isfinite(ppo.buf_act).all() and all(torch.isfinite(q).all() for q in ppo.policy.parameters())
    lo, hi = venv.action_low.to(torch.float64), venv.action_high.to(torch.float64)
    outside = 0
    for a, raw in zip(seen[-64:], ppo.buf_act):
        a = a.to(torch.float64)
        assert bool(((a >= lo) & (a <= hi)).all())          # every action handed to the env is inside the Box
        assert torch.equal(a.to(torch.float32), torch.from_numpy(np.clip(raw.cpu().numpy(), lo.cpu().numpy().astype(np.float32),
                                                                         hi.cpu().numpy().astype(np.float32))).to(a.device))
        outside += int((raw.to(torch.float64) < lo).sum() + (raw.to(torch.float64) > hi).sum())
    assert outside > 0                                      # a raw Gaussian around 0: the altitude and airspeed floors clip
    venv.close()


def test_a_four_action_env_keeps_its_clamp():
    venv = P.FixedwingWaypointsVecEnv(16, angle_representation="euler", seed=5)
    seen = []
    step_tensor = venv.step_tensor

    def spy(actions):
        seen.append(actions.detach().clone())
        return step_tensor(actions)
    venv.step_tensor = spy
    env = R.VecNormalizeDevice(venv)
    ppo = R.PPO(env, R.PPOConfig(n_steps=16, batch_size=64, n_epochs=1, seed=3, use_graphs=False, fused_collect=False, fused_update=False))
    with torch.no_grad():
        ppo.policy.log_std.fill_(1.0)                      # wide actions: the clamp matters
    ppo.collect_rollouts()
    torch.cuda.synchronize()
    assert len(seen) == 16
    for a, raw in zip(seen, ppo.buf_act):
        assert torch.equal(a, raw.clamp(-1.0, 1.0).to(venv.torch_dtype))
    assert any(bool((raw.abs() > 1.0).any()) for raw in ppo.buf_act)
    venv.close()


def test_fused_six_action_learner_accepts_the_base_env():
    venv = P.FixedwingWaypointsDirectVecEnv(256, **BASE_KW, seed=7)
    env = R.VecNormalizeDevice(venv)
    ppo = R.PPO(env, R.PPOConfig(n_steps=16, batch_size=256, n_epochs=2, seed=1, fused_six_actions=True))
    assert ppo.act_dim == 6 and ppo._collect_fused and not ppo._one_launch
    assert R.FusedPpoUpdate.applies(ppo.policy, ppo.cfg, env.obs_dim, 256, ppo.device)
    ppo.learn(2 * 16 * 256)
    torch.cuda.synchronize()
    assert ppo.num_timesteps == 2 * 16 * 256
    assert all(math.isfinite(v) for v in ppo.logs.values()), ppo.logs
    for name in ("buf_obs", "buf_act", "buf_val", "buf_rew"):
        assert torch.isfinite(getattr(ppo, name)).all(), name
    assert all(torch.isfinite(q).all() for q in ppo.policy.parameters())
    venv.close()


# ------------------------------------------------------------------------------------------------ 6. evaluation, checkpoint
def test_evaluate_returns_waypoint_scalars_for_both_envs():
    pol, mean, var = _controller()
    for venv, a in ((HighLevelCmdVecEnv(16, pol, (mean, var), seed=3, max_duration_seconds=4.0), 3),
                    (P.FixedwingWaypointsDirectVecEnv(16, **{**BASE_KW, "max_duration_seconds": 4.0}, seed=3), 6)):
        env = R.VecNormalizeDevice(venv, training=False, norm_reward=False)
        torch.manual_seed(5)
        policy = R.MlpPolicy(env.obs_dim, a).to(env.device)
        for use_graph in (True, False):
            r = evaluate.evaluate_policy(policy, env, n_eval_episodes=16, use_graph=use_graph)
            assert len(r.episode_rewards) == 16 and len(r.num_targets_reached) == 16 and len(r.is_success) == 16
            sc = r.scalars(num_targets_total=venv.cfg.num_targets)
            assert "eval/success_rate" in sc and "eval/wp1_reach_rate" in sc and all(math.isfinite(v) for v in sc.values()), sc
            assert not r.duck_strike and max(r.episode_lengths) <= 4 * 30 + 2
        venv.close()


def test_checkpoint_round_trips_the_tail(tmp_path):
    pol, mean, var = _controller()

    def make():
        venv = HighLevelCmdVecEnv(16, pol, (mean, var), seed=11)
        return R.PPO(R.VecNormalizeDevice(venv, gamma=0.995), R.PPOConfig(n_steps=8, batch_size=64, n_epochs=1, gamma=0.995, seed=4, use_graphs=False))
    a = make()
    a.learn(8 * 16)
    torch.cuda.synchronize()
    sa = a.env.venv.get_state()
    assert np.abs(sa[:, TAIL:TAIL + 3]).sum() > 0 and np.abs(sa[:, TAIL + 3:TAIL + 9]).sum() > 0      # a command and a six-wide action
    path = checkpoint.save(str(tmp_path / "hl.pt"), a)
    b = make()
    checkpoint.load(path, b, reset_num_timesteps=False, restore_env_state=True)
    np.testing.assert_array_equal(b.env.venv.get_state(), sa)
    assert torch.equal(b.env.venv.obs, a.env.venv.obs)
    # ... and the two go on identically
    raw = torch.randn((16, 3), dtype=torch.float64, device=a.device) * 20
    a.env.venv.step_tensor(raw); b.env.venv.step_tensor(raw)
    assert torch.equal(a.env.venv.obs, b.env.venv.obs) and np.array_equal(a.env.venv.get_state(), b.env.venv.get_state())
    # the low-level checkpoint format (what examples/train_lowlevel_cmd.py saves) builds the same controller
    ll = R.PPO(R.VecNormalizeDevice(P.FixedwingLowLevelVecEnv(16, seed=1)), R.PPOConfig(n_steps=8, batch_size=64, n_epochs=1, seed=2, use_graphs=False))
    ll.learn(8 * 16)
    lp = checkpoint.save(str(tmp_path / "low.pt"), ll)
    h = HighLevelCmdVecEnv(8, low_checkpoint=lp, seed=1)
    for (k, v), (k2, v2) in zip(h.low_policy.state_dict().items(), ll.policy.state_dict().items()):
        assert k == k2 and torch.equal(v, v2)
    assert torch.equal(h.low_mean, ll.env.obs_rms.mean) and torch.equal(h.low_var, ll.env.obs_rms.var) and h.clip_obs == 10.0
    h.reset_tensor(); h.step_tensor(torch.zeros((8, 3), dtype=torch.float64, device=h.device))
    torch.cuda.synchronize()
    assert torch.isfinite(h.low_action).all()
    for e in (a.env.venv, b.env.venv, ll.env.venv, h):
        e.close()
