"""The high-level command task with the frozen controller at 120 Hz inside the step kernel (``controller_hz=120``, ``fw_step_hl``;
DESIGN.md section 2e), against the project's existing kernels and torch:

1. ``fw_controller_forward`` against the torch forward of the same ``MlpPolicy``;
2. ``fw_step_hl`` at 30 Hz against four ``fw_controller_forward -> fw_step`` rounds of a twin handle at ``agent_hz=120``;
3. a controller with zero weight matrices against ``fw_step`` fed its constant output;
4. the env surface (``controller_hz``), rejected actions, the handles ``fw_step_hl`` refuses;
5. the fused collector's act side in front of ``step_low``;
6. hipGraph replay and the flight record.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib, highlevel
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R
from pyflyt_drone_amd.highlevel import HighLevelCmdVecEnv
from test_highlevel_120hz_cpu import fold_rewards

pytestmark = pytest.mark.gpu

TAIL = K.S_TASK
GUST_RANDOM = dict(enabled=True, mode="gust_sine", randomize_on_reset=True, randomize_gust_phase=True, gust_freq_hz=0.7,
                   wind_enu_mps_range=[[-2.0, 2.0], [-2.0, 2.0], [0.0, 0.0]], gust_amp_enu_mps_range=[[0.0, 3.0], [0.0, 3.0], [0.0, 1.0]])
WINDS = {"no_wind": None, "gust": GUST_RANDOM}
# the project's lockstep (float64) and one-step (float32) tolerances
TOL = {"float64": 1e-7, "float32": 2e-3}
CLIP, EPS = 10.0, 1e-8


@pytest.fixture(params=[1, 8], ids=["lane_per_env", "8_lanes_per_env"])
def lanes(request, monkeypatch):
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", str(request.param))
    return request.param


def _controller(seed=21, zero_weights=False):
    """a controller with random (seeded) weights whose actions use the whole of [-1, 1], and non-trivial statistics"""
    torch.manual_seed(seed)
    p = R.MlpPolicy(21, 6)
    with torch.no_grad():
        for q in p.parameters():
            q.add_(0.1 * torch.randn_like(q))
        p.action_net.weight.mul_(1.5)
        if zero_weights:
            for m in (p.pi_net[0], p.pi_net[2], p.action_net):
                m.weight.zero_()
            p.action_net.bias.copy_(torch.tensor([0.05, -0.08, 0.03, 0.02, -0.04, 1.7]))      # gentle surfaces, a clipped throttle
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
        p.log_std.copy_(torch.tensor([1.5, 5.0, 3.5]))
    return p


def _flat(policy, d):
    f = R.FusedPpoUpdate(policy, None, d)
    f.load_params_from_torch()
    return f.flat


class _Ctl:
    """the controller as the C entry points take it: flat image and statistics on the device"""
    def __init__(self, pol, mean, var, dev="cuda"):
        self.pol = pol.to(dev).eval()
        self.flat = _flat(self.pol, 21)
        self.mean = torch.as_tensor(mean, dtype=torch.float64, device=dev)
        self.var = torch.as_tensor(var, dtype=torch.float64, device=dev)

    def forward(self, rows, out):
        rc = _lib.lib().fw_controller_forward(R._p(self.flat), R._p(rows), int(rows.dtype == torch.float64), rows.shape[0], R._p(self.mean),
                                              R._p(self.var), CLIP, EPS, R._p(out), int(out.dtype == torch.float64), None)
        _lib.check(rc)
        return out

    def step_hl(self, env, low_action=None, tobs=True, info=True):
        a = K.FwStepHlArgs()
        a.low_params, a.low_mean, a.low_var, a.low_clip, a.low_eps = self.flat.data_ptr(), self.mean.data_ptr(), self.var.data_ptr(), CLIP, EPS
        a.obs, a.reward, a.terminated, a.truncated = env.obs.data_ptr(), env.rewards.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr()
        a.terminal_obs = env.terminal_obs.data_ptr() if tobs else None
        a.info_i32 = env.info.data_ptr() if info else None
        a.low_action = None if low_action is None else low_action.data_ptr()
        _lib.check(_lib.lib().fw_step_hl(env._h, C.byref(a), None), env._h)


def _command(env, raw, low_obs, cmd, rejected=None):
    _lib.check(_lib.lib().fw_command_hl(env._h, R._p(raw), int(raw.dtype == torch.float64), None, R._p(env.obs), R._p(low_obs), R._p(cmd),
                                        R._p(rejected), None), env._h)


def _box_commands(rng, n, dome):
    return np.stack([rng.uniform(-math.pi, math.pi, n), rng.uniform(0.0, dome, n), rng.uniform(0.0, 30.0, n)], axis=1)


# ------------------------------------------------------------------------------------------------ 1. fw_controller_forward
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_controller_forward_against_torch(dtype):
    n = 199
    pol, mean, var = _controller()
    ctl = _Ctl(pol, mean, var)
    g = np.random.default_rng(2)
    rows = mean + g.normal(0.0, 1.0, (n, 21)) * np.sqrt(var) * 1.5
    rows[:24] = mean + g.choice([-1.0, 1.0], (24, 21)) * np.sqrt(var) * g.uniform(8.0, 40.0, (24, 21))       # far beyond the clip
    rows[24:30, 3] = mean[3] + np.array([-1, 1, -1, 1, -1, 1]) * 10.0 * np.sqrt(var[3] + EPS)                      # on it
    td = torch.float64 if dtype == "float64" else torch.float32
    x = torch.as_tensor(rows, dtype=td, device="cuda")
    rows_t = x.cpu().numpy().astype(np.float64)             # float32: the rows as the kernel sees them
    z = (rows_t - mean) / np.sqrt(var + EPS)
    assert (np.abs(z) > CLIP).sum() > 100
    norm = np.clip(z, -CLIP, CLIP).astype(np.float32)
    with torch.no_grad():
        free = ctl.pol.action_net(ctl.pol.pi_net(torch.from_numpy(norm).cuda()))
    want = free.clamp(-1.0, 1.0)
    assert int((free.abs() > 1.0).sum()) > 20 and int((free.abs() < 1.0).sum()) > 200
    for out_dtype in (torch.float64, torch.float32):
        got = ctl.forward(x, torch.full((n, 6), -7.0, dtype=out_dtype, device="cuda"))
        torch.cuda.synchronize()
        worst = float((got.to(torch.float32) - want).abs().max())
        print(f"{dtype} rows, {out_dtype} out: worst |fw_controller_forward - torch| {worst:.3e}")
        torch.testing.assert_close(got.to(torch.float32), want, rtol=1e-5, atol=2e-6)
        assert float(got.abs().max()) == 1.0
    L = _lib.lib()
    assert L.fw_controller_forward(None, R._p(x), 1, n, R._p(ctl.mean), R._p(ctl.var), CLIP, EPS, R._p(got), 0, None) == K.FW_EINVAL
    assert L.fw_controller_forward(R._p(ctl.flat), R._p(x), 1, 0, R._p(ctl.mean), R._p(ctl.var), CLIP, EPS, R._p(got), 0, None) == K.FW_EINVAL


# ------------------------------------------------------------------------------------------------ 2. fw_step_hl against four 120 Hz steps
def _path_targets(rng, n):
    """waypoints on the start course (from (0, 0, 10) along +x at 20 m/s): the first within reach inside the first agent steps"""
    t = np.zeros((n, 4, 3))
    t[:, 0] = np.stack([rng.uniform(2.2, 6.0, n), rng.uniform(-0.6, 0.6, n), 10.0 + rng.uniform(-0.6, 0.6, n)], axis=1)
    t[:, 1] = t[:, 0] + np.stack([rng.uniform(2.5, 4.0, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)], axis=1)
    t[:, 2] = [0.0, 8.0, 10.0]
    t[:, 3] = [0.0, -8.0, 10.0]
    return t


@pytest.mark.parametrize("wind", list(WINDS))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_step_hl_against_four_120hz_steps_of_a_twin(dtype, wind, lanes):
    """Per agent step, H120 restarts from H30's pre-step state, so nothing accumulates: the figures are those of one agent step.
    Measured (MI355X): see DESIGN.md section 2e."""
    n, steps, seed, dome = 199, 60, 13, 14.0
    kw = dict(flight_dome_size=dome, max_duration_seconds=120.0, context_length=2, angle_representation="euler", wind_config=WINDS[wind],
              dtype=dtype, seed=seed, global_env_offset=640)
    H30 = P.FixedwingWaypointsDirectVecEnv(n, agent_hz=30, **kw)
    H120 = P.FixedwingWaypointsDirectVecEnv(n, agent_hz=120, **kw)
    assert H30.lanes_per_env == lanes == H120.lanes_per_env and H30.cfg.motor.noise_ratio > 0
    tol, td, dev = TOL[dtype], H30.torch_dtype, H30.device
    pol, mean, var = _controller()
    ctl = _Ctl(pol, mean, var)
    rng = np.random.default_rng(17)
    sc = dict(targets=_path_targets(rng, n))
    H30.reset_tensor(scenario=sc); H120.reset_tensor(scenario=sc)
    low30, cmd30 = torch.zeros((n, 21), dtype=td, device=dev), torch.zeros((n, 3), dtype=td, device=dev)
    low120, cmd120 = torch.zeros_like(low30), torch.zeros_like(cmd30)
    act = torch.zeros((n, 6), dtype=td, device=dev)
    la30 = torch.full((n, 6), -7.0, dtype=td, device=dev)
    NUM, COLL, OOB = K.INFO_NUM_TARGETS_REACHED, K.INFO_COLLISION, K.INFO_OUT_OF_BOUNDS
    real = np.r_[np.arange(K.S_POS, K.S_ACTION), K.S_NEW_DIST, np.arange(K.S_WIND, K.S_WIND + 7),
                 np.arange(K.S_TARGETS, K.S_TARGETS + 3 * K.FW_MAX_TARGETS), np.arange(TAIL, TAIL + K.SL_DIM)]
    ints = [K.S_TICK_COUNT, K.S_EPISODE, K.S_FLAGS, K.S_NUM_REACHED]
    worst = dict(obs=0.0, tobs=0.0, rew=0.0, state=0.0, low_action=0.0)
    ends_early = ends_last = reach_alive = 0
    for t in range(steps):
        pre = H30.get_state()
        H120.set_state(pre)
        H120.observe_tensor()
        raw = torch.as_tensor(_box_commands(rng, n, dome), device=dev)
        _command(H30, raw, low30, cmd30); _command(H120, raw, low120, cmd120)
        assert torch.equal(cmd30, cmd120), t
        # ---- H120: four rounds of (row -> controller -> one Aviary step as an agent step) ----
        snaps = []
        for k in range(4):
            row = torch.cat([H120.obs[:, 0:18], cmd120], dim=1).contiguous()
            ctl.forward(row, act)
            H120.step_tensor(act)
            torch.cuda.synchronize()
            snaps.append(dict(obs=H120.obs.cpu().numpy().astype(np.float64), rew=H120.rewards.cpu().numpy().astype(np.float64),
                              term=H120.terminated.cpu().numpy(), trunc=H120.truncated.cpu().numpy(), info=H120.info.cpu().numpy(),
                              tobs=H120.terminal_obs.cpu().numpy().astype(np.float64), state=H120.get_state(),
                              act=act.cpu().numpy().astype(np.float64)))
        done_k = np.stack([(s["term"] | s["trunc"]).astype(bool) for s in snaps])                   # [4, n]
        last = np.where(done_k.any(axis=0), done_k.argmax(axis=0), 3)
        reached = np.stack([np.r_[pre[:, K.S_NUM_REACHED]]] + [s["info"][:, NUM] for s in snaps])      # [5, n] (valid up to `last`)
        event = np.stack([(snaps[k]["info"][:, COLL] != 0) | (snaps[k]["info"][:, OOB] != 0) | (reached[k + 1] > reached[k]) for k in range(4)])
        pick = lambda name: np.stack([s[name] for s in snaps])[last, np.arange(n)]                  # noqa: E731
        want_rew = fold_rewards(np.stack([s["rew"] for s in snaps]), event, last)
        done = done_k[last, np.arange(n)]
        ends_early += int((done & (last < 3)).sum()); ends_last += int((done & (last == 3)).sum())
        live_k = np.arange(4)[:, None] <= last[None, :]
        reach_alive += int((live_k & (reached[1:] > reached[:-1]) & ~done_k).sum())
        # ---- H30: one launch ----
        ctl.step_hl(H30, low_action=la30)
        torch.cuda.synchronize()
        tag = f"{dtype} {wind} lanes {lanes} step {t}"
        info30, want_info = H30.info.cpu().numpy(), pick("info")
        assert np.array_equal(H30.terminated.cpu().numpy(), pick("term")), tag
        assert np.array_equal(H30.truncated.cpu().numpy(), pick("trunc")), tag
        # (the episode-length column counts agent steps: one on H30, last + 1 on H120, from the same start)
        cols = [c for c in range(K.FW_INFO_DIM) if c != K.INFO_EP_LEN]
        assert np.array_equal(info30[:, cols], want_info[:, cols]), tag
        assert np.array_equal(info30[:, K.INFO_EP_LEN], pre[:, K.S_STEP_COUNT] + 1), tag
        assert np.array_equal(want_info[:, K.INFO_EP_LEN], pre[:, K.S_STEP_COUNT] + last + 1), tag
        s30, s120 = H30.get_state(), pick("state")
        assert np.array_equal(s30[:, ints], s120[:, ints]), tag
        d = dict(obs=np.abs(H30.obs.cpu().numpy().astype(np.float64) - pick("obs")).max(),
                 rew=np.abs(H30.rewards.cpu().numpy().astype(np.float64) - want_rew).max(),
                 state=np.abs(s30[:, real] - s120[:, real]).max(),
                 low_action=np.abs(la30.cpu().numpy().astype(np.float64) - pick("act")).max())
        if done.any():
            d["tobs"] = np.abs(H30.terminal_obs.cpu().numpy().astype(np.float64)[done] - pick("tobs")[done]).max()
        for name, v in d.items():
            worst[name] = max(worst[name], float(v))
            assert v <= tol, (tag, name, v)
        # the observation and the tail show the last Aviary step's output (zeros after the auto-reset)
        assert np.array_equal(H30.obs.cpu().numpy()[~done, 12:18], la30.cpu().numpy()[~done]), tag
        assert not H30.obs.cpu().numpy()[done, 12:18].any(), tag
        if done.any():
            assert np.array_equal(H30.terminal_obs.cpu().numpy()[done, 12:18], la30.cpu().numpy()[done]), tag
    print(f"{dtype} {wind} lanes {lanes}: worst |diff| {worst}; episodes ended before the last Aviary step {ends_early}, at it {ends_last}; "
          f"waypoints reached without ending the episode {reach_alive}")
    assert ends_early > 0 and ends_last > 0 and reach_alive > 0, (ends_early, ends_last, reach_alive)
    c = H30.get_counters()
    assert c["resets"] == ends_early + ends_last
    H30.close(); H120.close()


# ------------------------------------------------------------------------------------------------ 3. a constant controller
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_constant_controller_equals_fw_step_with_its_output(dtype, lanes):
    n, steps, seed, dome = 199, 60, 7, 14.0
    kw = dict(flight_dome_size=dome, agent_hz=30, context_length=2, angle_representation="euler", wind_config=GUST_RANDOM, dtype=dtype, seed=seed)
    A, B = P.FixedwingWaypointsDirectVecEnv(n, **kw), P.FixedwingWaypointsDirectVecEnv(n, **kw)
    assert A.lanes_per_env == lanes
    pol, mean, var = _controller(zero_weights=True)
    ctl = _Ctl(pol, mean, var)
    td, tol = A.torch_dtype, TOL[dtype]
    rows = torch.as_tensor(np.random.default_rng(1).normal(0.0, 30.0, (n, 21)), dtype=td, device=A.device)
    const = ctl.forward(rows, torch.zeros((n, 6), dtype=td, device=A.device))
    torch.cuda.synchronize()
    assert torch.equal(const, const[0:1].expand(n, 6))                                              # the rate cannot matter
    np.testing.assert_array_equal(const[0].cpu().numpy(), np.array([0.05, -0.08, 0.03, 0.02, -0.04, 1.0], dtype=np.float32).astype(A.np_dtype))
    assert torch.equal(A.reset_tensor(), B.reset_tensor())
    la = torch.full((n, 6), -7.0, dtype=td, device=A.device)
    worst, dones = 0.0, 0
    for t in range(steps):
        ctl.step_hl(A, low_action=la)
        B.step_tensor(const)
        torch.cuda.synchronize()
        for name in ("terminated", "truncated", "info"):
            assert torch.equal(getattr(A, name), getattr(B, name)), (t, name)
        d = (B.terminated | B.truncated).bool()
        pairs = [(A.obs, B.obs), (A.rewards, B.rewards), (torch.as_tensor(A.get_state()), torch.as_tensor(B.get_state())), (la, const)]
        if d.any():
            pairs.append((A.terminal_obs[d], B.terminal_obs[d]))
        for x, y in pairs:
            diff = float((x.to(torch.float64) - y.to(torch.float64)).abs().max())
            worst = max(worst, diff)
            assert diff <= tol, (t, diff)
        dones += int(d.sum())
    print(f"{dtype} lanes {lanes}: worst |fw_step_hl - fw_step| {worst:.3e} over {steps} steps, {dones} auto-resets")
    assert dones > n                                      # every env ended at least once
    assert A.get_counters() == B.get_counters()
    A.close(); B.close()


# ------------------------------------------------------------------------------------------------ 4. the env surface
def test_step_tensor_is_command_hl_then_step_hl(lanes):
    n, steps, seed = 199, 16, 13
    pol, mean, var = _controller()
    E = HighLevelCmdVecEnv(n, pol, (mean, var), seed=seed, flight_dome_size=12.0, controller_hz=120)
    B = P.FixedwingWaypointsDirectVecEnv(n, flight_dome_size=12.0, max_duration_seconds=120.0, agent_hz=30, context_length=2,
                                         angle_representation="euler", seed=seed)
    assert E.lanes_per_env == lanes == B.lanes_per_env and E.controller_in_step and E.controller_hz == 120
    ctl = _Ctl(pol, mean, var)
    assert torch.equal(E.reset_tensor(), B.reset_tensor())
    low, cmd = torch.zeros((n, 21), dtype=torch.float64, device=B.device), torch.zeros((n, 3), dtype=torch.float64, device=B.device)
    la = torch.zeros((n, 6), dtype=torch.float64, device=B.device)
    rej = torch.zeros(1, dtype=torch.int32, device=B.device)
    rng = np.random.default_rng(17)
    dones = 0
    for t in range(steps):
        raw = torch.as_tensor(rng.normal(0.0, 1.0, (n, 3)) * np.array([2.0 * math.pi, 300.0, 40.0]) + np.array([0.0, 60.0, 15.0]), device=B.device)
        if t == 5:                                        # rows that keep the command of step 4
            raw[3, 0], raw[7, 1], raw[11] = float("nan"), float("inf"), float("nan")
            kept = E.command[[3, 7, 11]].clone()
        E.step_tensor(raw)
        _command(B, raw, low, cmd, rej)
        ctl.step_hl(B, low_action=la)
        torch.cuda.synchronize()
        for name in ("obs", "rewards", "terminated", "truncated", "info"):
            assert torch.equal(getattr(E, name), getattr(B, name)), (t, name)
        d = (B.terminated | B.truncated).bool()
        if d.any():
            assert torch.equal(E.terminal_obs[d], B.terminal_obs[d]), t
        assert torch.equal(E.low_action, la) and torch.equal(E.command, cmd) and torch.equal(E.low_obs, low), t
        assert np.array_equal(E.get_state(), B.get_state()), t
        if t == 5:
            assert torch.equal(E.command[[3, 7, 11]], kept) and int(E.rejected.item()) == 3 == int(rej.item())
        dones += int(d.sum())
    assert dones > 0
    E.close(); B.close()


@pytest.mark.parametrize("hz", [None, 30])
def test_controller_hz_none_and_agent_hz_are_the_path_without_the_keyword(hz):
    n, seed = 64, 5
    pol, mean, var = _controller()
    A = HighLevelCmdVecEnv(n, pol, (mean, var), seed=seed, controller_hz=hz)
    E = HighLevelCmdVecEnv(n, pol, (mean, var), seed=seed)
    assert not A.controller_in_step and A.controller_hz == 30 == E.controller_hz
    A.reset_tensor(); E.reset_tensor()
    rng = np.random.default_rng(3)
    for t in range(16):
        raw = torch.as_tensor(_box_commands(rng, n, 200.0), device=A.device)
        A.step_tensor(raw); E.step_tensor(raw)
        for name in ("obs", "rewards", "terminated", "truncated", "info", "low_action", "command", "low_obs"):
            assert torch.equal(getattr(A, name), getattr(E, name)), (t, name)
    assert np.array_equal(A.get_state(), E.get_state())
    A.close(); E.close()


def test_step_hl_refuses_other_tasks_the_quaternion_attitude_and_missing_pointers():
    pol, mean, var = _controller()
    ctl = _Ctl(pol, mean, var)
    L = _lib.lib()
    for env in (P.FixedwingWaypointsVecEnv(8, angle_representation="euler"), P.FixedwingLowLevelVecEnv(8),
                P.FixedwingWaypointsDirectVecEnv(8, angle_representation="quaternion")):
        env.reset_tensor()
        with pytest.raises(RuntimeError, match="fw_step_hl"):
            ctl.step_hl(env)
        a = K.FwStepHlArgs()
        assert L.fw_step_hl(env._h, C.byref(a), None) == K.FW_EUNSUPPORTED
        env.close()
    env = P.FixedwingWaypointsDirectVecEnv(8, angle_representation="euler")
    env.reset_tensor()
    assert L.fw_step_hl(env._h, None, None) == K.FW_EINVAL
    for field in ("low_params", "low_mean", "low_var", "obs", "reward", "terminated", "truncated"):
        a = K.FwStepHlArgs()
        a.low_params, a.low_mean, a.low_var, a.low_clip, a.low_eps = ctl.flat.data_ptr(), ctl.mean.data_ptr(), ctl.var.data_ptr(), CLIP, EPS
        a.obs, a.reward, a.terminated, a.truncated = env.obs.data_ptr(), env.rewards.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr()
        setattr(a, field, None)
        assert L.fw_step_hl(env._h, C.byref(a), None) == K.FW_EINVAL, field
    with pytest.raises(ValueError, match="fw_step_hl"):
        _lib.check(K.FW_EINVAL, env._h)
    ctl.step_hl(env, tobs=False, info=False)              # the optional outputs may be missing
    torch.cuda.synchronize()
    assert torch.isfinite(env.obs).all()
    env.close()


# ------------------------------------------------------------------------------------------------ 5. the fused collector
def test_fused_act_side_then_step_low_equals_step_tensor_of_a_twin(lanes):
    n, steps, seed = 16, 16, 3
    pol, mean, var = _controller()
    A = HighLevelCmdVecEnv(n, pol, (mean, var), seed=seed, flight_dome_size=12.0, controller_hz=120)
    E = HighLevelCmdVecEnv(n, pol, (mean, var), seed=seed, flight_dome_size=12.0, controller_hz=120)
    assert A.lanes_per_env == lanes
    A.reset_tensor(); E.reset_tensor()
    com = _commander()
    flat = _flat(com, 30)
    om = torch.linspace(-0.2, 0.3, 30, dtype=torch.float64, device=A.device)
    ov = torch.linspace(0.5, 2.0, 30, dtype=torch.float64, device=A.device)
    rng = torch.tensor([12345, 0], dtype=torch.int64, device=A.device)
    act_raw, logp = torch.zeros((n, 3), device=A.device), torch.zeros(n, device=A.device)
    clipped = 0
    for t in range(steps):
        a = K.FwCollectHlArgs()
        a.params, a.nets, a.deterministic, a.rng = flat.data_ptr(), 1, 0, rng.data_ptr()
        a.obs_mean, a.obs_var, a.clip_obs, a.eps_obs = om.data_ptr(), ov.data_ptr(), 10.0, 1e-8
        a.act_raw, a.logp = act_raw.data_ptr(), logp.data_ptr()
        A.collect_act_hl(a)
        A.step_low()
        E.step_tensor(act_raw)
        rng[1] += 1
        torch.cuda.synchronize()
        for name in ("obs", "rewards", "terminated", "truncated", "info", "command", "low_action"):
            assert torch.equal(getattr(A, name), getattr(E, name)), (t, name)
        lo, hi = A.action_low.to(torch.float32), A.action_high.to(torch.float32)
        clipped += int(((act_raw < lo) | (act_raw > hi)).sum())
    assert clipped > 0 and np.array_equal(A.get_state(), E.get_state())
    A.close(); E.close()


# ------------------------------------------------------------------------------------------------ 6. replay and recording
def test_graph_replay_equals_the_eager_loop():
    n, seed, per, replays = 199, 9, 8, 4
    pol, mean, var = _controller()
    A = HighLevelCmdVecEnv(n, pol, (mean, var), seed=seed, flight_dome_size=12.0, controller_hz=120)
    E = HighLevelCmdVecEnv(n, pol, (mean, var), seed=seed, flight_dome_size=12.0, controller_hz=120)
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
    assert dones > 0 and A.get_counters()["resets"] >= dones, (dones, A.get_counters())
    A.close(); E.close()


@pytest.mark.parametrize("fused", [False, True], ids=["torch_act", "fused_act"])
def test_flight_record_replayed_equals_eager(fused):
    n, T = 16, 24
    pol, mean, var = _controller()
    com = _commander()
    traces = []
    for graph_steps in (8, 0):
        venv = HighLevelCmdVecEnv(n, pol, (mean, var), seed=9, max_duration_seconds=4.0, controller_hz=120)
        env = R.VecNormalizeDevice(venv, training=False, norm_reward=False)
        traces.append(highlevel.fly(com, env, T, use_fused=fused, graph_steps=graph_steps))
        venv.close()
    a, b = traces
    assert a.trace.shape == (T, n, len(highlevel.HL_TRACE_COLS)) and np.isfinite(a.trace).all()
    np.testing.assert_array_equal(a.trace, b.trace)
    np.testing.assert_array_equal(a.start, b.start)
    np.testing.assert_array_equal(a.ended_at, b.ended_at)
    assert a.dt == 1.0 / 30.0
