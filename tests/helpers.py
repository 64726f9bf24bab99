"""Shared helpers for the parity tests (HIP path vs CPU oracle on identical inputs)."""
import numpy as np


def seeded_actions(rng, n, kind="uniform"):
    a = rng.uniform(-1.0, 1.0, size=(n, 4))
    if kind == "gentle":           # keeps most aircraft flying for a long time
        a[:, :3] *= 0.15
        a[:, 3] = rng.uniform(-0.2, 0.6, size=n)
    return a


def run_lockstep(hip_env, ora_env, steps, rng, kind="uniform", atol=1e-6, rtol=1e-9, check_state=True, state_atol=None,
                 rew_atol=None, after_reset=None, actions=None):
    """Step both implementations with the same actions; assert per-step agreement.
    Returns a dict of the worst deviations seen.  `rew_atol`: a bound of its own for the rewards (default: `atol`);
    `after_reset(hip_env, ora_env)`: called once after the first observations were compared (e.g. to set both states);
    `actions(rng, n)`: the actions of a step instead of seeded_actions(rng, n, kind)."""
    import torch
    n = hip_env.num_envs
    worst = dict(obs=0.0, rew=0.0, tobs=0.0, state=0.0, dones=0, resets=0)
    obs_h = hip_env.reset_tensor().cpu().numpy()
    obs_o = ora_env.reset()
    np.testing.assert_allclose(obs_h, obs_o, rtol=rtol, atol=atol)
    if after_reset is not None:
        after_reset(hip_env, ora_env)
    for t in range(steps):
        a = (seeded_actions(rng, n, kind) if actions is None else actions(rng, n)).astype(hip_env.np_dtype)
        o_obs, o_rew, o_term, o_trunc, o_tobs, o_info = ora_env.step(a)
        hip_env.step_tensor(torch.as_tensor(a, device=hip_env.device))
        h_obs = hip_env.obs.cpu().numpy(); h_rew = hip_env.rewards.cpu().numpy()
        h_term = hip_env.terminated.cpu().numpy(); h_trunc = hip_env.truncated.cpu().numpy()
        h_tobs = hip_env.terminal_obs.cpu().numpy(); h_info = hip_env.info.cpu().numpy()
        assert np.array_equal(h_term, o_term), f"terminated differs at step {t}: {np.nonzero(h_term != o_term)[0][:8]}"
        assert np.array_equal(h_trunc, o_trunc), f"truncated differs at step {t}"
        assert np.array_equal(h_info, o_info), f"info differs at step {t}: rows {np.nonzero((h_info != o_info).any(1))[0][:8]}"
        np.testing.assert_allclose(h_obs, o_obs, rtol=rtol, atol=atol, err_msg=f"obs step {t}")
        np.testing.assert_allclose(h_rew, o_rew, rtol=rtol, atol=atol if rew_atol is None else rew_atol, err_msg=f"reward step {t}")
        done = (o_term | o_trunc).astype(bool)
        if done.any() and hip_env.cfg.auto_reset:
            np.testing.assert_allclose(h_tobs[done], o_tobs[done], rtol=rtol, atol=atol, err_msg=f"terminal_obs step {t}")
            worst["tobs"] = max(worst["tobs"], float(np.abs(h_tobs[done] - o_tobs[done]).max()))
        worst["obs"] = max(worst["obs"], float(np.abs(h_obs - o_obs).max()))
        worst["rew"] = max(worst["rew"], float(np.abs(h_rew - o_rew).max()))
        worst["dones"] += int(done.sum())
    if check_state:
        sh, so = hip_env.get_state(), ora_env.get_state()
        np.testing.assert_allclose(sh, so, rtol=rtol, atol=atol if state_atol is None else state_atol, err_msg="final canonical state")
        worst["state"] = float(np.abs(sh - so).max())
    return worst


# ---- the direct-command and low-level kernels against the oracle's mode-0 path (tests/test_highlevel_gpu.py, tests/test_lowlevel_gpu.py)
def set_routing_mixer(cfg, triple):
    """The oracle's mode-0 mixer routes action components 0-2 to the three surfaces of `triple` and component 3 to the throttle,
    so it sees the actuator commands a direct-command kernel gets in those slots."""
    for a in range(6):
        for k in range(4):
            cfg.mixer[a][k] = 0.0
    for k, s in enumerate(triple):
        cfg.mixer[s][k] = 1.0
    cfg.mixer[5][3] = 1.0
    return cfg


def route(a4, triple):
    """The six actuator commands that the routing mixer of `triple` makes of four mode-0 actions."""
    a6 = np.zeros((a4.shape[0], 6), dtype=a4.dtype)
    a6[:, list(triple)] = a4[:, :3]
    a6[:, 5] = a4[:, 3]
    return a6


def as_oracle_obs(o, att=12):
    """The columns a direct-command observation shares with the oracle's: the pose block (`att` wide: 12 Euler, 13 quaternion)
    and everything behind the action block, which is six wide in the kernel (and four in the oracle)."""
    return np.concatenate([o[:, 0:att], o[:, att + 6:]], axis=1)


def oracle_obs_without_action(o, att=12):
    """... and the same columns of the oracle's observation."""
    return np.concatenate([o[:, 0:att], o[:, att + 4:]], axis=1)


def run_direct_lockstep(hip_env, ora_env, triple, steps, rng, atol=1e-7, actions=None):
    """The waypoints task under six direct actuator commands against the oracle's waypoints task behind the routing mixer of
    `triple`: observations (without the action block), rewards, terminal observations and, after every step, the state
    (without the action and the task tail, which the two sides fill differently) within `atol`; flags and info exactly equal.
    Returns the worst deviations."""
    import torch
    from pyflyt_drone_amd import config as K
    n = hip_env.num_envs
    att = 12 if hip_env.cfg.angle_representation == 0 else 13
    tol = dict(rtol=0, atol=atol)
    oh, oo = hip_env.reset_tensor().cpu().numpy(), ora_env.reset()
    np.testing.assert_allclose(as_oracle_obs(oh, att), oracle_obs_without_action(oo, att), **tol)
    assert not oh[:, att:att + 6].any()
    keep = np.ones(K.FW_STATE_DIM, dtype=bool)
    keep[K.S_ACTION:K.S_ACTION + 4] = False
    keep[K.S_TASK:] = False
    worst = dict(obs=0.0, rew=0.0, tobs=0.0, state=0.0, dones=0)
    for t in range(steps):
        a4 = rng.uniform(-1.0, 1.0, size=(n, 4)) if actions is None else actions(rng, n)
        a6 = route(a4, triple)
        o_obs, o_rew, o_term, o_trunc, o_tobs, o_info = ora_env.step(a4)
        hip_env.step_tensor(torch.as_tensor(a6, device=hip_env.device))
        h_obs, h_tobs, h_rew = hip_env.obs.cpu().numpy(), hip_env.terminal_obs.cpu().numpy(), hip_env.rewards.cpu().numpy()
        assert np.array_equal(hip_env.terminated.cpu().numpy(), o_term), f"terminated differs at step {t}"
        assert np.array_equal(hip_env.truncated.cpu().numpy(), o_trunc), f"truncated differs at step {t}"
        assert np.array_equal(hip_env.info.cpu().numpy(), o_info), f"info differs at step {t}"
        done = (o_term | o_trunc).astype(bool)
        np.testing.assert_allclose(as_oracle_obs(h_obs, att), oracle_obs_without_action(o_obs, att), err_msg=f"obs step {t}", **tol)
        np.testing.assert_allclose(h_rew, o_rew, err_msg=f"reward step {t}", **tol)
        np.testing.assert_array_equal(h_obs[~done, att:att + 6], a6[~done])
        assert not h_obs[done, att:att + 6].any()
        worst["obs"] = max(worst["obs"], float(np.abs(as_oracle_obs(h_obs, att) - oracle_obs_without_action(o_obs, att)).max()))
        worst["rew"] = max(worst["rew"], float(np.abs(h_rew - o_rew).max()))
        if done.any():
            d = as_oracle_obs(h_tobs[done], att) - oracle_obs_without_action(o_tobs[done], att)
            np.testing.assert_allclose(d, 0.0, err_msg=f"terminal obs step {t}", **tol)
            worst["tobs"] = max(worst["tobs"], float(np.abs(d).max()))
        sh, so = hip_env.get_state(), ora_env.get_state()
        np.testing.assert_allclose(sh[:, keep], so[:, keep], err_msg=f"state step {t}", **tol)
        worst["state"] = max(worst["state"], float(np.abs(sh[:, keep] - so[:, keep]).max()))
        worst["dones"] += int(done.sum())
    return worst


def run_lowlevel_lockstep(hip_env, ora_env, triple, steps, rng, atol=1e-7, actions=None):
    """The low-level kernel's rigid state and actuators against the oracle's mode-0 path behind the routing mixer of `triple`,
    for every env until its first episode end on either side (the oracle has no low-level task).  Returns the worst deviation
    and the number of env-steps compared."""
    import torch
    from pyflyt_drone_amd import config as K
    n = hip_env.num_envs
    hip_env.reset_tensor(); ora_env.reset()
    alive = np.ones(n, dtype=bool)
    rigid = slice(0, K.S_ACT + K.FW_NUM_ACTUATORS)
    worst = dict(state=0.0, compared=0)
    np.testing.assert_allclose(hip_env.get_state()[:, rigid], ora_env.get_state()[:, rigid], rtol=0, atol=atol, err_msg="start state")
    for t in range(steps):
        if actions is None:
            a4 = rng.uniform(-1.0, 1.0, size=(n, 4))
            a4[:, :3] *= 0.3
        else:
            a4 = actions(rng, n)
        _, _, o_term, o_trunc, _, _ = ora_env.step(a4)
        hip_env.step_tensor(torch.as_tensor(route(a4, triple), device=hip_env.device))
        done = (o_term | o_trunc).astype(bool) | (hip_env.terminated | hip_env.truncated).cpu().numpy().astype(bool)
        live = alive & ~done
        sh, so = hip_env.get_state(), ora_env.get_state()
        np.testing.assert_allclose(sh[live][:, rigid], so[live][:, rigid], rtol=0, atol=atol, err_msg=f"rigid state step {t}")
        if live.any():
            worst["state"] = max(worst["state"], float(np.abs(sh[live][:, rigid] - so[live][:, rigid]).max()))
        worst["compared"] += int(live.sum())
        alive &= ~done
    return worst
