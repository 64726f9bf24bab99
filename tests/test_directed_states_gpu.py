"""The corner cases of tests/test_device_functions_gpu.py through the PRODUCTION kernels: the states of tests/directed_states.py
are set on the kernel and on the CPU oracle, both fly one agent step, and everything is compared as the lockstep tests compare
it (1e-7 absolute on observation, reward and state; flags and info exactly equal).  A probe kernel holds its own compiled copy of
every inline function; this is the check that the copies inside the step kernels take the same branches to the same result.

Branches entered (tests/test_device_functions_cpu.py asserts that each state is in its branch and well conditioned):
quat_integrate's angular-motion clamp (|w| > 188 rad/s), the exact-reciprocal paths of normalize_quat / two_over_norm2 /
1/sqrt(1 + e) (|q| = 1 +- 2e-4 and 3), post-stall on every surface, reverse flow, exact reverse flow (alpha = atan2(-0, v_f < 0):
the sign bit), sideways flow, V = 0, and both sides of the gimbal guard.
"""
import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import config as K
import directed_states as D
from helpers import as_oracle_obs, oracle_obs_without_action, route

pytestmark = pytest.mark.gpu
TOL = dict(rtol=0, atol=1e-7)

MAPPINGS = {"lane_per_env": ("1", "1"), "8_lanes_per_env": ("8", "1"), "8_lanes_2_waves_per_simd": ("8", "2")}
CASES = [(leg, m) for leg in ("waypoints", "waypoints_gust") for m in MAPPINGS] + [(leg, m) for leg in ("direct", "lowlevel") for m in list(MAPPINGS)[:2]]


@pytest.mark.parametrize("leg,mapping", CASES)
def test_one_step_from_the_directed_states(oracle, monkeypatch, leg, mapping):
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", MAPPINGS[mapping][0])
    monkeypatch.setenv("FWSIM_G8_WAVES", MAPPINGS[mapping][1])          # (the default sizes stay off the two-wave build: ask for it)
    cfg, ora_cfg, kind, triple = D.legs()[leg]
    n = D.NUM_ENVS
    hip = P.FixedwingVecEnv(cfg, n, seed=5)
    ora = oracle.OracleEnv(ora_cfg, n, seed=5)
    assert hip.lanes_per_env == int(MAPPINGS[mapping][0]) and hip.g8_waves == int(MAPPINGS[mapping][1])
    hip.reset_tensor(); ora.reset()
    sh, so = hip.get_state(), ora.get_state()
    names = D.apply(sh)
    assert D.apply(so) == names and set(names) == set(D.BRANCHES)
    rigid = slice(0, K.S_ACT + K.FW_NUM_ACTUATORS)
    np.testing.assert_array_equal(sh[:, :K.S_ACT], so[:, :K.S_ACT])
    hip.set_state(sh); ora.set_state(so)
    a4 = D.actions(n)
    o_obs, o_rew, o_term, o_trunc, o_tobs, o_info = ora.step(a4)
    a = a4 if kind == "waypoints" else route(a4, triple)
    hip.step_tensor(torch.as_tensor(a.astype(hip.np_dtype), device=hip.device))
    h_obs, h_rew = hip.obs.cpu().numpy(), hip.rewards.cpu().numpy()
    h_term, h_trunc, h_info = hip.terminated.cpu().numpy(), hip.truncated.cpu().numpy(), hip.info.cpu().numpy()
    sh, so = hip.get_state(), ora.get_state()
    worst = {}
    if kind == "lowlevel":
        # the oracle has no low-level task: the rigid state and the actuators of every env that did not end its episode
        live = ~((o_term | o_trunc).astype(bool) | (h_term | h_trunc).astype(bool))
        assert live.sum() >= n - 5
        worst["state"] = np.abs(sh[live][:, rigid] - so[live][:, rigid]).max(axis=1)
        names = [m for m, l in zip(names, live) if l]
    else:
        assert np.array_equal(h_term, o_term) and np.array_equal(h_trunc, o_trunc), "flags differ"
        assert np.array_equal(h_info, o_info), f"info differs in rows {np.nonzero((h_info != o_info).any(1))[0][:8]}"
        keep = np.ones(K.FW_STATE_DIM, dtype=bool)
        if kind == "direct":
            h_obs, o_obs = as_oracle_obs(h_obs, 12), oracle_obs_without_action(o_obs, 12)
            keep[K.S_ACTION:K.S_ACTION + 4] = False
            keep[K.S_TASK:] = False
        worst["obs"] = np.abs(h_obs - o_obs).max(axis=1)
        worst["rew"] = np.abs(h_rew - o_rew)
        worst["state"] = np.abs(sh[:, keep] - so[:, keep]).max(axis=1)
    for what, v in worst.items():
        per = {b: float(v[[m == b for m in names]].max()) for b in D.BRANCHES}
        print(f"{leg} {mapping} {what}: " + ", ".join(f"{b} {e:.1e}" for b, e in per.items()))
    for what, v in worst.items():
        assert np.isfinite(v).all() and v.max() <= 1e-7, (what, names[int(np.argmax(v))], float(v.max()))
