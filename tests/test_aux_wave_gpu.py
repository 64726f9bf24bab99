"""The headline step kernel with a noise wave (fwsim.hip: fw_step_kernel_g8x, step_body AUX): a second wave per step workgroup
draws the launch's motor noise, the step wave picks it up from LDS behind one workgroup barrier.

fw_create picks it for the axis-aligned f64 kernel with motor noise, up to 4096 envs; FWSIM_AUX_WAVE=0|1 overrides.  The results
must be bit-identical to the one-wave kernel (twins: the same config, seed and actions, one handle created under FWSIM_AUX_WAVE=0)
and track the CPU oracle at the parity suite's tolerance.  Shapes: 8 envs = one full tile, 11 = a ragged second tile with
inactive lanes, 64 = 8 tiles (the XCD block map is active).  The configs end episodes early (a 0.5 s time limit, a 14 m dome) so
that the short traces cover auto-resets -- whole tiles resetting in one step among them -- with the pre-sampled scenario, with the
in-kernel fallback (FWSIM_NO_SHADOW=1), and without auto-reset (done envs stay done and draw no noise).
"""
import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from helpers import run_lockstep, seeded_actions
from test_axis_aligned_gpu import _tilted_config

pytestmark = pytest.mark.gpu

SEED = 7
# (config overrides, envs, steps, episodes that end in the CPU oracle's trace)
CASES = {
    "limit_n8": (dict(max_duration_seconds=0.5), 8, 40, 16),        # all truncations; twice every env of the tile resets in one step
    "limit_n11": (dict(max_duration_seconds=0.5), 11, 40, 22),
    "dome_n11": (dict(flight_dome_size=14.0), 11, 60, 44),          # terminations, up to 9 in one step
    "dome_n64": (dict(flight_dome_size=14.0), 64, 60, 256),
    "default_n64": (dict(), 64, 150, 59),
}
OUTPUTS = ("obs", "rewards", "terminated", "truncated", "terminal_obs", "info")


def _aux(env):
    return int(_lib.lib().fw_aux_wave(env._h))


def _twins(monkeypatch, n, **kw):
    """(noise-wave handle, one-wave handle) of the same config and seed"""
    monkeypatch.delenv("FWSIM_AUX_WAVE", raising=False)
    new = P.FixedwingVecEnv(K.train_waypoints_v3_config(**kw), n, device=0, seed=SEED)
    monkeypatch.setenv("FWSIM_AUX_WAVE", "0")
    old = P.FixedwingVecEnv(K.train_waypoints_v3_config(**kw), n, device=0, seed=SEED)
    monkeypatch.delenv("FWSIM_AUX_WAVE")
    assert _aux(new) == 1 and _aux(old) == 0
    return new, old


def _run_twins(new, old, n, steps):
    """Drive both with the same actions; every output equal after every step, state and counters at the end.  Returns (dones, counters)."""
    assert np.array_equal(new.reset_tensor().cpu().numpy(), old.reset_tensor().cpu().numpy())
    rng = np.random.default_rng(5)
    dones = 0
    for t in range(steps):
        a = torch.as_tensor(seeded_actions(rng, n), device=new.device)
        new.step_tensor(a); old.step_tensor(a)
        for name in OUTPUTS:
            x, y = getattr(new, name).cpu().numpy(), getattr(old, name).cpu().numpy()
            assert np.array_equal(x, y), f"{name} differs at step {t}: rows {np.nonzero((x != y).reshape(n, -1).any(1))[0][:8]}"
        dones += int((new.terminated | new.truncated).sum())
    assert np.array_equal(new.get_state(), old.get_state())
    cn, co = new.get_counters(), old.get_counters()
    assert cn == co
    return dones, cn


def test_selection(monkeypatch):
    monkeypatch.delenv("FWSIM_AUX_WAVE", raising=False)
    cfg = K.train_waypoints_v3_config
    assert _aux(P.FixedwingVecEnv(cfg(), 4096, device=0, seed=1)) == 1
    assert _aux(P.FixedwingVecEnv(cfg(dtype="float32"), 4096, device=0, seed=1)) == 0
    assert _aux(P.FixedwingVecEnv(cfg(wind_config=K.TRAIN_OBJLOCK_WIND), 4096, device=0, seed=1)) == 0
    assert _aux(P.FixedwingVecEnv(_tilted_config(), 4096, device=0, seed=1)) == 0
    assert _aux(P.FixedwingVecEnv(cfg(motor_noise=False), 4096, device=0, seed=1)) == 0
    assert _aux(P.FixedwingVecEnv(cfg(), 4097, device=0, seed=1)) == 0
    monkeypatch.setenv("FWSIM_AUX_WAVE", "0")
    assert _aux(P.FixedwingVecEnv(cfg(), 4096, device=0, seed=1)) == 0
    # the override forces the kernel only where its row exists
    monkeypatch.setenv("FWSIM_AUX_WAVE", "1")
    assert _aux(P.FixedwingVecEnv(cfg(), 4097, device=0, seed=1)) == 1
    assert _aux(P.FixedwingVecEnv(cfg(dtype="float32"), 64, device=0, seed=1)) == 0
    assert _aux(P.FixedwingVecEnv(cfg(motor_noise=False), 64, device=0, seed=1)) == 0


@pytest.mark.parametrize("case", list(CASES))
def test_twins_bit_identical(monkeypatch, case):
    kw, n, steps, ends = CASES[case]
    new, old = _twins(monkeypatch, n, **kw)
    dones, ctr = _run_twins(new, old, n, steps)
    assert dones == ends > 0, "the trace did not cover the auto-resets it is meant to"
    assert ctr["resets"] > 0 and ctr["scenario_hits"] > 0


@pytest.mark.parametrize("case", ["dome_n11", "dome_n64"])
def test_twins_bit_identical_on_the_fallback_path(monkeypatch, case):
    kw, n, steps, ends = CASES[case]
    monkeypatch.setenv("FWSIM_NO_SHADOW", "1")
    new, old = _twins(monkeypatch, n, **kw)
    dones, ctr = _run_twins(new, old, n, steps)
    assert dones == ends > 0 and ctr["fallbacks"] > 0 and ctr["scenario_hits"] == 0


def test_twins_bit_identical_without_auto_reset(monkeypatch):
    n = 11
    new, old = _twins(monkeypatch, n, flight_dome_size=14.0, auto_reset=False)
    dones, ctr = _run_twins(new, old, n, 30)
    assert dones > 0 and ctr["resets"] == 0          # done envs stay done (and are reported done again every step)


@pytest.mark.parametrize("case", list(CASES))
def test_tracks_oracle(monkeypatch, case):
    from oracle import fw_oracle as O
    monkeypatch.delenv("FWSIM_AUX_WAVE", raising=False)
    kw, n, steps, ends = CASES[case]
    cfg = K.train_waypoints_v3_config(**kw)
    env = P.FixedwingVecEnv(cfg, n, device=0, seed=SEED)
    assert _aux(env) == 1
    worst = run_lockstep(env, O.OracleEnv(cfg, n, seed=SEED), steps, np.random.default_rng(5), atol=1e-7)
    assert worst["dones"] == ends > 0
