"""The headline step kernel compiled for the training config's shape (fwsim.hip: fw_step_kernel_g8xs, step_body SH =
ShapeTrainWaypoints): step_ratio 4, 2 ticks per control step, 2 of 8 waypoints in a 28-word euler row, sparse reward, motor noise
and the gyroscopic term are constants of the kernel, and max_steps / auto_reset / dome / reach are loaded once per launch.

fw_create picks it where the noise-wave kernel (fw_step_kernel_g8x) is picked and the config has exactly that shape;
FWSIM_STEP_SHAPE=0 turns it off and nothing turns it on elsewhere.  Only integers became constants, so the results must be
bit-identical to the noise-wave kernel (twins: the same config, seed and actions, one handle created under FWSIM_STEP_SHAPE=0)
and track the CPU oracle at the parity suite's tolerance.  Shapes and traces are those of tests/test_aux_wave_gpu.py: 8 envs = one
full tile, 11 = a ragged second tile with inactive lanes, 64 = 8 tiles (the XCD block map is active); a 0.5 s time limit and a
14 m dome end episodes early, so the short traces cover auto-resets -- whole tiles resetting in one step among them -- with the
pre-sampled scenario, with the in-kernel fallback (FWSIM_NO_SHADOW=1), and without auto-reset.  max_steps, dome and auto_reset
differ between those configs and are not part of the shape: the kernel must be selected for all of them.
"""
import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from helpers import run_lockstep, seeded_actions

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
# one field of the shape (or of the noise-wave row under it) changed at a time: (config overrides, envs)
OFF_SHAPE = {
    "agent_hz_60": (dict(agent_hz=60), 4096),
    "context_3": (dict(context_length=3), 4096),
    "targets_4": (dict(num_targets=4), 4096),
    "dense_reward": (dict(sparse_reward=False), 4096),
    "quaternion": (dict(angle_representation="quaternion"), 4096),
    "no_motor_noise": (dict(motor_noise=False), 4096),
    "float32": (dict(dtype="float32"), 4096),
    "wind": (dict(wind_config=K.TRAIN_OBJLOCK_WIND), 4096),
    "envs_4097": (dict(), 4097),
}


def _shape(env):
    return int(_lib.lib().fw_step_shape(env._h))


def _twins(monkeypatch, n, **kw):
    """(fixed-shape handle, run-time-shape handle) of the same config and seed"""
    monkeypatch.delenv("FWSIM_STEP_SHAPE", raising=False)
    new = P.FixedwingVecEnv(K.train_waypoints_v3_config(**kw), n, device=0, seed=SEED)
    monkeypatch.setenv("FWSIM_STEP_SHAPE", "0")
    old = P.FixedwingVecEnv(K.train_waypoints_v3_config(**kw), n, device=0, seed=SEED)
    monkeypatch.delenv("FWSIM_STEP_SHAPE")
    assert _shape(new) == 1 and _shape(old) == 0
    assert int(_lib.lib().fw_aux_wave(new._h)) == 1 and int(_lib.lib().fw_aux_wave(old._h)) == 1
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


def test_selected_for_the_training_config(monkeypatch):
    monkeypatch.delenv("FWSIM_STEP_SHAPE", raising=False)
    monkeypatch.delenv("FWSIM_AUX_WAVE", raising=False)
    cfg = K.train_waypoints_v3_config
    assert _shape(P.FixedwingVecEnv(cfg(), 4096, device=0, seed=1)) == 1
    monkeypatch.setenv("FWSIM_STEP_SHAPE", "0")
    assert _shape(P.FixedwingVecEnv(cfg(), 4096, device=0, seed=1)) == 0
    # 1 asks for nothing the config does not have: a kernel with another shape compiled in would compute another task
    monkeypatch.setenv("FWSIM_STEP_SHAPE", "1")
    assert _shape(P.FixedwingVecEnv(cfg(), 4096, device=0, seed=1)) == 1
    for name, (kw, n) in OFF_SHAPE.items():
        assert _shape(P.FixedwingVecEnv(cfg(**kw), n, device=0, seed=1)) == 0, name
    # ... and it follows the noise-wave row, not the env count as such
    monkeypatch.setenv("FWSIM_AUX_WAVE", "0")
    assert _shape(P.FixedwingVecEnv(cfg(), 4096, device=0, seed=1)) == 0


@pytest.mark.parametrize("name", list(OFF_SHAPE))
def test_off_shape_configs_keep_their_kernel_and_the_oracle(monkeypatch, name):
    """One field off the shape: the run-time-shape kernels step the config as before (5 steps against the CPU oracle)."""
    from oracle import fw_oracle as O
    monkeypatch.delenv("FWSIM_STEP_SHAPE", raising=False)
    kw, n_sel = OFF_SHAPE[name]
    n = n_sel if name == "envs_4097" else 11          # (the env count is the field here; the others are per config)
    cfg = K.train_waypoints_v3_config(**kw)
    env = P.FixedwingVecEnv(cfg, n, device=0, seed=SEED)
    assert _shape(env) == 0
    # float32 against the float64 oracle: the suite's own figure for one agent step from equal states is 2e-3
    # (test_parity_gpu.py, test_f32_throughput_mode_single_step_error); five steps add up to at most five times that
    atol = 5 * 2e-3 if name == "float32" else 1e-7
    ocfg = K.train_waypoints_v3_config(**{**kw, "dtype": "float64"})
    run_lockstep(env, O.OracleEnv(ocfg, n, seed=SEED), 5, np.random.default_rng(5), kind="gentle", atol=atol, rtol=0)


def test_off_by_the_environment_variable_tracks_the_oracle(monkeypatch):
    from oracle import fw_oracle as O
    monkeypatch.setenv("FWSIM_STEP_SHAPE", "0")
    cfg = K.train_waypoints_v3_config()
    env = P.FixedwingVecEnv(cfg, 11, device=0, seed=SEED)
    assert _shape(env) == 0
    run_lockstep(env, O.OracleEnv(cfg, 11, seed=SEED), 5, np.random.default_rng(5), kind="gentle", atol=1e-7, rtol=0)


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
    assert dones == ends > 0 and ctr["resets"] > 0 and ctr["fallbacks"] > 0 and ctr["scenario_hits"] == 0


def test_twins_bit_identical_without_auto_reset(monkeypatch):
    n = 11
    new, old = _twins(monkeypatch, n, flight_dome_size=14.0, auto_reset=False)      # (auto_reset is not part of the shape: selected)
    dones, ctr = _run_twins(new, old, n, 30)
    assert dones > 0 and ctr["resets"] == 0          # done envs stay done (and are reported done again every step)


@pytest.mark.parametrize("case", list(CASES))
def test_tracks_oracle(monkeypatch, case):
    from oracle import fw_oracle as O
    monkeypatch.delenv("FWSIM_STEP_SHAPE", raising=False)
    kw, n, steps, ends = CASES[case]
    cfg = K.train_waypoints_v3_config(**kw)
    env = P.FixedwingVecEnv(cfg, n, device=0, seed=SEED)
    assert _shape(env) == 1
    worst = run_lockstep(env, O.OracleEnv(cfg, n, seed=SEED), steps, np.random.default_rng(5), atol=1e-7)
    assert worst["dones"] == ends > 0


@pytest.mark.parametrize("case", ["dome_n11", "dome_n64"])
def test_tracks_oracle_on_the_fallback_path(monkeypatch, case):
    from oracle import fw_oracle as O
    monkeypatch.delenv("FWSIM_STEP_SHAPE", raising=False)
    monkeypatch.setenv("FWSIM_NO_SHADOW", "1")
    kw, n, steps, ends = CASES[case]
    cfg = K.train_waypoints_v3_config(**kw)
    env = P.FixedwingVecEnv(cfg, n, device=0, seed=SEED)
    assert _shape(env) == 1
    worst = run_lockstep(env, O.OracleEnv(cfg, n, seed=SEED), steps, np.random.default_rng(5), atol=1e-7)
    assert worst["dones"] == ends > 0


def test_tracks_oracle_without_auto_reset(monkeypatch):
    from oracle import fw_oracle as O
    monkeypatch.delenv("FWSIM_STEP_SHAPE", raising=False)
    cfg = K.train_waypoints_v3_config(flight_dome_size=14.0, auto_reset=False)
    env = P.FixedwingVecEnv(cfg, 11, device=0, seed=SEED)
    assert _shape(env) == 1
    worst = run_lockstep(env, O.OracleEnv(cfg, 11, seed=SEED), 30, np.random.default_rng(5), atol=1e-7)
    assert worst["dones"] > 0
