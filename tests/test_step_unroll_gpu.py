"""The fixed-shape step kernel (fw_step_kernel_g8xs) with its tick loop unrolled: both ticks of an Aviary step are one loop body.

Unrolled, the second copy of the tick came out with two groups of sums contracted into FMAs differently from the rolled body of
every other step kernel (R^T v and R^T w in front of the tick, the rotation matrix behind it); the fixed shape spells them out
(fwsim_device.hpp: mtv_fma, rot_from_unit_quat_fma), and the kernel must not differ from the rolled one by a bit -- on the
corner-case states that enter the rare branches of the tick (in both copies), and on traces where envs of one tile end their
agent steps after different sub-steps, so that lanes whose env is finished sit out ticks beside lanes that run them.

Twins as in tests/test_step_shape_gpu.py: the same config, seed and actions on a second handle created under FWSIM_STEP_SHAPE=0,
which runs the rolled kernel of the run-time shape.  All six outputs must be equal after every step, state and counters
at the end.

The traces (seed 7, uniform actions from default_rng(5), 14 m dome) were chosen on the CPU oracle alone: with auto_reset=False the
first env leaves the dome in step 11 and every env is done within the first 15 steps, and in between envs
finish after sub-step 0, 1 and 2 of a step (tick advances 2, 4 and 6 instead of 8) beside envs of the same tile that step on --
at 11 envs also in the ragged second tile, whose other five rows are inactive lanes.  The steps behind that run with every env
done at entry (the stale observation of bare-Gymnasium mode).
"""
import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
import directed_states as D
from helpers import run_lockstep, seeded_actions

pytestmark = pytest.mark.gpu

SEED = 7
OUTPUTS = ("obs", "rewards", "terminated", "truncated", "terminal_obs", "info")
DOME = dict(flight_dome_size=14.0)
MID_STEPS, STALE_STEPS = 15, 10          # every env of the oracle's trace is done within 15 steps; then ten steps done at entry
TICKS_PER_STEP = 8                       # step_ratio 4 x 2 ticks per Aviary step
SIZES = (8, 11, 64)


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
    return new, old


def _step_both(new, old, a, t):
    a = torch.as_tensor(a, device=new.device)
    new.step_tensor(a); old.step_tensor(a)
    n = new.num_envs
    for name in OUTPUTS:
        x, y = getattr(new, name).cpu().numpy(), getattr(old, name).cpu().numpy()
        assert np.array_equal(x, y), f"{name} differs at step {t}: rows {np.nonzero((x != y).reshape(n, -1).any(1))[0][:8]}"


def _same_at_the_end(new, old):
    assert np.array_equal(new.get_state(), old.get_state())
    assert new.get_counters() == old.get_counters()


def test_directed_states_twins(monkeypatch):
    """Stall on both sides, reverse flow, V = 0, the angular clamp and both renormalisation paths of the quaternion, in both
    copies of the unrolled tick: three agent steps from the states of tests/directed_states.py."""
    n = D.NUM_ENVS
    new, old = _twins(monkeypatch, n)
    assert np.array_equal(new.reset_tensor().cpu().numpy(), old.reset_tensor().cpu().numpy())
    sn, so = new.get_state(), old.get_state()
    names = D.apply(sn)
    assert D.apply(so) == names and set(names) == set(D.BRANCHES)
    assert np.array_equal(sn, so)
    new.set_state(sn); old.set_state(so)
    for t in range(3):
        _step_both(new, old, D.actions(n, seed=7 + t), t)
    assert np.isfinite(new.obs.cpu().numpy()).all()
    _same_at_the_end(new, old)


@pytest.mark.parametrize("n", SIZES)
def test_mid_step_finishes_without_auto_reset(monkeypatch, n):
    new, old = _twins(monkeypatch, n, auto_reset=False, **DOME)
    assert np.array_equal(new.reset_tensor().cpu().numpy(), old.reset_tensor().cpu().numpy())
    rng = np.random.default_rng(5)
    tick = new.get_state()[:, K.S_TICK_COUNT].copy()
    finished_after, mixed_tiles, ragged = set(), 0, 0
    for t in range(MID_STEPS):
        _step_both(new, old, seeded_actions(rng, n), t)
        now = new.get_state()[:, K.S_TICK_COUNT]
        adv = (now - tick).astype(int); tick = now.copy()
        assert ((adv >= 0) & (adv <= TICKS_PER_STEP) & (adv % 2 == 0)).all()
        finished_after |= {a // 2 - 1 for a in adv if 0 < a < TICKS_PER_STEP}
        for first in range(0, n, 8):
            a = adv[first:first + 8]
            mid = a[(a > 0) & (a < TICKS_PER_STEP)]
            if mid.size and (a > mid.min()).any():         # an env finished while another of its tile stepped on
                mixed_tiles += 1
                ragged += int(a.size < 8)
    assert finished_after == {0, 1, 2}, "the trace does not end agent steps after each of sub-steps 0, 1 and 2"
    assert mixed_tiles > 0, "no tile held a finished and a stepping env together"
    if n % 8:
        assert ragged > 0, "the ragged tile held no finished env beside a stepping one (and its inactive lanes)"
    done = (new.terminated | new.truncated).cpu().numpy().astype(bool)
    assert done.all()
    # every env is done at entry from here on: the stale observation, no tick, in both kernels
    for t in range(MID_STEPS, MID_STEPS + STALE_STEPS):
        _step_both(new, old, seeded_actions(rng, n), t)
    assert np.array_equal(new.get_state()[:, K.S_TICK_COUNT], tick)
    _same_at_the_end(new, old)
    assert new.get_counters()["resets"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_mid_step_finishes_with_auto_reset(monkeypatch, n):
    new, old = _twins(monkeypatch, n, **DOME)
    assert np.array_equal(new.reset_tensor().cpu().numpy(), old.reset_tensor().cpu().numpy())
    rng = np.random.default_rng(5)
    dones = 0
    for t in range(MID_STEPS + STALE_STEPS):
        _step_both(new, old, seeded_actions(rng, n), t)
        dones += int((new.terminated | new.truncated).sum())
    assert dones >= n                                       # (every env leaves the dome within 13 steps)
    _same_at_the_end(new, old)
    assert new.get_counters()["resets"] > 0


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_mid_step_traces_track_the_oracle(oracle, monkeypatch, n, auto_reset):
    monkeypatch.delenv("FWSIM_STEP_SHAPE", raising=False)
    cfg = K.train_waypoints_v3_config(auto_reset=auto_reset, **DOME)
    env = P.FixedwingVecEnv(cfg, n, device=0, seed=SEED)
    assert _shape(env) == 1
    worst = run_lockstep(env, oracle.OracleEnv(cfg, n, seed=SEED), MID_STEPS + STALE_STEPS, np.random.default_rng(5), atol=1e-7)
    assert worst["dones"] >= n
