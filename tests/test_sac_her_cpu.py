"""Hindsight goal relabelling from the replay ring, without a GPU: the exported symbols, the config rules, and sac.her_rows_reference
(the numpy statement of fw_replay_sample_her's contract, which tests/test_sac_her_gpu.py holds the kernel to) against per-env trajectory
lists that know nothing of ring arithmetic, with the known answers of a goal the transition itself achieved."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import sac as S

import her_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fw_sizeof_her_task", "fw_replay_sample_her", "fw_her_reward")
TASKS = {0: S.HerTask(0, 0.0, 0.0), 1: S.HerTask(1, HC.DOME, HC.MIN_SPEED)}


def test_the_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "fwsim.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", header), name
    assert "typedef struct fw_her_task" in header and C.sizeof(S.HerTask) == 12
    assert K.FW_ABI_VERSION == 7                                 # functions were added, none changed
    L = _lib.lib()                                               # the library has them too, and agrees on the struct
    for name in NEW:
        assert hasattr(L, name), name
    assert L.fw_sizeof_her_task() == C.sizeof(S.HerTask) and L.fw_abi_version() == 7


def test_config_validation():
    c = S.SACConfig()
    assert c.her_goals == 0 and c.her_horizon == 64 and c.her_relabel_prob == 0.0 and S.MAX_HER_HORIZON == 64
    assert S.SACConfig(her_goals=4).her_relabel_prob == 0.8 and S.SACConfig(her_goals=1, her_horizon=1).her_relabel_prob == 0.5
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError):
            S.SACConfig(her_goals=bad)
    for bad in (0, 65, -3, 7.5, False):
        with pytest.raises(ValueError):
            S.SACConfig(her_goals=4, her_horizon=bad)
    with pytest.raises(ValueError, match="not built"):           # HER with n-step returns
        S.SACConfig(her_goals=4, n_steps=3)
    assert S.SACConfig(her_goals=0, n_steps=3).n_steps == 3       # (either alone is fine)


def test_buffer_rules():
    off = S.ReplayBufferDevice(40, 4, 21, 6, "cpu")
    assert off.ends is None and off.her_goals == 0               # off: no side ring at all
    on = S.ReplayBufferDevice(40, 4, 21, 6, "cpu", her_goals=4, her_horizon=8, her_task=TASKS[0])
    assert on.ends.dtype == torch.uint8 and on.ends.shape == (40,) and on.her_prob == 0.8 and on.n_steps == 1
    for kw in (dict(her_goals=4), dict(her_goals=4, her_task=TASKS[0], n_steps=3), dict(her_goals=-1), dict(her_horizon=65),
               dict(her_goals=4, her_task=TASKS[0], her_horizon=0)):
        with pytest.raises(ValueError):
            S.ReplayBufferDevice(40, 4, 21, 6, "cpu", **kw)
    with pytest.raises(ValueError):                              # not the low-level task's rows
        S.ReplayBufferDevice(40, 4, 5, 2, "cpu", her_goals=4, her_task=TASKS[0])
    # checkpoints carry `ends` under the n-step rules
    on.ends.copy_(torch.arange(40) % 4); on.ring.normal_(); on.counters.copy_(torch.tensor([8, 40, 12, 5]))
    sd = on.state_dict(include_buffer=True)
    assert torch.equal(sd["ends"], on.ends) and "ends" not in on.state_dict() and "ends" not in off.state_dict(include_buffer=True)
    other = S.ReplayBufferDevice(40, 4, 21, 6, "cpu", her_goals=1, her_task=TASKS[1])
    other.load_state_dict(sd)
    assert torch.equal(other.ends, on.ends) and torch.equal(other.ring, on.ring)
    other.load_state_dict(on.state_dict())
    assert int(other.ends.sum()) == 0 and other.counters.tolist() == [0, 0, 12, 5]
    with pytest.raises(ValueError):                              # rows without ends cannot serve a relabelling learner
        on.load_state_dict(off.state_dict(include_buffer=True))


def test_her_task_of_the_env_configs():
    t = S.her_task_of(K.lowlevel_config())
    assert (t.variant, t.dome) == (0, 100.0)
    c = K.lowlevel_demo_config()
    t = S.her_task_of(c)
    assert (t.variant, t.dome, t.min_speed) == (1, float(c.flight_dome_size), float(c.lowlevel_min_speed)) and t.min_speed > 0
    for bad in (None, K.train_waypoints_v3_config()):
        with pytest.raises(ValueError):
            S.her_task_of(bad)


def test_the_script_places_the_ends_the_cases_need():
    stores = HC.script()
    for t, s in enumerate(stores):
        for e in range(HC.N_ENVS):
            assert (int(s[5][e]), int(s[6][e])) == HC.ENDS.get((t, e), (0, 0))
    kinds = set(HC.ENDS.values())
    assert kinds == {(1, 0), (0, 1), (1, 1)}
    assert any(t == HC.HALF - 1 for t, _ in HC.ENDS) and any(t == HC.STEPS - 1 for t, _ in HC.ENDS)      # an end in each newest step
    for stored in (HC.HALF, HC.STEPS):
        traj = HC.trajectories(stores[:stored])
        lengths = {HC.candidates(traj, e, t, 64) for e in range(HC.N_ENVS) for t in range(len(traj[e]))}
        assert len(lengths) >= 4 and min(lengths) == 1           # episodes of unequal lengths
    ring, cursor, size = HC.numpy_ring(stores)
    assert cursor == (HC.STEPS - HC.RING_STEPS) * HC.N_ENVS and cursor != 0 and size == len(ring)          # wrapped, not back at row 0
    ring, cursor, size = HC.numpy_ring(stores[:HC.HALF])
    assert size == HC.HALF * HC.N_ENVS == len(ring) // 2
    # inside an episode the goal columns stay, and a step's next_obs is the next step's obs
    a, b = stores[5], stores[6]
    assert np.array_equal(a[3], b[0]) and np.array_equal(a[0][:, 18:], a[3][:, 18:])


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("stored", [HC.HALF, HC.STEPS], ids=["half_full", "wrapped"])
@pytest.mark.parametrize("horizon", HC.HORIZONS)
def test_reference_against_the_trajectory_lists(horizon, stored, variant):
    stores = HC.script()[:stored]
    ring, cursor, size = HC.numpy_ring(stores)
    ends, traj, task = HC.numpy_ends(stores), HC.trajectories(stores), TASKS[variant]
    rng = np.random.default_rng(horizon)
    seen_j = set()
    for rep in range(6):
        idx = rng.permutation(size)
        draw = rng.integers(0, 2 ** 32, size, dtype=np.uint64)
        if rep == 0:
            draw[:] = 2 ** 32 - 1                                # the furthest candidate of every row
        relabel = rng.random(size) < 0.7 if rep else np.ones(size, dtype=bool)
        rows, js = S.her_rows_reference(ring, ends, cursor, size, HC.N_ENVS, idx, relabel, draw, horizon, task)
        assert rows.dtype == np.float32 and rows.shape == (size, HC.ROW) and js.dtype == np.int32
        assert np.array_equal(js >= 0, relabel)
        # a goal never comes from another episode, from beyond the newest row or from further than horizon - 1 steps ahead
        for e, t, j in HC.check_rows(rows, js, draw, traj, horizon, f"{stored} stores, rep {rep}"):
            assert j <= horizon - 1 and t + j < len(traj[e])
            if j >= 0:
                seen_j.add(j)
        # rows that are not relabelled equal the ring rows
        keep = ~relabel
        assert np.array_equal(rows[keep].view(np.uint32), ring[idx[keep]].view(np.uint32))
        # the reward of a relabelled row is the task's reward for its new goal, rounded once
        for b in np.flatnonzero(relabel):
            want = S.her_reward_reference(rows[b, HC.NOBS:HC.NOBS + 18], rows[b, 18:21], rows[b, -1], task)
            assert rows[b, HC.RCOL] == np.float32(want)
    longest = min(horizon, min(stored, HC.RING_STEPS))
    assert max(seen_j) == longest - 1 and min(seen_j) == 0       # (env 3 / env 2 fly through the whole window)


@pytest.mark.parametrize("stored", [HC.HALF, HC.STEPS])
def test_known_answers_for_a_goal_the_transition_itself_achieved(stored):
    stores = HC.script()[:stored]
    ring, cursor, size = HC.numpy_ring(stores)
    ends, idx = HC.numpy_ends(stores), np.arange(size)
    zero, ones = np.zeros(size, dtype=np.uint64), np.ones(size, dtype=bool)            # draw 0: j* = 0 whatever k is
    rows, js = S.her_rows_reference(ring, ends, cursor, size, HC.N_ENVS, idx, ones, zero, 64, TASKS[0])
    assert (js == 0).all()
    done = ring[idx, -1] != 0
    assert done.any() and not done.all()
    # variant 0: all three errors vanish, 0.1 is left, and 100 less where the step terminated
    assert np.array_equal(rows[~done, HC.RCOL], np.full(int((~done).sum()), np.float32(0.1)))
    assert np.array_equal(rows[done, HC.RCOL], np.full(int(done.sum()), np.float32(0.1 - 100.0)))
    assert np.array_equal(rows[:, 18:21], S.her_achieved_goal(ring[idx, HC.NOBS:HC.NOBS + 21]))
    # variant 1: the three tracking terms are exactly 0 -- what is left is the other four terms, added in the reward's own order, bit for bit
    rows1, _ = S.her_rows_reference(ring, ends, cursor, size, HC.N_ENVS, idx, ones, zero, 64, TASKS[1])
    no = ring[idx, HC.NOBS:HC.NOBS + 21].astype(np.float64)
    speed, rho = rows1[:, 20].astype(np.float64), np.sqrt(no[:, 9] * no[:, 9] + no[:, 10] * no[:, 10])
    aa = np.zeros(size)
    for k in range(12, 18):
        aa = aa + no[:, k] * no[:, k]
    rest = -0.3 * np.maximum(np.abs(no[:, 3]) - 35.0 * np.pi / 180.0, 0.0)
    rest = rest - 0.3 * np.maximum(np.abs(no[:, 4]) - 20.0 * np.pi / 180.0, 0.0)
    rest = rest - 0.05 * np.sqrt(aa)
    rest = rest - np.maximum(rho - HC.DOME, 0.0)
    rest = np.where(speed < HC.MIN_SPEED, rest - 2.0, rest)
    full = S.her_reward_reference(ring[idx, HC.NOBS:HC.NOBS + 21], rows1[:, 18:21], ring[idx, -1], TASKS[1])
    assert np.array_equal(full, rest) and np.array_equal(rows1[:, HC.RCOL], rest.astype(np.float32))
    for col, off, weight in ((18, 0.5, 1.5), (19, 3.0, 1.2), (20, 2.0, 0.8)):          # and each term alone costs its weight times the error
        g = rows1[:, 18:21].copy()
        g[:, col - 18] += np.float32(off)
        err = np.abs(g[:, col - 18].astype(np.float64) - rows1[:, col].astype(np.float64))
        if col == 18:
            err = np.abs((err + np.pi) % (2 * np.pi) - np.pi)
        moved = S.her_reward_reference(ring[idx, HC.NOBS:HC.NOBS + 21], g, ring[idx, -1], TASKS[1])
        assert np.abs((full - moved) - weight * err).max() <= 1e-12 * np.abs(full).max()
    assert (speed < HC.MIN_SPEED).any() and (rho > HC.DOME).any() and (np.abs(no[:, 3]) > 35.0 * np.pi / 180.0).any()      # the script exercises the penalties


def test_reference_rejects_what_the_entry_point_rejects():
    stores = HC.script()
    ring, cursor, size = HC.numpy_ring(stores)
    ends = HC.numpy_ends(stores)
    ok = (np.arange(4), np.ones(4, dtype=bool), np.zeros(4, dtype=np.uint64))
    for h in (0, 65):
        with pytest.raises(ValueError):
            S.her_rows_reference(ring, ends, cursor, size, HC.N_ENVS, *ok, h, TASKS[0])
    with pytest.raises(ValueError):
        S.her_rows_reference(ring[:, :49], ends, cursor, size, HC.N_ENVS, *ok, 8, TASKS[0])
    with pytest.raises(ValueError):
        S.her_rows_reference(ring, ends, cursor, size, HC.N_ENVS, np.array([size]), np.ones(1), np.zeros(1), 8, TASKS[0])
    with pytest.raises(ValueError):
        S.her_rows_reference(ring, ends, cursor, size, HC.N_ENVS, *ok, 8, S.HerTask(2, 0.0, 0.0))
