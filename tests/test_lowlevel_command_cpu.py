"""Commanding the low-level controller without a GPU: the step-response figures (command.response_figures, DESIGN.md section 2d
"Commanding the controller") on hand-built traces, step_schedule, and the argument checks of fly and FixedwingLowLevelVecEnv.command."""
import math
import types

import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import command as CMD
from pyflyt_drone_amd import config as K

DT = CMD.AGENT_DT


def _trace(T, N):
    """a trace of N envs holding (psi, h, V) = (0, 10, 15) with actual values on the command, start rows the same"""
    tr = np.zeros((T, N, 8))
    tr[:, :, 0:6] = [0.0, 0.0, 10.0, 10.0, 15.0, 15.0]
    start = tr[0].copy()
    return tr, start


def _ct(tr, start, ended=None):
    N = tr.shape[1]
    return CMD.CommandTrace(trace=tr, start=start, schedule=np.zeros((tr.shape[0], N, 3)), dt=DT,
                            ended_at=np.full(N, -1) if ended is None else np.asarray(ended))


def test_altitude_step_by_hand():
    """h: 10 -> 20 at t0 = 0 over 20 steps; y = 10, 12, 14, 16, 18, 19.5, 20.5, 21, 20.8, 20.3, 20.1, 20.0 ... 20.0."""
    T = 20
    tr, start = _trace(T, 1)
    y = np.array([12, 14, 16, 18, 19.5, 20.5, 21, 20.8, 20.3, 20.1] + [20.0] * 10, dtype=float)
    tr[:, 0, 2], tr[:, 0, 3] = 20.0, y
    res = CMD.response_figures(_ct(tr, start))
    (s,) = [r for r in res["steps"] if r["axis"] == "altitude"]
    assert (s["env"], s["t0"], s["t1"], s["delta"]) == (0, 0, T, 10.0)
    # |e| <= 1 first at row 4 (y = 19.5): 5 steps after the command
    assert s["t90"] == pytest.approx(5 * DT)
    assert s["overshoot"] == pytest.approx(0.1)                # max y = 21: 1 m beyond a 10 m step
    # band = max(0.5, 0.5) = 0.5: rows 6 (21) and 7 (20.8) are outside, from row 8 (20.3) on it stays inside
    assert s["settling"] == pytest.approx(9 * DT)
    assert s["ss_error"] == pytest.approx(0.0)                 # last 10 % = 2 rows at 20.0
    assert res["summary"]["altitude_steps"] == 1 and res["summary"]["altitude_reached"] == 1.0
    # the other axes did not move: below their floors, no steps
    assert res["summary"]["heading_steps"] == 0 and res["summary"]["airspeed_steps"] == 0
    assert math.isnan(res["summary"]["heading_t90"])
    e = 20.0 - y
    assert res["summary"]["altitude_mae"] == pytest.approx(np.mean(np.abs(e)))
    assert res["summary"]["altitude_rmse"] == pytest.approx(math.sqrt(np.mean(e * e)))
    assert res["summary"]["survival_rate"] == 1.0


def test_second_segment_starts_from_the_row_before_it_and_the_floor_drops_small_steps():
    T = 40
    tr, start = _trace(T, 1)
    tr[:20, 0, 4] = 15.3                                        # V: 15 -> 15.3 (below the 0.5 m/s floor) ...
    tr[20:, 0, 4] = 13.0                                        # ... then 15.3 -> 13 at t0 = 20
    tr[:, 0, 5] = 15.0
    tr[19, 0, 5] = 15.2                                         # y0 of the second segment: the row before it
    tr[20:, 0, 5] = np.linspace(14.0, 13.1, 20)
    res = CMD.response_figures(_ct(tr, start))
    steps = [r for r in res["steps"] if r["axis"] == "airspeed"]
    assert len(steps) == 1
    (s,) = steps
    assert (s["t0"], s["t1"]) == (20, 40)
    assert s["delta"] == pytest.approx(13.0 - 15.2)
    # never within 0.22 m/s (0.1 |delta|): y ends at 13.1 -> |e| = 0.1 at the last row only
    ae = np.abs(13.0 - np.linspace(14.0, 13.1, 20))
    first = int(np.nonzero(ae <= 0.22)[0][0])
    assert s["t90"] == pytest.approx((first + 1) * DT)
    assert s["overshoot"] == 0.0
    assert s["ss_error"] == pytest.approx(np.mean(ae[-2:]))    # 10 % of 20 rows


def test_heading_step_wraps_across_pi():
    """psi: command 3.0 from an actual -3.0: the short way is -0.283 rad (across +-pi), not +6.0"""
    T = 10
    tr, start = _trace(T, 1)
    start[0, 1] = -3.0
    tr[:, 0, 0] = 3.0
    y = np.array([-3.05, -3.1, 3.13, 3.05, 3.01, 2.97, 2.99, 3.0, 3.0, 3.0])
    tr[:, 0, 1] = y
    res = CMD.response_figures(_ct(tr, start))
    (s,) = [r for r in res["steps"] if r["axis"] == "heading"]
    d = (3.0 - (-3.0) + math.pi) % (2 * math.pi) - math.pi
    assert d == pytest.approx(6.0 - 2 * math.pi) and s["delta"] == pytest.approx(d)
    e = (3.0 - y + math.pi) % (2 * math.pi) - math.pi
    first = int(np.nonzero(np.abs(e) <= 0.1 * abs(d))[0][0])
    assert first == 4 and s["t90"] == pytest.approx(5 * DT)
    assert s["overshoot"] == pytest.approx(max(0.0, np.max(-np.sign(d) * e)) / abs(d))
    assert s["overshoot"] == pytest.approx(0.03 / abs(d))      # y = 2.97 is 0.03 past the command in the direction of the step
    assert res["summary"]["heading_mae"] == pytest.approx(np.mean(np.abs(e)))


def test_an_env_that_terminates_mid_segment():
    """env 1 terminates at step 5: its steps after the end are excluded, the segment is cut there, a never-settled step is NaN"""
    T = 12
    tr, start = _trace(T, 2)
    tr[:, :, 2] = 14.0                                          # h: 10 -> 14 for both envs
    tr[:, 0, 3] = np.linspace(11.0, 14.0, T)
    tr[:, 1, 3] = [10.5, 10.0, 9.0, 7.0, 4.0, 0.9] + [10.0] * 6      # env 1 falls; rows 6.. belong to a new episode
    tr[5, 1, 7] = CMD.FLAG_TERMINATED
    res = CMD.response_figures(_ct(tr, start, ended=[-1, 5]))
    by_env = {r["env"]: r for r in res["steps"] if r["axis"] == "altitude"}
    assert by_env[1]["t1"] == 6 and by_env[1]["steps"] == 6
    assert math.isnan(by_env[1]["t90"]) and math.isnan(by_env[1]["settling"])
    assert by_env[1]["ss_error"] == pytest.approx(14.0 - 0.9)
    assert by_env[0]["t1"] == T
    e0, e1 = 14.0 - tr[:, 0, 3], 14.0 - tr[:6, 1, 3]
    n = T + 6
    assert res["summary"]["altitude_mae"] == pytest.approx((np.abs(e0).sum() + np.abs(e1).sum()) / n)
    assert res["summary"]["altitude_reached"] == 0.5
    assert res["summary"]["altitude_t90"] == pytest.approx(by_env[0]["t90"])      # the median of the finite ones
    assert res["summary"]["survival_rate"] == 0.5


def test_step_schedule_shapes_and_broadcasting():
    s = CMD.step_schedule([(3, (0.0, 10.0, 15.0)), (2, (1.0, 12.0, 16.0))], 4, "cpu")
    assert s.shape == (5, 4, 3) and s.dtype == torch.float64 and s.is_contiguous()
    assert torch.equal(s[:3], torch.tensor([0.0, 10.0, 15.0], dtype=torch.float64).expand(3, 4, 3))
    assert torch.equal(s[3:], torch.tensor([1.0, 12.0, 16.0], dtype=torch.float64).expand(2, 4, 3))
    per_env = np.arange(12, dtype=float).reshape(4, 3)
    s = CMD.step_schedule([(2, per_env), (1, torch.zeros(3))], 4)
    assert s.shape == (3, 4, 3)
    np.testing.assert_array_equal(s[0].numpy(), per_env)
    np.testing.assert_array_equal(s[1].numpy(), per_env)
    assert not s[2].any()
    with pytest.raises(ValueError):
        CMD.step_schedule([(2, np.zeros((3, 3)))], 4)
    with pytest.raises(ValueError):
        CMD.step_schedule([(0, (0.0, 10.0, 15.0))], 4)
    with pytest.raises(ValueError):
        CMD.step_schedule([], 4)


def _stub_env(max_steps=100, n=4, training=False, task=K.FW_TASK_LOWLEVEL):
    cfg = K.lowlevel_config(max_episode_steps=max_steps)
    cfg.task = task
    return types.SimpleNamespace(venv=types.SimpleNamespace(cfg=cfg), training=training, num_envs=n)


def test_fly_refuses_schedules_longer_than_an_episode():
    sched = CMD.step_schedule([(101, (0.0, 10.0, 15.0))], 4)
    with pytest.raises(ValueError, match="longer than an episode"):
        CMD.fly(None, _stub_env(100), sched)
    with pytest.raises(ValueError, match="training=False"):
        CMD.fly(None, _stub_env(200, training=True), sched)
    with pytest.raises(ValueError, match="low-level"):
        CMD.fly(None, _stub_env(200, task=K.FW_TASK_WAYPOINTS), sched)
    with pytest.raises(ValueError, match="shape"):
        CMD.fly(None, _stub_env(200, n=3), sched)


def test_command_checks_its_arguments_before_the_device():
    env = object.__new__(P.FixedwingLowLevelVecEnv)        # (no device needed for the checks)
    env.num_envs, env.device = 4, torch.device("cpu")
    for bad in (np.zeros((4, 2)), np.zeros((3, 3)), np.zeros(4), np.zeros((1, 4, 3))):
        with pytest.raises(ValueError, match="cmd must have shape"):
            env.command(bad)
    with pytest.raises(ValueError, match="mask"):
        env.command(np.zeros(3), mask=np.ones(3))
