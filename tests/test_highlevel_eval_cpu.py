"""The high-level command task's evaluation figures on the host: evaluate._track_terms_hl (the torch statement of fw_eval_track_hl)
against a plain-Python loop, EvalResult.command_scalars on hand-filled results, highlevel.trace_rows_hl against numpy, and the
EvalCallback keyword (DESIGN.md section 2e "Evaluation")."""
import math

import numpy as np
import pytest
import torch

from pyflyt_drone_amd import evaluate, highlevel

ALT_HIGH, SPEED_HIGH = 200.0, 30.0


def _wrap(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def _rows():
    """64 random rows, then hand-made ones: heading pairs across +-pi, first steps, commands on each of the four bounds and just inside"""
    rng = np.random.default_rng(11)
    n = 64
    o = rng.normal(0.0, 4.0, size=(n, 30))
    c = np.stack([rng.uniform(-math.pi, math.pi, n), rng.uniform(5.0, 195.0, n), rng.uniform(1.0, 29.0, n)], axis=1)
    p = np.stack([rng.uniform(-math.pi, math.pi, n), rng.uniform(5.0, 195.0, n), rng.uniform(1.0, 29.0, n)], axis=1)
    first = rng.random(n) < 0.25
    # heading: command and actual / previous command on either side of the wrap -- the short way round is 0.2 rad, not 2 pi - 0.2
    c[0, 0], o[0, 5], p[0, 0] = math.pi - 0.1, -math.pi + 0.1, -math.pi + 0.1
    c[1, 0], o[1, 5], p[1, 0] = -math.pi + 0.05, math.pi - 0.05, math.pi - 0.15
    c[2, 0], o[2, 5], p[2, 0] = -math.pi, math.pi, math.pi                       # exactly on the edge
    first[:3] = False
    first[3:6] = True                                                          # first steps: no command change whatever p holds
    p[3:6] = 1e3
    # the four bounds, each alone, and one row just inside all of them
    c[6, 1:], c[7, 1:], c[8, 1:], c[9, 1:] = (0.0, 15.0), (ALT_HIGH, 15.0), (100.0, 0.0), (100.0, SPEED_HIGH)
    c[10, 1:] = (np.nextafter(ALT_HIGH, 0.0), np.nextafter(SPEED_HIGH, 0.0))
    c[11, 1:] = (np.nextafter(0.0, 1.0), np.nextafter(0.0, 1.0))
    return o, c, p, first


def test_track_terms_hl_follow_the_definitions():
    o, c, p, first = _rows()
    got = evaluate._track_terms_hl(torch.as_tensor(o), torch.as_tensor(c), torch.as_tensor(p), torch.as_tensor(first),
                                   ALT_HIGH, SPEED_HIGH)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(o), 11) and got.device.type == "cpu"
    got = got.numpy()
    for i in range(len(o)):
        e_psi = _wrap(c[i, 0] - o[i, 5])
        e_h = c[i, 1] - o[i, 11]
        e_v = c[i, 2] - math.sqrt(o[i, 6] ** 2 + o[i, 7] ** 2 + o[i, 8] ** 2)
        w = math.sqrt(o[i, 0] ** 2 + o[i, 1] ** 2 + o[i, 2] ** 2)
        if first[i]:
            d = (0.0, 0.0, 0.0)
        else:
            d = (abs(_wrap(c[i, 0] - p[i, 0])), abs(c[i, 1] - p[i, 1]), abs(c[i, 2] - p[i, 2]))
        sat = 1.0 if (c[i, 1] <= 0.0 or c[i, 1] >= ALT_HIGH or c[i, 2] <= 0.0 or c[i, 2] >= SPEED_HIGH) else 0.0
        want = [abs(e_psi), e_psi * e_psi, abs(e_h), e_h * e_h, abs(e_v), e_v * e_v, w, *d, sat]
        np.testing.assert_allclose(got[i], want, rtol=1e-13, atol=1e-15, err_msg=str(i))
    # the hand-made rows say what they were made to say
    assert got[0, 0] == pytest.approx(0.2, abs=1e-12) and got[0, 7] == pytest.approx(0.2, abs=1e-12)
    assert got[1, 0] == pytest.approx(0.1, abs=1e-12) and got[1, 7] == pytest.approx(0.2, abs=1e-12)
    assert got[2, 0] == 0.0 and got[2, 7] == 0.0
    assert (got[3:6, 7:10] == 0.0).all()
    assert got[6:10, 10].tolist() == [1.0, 1.0, 1.0, 1.0] and got[10, 10] == 0.0 and got[11, 10] == 0.0
    assert evaluate.HL_TRACK_SUMS[:7] == evaluate.TRACK_SUMS and len(evaluate.HL_TRACK_SUMS) == 11


def test_track_terms_hl_take_float32_rows_in_double():
    o, c, p, first = _rows()
    o32, c32 = o.astype(np.float32), c.astype(np.float32)
    a = evaluate._track_terms_hl(torch.as_tensor(o32), torch.as_tensor(c32), torch.as_tensor(p), torch.as_tensor(first), ALT_HIGH, SPEED_HIGH)
    b = evaluate._track_terms_hl(torch.as_tensor(o32.astype(np.float64)), torch.as_tensor(c32.astype(np.float64)), torch.as_tensor(p),
                                 torch.as_tensor(first), ALT_HIGH, SPEED_HIGH)
    assert a.dtype == torch.float64 and torch.equal(a, b)


def _two_episodes():
    # a 10-step episode with jumpy, saturated commands and a 90-step one with calm commands
    r = evaluate.EvalResult([-50.0, -20.0], [10, 90])
    r.add_command([20.0, 60.0, 30.0, 150.0, 5.0, 4.0, 2.0, 9.0, 18.0, 4.5, 10.0])
    r.add_command([9.0, 1.8, 18.0, 5.4, 4.5, 0.9, 45.0, 0.98, 1.96, 9.8, 0.0])
    r.rejected_actions = 3
    return r


def test_command_scalars_pool_over_steps_and_divide_the_changes_by_the_step_pairs():
    r = _two_episodes()
    sc = r.command_scalars()
    assert set(sc) == {"eval/cmd_heading_mae", "eval/cmd_heading_rmse", "eval/cmd_altitude_mae", "eval/cmd_altitude_rmse",
                       "eval/cmd_airspeed_mae", "eval/cmd_airspeed_rmse", "eval/ang_vel_mean", "eval/cmd_heading_delta",
                       "eval/cmd_altitude_delta", "eval/cmd_airspeed_delta", "eval/cmd_saturation_rate", "eval/rejected_actions"}
    assert sc["eval/cmd_heading_mae"] == pytest.approx((20.0 + 9.0) / 100)
    assert sc["eval/cmd_heading_rmse"] == pytest.approx(math.sqrt((60.0 + 1.8) / 100))
    assert sc["eval/cmd_altitude_mae"] == pytest.approx((30.0 + 18.0) / 100)
    assert sc["eval/cmd_altitude_rmse"] == pytest.approx(math.sqrt((150.0 + 5.4) / 100))
    assert sc["eval/cmd_airspeed_mae"] == pytest.approx((5.0 + 4.5) / 100)
    assert sc["eval/cmd_airspeed_rmse"] == pytest.approx(math.sqrt((4.0 + 0.9) / 100))
    assert sc["eval/ang_vel_mean"] == pytest.approx((2.0 + 45.0) / 100)
    # 100 steps in 2 episodes: 98 pairs of consecutive steps
    assert sc["eval/cmd_heading_delta"] == pytest.approx((9.0 + 0.98) / 98)
    assert sc["eval/cmd_altitude_delta"] == pytest.approx((18.0 + 1.96) / 98)
    assert sc["eval/cmd_airspeed_delta"] == pytest.approx((4.5 + 9.8) / 98)
    assert sc["eval/cmd_saturation_rate"] == pytest.approx(10.0 / 100)
    assert sc["eval/rejected_actions"] == 3
    # pooled, not the mean of the episodes' means: (20/10 + 9/90) / 2 = 1.05 against 0.29
    assert abs((20.0 / 10 + 9.0 / 90) / 2 - sc["eval/cmd_heading_mae"]) > 0.5
    assert abs((10.0 / 10 + 0.0 / 90) / 2 - sc["eval/cmd_saturation_rate"]) > 0.3


def test_command_deltas_are_zero_when_no_episode_has_a_second_step():
    r = evaluate.EvalResult([1.0, 2.0, 3.0], [1, 1, 1])
    for _ in range(3):
        r.add_command([0.1, 0.01, 2.0, 4.0, 1.0, 1.0, 0.3, 0.0, 0.0, 0.0, 1.0])
    sc = r.command_scalars()
    assert sc["eval/cmd_heading_delta"] == sc["eval/cmd_altitude_delta"] == sc["eval/cmd_airspeed_delta"] == 0.0
    assert sc["eval/cmd_saturation_rate"] == 1.0 and sc["eval/cmd_altitude_mae"] == pytest.approx(2.0)


def test_the_two_sets_of_figures_keep_to_their_tasks():
    hl = _two_episodes()
    assert hl.tracking_scalars() == {} and hl.survived == []
    assert set(hl.scalars()) == {"eval/mean_reward", "eval/mean_ep_length"}
    plain = evaluate.EvalResult([1.0], [5])
    assert plain.command_scalars() == {} and plain.rejected_actions == 0
    ll = evaluate.EvalResult([-50.0], [10])
    ll.add_tracking([20.0, 60.0, 30.0, 150.0, 5.0, 4.0, 2.0], survived=False)
    assert ll.command_scalars() == {} and ll.tracking_scalars() != {}


def test_trace_rows_hl_against_numpy():
    rng = np.random.default_rng(5)
    n = 37
    o = rng.normal(0.0, 3.0, size=(n, 30))
    c = rng.normal(0.0, 3.0, size=(n, 3))
    info = rng.integers(0, 5, size=(n, 4)).astype(np.int32)
    flag = rng.integers(0, 3, size=n)
    got = highlevel.trace_rows_hl(torch.as_tensor(o), torch.as_tensor(c), torch.as_tensor(info), torch.as_tensor(flag)).numpy()
    want = np.stack([c[:, 0], o[:, 5], c[:, 1], o[:, 11], c[:, 2], np.sqrt(o[:, 6] ** 2 + o[:, 7] ** 2 + o[:, 8] ** 2),
                     np.sqrt(o[:, 0] ** 2 + o[:, 1] ** 2 + o[:, 2] ** 2), o[:, 9], o[:, 10], info[:, 0].astype(np.float64),
                     flag.astype(np.float64)], axis=1)
    np.testing.assert_allclose(got, want, rtol=1e-15, atol=0)
    for k in (0, 1, 2, 3, 4, 7, 8, 9, 10):                                    # the copied columns: bit for bit
        np.testing.assert_array_equal(got[:, k], want[:, k])
    bare = highlevel.trace_rows_hl(torch.as_tensor(o.astype(np.float32)), torch.as_tensor(c.astype(np.float32))).numpy()
    assert bare.dtype == np.float64 and (bare[:, 9] == 0).all() and (bare[:, 10] == 0).all()
    assert len(highlevel.HL_TRACE_COLS) == 11 == got.shape[1]
    assert highlevel.HL_TRACE_COLS[0] == "heading_cmd" and highlevel.HL_TRACE_COLS[-2:] == ("targets_reached", "flag")


def test_eval_callback_stores_use_fused():
    assert evaluate.EvalCallback(None).use_fused is None
    assert evaluate.EvalCallback(None, use_fused=True).use_fused is True
    assert evaluate.EvalCallback(None, use_fused=False).use_fused is False
