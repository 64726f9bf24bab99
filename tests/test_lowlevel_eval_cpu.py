"""The low-level controller's evaluation figures (EvalResult.tracking_scalars) on hand-built results."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from pyflyt_drone_amd import _lib, evaluate
from pyflyt_drone_amd import config as K


def _two_episodes():
    # a short episode with large errors that crashed, a long one with small errors that was truncated
    r = evaluate.EvalResult([-50.0, -20.0], [10, 90])
    r.add_tracking([20.0, 60.0, 30.0, 150.0, 5.0, 4.0, 2.0], survived=False)       # |e_psi|, e_psi^2, |e_h|, e_h^2, |e_V|, e_V^2, w
    r.add_tracking([9.0, 1.8, 18.0, 5.4, 4.5, 0.9, 45.0], survived=True)
    return r


def test_tracking_scalars_pool_over_steps_not_over_episodes():
    r = _two_episodes()
    sc = r.tracking_scalars()
    assert set(sc) == {"eval/heading_mae", "eval/heading_rmse", "eval/altitude_mae", "eval/altitude_rmse", "eval/airspeed_mae",
                       "eval/airspeed_rmse", "eval/ang_vel_mean", "eval/survival_rate"}
    assert sc["eval/heading_mae"] == pytest.approx((20.0 + 9.0) / 100)
    assert sc["eval/heading_rmse"] == pytest.approx(math.sqrt((60.0 + 1.8) / 100))
    assert sc["eval/altitude_mae"] == pytest.approx((30.0 + 18.0) / 100)
    assert sc["eval/altitude_rmse"] == pytest.approx(math.sqrt((150.0 + 5.4) / 100))
    assert sc["eval/airspeed_mae"] == pytest.approx((5.0 + 4.5) / 100)
    assert sc["eval/airspeed_rmse"] == pytest.approx(math.sqrt((4.0 + 0.9) / 100))
    assert sc["eval/ang_vel_mean"] == pytest.approx((2.0 + 45.0) / 100)
    assert sc["eval/survival_rate"] == 0.5
    # the mean of per-episode averages is another figure here: (20/10 + 9/90) / 2 = 1.05, against 0.29 pooled
    per_episode = (20.0 / 10 + 9.0 / 90) / 2
    assert abs(per_episode - sc["eval/heading_mae"]) > 0.5


def test_rmse_is_at_least_mae():
    sc = _two_episodes().tracking_scalars()
    for q in ("heading", "altitude", "airspeed"):
        assert sc[f"eval/{q}_rmse"] >= sc[f"eval/{q}_mae"]


def test_scalars_keep_their_keys_and_other_tasks_get_no_tracking_figures():
    r = _two_episodes()
    assert set(r.scalars()) == {"eval/mean_reward", "eval/mean_ep_length"}
    assert r.tracking_scalars().keys().isdisjoint(r.scalars())
    assert evaluate.EvalResult([1.0], [5]).tracking_scalars() == {}


def test_track_terms_follow_the_definitions():
    """evaluate._track_terms (the step-by-step loop's statement of fw_eval_track_ll) on random rows, against the definitions in
    plain Python: e_psi = (o[18] - o[5] + pi) % 2 pi - pi, e_h = o[19] - o[11], e_V = o[20] - |o[6:9]|, w = |o[0:3]|."""
    rng = np.random.default_rng(3)
    o = rng.normal(0.0, 4.0, size=(64, 21))
    o[:8, 18], o[:8, 5] = math.pi, -math.pi                  # heading errors on the wrap's edge
    got = evaluate._track_terms(torch.as_tensor(o)).numpy()
    for i, row in enumerate(o):
        e_psi = (row[18] - row[5] + math.pi) % (2 * math.pi) - math.pi
        e_h, e_v = row[19] - row[11], row[20] - math.sqrt(sum(x * x for x in row[6:9]))
        want = [abs(e_psi), e_psi ** 2, abs(e_h), e_h ** 2, abs(e_v), e_v ** 2, math.sqrt(sum(x * x for x in row[0:3]))]
        np.testing.assert_allclose(got[i], want, rtol=1e-14, atol=1e-15)
    assert got[:8, 0].max() <= math.pi


def test_fw_eval_track_ll_refuses_bad_arguments_before_touching_a_buffer():
    L = _lib.lib()
    bufs = [np.zeros(64) for _ in range(17)]                 # host memory: only the addresses are looked at
    p = [b.ctypes.data_as(C.c_void_p) for b in bufs]

    def call(obs=p[4], obs_dim=21, N=8, E=2):
        return L.fw_eval_track_ll(p[0], 1, p[1], p[2], None, 0, obs, p[5], 1, obs_dim, p[6], p[7], p[8], p[9], p[10], p[11], p[12],
                                  p[13], p[14], None, p[15], N, E, None)
    assert call(obs=None) == K.FW_EINVAL
    assert call(obs_dim=20) == K.FW_EINVAL and "obs_dim must be 21" in L.fw_last_error(None).decode()
    assert call(E=0) == K.FW_EINVAL and call(N=-1) == K.FW_EINVAL
    assert L.fw_eval_track_ll(None, 1, None, None, None, 0, None, None, 1, 21, *([None] * 11), 8, 2, None) == K.FW_EINVAL
