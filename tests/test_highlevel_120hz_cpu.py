"""The controller-rate knob of the high-level command task (``controller_hz``), the parts that need no GPU:
the validation of the knob, and the reward fold the GPU test uses to compose one 30 Hz agent step from four 120 Hz ones."""
import numpy as np
import pytest

from pyflyt_drone_amd import rollout as R
from pyflyt_drone_amd.highlevel import CONTROL_HZ, HighLevelCmdVecEnv, check_controller_hz


def fold_rewards(r, event, last):
    """The reward of one agent step of ``K`` Aviary steps from the rewards ``r[K, N]`` of the same Aviary steps taken as agent
    steps of their own (``agent_hz = 120``).  The agent step starts at -0.1 (fixedwing_base_env.py:325-331); an Aviary step that
    reported a collision, an out-of-bounds or a waypoint reach (``event[K, N]``) replaces the reward by its own, any other adds
    its own less the -0.1 it started from.  Env ``i`` ran the Aviary steps ``0 .. last[i]`` (the early break at a done flag)."""
    r, event, last = np.asarray(r, dtype=np.float64), np.asarray(event, dtype=bool), np.asarray(last)
    out = np.full(r.shape[1], -0.1)
    for k in range(r.shape[0]):
        live = k <= last
        out = np.where(live & event[k], r[k], np.where(live, out + (r[k] + 0.1), out))
    return out


@pytest.mark.parametrize("hz", [7, 60, 240])
def test_controller_hz_is_validated_before_any_device_work(hz):
    pol = R.MlpPolicy(21, 6)
    rms = (np.zeros(21), np.ones(21))
    with pytest.raises(ValueError, match="controller_hz"):
        HighLevelCmdVecEnv(4, pol, rms, controller_hz=hz, device="cuda:0")
    with pytest.raises(ValueError, match="controller_hz"):
        check_controller_hz(hz, 30)


def test_controller_hz_values_that_name_a_path():
    assert CONTROL_HZ == 120
    assert check_controller_hz(None, 30) is False and check_controller_hz(30, 30) is False
    assert check_controller_hz(120, 30) is True and check_controller_hz(120, 60) is True
    assert check_controller_hz(120, 120) is False           # the agent step is one Aviary step: today's path is already 120 Hz
    for bad in (0, -120, 120.5, True, "120"):
        with pytest.raises((ValueError, TypeError)):
            check_controller_hz(bad, 30)


def test_reward_fold_against_a_plain_loop():
    g = np.random.default_rng(3)
    K_, n = 4, 257
    shaping = g.uniform(0.0, 2.0, (K_, n))
    event = g.uniform(size=(K_, n)) < 0.2
    r = np.where(event, g.choice([-100.0, 100.0, -100.0 + 0.37], size=(K_, n)), -0.1 + shaping)
    last = g.integers(0, K_, n)
    last[:8] = [0, 1, 2, 3, 3, 3, 0, 2]
    want = np.empty(n)
    for i in range(n):
        acc = -0.1
        for k in range(int(last[i]) + 1):
            if event[k, i]:
                acc = r[k, i]
            else:
                acc += r[k, i] + 0.1
        want[i] = acc
    got = fold_rewards(r, event, last)
    np.testing.assert_array_equal(got, want)
    # the shapes the fold is for: no event in four steps is -0.1 plus the four shaping terms; an event in the last step is its reward
    i = int(np.argmax((~event).all(axis=0) & (last == 3)))
    assert (~event[:, i]).all() and last[i] == 3
    np.testing.assert_allclose(got[i], -0.1 + shaping[:, i].sum(), rtol=0, atol=1e-12)
    j = int(np.argmax(event[3] & (last == 3)))
    assert event[3, j] and got[j] == r[3, j]
