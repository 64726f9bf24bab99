"""The high-level command task (train/train_highlevel_cmd.py:35-181) without a GPU: the direct-command waypoints task through the
host functions of the library, the numpy statement of the command conditioning on cases worked out by hand from the reference's
lines, and the argument errors of ``HighLevelCmdVecEnv`` that need no device."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R
from pyflyt_drone_amd.highlevel import HighLevelCmdVecEnv, condition_command


def _abi_validate(cfg):
    buf = C.create_string_buffer(256)
    rc = _lib.lib().fw_validate_config(C.byref(cfg), buf, 256)
    return rc, buf.value.decode()


def test_abi_accepts_the_task_and_reports_its_widths():
    L = _lib.lib()
    for rep, want in (("euler", 30), ("quaternion", 31)):
        c = K.waypoints_direct_config(angle_representation=rep, context_length=2)
        assert c.task == K.FW_TASK_WAYPOINTS_DIRECT
        assert _abi_validate(c) == (K.FW_OK, "")
        assert L.fw_obs_dim(C.byref(c)) == want == K.obs_dim(c)
        assert L.fw_act_dim(C.byref(c)) == 6 == K.act_dim(c)
    c = K.waypoints_direct_config(angle_representation="euler", context_length=3)
    assert L.fw_obs_dim(C.byref(c)) == 33
    _lib.validate(K.highlevel_config(wind_config={"enabled": True, "mode": "gust_sine", "randomize_on_reset": True}))
    c = K.waypoints_direct_config()
    c.agent_hz = 50                                       # validated as the waypoints task is
    rc, msg = _abi_validate(c)
    assert rc == K.FW_EINVAL and "agent_hz" in msg


def test_highlevel_config_is_the_reference_constructor():
    c = K.highlevel_config()                              # :51-62, 78-88
    assert c.task == K.FW_TASK_WAYPOINTS_DIRECT and c.angle_representation == 0
    assert (c.flight_dome_size, c.max_duration_seconds, c.agent_hz, c.context_length) == (200.0, 120.0, 30, 2)
    assert c.num_targets == 4 and c.goal_reach_distance == 2.0 and c.sparse_reward == 0      # the upstream defaults
    assert c.warmup_aviary_steps == 10 and list(c.start_vel) == [20.0, 0.0, 0.0] and c.wind_mode == K.FW_WIND_OFF
    assert K.obs_dim(c) == 30 and K.act_dim(c) == 6


def test_the_other_tasks_keep_their_widths_and_the_config_its_size():
    L = _lib.lib()
    assert C.sizeof(K.FwConfig) == L.fw_sizeof_config()
    assert L.fw_abi_version() == K.FW_ABI_VERSION == 7
    for cfg, obs, act in ((K.train_waypoints_v3_config(), 28, 4), (K.waypoints_config(), 29, 4), (K.lowlevel_config(), 21, 6),
                          (K.train_objlock_config(), None, 4), (K.train_waypoint_objlock_config(), None, 4)):
        assert L.fw_act_dim(C.byref(cfg)) == act == K.act_dim(cfg)
        assert L.fw_obs_dim(C.byref(cfg)) == K.obs_dim(cfg)
        if obs is not None:
            assert K.obs_dim(cfg) == obs
    c = K.waypoints_config()
    c.task = 6                                            # beyond the last
    rc, msg = _abi_validate(c)
    assert rc == K.FW_EINVAL and "unknown task" in msg


PI = math.pi


@pytest.mark.parametrize("raw, want", [
    # heading: Box clip to [-pi, pi] (:97-101), then (a + pi) % 2 pi - pi (:132, 164)
    ((4.0, 10.0, 15.0), (-PI, 10.0, 15.0)),               # 4.0 -> pi -> (2 pi) % (2 pi) - pi = -pi
    ((-4.0, 10.0, 15.0), (-PI, 10.0, 15.0)),              # -4.0 -> -pi -> 0 % (2 pi) - pi = -pi
    ((PI, 10.0, 15.0), (-PI, 10.0, 15.0)),
    # altitude: [0, dome] (dome 200)
    ((0.0, -5.0, 15.0), (0.0, 0.0, 15.0)),
    ((0.0, 250.0, 15.0), (0.0, 200.0, 15.0)),
    # airspeed: the Box's [0, 30] is inside the env's own [0, 100] (:166)
    ((0.0, 10.0, 45.0), (0.0, 10.0, 30.0)),
    ((0.0, 10.0, -1.0), (0.0, 10.0, 0.0)),
    # in range: unchanged
    ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
    ((-PI, 200.0, 30.0), (-PI, 200.0, 30.0)),
])
def test_condition_command_on_hand_worked_cases(raw, want):
    got = condition_command(np.array(raw), 200.0)
    assert got.dtype == np.float64 and got.shape == (3,)
    np.testing.assert_array_equal(got[1:], want[1:])
    np.testing.assert_array_equal(got[0], want[0])


def test_condition_command_keeps_an_in_range_triple_and_broadcasts():
    a = np.array([[1.25, 42.0, 17.5], [-2.0, 199.0, 29.0]])
    got = condition_command(a, 200.0)
    # the wrap of an in-range heading is the identity up to the rounding of (a + pi) - pi: one ulp of pi at most
    np.testing.assert_allclose(got[:, 0], a[:, 0], rtol=0, atol=2 ** -51)
    np.testing.assert_array_equal(got[:, 1:], a[:, 1:])
    assert (got[:, 0] == (a[:, 0] + PI) % (2 * PI) - PI).all()
    assert condition_command(np.array([0.0, 150.0, 5.0]), 100.0)[1] == 100.0        # the dome is the caller's


def test_a_missing_checkpoint_raises_file_not_found(tmp_path):
    with pytest.raises(FileNotFoundError):
        HighLevelCmdVecEnv(4, low_checkpoint=str(tmp_path / "no_such_model.pt"))


def test_a_controller_of_another_shape_is_refused():
    rms = (np.zeros(21), np.ones(21))
    for bad in (R.MlpPolicy(21, 4), R.MlpPolicy(28, 6), R.MlpPolicy(21, 6, hidden=(32, 32)), R.MlpPolicy(21, 6, hidden=(64,)),
                torch.nn.Linear(21, 6)):
        with pytest.raises(ValueError, match="21 -> 64 -> 64 -> 6"):
            HighLevelCmdVecEnv(4, bad, rms)
    with pytest.raises(ValueError, match="21 entries"):
        HighLevelCmdVecEnv(4, R.MlpPolicy(21, 6), (np.zeros(20), np.ones(20)))
    with pytest.raises(ValueError):
        HighLevelCmdVecEnv(4)                             # no controller at all
    with pytest.raises(ValueError):
        HighLevelCmdVecEnv(4, R.MlpPolicy(21, 6), rms, render_mode="human")


def test_a_checkpoint_of_another_policy_is_refused(tmp_path):
    from pyflyt_drone_amd import checkpoint
    p = R.MlpPolicy(28, 4)
    path = str(tmp_path / "waypoints.pt")
    torch.save({"format_version": checkpoint.FORMAT_VERSION, "policy": p.state_dict(),
                "vecnormalize": {"obs_rms": {"mean": torch.zeros(28), "var": torch.ones(28), "count": torch.ones(1)}}}, path)
    with pytest.raises(ValueError, match="21 -> 64 -> 64 -> 6"):
        HighLevelCmdVecEnv(4, low_checkpoint=path)


def test_clip_actions_is_the_box_where_the_env_has_one_and_the_old_clamp_elsewhere():
    class Plain:
        pass

    class Boxed:
        action_low = torch.tensor([-PI, 0.0, 0.0], dtype=torch.float32)
        action_high = torch.tensor([PI, 200.0, 30.0], dtype=torch.float32)

    g = torch.Generator().manual_seed(3)
    a4 = torch.randn((64, 4), generator=g) * 2
    assert torch.equal(R.clip_actions(a4, Plain()), a4.clamp(-1.0, 1.0))
    a3 = torch.randn((64, 3), generator=g) * torch.tensor([5.0, 300.0, 50.0])
    want = np.clip(a3.numpy(), Boxed.action_low.numpy(), Boxed.action_high.numpy())      # SB3: np.clip(actions, space.low, space.high)
    np.testing.assert_array_equal(R.clip_actions(a3, Boxed()).numpy(), want)
