"""The low-level task's second variant -- the FixedwingLowLevelEnv that the reference's examples/lowlevel.py defines for its SAC run --
without a GPU: the config builder, the three former reserved words through the C ABI, and what stays as it was."""
import ctypes as C
import math

import pytest

from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K


def _abi_validate(cfg):
    buf = C.create_string_buffer(256)
    rc = _lib.lib().fw_validate_config(C.byref(cfg), buf, 256)
    return rc, buf.value.decode()


def _clock_steps(max_duration_seconds, agent_hz):
    """examples/lowlevel.py:66, 125, 206 run on the host: the step at which `_elapsed_time_s >= max_duration_seconds` first holds"""
    dt, t, k = 1.0 / float(agent_hz), 0.0, 0
    while True:
        k += 1
        t += dt
        if t >= max_duration_seconds:
            return k


def test_builder_defaults_are_the_scripts_constructor():
    c = K.lowlevel_demo_config()
    assert c.task == K.FW_TASK_LOWLEVEL == 3 and c.lowlevel_variant == K.FW_LL_VARIANT_SAC_DEMO == 1
    assert (c.physics_hz, c.control_hz, c.agent_hz, c.warmup_aviary_steps) == (240, 120, 120, 0)     # the script's agent_hz is only its clock
    assert list(c.start_pos) == [0.0, 0.0, 120.0] and list(c.start_orn) == [0.0, 0.0, 0.0]        # :75-76
    assert list(c.start_vel) == [25.0, 0.0, 0.0]                                                   # :77
    assert list(c.lowlevel_speed_range) == [20.0, 35.0] and list(c.lowlevel_height_range) == [100.0, 200.0]
    assert c.flight_dome_size == 800.0 and c.lowlevel_min_speed == 8.0 and c.lowlevel_fixed_heading == 0
    assert c.num_targets == 0 and c.wind_mode == K.FW_WIND_OFF and c.auto_reset == 1
    assert K.obs_dim(c) == 21 and K.act_dim(c) == 6
    # 60 s at 30 Hz is 1801 steps, not 1800: after 1800 additions of 1/30 the float64 sum is still below 60.0
    t = 0.0
    for _ in range(1800):
        t += 1.0 / 30.0
    assert t < 60.0 <= t + 1.0 / 30.0
    assert c.lowlevel_max_episode_steps == 1801 == _clock_steps(60.0, 30)


@pytest.mark.parametrize("seconds, hz", [(60.0, 30), (120.0, 30), (60.0, 60), (60.0, 120), (30.0, 40), (1.0, 30), (40.0 / 30.0, 30), (7.3, 24),
                                         (0.01, 30), (60.0, 7)])
def test_step_limit_follows_the_running_sum_not_a_product(seconds, hz):
    c = K.lowlevel_demo_config(max_duration_seconds=seconds, agent_hz=hz)
    want = _clock_steps(seconds, hz)
    assert c.lowlevel_max_episode_steps == want == K.lowlevel_demo_episode_steps(seconds, hz)
    assert math.ceil(seconds * hz - 1e-9) <= want <= math.ceil(seconds * hz - 1e-9) + 1         # the product is off by at most the one step
    assert c.agent_hz == 120 and c.max_duration_seconds == seconds


def test_builder_keywords():
    w = {"enabled": True, "mode": "constant", "randomize_on_reset": True, "wind_enu_mps_range": [[-1, 1], [-2, 2], [0, 0]]}
    c = K.lowlevel_demo_config(flight_dome_size=60, max_duration_seconds=2.0, agent_hz=20, start_height_m=50, start_speed_mps=18,
                               min_speed_mps=9.5, target_speed_range=(12, 14), target_height_range=(40, 70),
                               target_heading_random=False, dtype="float32", motor_noise=False, auto_reset=False, wind_config=w)
    assert c.flight_dome_size == 60.0 and list(c.start_pos) == [0.0, 0.0, 50.0] and list(c.start_vel) == [18.0, 0.0, 0.0]
    assert c.lowlevel_min_speed == 9.5 and c.lowlevel_fixed_heading == 1 and c.lowlevel_variant == 1
    assert list(c.lowlevel_speed_range) == [12.0, 14.0] and list(c.lowlevel_height_range) == [40.0, 70.0]
    assert c.lowlevel_max_episode_steps == _clock_steps(2.0, 20)
    assert c.dtype == K.FW_F32 and c.motor.noise_ratio == 0.0 and c.auto_reset == 0 and c.wind_mode == K.FW_WIND_CONSTANT
    assert _abi_validate(c) == (K.FW_OK, "")
    with pytest.raises(ValueError, match="render mode"):
        K.lowlevel_demo_config(render_mode="human")
    with pytest.raises(ValueError, match="min_speed_mps"):
        K.lowlevel_demo_config(min_speed_mps=-1.0)
    with pytest.raises(ValueError):
        K.lowlevel_demo_config(agent_hz=0)
    with pytest.raises(ValueError, match="10 000 000 steps"):                      # the clock's sum is walked step by step: bounded
        K.lowlevel_demo_config(max_duration_seconds=1.0e9)
    with pytest.raises(ValueError):
        K.lowlevel_demo_config(wind_config={"enabled": True, "mode": "tornado"})


def test_abi_accepts_the_variant_with_the_tasks_widths():
    c = K.lowlevel_demo_config()
    assert _abi_validate(c) == (K.FW_OK, "")
    assert _lib.lib().fw_obs_dim(C.byref(c)) == 21 and _lib.lib().fw_act_dim(C.byref(c)) == 6
    assert C.sizeof(K.FwConfig) == _lib.lib().fw_sizeof_config() and _lib.lib().fw_abi_version() == K.FW_ABI_VERSION == 7
    _lib.validate(K.lowlevel_demo_config(target_heading_random=False, wind_config={"enabled": True, "mode": "gust_sine",
                                                                                   "randomize_on_reset": True}))


@pytest.mark.parametrize("mutate, words", [
    (dict(lowlevel_variant=2), "lowlevel_variant"),
    (dict(lowlevel_variant=-1), "lowlevel_variant"),
    (dict(lowlevel_min_speed=-0.5), "lowlevel_min_speed"),
    (dict(lowlevel_min_speed=float("nan")), "lowlevel_min_speed"),
    (dict(lowlevel_min_speed=float("inf")), "lowlevel_min_speed"),
    (dict(lowlevel_fixed_heading=2), "lowlevel_fixed_heading"),
    (dict(lowlevel_fixed_heading=-1), "lowlevel_fixed_heading"),
    (dict(agent_hz=30), "agent_hz 120"),                          # the task's rule holds for the variant too
    (dict(control_hz=240), "control_hz 120"),
    (dict(num_targets=2), "num_targets must be 0"),
    (dict(lowlevel_max_episode_steps=0), "lowlevel_max_episode_steps"),
])
def test_abi_rejects(mutate, words):
    c = K.lowlevel_demo_config()
    for k, v in mutate.items():
        setattr(c, k, v)
    rc, msg = _abi_validate(c)
    assert rc == K.FW_EINVAL and words in msg, msg
    with pytest.raises(ValueError, match=words):
        _lib.validate(c)


def test_every_other_builder_leaves_the_three_words_zero():
    others = (K.lowlevel_config(), K.lowlevel_config_from_reference_kwargs(), K.train_waypoints_v3_config(), K.waypoints_config(),
              K.waypoints_direct_config(), K.highlevel_config(), K.train_objlock_config(), K.objlock_config(),
              K.train_waypoint_objlock_config(), K.waypoint_objlock_config())
    for c in others:
        assert (c.lowlevel_variant, c.lowlevel_fixed_heading, c.lowlevel_min_speed) == (0, 0, 0.0), c.task
        assert not any(c.reserved_i) and not any(c.reserved_d)
        assert _abi_validate(c) == (K.FW_OK, "")
    # the words sit where the reserved ones sat: nothing behind them moved
    F = K.FwConfig
    assert F.lowlevel_variant.offset == F.lowlevel_max_episode_steps.offset + 4 and F.lowlevel_fixed_heading.offset == F.lowlevel_variant.offset + 4
    assert F.reserved_i.offset == F.lowlevel_fixed_heading.offset + 4 and F.reserved_i.size == 16
    assert F.flight_dome_size.offset == F.reserved_i.offset + 16
    assert F.lowlevel_min_speed.offset == F.lowlevel_height_range.offset + 16 and F.reserved_d.offset == F.lowlevel_min_speed.offset + 8
    assert F.reserved_d.offset + 24 == C.sizeof(F)


def test_the_variant_words_do_not_reach_other_tasks_or_the_first_variant():
    # the words are real fields of the structure (not attributes of one Python object): what is written here reaches the C side
    F = K.FwConfig
    assert isinstance(F.lowlevel_variant.offset, int) and F.lowlevel_variant.size == 4 and F.lowlevel_min_speed.size == 8
    # a waypoints config with junk in the low-level words is still a valid waypoints config: the words belong to FW_TASK_LOWLEVEL
    c = K.train_waypoints_v3_config()
    c.lowlevel_variant, c.lowlevel_fixed_heading, c.lowlevel_min_speed = 7, 5, -3.0
    assert bytes(c) != bytes(K.train_waypoints_v3_config())
    assert _abi_validate(c) == (K.FW_OK, "")
    # ... and the first variant ignores the two words of the second, as it did while they were reserved; its own selector it checks
    c = K.lowlevel_config()
    c.lowlevel_fixed_heading, c.lowlevel_min_speed = 5, float("nan")
    assert c.lowlevel_variant == 0 and bytes(c) != bytes(K.lowlevel_config())
    assert _abi_validate(c) == (K.FW_OK, "")
    c.lowlevel_variant = 1
    rc, msg = _abi_validate(c)
    assert rc == K.FW_EINVAL and "lowlevel_fixed_heading" in msg


@pytest.mark.parametrize("task", [4, 6])
def test_ids_four_and_six_are_still_no_tasks(task):
    for c in (K.lowlevel_demo_config(), K.lowlevel_config()):
        c.task = task
        rc, msg = _abi_validate(c)
        assert rc == K.FW_EINVAL and "unknown task" in msg


def test_package_exports():
    import pyflyt_drone_amd as P
    assert P.lowlevel_demo_config is K.lowlevel_demo_config
    assert issubclass(P.FixedwingLowLevelDemoVecEnv, P.FixedwingVecEnv)
    assert {"FixedwingLowLevelDemoVecEnv", "lowlevel_demo_config"} <= set(P.__all__)
