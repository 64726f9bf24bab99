"""The step kernels against the CPU oracle OFF the shipped airframe, rates and start pose (tests/fuzz_configs.py).

The kernels never read fw_config: build_params (csrc/fwsim.hip) folds it once into Params<T> -- per-surface constants, the motor
wrench, inertia and its inverse, the gust rotation, step_ratio and ticks_per_aviary, the cached warm-up state -- and every
kernel family reads that block its own way (scalar loads with one lane per env; through an opaque pointer with 8 lanes; volatile
LDS with two waves per SIMD; the axis-aligned tick that drops terms).  Everywhere else in the suite those folds and read paths are
checked at one point of parameter space; here every folded field moves at once.

Tolerances are those of test_parity_gpu.py::test_lockstep_f64: 1e-7 absolute on observations, rewards, terminal observations
and the final state; 2e-5 on ObjLock's float32-rounded observations only; terminated, truncated and info exactly equal.
tests/test_fuzz_configs_cpu.py holds, on the oracle alone, that every trace flown here is finite, contains episode ends and
amplifies a rounding-level difference by less than 1e4, so that the tolerance means the same here as at the shipped point.

Which row of the kernel table (env_kernels_of, csrc/fwsim.hip) each config reaches is listed in profiles/fuzz_parity_margin.txt.
"""
import numpy as np
import pytest

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
import fuzz_configs as F
from helpers import run_direct_lockstep, run_lockstep, run_lowlevel_lockstep

pytestmark = pytest.mark.gpu

TOL = 1e-7
OBJLOCK_OBS_TOL = 2e-5
MAPPINGS = {"lane_per_env": ("1", "1"), "8_lanes_per_env": ("8", "1"), "8_lanes_2_waves_per_simd": ("8", "2")}


@pytest.fixture(params=["lane_per_env", "8_lanes_per_env"])
def lanes(request, monkeypatch):
    """Both lane mappings of the kernels (fwsim_device.hpp)."""
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", MAPPINGS[request.param][0])
    monkeypatch.setenv("FWSIM_G8_WAVES", "1")
    return int(MAPPINGS[request.param][0])


@pytest.fixture(params=list(MAPPINGS))
def lanes3(request, monkeypatch):
    """... and, for the waypoints kernels, the 8-lane mapping built for two waves per SIMD."""
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", MAPPINGS[request.param][0])
    monkeypatch.setenv("FWSIM_G8_WAVES", MAPPINGS[request.param][1])
    return request.param


def _pair(oracle, cfg, ora_cfg=None):
    return (P.FixedwingVecEnv(cfg, F.NUM_ENVS, seed=F.SEED), oracle.OracleEnv(cfg if ora_cfg is None else ora_cfg, F.NUM_ENVS, seed=F.SEED))


def _fly(hip, ora, mode, steps, after_reset=None):
    obj = hip.cfg.task == K.FW_TASK_OBJLOCK
    worst = run_lockstep(hip, ora, steps, np.random.default_rng(F.ACTION_SEED), atol=OBJLOCK_OBS_TOL if obj else TOL, rtol=0, rew_atol=TOL,
                         state_atol=TOL, after_reset=after_reset, actions=lambda rng, n: F.actions_of(mode, rng, n))
    print(f"worst |diff| {worst}")
    assert worst["obs"] <= (OBJLOCK_OBS_TOL if obj else TOL) and worst["rew"] <= TOL and worst["state"] <= TOL
    assert worst["dones"] > 0, "the trace was meant to contain an episode end"
    return worst


@pytest.mark.parametrize("i", range(F.N_WAYPOINTS))
def test_waypoints_off_the_default_vehicle(oracle, i, lanes3):
    cfg = F.waypoints(i)
    hip, ora = _pair(oracle, cfg)
    assert hip.lanes_per_env == int(MAPPINGS[lanes3][0]) and hip.g8_waves == int(MAPPINGS[lanes3][1])
    # the axis-aligned tick: the f64 wind-free kernel of the one-wave 8-lane build, and only with the geometry of that family
    want_ax = F.is_axis_aligned_family(i) and cfg.wind_mode == K.FW_WIND_OFF and lanes3 == "8_lanes_per_env"
    assert int(_lib.lib().fw_axis_aligned(hip._h)) == (1 if want_ax else 0)
    _fly(hip, ora, "uniform", F.WAYPOINT_STEPS)


@pytest.mark.parametrize("i", F.RESET_PATH_CONFIGS)
def test_every_reset_path_off_the_default_start(oracle, i, lanes, monkeypatch):
    """The ways an auto-reset is served -- the cached warm-up state (wind-free; with pre-sampled waypoints on the 8-lane
    mapping), the pre-simulated episode start (wind) and the warm-up inside the step kernel (FWSIM_NO_SHADOW=1) -- all meet the
    oracle off the shipped start pose and warm-up length; the counters say which one a run took."""
    cfg = F.waypoints(i)
    windy = cfg.wind_mode != K.FW_WIND_OFF
    hip, ora = _pair(oracle, cfg)
    _fly(hip, ora, "uniform", F.WAYPOINT_STEPS)
    c = hip.get_counters()
    assert c["resets"] > 0
    if windy:
        assert c["shadow_hits"] > 0, c
    elif lanes == 8:
        assert c["scenario_hits"] > 0 and c["shadow_hits"] == 0, c
    else:                                                   # wind-free, one lane per env: nothing to hand off, the cached warm-up serves every reset
        assert c["fallbacks"] == c["resets"], c
    hip.close()
    monkeypatch.setenv("FWSIM_NO_SHADOW", "1")
    hip, ora = _pair(oracle, cfg)
    _fly(hip, ora, "uniform", F.WAYPOINT_STEPS)
    c = hip.get_counters()
    assert c["fallbacks"] == c["resets"] > 0 and c["shadow_hits"] == 0 and c["scenario_hits"] == 0, c


def _aim(oracle):
    def start(hip, ora):
        s = F.aim_at_the_duck(oracle, ora.get_state(), np.random.default_rng(8))
        hip.set_state(s); ora.set_state(s)
        tol = OBJLOCK_OBS_TOL if hip.cfg.task == K.FW_TASK_OBJLOCK else TOL
        np.testing.assert_allclose(hip.observe_tensor().cpu().numpy(), ora.observe(), rtol=0, atol=tol)
    return start


def _camera_traces(oracle, task, i, lanes, capture_wave=False):
    make = F.objlock if task == "objlock" else F.combined
    for aimed in (False, True):
        hip, ora = _pair(oracle, make(i, aimed=aimed))
        assert hip.lanes_per_env == lanes and hip.capture_wave == capture_wave
        if aimed:                   # aimed at the duck: frames with the duck in them, lock counters, strikes
            _fly(hip, ora, "aimed", F.AIMED_STEPS, after_reset=_aim(oracle))
        else:                       # the env's own resets
            _fly(hip, ora, "gentle", F.CAMERA_STEPS)
        assert hip.get_counters()["capture_wave_timeouts"] == 0
        hip.close()


@pytest.mark.parametrize("i", range(F.N_CAMERA))
@pytest.mark.parametrize("task", ["objlock", "combined"])
def test_camera_tasks_off_the_default_vehicle(oracle, task, i, lanes):
    _camera_traces(oracle, task, i, lanes)


@pytest.mark.parametrize("task,i", F.CAPTURE_WAVE_CONFIGS)
def test_camera_tasks_off_the_default_vehicle_with_a_capture_wave(oracle, task, i, monkeypatch):
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", "8"); monkeypatch.setenv("FWSIM_CAPTURE_WAVE", "1")
    _camera_traces(oracle, task, i, 8, capture_wave=True)


@pytest.mark.parametrize("i,triple", list(zip(F.DIRECT_VEHICLES, F.TRIPLES)))
def test_direct_command_kernels_off_the_default_vehicle(oracle, i, triple, lanes):
    wd, wp = F.direct_pair(i, triple)
    hip, ora = _pair(oracle, wd, wp)
    assert hip.lanes_per_env == lanes and hip.act_dim == 6
    worst = run_direct_lockstep(hip, ora, triple, F.DIRECT_STEPS, np.random.default_rng(F.ACTION_SEED), atol=TOL,
                                actions=lambda rng, n: F.actions_of("direct", rng, n))
    print(f"worst |diff| {worst}")
    assert worst["dones"] > 0
    c = hip.get_counters()
    assert c["resets"] == worst["dones"] == c["fallbacks"]


@pytest.mark.parametrize("i,triple", list(zip(F.DIRECT_VEHICLES, F.TRIPLES)))
def test_lowlevel_kernels_off_the_default_vehicle(oracle, i, triple, lanes):
    ll, wp = F.lowlevel_pair(i, triple)
    assert (ll.physics_hz, ll.control_hz, ll.agent_hz, ll.warmup_aviary_steps) == (240, 120, 120, 0)
    hip, ora = _pair(oracle, ll, wp)
    assert hip.lanes_per_env == lanes
    worst = run_lowlevel_lockstep(hip, ora, triple, F.DIRECT_STEPS, np.random.default_rng(F.ACTION_SEED), atol=TOL,
                                  actions=lambda rng, n: F.actions_of("lowlevel", rng, n))
    print(f"worst |diff| {worst}")
    assert worst["compared"] > F.NUM_ENVS * F.DIRECT_STEPS // 2, worst
