"""Conditions on the inputs of tests/test_fuzz_parity_gpu.py, checked on the CPU oracle alone.

A parity test off the shipped airframe is only worth its tolerance if the traces it flies are valid, finite, eventful and well
conditioned.  For every trace of fuzz_configs.legs() -- every one, nothing is skipped or filtered:

* fw_validate_config and the oracle both accept the config;
* the oracle's trace (same seeds, env count and actions as the GPU test) is finite and contains an episode end;
* conditioning: a second oracle stepped with the actions times 1 + 1e-13 N(0, 1) stays within 1e-9 of the first in
  observations, rewards and final state, with identical flags and info.  A rounding-level difference is therefore amplified
  by 1e4 at the most, which leaves an honest kernel four orders of magnitude inside the 1e-7 parity tolerance.  ObjLock
  observations are float32-rounded (one ulp can flip): there the bound is the parity tolerance, 2e-5.

Plus: the generator still produces the config bytes stored in the two fuzz golden files (a change of numpy's stream shows up
here, not as a parity failure); the aimed camera traces see the duck; and the oracle's own surface fold agrees with a numpy
restatement of the formulas for every fuzz vehicle.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
import fuzz_configs as F

GOLD = os.path.join(os.path.dirname(__file__), "golden")
LEGS = {name: (mode, steps, cfg) for name, mode, steps, cfg in F.legs()}
RIGID = slice(0, K.S_ACT + K.FW_NUM_ACTUATORS)


def oracle_trace(oracle, cfg, mode, steps, perturb=None):
    """The oracle's side of the GPU test's trace; `perturb`: a generator for the relative 1e-13 noise on the actions."""
    n = F.NUM_ENVS
    env = oracle.OracleEnv(cfg, n, seed=F.SEED)
    rng = np.random.default_rng(F.ACTION_SEED)
    obs, rew, flags, visible = [env.reset()], [], [], 0
    if mode == "aimed":
        env.set_state(F.aim_at_the_duck(oracle, env.get_state(), np.random.default_rng(8)))
        obs.append(env.observe())
    for _ in range(steps):
        a = F.actions_of(mode, rng, n)
        if perturb is not None:
            a = a * (1.0 + 1e-13 * perturb.normal(size=a.shape))
        o, r, te, tr, to, info = env.step(a)
        done = (te | tr).astype(bool)
        obs.append(o); obs.append(to[done]); rew.append(r)
        flags.append(np.concatenate([te[:, None], tr[:, None], info], axis=1))
        if mode == "aimed":
            visible += int((env.get_state()[:, K.S_TASK + K.ST_FRAME] > 0.5).sum())
    return dict(obs=np.concatenate([o.ravel() for o in obs]), rew=np.array(rew), flags=np.array(flags), state=env.get_state(),
                visible=visible)


def test_no_trace_is_left_out():
    """The share of generated configs that the tests leave out is zero: the legs are the generator's whole ranges."""
    assert len(LEGS) == F.N_WAYPOINTS + 4 * F.N_CAMERA + 2 * F.N_DIRECT == 80
    assert [n for n in LEGS if n.startswith("waypoints-")] == [f"waypoints-{i}" for i in range(32)]
    for task in ("objlock", "objlock-aimed", "combined", "combined-aimed"):
        assert all(f"{task}-{i}" in LEGS for i in range(9))
    # what the set was built to reach: every rate pair and step ratio, the general and the axis-aligned family with and without wind
    wp = [F.waypoints(i) for i in range(F.N_WAYPOINTS)]
    assert {(c.physics_hz, c.control_hz) for c in wp} == set(F.RATES) and {120 // c.agent_hz for c in wp} == {1, 2, 3, 4, 5, 8, 12}
    assert {(F.is_axis_aligned_family(i), c.wind_mode != K.FW_WIND_OFF) for i, c in enumerate(wp)} == {(a, w) for a in (False, True) for w in (False, True)}
    assert {c.n_collision_pts for c in wp} >= {0, 1, 8} and {c.warmup_aviary_steps for c in wp} >= {0, 13}
    assert {c.num_targets for c in wp} == set(range(9)) and {c.context_length for c in wp} == set(range(10))
    assert {c.wind_coupling for c in wp if c.wind_mode} == {K.FW_WIND_COUPLE_FORCE, K.FW_WIND_COUPLE_AIRSPEED}


@pytest.mark.parametrize("name", list(LEGS))
def test_config_is_accepted_by_both_sides(oracle, name):
    cfg = LEGS[name][2]
    _lib.validate(cfg)
    buf = C.create_string_buffer(256)
    assert oracle.lib().fwo_validate_config(C.byref(cfg), buf, 256) == 0, buf.value
    oracle.OracleEnv(cfg, 1, seed=0).close()
    assert int(cfg.agent_hz * cfg.max_duration_seconds) <= 40 or name.startswith("lowlevel-")


@pytest.mark.parametrize("name", list(LEGS))
def test_trace_is_finite_eventful_and_well_conditioned(oracle, name):
    mode, steps, cfg = LEGS[name]
    a = oracle_trace(oracle, cfg, mode, steps)
    b = oracle_trace(oracle, cfg, mode, steps, perturb=np.random.default_rng(99))
    for key in ("obs", "rew", "state"):
        assert np.isfinite(a[key]).all(), key
    ends = int(a["flags"][:, :, :2].any(axis=2).sum())
    if mode == "lowlevel":
        # the one leg built to have no episode end on the oracle's side (tests/test_lowlevel_gpu.py: the oracle has no low-level
        # task; the comparison is the rigid state until the kernel's first episode end, and that is what is conditioned here --
        # its waypoint columns are of the size of its 1e7 m dome)
        assert ends == 0
        assert np.abs(a["state"][:, RIGID] - b["state"][:, RIGID]).max() <= 1e-9
        return
    assert ends > 0, "the trace was meant to contain an episode end"
    assert np.array_equal(a["flags"], b["flags"]), "a 1e-13 perturbation changed a flag or an info word"
    assert a["obs"].shape == b["obs"].shape
    d = {key: float(np.abs(a[key] - b[key]).max()) for key in ("obs", "rew", "state")}
    print(f"{name}: {ends} episode ends, amplified to {d}")
    assert d["obs"] <= (2e-5 if cfg.task == K.FW_TASK_OBJLOCK else 1e-9) and d["rew"] <= 1e-9 and d["state"] <= 1e-9, d
    if mode == "aimed":
        print(f"{name}: duck in the frame for {a['visible']} env-steps")
        assert a["visible"] >= F.AIMED_MIN_VISIBLE


@pytest.mark.parametrize("name,make", [("fuzz_waypoints_480hz_gust", lambda: F.waypoints(1)), ("fuzz_combined_obstacles", lambda: F.combined(2))])
def test_generator_reproduces_the_golden_config_bytes(name, make):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    cfg = make()
    assert g["fw_config"].size == C.sizeof(K.FwConfig)
    np.testing.assert_array_equal(F.config_bytes(cfg), g["fw_config"], err_msg="the generator's random stream has changed")
    assert cfg.physics_hz // cfg.control_hz == 4 and cfg.wind_mode != K.FW_WIND_OFF
    assert cfg.num_obstacles > 0 or cfg.task == K.FW_TASK_WAYPOINTS


def test_generated_vehicles_keep_their_invariants():
    """Orthonormal surface axes (rotated together), unit thrust axis, the two families, positive-definite inertia."""
    for i in range(F.N_WAYPOINTS):
        c = F.waypoints(i)
        for s in range(K.FW_NUM_SURFACES):
            L, Fw = np.array(c.surfaces[s].lift_unit[:]), np.array(c.surfaces[s].forward_unit[:])
            assert abs(L @ L - 1) < 1e-14 and abs(Fw @ Fw - 1) < 1e-14 and abs(L @ Fw) < 1e-14
            if F.is_axis_aligned_family(i):
                assert list(Fw) == [1, 0, 0] and list(L) in ([0, 1, 0], [0, 0, 1])
        I = c.inertia
        assert (np.linalg.eigvalsh([[I[0], I[3], I[4]], [I[3], I[1], I[5]], [I[4], I[5], I[2]]]) > 0).all()
        assert any(I[3:6]) != F.is_axis_aligned_family(i)
        assert abs(np.linalg.norm(c.motor.thrust_unit[:]) - 1) < 1e-14
    fam = [F.waypoints(i) for i in range(F.N_WAYPOINTS) if F.is_axis_aligned_family(i)]
    lifts = {(s, tuple(c.surfaces[s].lift_unit[:])) for c in fam for s in range(K.FW_NUM_SURFACES)}
    assert len(lifts) == 2 * K.FW_NUM_SURFACES, "every surface of the axis-aligned family was meant to lift along e_y and along e_z"


@pytest.mark.parametrize("i", range(F.N_WAYPOINTS))
def test_oracle_surface_fold_against_a_numpy_restatement(oracle, i):
    """PyFlyt LiftingSurface.__init__, restated: area, aspect ratio, the 3-D lift slope, flap effectiveness."""
    c = F.vehicle(i, K.waypoints_config())
    for s in range(K.FW_NUM_SURFACES):
        sp = c.surfaces[s]
        area, ar = np.float64(sp.chord) * sp.span, np.float64(sp.span) / sp.chord
        cl3 = sp.Cl_alpha_2D * (ar / (ar + ((2.0 * (ar + 4.0)) / (ar + 2.0))))
        theta_f = np.arccos(2.0 * sp.flap_to_chord - 1.0)
        tau_f = 1.0 - ((theta_f - np.sin(theta_f)) / math.pi)
        got = oracle.surface_constants(sp)
        # products, quotients and acos: two ulps between libm and numpy.  tau_f is a difference: an ulp of theta_f in [2, 4) is
        # 4.4e-16 absolute, sin and the two roundings add less than another, and the result near 0.5 inherits them absolutely
        np.testing.assert_allclose(got[:4], [area, ar, cl3, theta_f], rtol=4e-16, atol=0)
        np.testing.assert_allclose(got[4], tau_f, rtol=0, atol=1e-15)
        assert 0.0 < tau_f < 1.0 and 0.5 < ar < 12.0
