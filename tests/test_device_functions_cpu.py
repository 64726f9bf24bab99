"""Ties down tests/device_reference.py, the reference of tests/test_device_functions_gpu.py, without a GPU: its longdouble
elementary functions against mpmath at 40 digits, the float64 run of every restatement against the oracle's export of the same
function, the caps of every input set, and the E_ref constants written into the GPU test."""
import numpy as np
import pytest

from pyflyt_drone_amd import config as K
import device_reference as R
import directed_states as D
from device_e_ref import E_REF

LD = R.LD
EPS = 2.0 ** -52


def test_longdouble_is_the_extended_type():
    R.require_longdouble()
    assert R.pi_of(LD) != LD(np.pi) and abs(float(R.pi_of(LD) - LD(np.pi)) - 1.2246467991473532e-16) < 1e-19


def _mpf(x):
    """a longdouble as an exact mpmath number (two float64 halves)"""
    import mpmath
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


@pytest.mark.parametrize("name", ["rcp", "sqrt", "sin", "sincos.cos", "sin.far", "sincos.cos.far", "asin", "log", "div", "atan2"])
def test_longdouble_functions_against_mpmath(name):
    """The reference's own error: numpy's longdouble functions (glibc's 80-bit libm) within 2 units of the 64-bit mantissa of
    mpmath's 40-digit value, on every 16th point of the input set -- four thousand times finer than a float64 ulp."""
    import mpmath
    mpmath.mp.dps = 40
    R.require_longdouble()
    fn = dict(rcp=lambda a: 1 / a[0], sqrt=lambda a: mpmath.sqrt(a[0]), sin=lambda a: mpmath.sin(a[0]), asin=lambda a: mpmath.asin(a[0]),
              log=lambda a: mpmath.log(a[0]), div=lambda a: a[0] / a[1], atan2=lambda a: mpmath.atan2(a[0], a[1]))
    fn["sincos.cos"] = lambda a: mpmath.cos(a[0])
    fn["sin.far"], fn["sincos.cos.far"] = fn["sin"], fn["sincos.cos"]
    op, col, x, ref, _, _ = R.math_case(name, np.float64)
    checked = 0
    for row, r in list(zip(x, ref))[::16]:
        if not np.isfinite(float(r)) or (name in ("rcp", "div") and row[-1] == 0):
            continue
        true = fn[name]([mpmath.mpf(float(v)) for v in row])
        err = abs(_mpf(r) - true)
        assert err <= 2 * mpmath.mpf(2) ** -63 * max(abs(true), mpmath.mpf(2) ** -1000), (name, row, r)
        checked += 1
    assert checked > 100


def test_float64_restatements_against_the_oracle_exports(oracle):
    """Each numpy restatement, run in float64, against the C function of the same name.  Both are plain float64 evaluations of the
    same formulas, each within its own E_ref of the longdouble run, so they are within the sum of the two of each other; the integer
    functions agree exactly."""
    rng = np.random.default_rng(40)
    for veh in R.VEHICLES:
        cfg = R.vehicle_config(veh)
        for g in R.SURF_GROUPS:
            rows = R.surface_inputs(cfg, np.float64, g)
            ref, d = R.surface_wrench(cfg, rows, LD, detail=True)
            a, b = R.surface_wrench(cfg, rows, np.float64), R.oracle_surface_wrench(oracle, cfg, rows)
            ea, eb = R.normalised_error(a, ref, d["scale"]), R.normalised_error(b, ref, d["scale"])
            assert R.normalised_error(a, b.astype(LD), d["scale"]) <= ea + eb + 4 * EPS, (veh, g)
            assert max(ea, eb) <= 2 * E_REF[R.e_ref_key("surface", g, np.float64)]
    q = R.euler_inputs(np.float64, "random")
    # products and sums of unit-size terms, an atan2 / asin behind them: a few ulps of pi between libm and numpy
    np.testing.assert_allclose(R.euler_from_quat(q)[0], [oracle.euler_from_quat(r) for r in q], rtol=0, atol=16 * EPS)
    np.testing.assert_allclose(R.rot_from_quat(q), [oracle.mat_from_quat(r).reshape(9) for r in q], rtol=0, atol=4 * EPS)
    ql = R.euler_inputs(np.float64, "locked")
    np.testing.assert_allclose(R.euler_from_quat(ql)[0], [oracle.euler_from_quat(r) for r in ql], rtol=0, atol=16 * EPS)
    # near the guard roll and yaw are atan2 of two numbers of the size of cos^2(pitch) >= 2e-5, each a difference of unit-size
    # products: a few ulps of 1 in them are 1e-10 in the angle
    qn = R.euler_inputs(np.float64, "near_guard")
    np.testing.assert_allclose(R.euler_from_quat(qn)[0], [oracle.euler_from_quat(r) for r in qn], rtol=0, atol=16 * EPS / 2e-5)
    # roll and yaw at +-pi: the two sides of atan2's cut are one angle
    qw = R.euler_inputs(np.float64, "wrap")
    dw = (R.euler_from_quat(qw)[0] - np.array([oracle.euler_from_quat(r) for r in qw])).astype(LD)
    dw[:, [0, 2]] = R.circular(dw[:, [0, 2]])
    assert np.abs(np.asarray(dw, dtype=np.float64)).max() <= 16 * EPS
    e = rng.uniform(-np.pi, np.pi, (64, 3))
    np.testing.assert_allclose(R.quat_from_euler(e), [oracle.quat_from_euler(r) for r in e], rtol=0, atol=4 * EPS)
    w = rng.integers(0, 2 ** 32, (64, 6), dtype=np.uint64).astype(np.uint32)
    w[0] = 0xFFFFFFFF
    np.testing.assert_array_equal(R.philox4x32_10(w[:, :4], w[:, 4:]), [oracle.philox(r[:4], r[4:]) for r in w])
    # rng_normal2: the oracle's two 64-bit words are the halves of one Philox block (stream 1, counter = the Aviary step)
    seed = 0x123456789ABCDEF
    for env, ep, astep in ((0, 0, 0), (7, 3, 11), (2 ** 31 + 5, 2, 2 ** 20)):
        o = R.philox4x32_10(np.array([[astep, ep, env, 1]], dtype=np.uint64), np.array([[seed & 0xFFFFFFFF, seed >> 32]], dtype=np.uint64)).astype(np.uint64)
        a, b = (o[:, 1] << np.uint64(32)) | o[:, 0], (o[:, 3] << np.uint64(32)) | o[:, 2]
        np.testing.assert_allclose(R.normal2_from_words(a, b, np.float64)[0], oracle.rng_normal2(seed, env, ep, astep), rtol=0, atol=16 * EPS)
    cfg = R.vehicle_config("shipped", wind=R.GUST)
    c = R.case("wind", np.float64)
    rows = c["rows"]
    got = R.gust_wind(rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7] + rows[:, 8], R.GUST["gust_freq_hz"], 240, np.float64)
    want = [oracle.wind_at(cfg, r[0:3], r[3:6], r[6], (r[7] + r[8]) / 240.0) for r in rows]
    # the argument 2 pi f t + phase reaches 190 rad: half an ulp of it, 1.4e-14, times the amplitude (<= 3)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_input_sets_obey_their_caps(dtype):
    """Conditions on the inputs, held here so that no row is ever left out at run time: every value is representable in the
    dtype; every surface row is SURF_CAP from the model's discontinuities (and the sets keep post-stall, reverse-flow and V = 0
    rows); every Euler row is EULER_CAP from the gimbal guard and on the reference's side of it in the working precision;
    the clamp of the quaternion step is approached from both sides but not met."""
    R.require_longdouble()
    for veh in R.VEHICLES:
        cfg = R.vehicle_config(veh)
        for g in R.surf_groups(dtype):
            rows = R.surface_inputs(cfg, dtype, g)
            np.testing.assert_array_equal(rows, R.representable(rows, dtype))
            ok, d = R.surface_caps_ok(cfg, rows, R.surface_cap(dtype, g))
            assert ok.all() and len(rows) >= (595 if dtype is np.float64 or g[1] == 0 else 340) and R.surface_cap(dtype, g) >= R.SURF_CAP
            assert (~np.asarray(d["nostall"])).sum() > 100 and np.asarray(d["nostall"]).sum() > 30
    for group in ("random", "near_guard", "locked", "wrap"):
        q = R.euler_inputs(dtype, group)
        np.testing.assert_array_equal(q, R.representable(q, dtype))
        ql = q.astype(LD)
        sarg = np.asarray(-2 * (ql[:, 0] * ql[:, 2] - ql[:, 3] * ql[:, 1]), dtype=np.float64)
        assert (np.abs(np.abs(sarg) - R.GUARD) >= R.EULER_CAP[dtype]).all(), group
        assert np.array_equal(R.euler_from_quat(ql)[1], R.euler_from_quat(q.astype(dtype))[1]), group
        if group == "near_guard":
            assert (np.abs(sarg) > np.cos(1.1e-3 + np.arccos(R.GUARD))).all() and (sarg > 0).any() and (sarg < 0).any()
    rows = R.quat_step_inputs(dtype, 240)
    np.testing.assert_array_equal(rows, R.representable(rows, dtype))
    wl = rows[:, :3].astype(LD)
    x = np.asarray(np.sqrt((wl * wl).sum(axis=1)) / 240 / (R.pi_of(LD) / 4) - 1, dtype=np.float64)
    off = 1e-9 if dtype is np.float64 else 1e-5
    assert (np.abs(x) >= off / 2).all() and (np.abs(x) <= 2 * off).sum() >= 2 * len(R.QUAT_SCALES)
    assert np.array_equal(R.quat_step(wl, rows[:, 3:].astype(LD), 240)[1], R.quat_step(rows[:, :3].astype(dtype), rows[:, 3:].astype(dtype), 240)[1])
    d = (rows[:, 3:].astype(LD) ** 2).sum(axis=1)
    assert (np.abs(d - 1) < 1e-4).any() and ((np.abs(d - 1) >= 1e-4) & (d < 1.001)).any() and (d > 8).any(), "both sides of the series switch, and far off"
    for veh in R.AX_VEHICLES if dtype is np.float64 else ():
        cfg = R.vehicle_config(veh)
        rows, expect = R.ax_wave_inputs(cfg)
        assert sorted(set(expect.tolist())) == [0, 1, 40] and (expect == 1).sum() == 40
        for s in range(5):
            r = rows.copy(); r[:, 0] = s
            assert R.surface_caps_ok(cfg, r)[0].all()


def test_e_ref_constants_of_the_gpu_test(oracle):
    """The E_ref figures written into tests/test_device_functions_gpu.py, recomputed: none may have moved by more than a factor 2."""
    R.require_longdouble()
    table = R.e_ref_table(oracle)
    assert set(table) == set(E_REF)
    for key, v in table.items():
        print(f"{key:40s} E_ref {v:.3e}   (written: {E_REF[key]:.3e})")
    for key, v in table.items():
        assert 0.5 * E_REF[key] <= v <= 2.0 * E_REF[key], (key, v, E_REF[key])


@pytest.mark.parametrize("leg", ["waypoints", "waypoints_gust", "direct", "lowlevel"])
def test_directed_states_are_finite_and_well_conditioned(oracle, leg):
    """On the oracle alone, for the one agent step tests/test_directed_states_gpu.py flies from the states of
    tests/directed_states.py: everything finite; a 1e-13 perturbation of the rigid state changes no flag and no info word and moves
    observation, reward and state by at most 1e-9 -- except the state that sits on the reverse-flow discontinuity, which must be
    seen to jump; and every branch the states are there for is present."""
    _, cfg, _, _ = D.legs()[leg]

    def fly(perturb):
        ora = oracle.OracleEnv(cfg, D.NUM_ENVS, seed=5)
        ora.reset()
        s = ora.get_state()
        names = D.apply(s)
        if perturb:
            s[:, :K.S_ACT] += np.random.default_rng(99).uniform(-1e-13, 1e-13, (len(s), K.S_ACT))
        ora.set_state(s)
        out = ora.step(D.actions(D.NUM_ENVS))
        return names, s, out, ora.get_state()

    names, s0, a, sa = fly(False)
    _, _, b, sb = fly(True)
    assert set(names) == set(D.BRANCHES) and len(names) == 65
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all() and np.isfinite(sa).all()
    for k in (2, 3, 5):
        assert np.array_equal(a[k], b[k]), "a 1e-13 perturbation changed a flag or an info word"
    on_edge = np.array([n in D.ON_A_DISCONTINUITY for n in names])
    d = dict(obs=np.abs(a[0] - b[0]).max(axis=1), rew=np.abs(a[1] - b[1]), state=np.abs(sa - sb).max(axis=1))
    if leg == "lowlevel":
        # what the GPU test compares there is the rigid state and the actuators (the oracle has no low-level task; the waypoint
        # columns of this stand-in are of the size of its 1e7 m dome)
        rigid = slice(0, K.S_ACT + K.FW_NUM_ACTUATORS)
        d = dict(state=np.abs(sa[:, rigid] - sb[:, rigid]).max(axis=1))
    print({k: float(v[~on_edge].max()) for k, v in d.items()}, "on the discontinuity:", float(d["state"][on_edge].max()))
    for k, v in d.items():
        assert v[~on_edge].max() <= 1e-9, k
    # (a perturbation that leaves v_l on the side the exact zero takes changes little; one that crosses is seen to jump)
    assert d["state"][on_edge].max() > 1e-6, "the reverse-flow states were meant to sit on the +-pi discontinuity"
    # each state enters the branch it is named for (240 Hz physics in every leg)
    by = {n: np.array([m == n for m in names]) for n in D.BRANCHES}
    w = np.linalg.norm(s0[:, K.S_OMEGA:K.S_OMEGA + 3], axis=1)
    assert (w[by["fast_spin"]] / 240 > np.pi / 4).all() and (w[~by["fast_spin"]] / 240 < 0.1).all()
    q = s0[:, K.S_QUAT:K.S_QUAT + 4]
    n2 = (q * q).sum(axis=1)
    assert (np.abs(n2[by["quat_near_unit"]] - 1) >= 1e-4).all() and (n2[by["quat_far"]] > 8.9).all()
    assert {float(np.sign(x - 1)) for x in n2[by["quat_near_unit"]]} == {-1.0, 1.0}
    qu = q / np.sqrt(n2)[:, None]
    sarg = -2 * (qu[:, 0] * qu[:, 2] - qu[:, 3] * qu[:, 1])
    assert (np.abs(sarg[by["guard_inside"]]) >= R.GUARD + 1e-9).all() and {float(np.sign(x)) for x in sarg[by["guard_inside"]]} == {-1.0, 1.0}
    go = np.abs(sarg[by["guard_outside"]])
    assert (go <= R.GUARD - 1e-9).all() and (go > np.cos(np.arccos(R.GUARD) + 1.1e-3)).all()
    assert (s0[by["zero_velocity"], K.S_VEL:K.S_VEL + 3] == 0).all()
    vb = np.array([oracle.mat_from_quat(r).T @ v for r, v in zip(q, s0[:, K.S_VEL:K.S_VEL + 3])])
    assert (vb[by["backward"] | by["reverse_exact"], 0] < -7).all() and (np.abs(vb[by["sideways"], 1]) > 7).all()
    assert (vb[by["reverse_exact"], 1:] == 0).all()
    rows = np.array([np.concatenate([[sfc, 0.0], vb[i], np.zeros(6)]) for i in np.nonzero(by["deep_stall"])[0] for sfc in range(5)])
    assert not np.asarray(R.surface_wrench(cfg, rows, LD, detail=True)[1]["nostall"]).any(), "every surface deep in stall"


def test_the_part_of_half_pi_that_the_two_word_reduction_leaves_out():
    """PIO2_LEFT_OUT, the per-quadrant term of sincos_'s far-domain bound, from the two constants of csrc/fwsim_device.hpp."""
    import mpmath
    import os
    mpmath.mp.dps = 60
    left = abs(mpmath.pi / 2 - mpmath.mpf(R.PIO2_HI) - mpmath.mpf(R.PIO2_LO))
    assert abs(left - mpmath.mpf(R.PIO2_LEFT_OUT)) < mpmath.mpf(10) ** -45
    src = open(os.path.join(os.path.dirname(__file__), "..", "pyflyt-drone_amd", "csrc", "fwsim_device.hpp")).read()
    assert "PIO2_HI = 1.57079632679489655800e+00, PIO2_LO = 6.12323399573676603587e-17" in src
