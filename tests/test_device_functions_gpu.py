"""The device building blocks of csrc/fwsim_device.hpp one function at a time, through the test hook fw_probe, against the
longdouble run of tests/device_reference.py.

Two kinds of bound, neither taken from what the kernels give:

* The hand-written float64 math (M<double>) is held to the claim in its own source: rcp_ / div_ / sqrt_ within 1 ulp of the
  longdouble result; sincos_ / sin_ / atan2_ / asin_ within 4.5e-16 absolute, and within 4 ulp of the reference where
  |reference| < 0.25 (the absolute bound is loose there, and small angles of attack live there).  Beyond |x| = 2 pi the
  relative half of sincos_ / sin_ carries one more term, stated in the source: the two-word Cody-Waite reduction leaves
  1.5e-33 of pi/2 out, so the reduced argument of quadrant count k = rint(x * 2/pi) is off by |k| * 1.5e-33 and a result below
  0.25 is held to 4 ulp + |k| * 1.5e-33 (device_reference.PIO2_LEFT_OUT, a property of the two constants, recomputed with mpmath
  on the CPU).  The one far-domain caller, the gust clock, needs the absolute figure alone.  There is no validation limit on
  the clock's argument 2 pi f t + phase (gust_freq_hz is unbounded); the reduction is exact while k fits an int, |x| < 3.3e9,
  and the far domain here runs to 1e9 -- 0.2 Hz gusts for 25 years.
* float32 (M<float> is the device libm) and every composite function: the kernel may be 8 x E_ref from the longdouble result,
  with a floor of 4 machine epsilons, both times the natural scale of the output.  E_ref is the worst normalised error of the
  PLAIN evaluation in the working precision (the oracle's C function where it exports one, else the numpy restatement run in
  that precision) on the same input set, computed on the CPU, written below, and recomputed by
  tests/test_device_functions_cpu.py, which fails if a figure moved by more than a factor 2.  The 8 pays for the kernel's
  different association at equal conditioning (one shared reciprocal, v_f / V for cos(alpha), series for divisions, the DPP
  sum order); a wrong coefficient, sign, branch or constant fold shows at 1e-6 relative or worse.

Every figure is printed before it is asserted; with FWSIM_MARGIN_OUT=<file> the session writes them all there
(profiles/device_functions_margin.txt is such a file).
"""
import ctypes as C
import os

import numpy as np
import pytest

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
import device_reference as R
from device_e_ref import E_REF

pytestmark = pytest.mark.gpu
LD = R.LD

ABS_CLAIM, ULP_CLAIM, SMALL = 4.5e-16, 4.0, 0.25          # the claim of csrc/fwsim_device.hpp for sincos_ / sin_ / atan2_ / asin_
DTYPES = {"float64": np.float64, "float32": np.float32}

_MARGIN = []


def record(function, dtype, variant, bound, source, measured):
    line = f"{function:34s} {dtype:8s} {variant:12s} bound {bound:<28s} [{source}]  measured {measured}"
    print(line)
    _MARGIN.append(line)


@pytest.fixture(scope="module", autouse=True)
def margin_file():
    yield
    path = os.environ.get("FWSIM_MARGIN_OUT")
    if path and _MARGIN:
        with open(path, "a") as f:
            f.write("\n".join(_MARGIN) + "\n")


@pytest.fixture(scope="module")
def handles():
    """One small env per (vehicle, dtype, wind) on demand: fw_probe takes its constants and its dtype from a handle."""
    made = {}

    def get(vehicle="shipped", dtype="float64", wind=None):
        key = (vehicle, dtype, wind is not None)
        if key not in made:
            made[key] = P.FixedwingVecEnv(R.vehicle_config(vehicle, dtype, wind), 8, seed=77)
        return made[key]
    yield get
    for env in made.values():
        env.close()


def probe(env, op, variant, rows, check=True):
    """fw_probe on host rows [n, in_cols] -> host [n, out_cols]; the output buffer carries a guard row that must stay untouched."""
    import torch
    cin, cout, _ = R.SHAPES[(op, variant)]
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, cin)
    n = len(rows)
    x = torch.as_tensor(rows, device=env.device)
    out = torch.full((n + 1, cout), -12345.0, dtype=torch.float64, device=env.device)
    rc = _lib.lib().fw_probe(env._h, op, variant, C.c_void_p(x.data_ptr()), cin, C.c_void_p(out.data_ptr()), cout, n, env._stream())
    if not check:
        return rc
    _lib.check(rc, env._h)
    o = out.cpu().numpy()
    assert (o[n] == -12345.0).all(), "fw_probe wrote past its last row"
    return o[:n]


def probe_counts(env, op, variant, rows, exact=True, within=None):
    """The full launch, and launches of the first 1, 9, 65 and 520 rows (a partly filled group, a partly filled wave, more than
    one workgroup): the rows are independent, so a shorter launch reproduces its rows bit for bit.  `exact=False` (surface_wrench_ax,
    whose path depends on what the other lanes of the wave hold): `within(out, n)` checks a shorter launch under the bound."""
    full = probe(env, op, variant, rows)
    for n in R.ROW_COUNTS:
        if n > len(rows):
            continue
        short = probe(env, op, variant, rows[:n])
        if exact:
            np.testing.assert_array_equal(short, full[:n], err_msg=f"{n} rows")
        else:
            within(short, n)
    return full


def derived_bound(key, dt):
    return max(8.0 * E_REF[key], 4.0 * R.eps_of(dt))


# ------------------------------------------------------------------------------------------------ the hook itself
def test_fw_probe_rejects_bad_arguments(handles):
    import torch
    env, f32 = handles(), handles(dtype="float32")
    L = _lib.lib()
    x = torch.zeros((8, 16), dtype=torch.float64, device=env.device)
    o = torch.zeros((8, 80), dtype=torch.float64, device=env.device)
    px, po, st = C.c_void_p(x.data_ptr()), C.c_void_p(o.data_ptr()), env._stream()
    assert L.fw_probe(env._h, R.MATH1, 0, px, 1, po, 7, 8, st) == K.FW_OK
    for args in ((99, 0, px, 1, po, 7, 8), (R.MATH1, 1, px, 1, po, 7, 8), (R.SURFACE, 4, px, 11, po, 6, 8), (R.MATH1, 0, None, 1, po, 7, 8),
                 (R.MATH1, 0, px, 1, None, 7, 8), (R.MATH1, 0, px, 1, po, 7, 0), (R.MATH1, 0, px, 1, po, 7, -3), (R.MATH1, 0, px, 2, po, 7, 8),
                 (R.MATH1, 0, px, 1, po, 6, 8), (R.GROUP, 0, px, 16, po, 10, 1)):
        assert L.fw_probe(env._h, *args, st) == K.FW_EINVAL, args
        assert b"fw_probe" in L.fw_last_error(env._h)
    assert L.fw_probe(None, R.MATH1, 0, px, 1, po, 7, 8, st) == K.FW_EINVAL
    # a variant the dtype / the airframe has no kernel for
    assert L.fw_probe(f32._h, R.SURFACE, R.SURFACE_AX, px, 11, po, 6, 1, st) == K.FW_EUNSUPPORTED
    assert "fuzz2" not in R.AX_VEHICLES
    assert L.fw_probe(handles("fuzz2")._h, R.SURFACE, R.SURFACE_AX, px, 11, po, 6, 1, st) == K.FW_EUNSUPPORTED
    assert L.fw_probe(env._h, R.SURFACE, R.SURFACE_AX, px, 11, po, 6, 1, st) == K.FW_OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ float64 elementary math
@pytest.mark.parametrize("name", ["rcp", "sqrt", "div"])
def test_f64_rcp_div_sqrt_within_one_ulp(handles, name):
    """Hardware seed + Newton steps against the correctly rounded longdouble result: within 1 ulp, over random mantissas at
    exponents +-100, 1, powers of two and the extremes the physics hands them (device_reference.PHYSICS_EXTREMES_*)."""
    R.require_longdouble()
    op, col, x, ref, _, _ = R.math_case(name, np.float64)
    got = probe_counts(handles(), op, 0, x)[:, col]
    u = R.ulps(got, ref, np.float64)
    record(name + "_", "float64", "-", "1 ulp", "claim in fwsim_device.hpp", f"{u.max():.3f} ulp at {x[u.argmax()]}")
    assert np.isfinite(got).all() and u.max() <= 1.0
    if name == "sqrt":
        assert got[x[:, 0] == 0.0].tolist() == [0.0] * int((x[:, 0] == 0.0).sum()), "sqrt_(0) must be 0, not the NaN of 0 * rsq(0)"


@pytest.mark.parametrize("name", ["sin", "sincos.sin", "sincos.cos", "asin", "atan2", "sin.far", "sincos.sin.far", "sincos.cos.far"])
def test_f64_trig_within_the_claim(handles, name):
    R.require_longdouble()
    op, col, x, ref, _, _ = R.math_case(name, np.float64)
    got = probe_counts(handles(), op, 0, x)[:, col]
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    u = R.ulps(got, ref, np.float64)
    small = np.abs(ref) < SMALL
    far = name.endswith(".far")
    # the relative half: 4 ulp of the reference, plus (far domain) what the two-word reduction leaves out of k * pi/2
    k = np.abs(np.rint(x[:, 0] * (2 / np.pi))) if far else 0.0
    allowed = ULP_CLAIM * np.spacing(np.abs(np.asarray(ref, dtype=np.float64))).astype(LD) + k * LD(R.PIO2_LEFT_OUT)
    excess = np.asarray(np.abs(got.astype(LD) - ref) / allowed, dtype=np.float64)
    worst_u = float(u[small].max()) if small.any() else 0.0
    record(name.replace(".far", "") + ("_ far" if far else "_"), "float64", "-", "4.5e-16 abs, 4 ulp" + (" + |k| 1.5e-33" if far else "") + " below 0.25",
           "claim in fwsim_device.hpp", f"{err.max():.3e} abs; {worst_u:.3f} ulp where |ref| < 0.25, {excess[small].max():.3f} of the relative bound")
    assert np.isfinite(got).all() and err.max() <= ABS_CLAIM
    assert excess[small].max() <= 1.0, f"{worst_u} ulp; worst at {x[small][excess[small].argmax()]}"
    if not far:
        assert worst_u <= ULP_CLAIM


def test_f64_atan2_signed_zeros_follow_libm(handles):
    """atan2_ takes the sign BIT of y, as libm does: a -0 numerator in front of a negative x is -pi.  (It was +pi while the sign
    test was `y < 0`: a surface in exact reverse flow, v_l = +0, then stalled on the other side than the oracle's --
    tests/test_directed_states_gpu.py flies that state.)"""
    pts = np.array([[-0.0, -1.0], [0.0, -1.0], [-0.0, 1.0], [0.0, 1.0], [-0.0, 0.0], [0.0, 0.0], [-0.0, -2.0 ** 20], [-0.0, -2.0 ** -20]])
    got = probe(handles(), R.MATH2, 0, pts)[:, 1]
    want = np.arctan2(pts[:, 0], pts[:, 1])
    want[5] = 0.0
    assert want[0] == -np.pi and want[1] == np.pi
    np.testing.assert_array_equal(got[[0, 1, 6, 7]], want[[0, 1, 6, 7]])
    np.testing.assert_array_equal(np.abs(got[[2, 3, 4, 5]]), [0.0, 0.0, 0.0, 0.0])
    assert np.signbit(got[2]) and not np.signbit(got[3]), "atan2(-0, x > 0) = -0"


# ------------------------------------------------------------------------------------------------ derived bounds: elementary
@pytest.mark.parametrize("dtype,name", [("float32", n) for n in R.F32_MATH] + [("float64", n) for n in R.F64_DERIVED_MATH])
def test_libm_math_within_the_derived_bound(handles, dtype, name):
    R.require_longdouble()
    dt = DTYPES[dtype]
    op, col, x, ref, _, scale = R.math_case(name, dt)
    got = probe_counts(handles(dtype=dtype), op, 0, x)[:, col]
    key = R.e_ref_key(name, None, dt)
    bound = derived_bound(key, dt)
    worst = R.normalised_error(got, ref, scale)
    record(name, dtype, "-", f"{bound:.3e} of the scale", f"max(8 E_ref, 4 eps), E_ref {E_REF[key]:.3e}", f"{worst:.3e}")
    assert np.isfinite(got).all() and worst <= bound


# ------------------------------------------------------------------------------------------------ derived bounds: composites
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name,group", [c for c in R.COMPOSITE if c[0] != "surface"])
def test_composite_within_the_derived_bound(handles, dtype, name, group):
    """rot_from_quat / rot_from_unit_quat / normalize_quat / two_over_norm2 (both sides of its |e| < 1e-4 series switch and |q| = 3:
    the exact-reciprocal path), euler_from_quat on both sides of the gimbal guard, per lane and in its 8-lane form on groups at every
    position of the wave, quat_from_euler, quat_integrate (the |w| dt > pi/4 clamp from both sides, un-normalised q: the exact
    1/sqrt path), the Box-Muller half of rng_normal2, and the gust rotation against wind_at."""
    R.require_longdouble()
    dt = DTYPES[dtype]
    c = R.case(name, dt, group=group)
    env = handles(dtype=dtype, wind=R.GUST) if name == "wind" else handles(dtype=dtype)
    key = R.e_ref_key(name, group, dt)
    bound = derived_bound(key, dt)
    for v in c["variants"]:
        out = probe_counts(env, c["op"], v, c["rows"])
        if (c["op"], v) == (R.EULER, R.EULER_LANES8):
            # every lane of the group holds the handed-round result: the eight copies are one value, bit for bit
            out = out.reshape(len(out), 8, 4)
            np.testing.assert_array_equal(out, np.repeat(out[:, :1], 8, axis=1), err_msg="the lanes of a group disagree")
            out = out[:, 0]
        d = out[:, c["cols"]].astype(LD) - c["ref"]
        if c.get("circular"):
            d[:, [0, 2]] = R.circular(d[:, [0, 2]])
        worst = R.normalised_error(d + c["ref"], c["ref"], c["scale"])
        record(name + ("" if group is None else ":" + group), dtype, f"variant {v}", f"{bound:.3e} of the scale", f"max(8 E_ref, 4 eps), E_ref {E_REF[key]:.3e}", f"{worst:.3e}")
        assert np.isfinite(out[:, c["cols"]]).all() and worst <= bound, (name, group, v)
        if name == "euler":
            np.testing.assert_array_equal(out[:, 3] != 0, c["lock"], err_msg="the gimbal guard was taken on another side than the reference's")
            assert c["lock"].all() == (group == "locked") and c["lock"].any() == (group == "locked")
    if name == "quat_step":
        assert 4 < c["clamped"].sum() < len(c["rows"]) - 4, "both sides of the angular-motion clamp"
    if name == "wind":
        np.testing.assert_allclose(out[:, 0:3], out[:, 3:6], rtol=0, atol=bound * np.asarray(c["scale"][:, :3], dtype=np.float64).max())


SURFACE_CASES = [(v, g, d) for v in R.VEHICLES for d, dt in DTYPES.items() for g in R.surf_groups(dt)]


@pytest.mark.parametrize("vehicle,group,dtype", SURFACE_CASES, ids=[f"{v}-V{g[0]:g}-rate{g[1]:g}-{d}" for v, g, d in SURFACE_CASES])
def test_surface_wrench_every_variant(handles, dtype, vehicle, group):
    """One surface's force and torque from every copy of the function the handle has -- constants by scalar load, in registers, in
    LDS, and (float64, axis-aligned airframes) surface_wrench_ax -- with alpha through the full circle: pre-stall, post-stall on
    both sides, +-pi/2, reverse flow, V = 0."""
    R.require_longdouble()
    dt = DTYPES[dtype]
    c = R.case("surface", dt, group=group, vehicle=vehicle)
    env = handles(vehicle, dtype)
    key = R.e_ref_key("surface", group, dt)
    bound = derived_bound(key, dt)
    d = c["detail"]
    stalled = ~np.asarray(d["nostall"])
    assert stalled.sum() > 100 and (~stalled).sum() > 30 and (np.abs(np.asarray(d["alpha"], dtype=np.float64)) > 3.0).any(), "post-stall, pre-stall and reverse flow"
    assert group[1] != 0 or (np.asarray(d["V"]) == 0).sum() == 5, "V = 0 exactly"
    variants = list(c["variants"]) + ([R.SURFACE_AX] if dtype == "float64" and vehicle in R.AX_VEHICLES else [])
    for v in variants:
        def within(short, n):
            e = R.normalised_error(short, c["ref"][:n], c["scale"][:n])
            assert np.isfinite(short).all() and e <= bound, (vehicle, group, v, n, e)
        out = probe_counts(env, R.SURFACE, v, c["rows"], exact=v != R.SURFACE_AX, within=within)
        worst = R.normalised_error(out, c["ref"], c["scale"])
        record(f"surface_wrench {vehicle} V={group[0]:g} rate={group[1]:g}", dtype, ("scalar", "registers", "lds", "ax")[v], f"{bound:.3e} of the scale",
               f"max(8 E_ref, 4 eps), E_ref {E_REF[key]:.3e}", f"{worst:.3e}")
        assert np.isfinite(out).all() and worst <= bound, (vehicle, group, v)


@pytest.mark.parametrize("vehicle", ["shipped", "fuzz3"])
def test_surface_wrench_ax_shortcut_taken_and_refused(handles, vehicle):
    """surface_wrench_ax skips the post-stall arithmetic when no lane of the WAVE is stalled: waves that are wholly pre-stall
    (shortcut taken), waves in which exactly one lane of one group is stalled -- every group and surface in turn -- (refused by a
    single lane), and wholly stalled waves.  A row is a group; its five surfaces are read in five launches of the same waves."""
    R.require_longdouble()
    cfg = R.vehicle_config(vehicle)
    rows, expect = R.ax_wave_inputs(cfg)
    env = handles(vehicle)
    key = "surface_ax:float64"
    bound = derived_bound(key, np.float64)
    worst, stalled = 0.0, np.zeros(len(rows), int)
    for s in range(5):
        r = rows.copy(); r[:, 0] = s
        ref, d = R.surface_wrench(cfg, r, LD, detail=True)
        stalled += ~np.asarray(d["nostall"])
        out = probe(env, R.SURFACE, R.SURFACE_AX, r)
        worst = max(worst, R.normalised_error(out, ref, d["scale"]))
    np.testing.assert_array_equal(stalled.reshape(-1, 8).sum(axis=1), expect)
    record(f"surface_wrench_ax waves {vehicle}", "float64", "ax", f"{bound:.3e} of the scale", f"max(8 E_ref, 4 eps), E_ref {E_REF[key]:.3e}", f"{worst:.3e}")
    assert worst <= bound


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_surface_in_exact_reverse_flow(handles, dtype):
    """v_f < 0 with v_l an exact zero: alpha is +pi or -pi by the sign bit of -v_l alone, and the two sides differ in the pitching
    moment (|alpha_eff| differs by 2 |alpha_0|).  Every variant must take libm's side, -pi, as the reference and the oracle do."""
    R.require_longdouble()
    dt = DTYPES[dtype]
    cfg = R.vehicle_config("shipped")
    rows = np.array([np.concatenate([[s, a], [-10.0, z, z], np.zeros(6)]) for s in range(5) for a in (-1.0, 0.5) for z in (0.0, -0.0)])
    ref, d = R.surface_wrench(cfg, rows, LD, detail=True)
    alpha = np.asarray(d["alpha"], dtype=np.float64)
    # (v_b + w x r - wind turns either zero into +0, so v_l = +0 and libm's alpha = atan2(-0, -10) is -pi on every row)
    assert (alpha == -np.pi).all()
    bound = derived_bound(R.e_ref_key("surface", (10.0, 0.0), dt), dt)
    for v in (R.SURFACE_SCALAR, R.SURFACE_REGS, R.SURFACE_LDS) + ((R.SURFACE_AX,) if dtype == "float64" else ()):
        out = probe(handles(dtype=dtype), R.SURFACE, v, rows)
        worst = R.normalised_error(out, ref, d["scale"])
        record("surface_wrench reverse flow +-0", dtype, ("scalar", "registers", "lds", "ax")[v], f"{bound:.3e} of the scale", "E_ref of V=10, rate=0", f"{worst:.3e}")
        assert worst <= bound, v


# ------------------------------------------------------------------------------------------------ exact: lanes and integers
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_group_helpers_exact(handles, dtype):
    """group_sum / group_min / group_or / group_any / lane_pick5 / lane_act_scatter + gather on integers: exact, on every group of
    a wave, with partly filled last waves."""
    rng = np.random.default_rng(31)
    n = 520
    v = rng.integers(-1000, 1000, (n, 8)).astype(np.float64)
    b = rng.integers(0, 2 ** 32, (n, 8)).astype(np.float64)
    b[::3] = np.floor(b[::3] / 2) * 2                      # rows without an odd word: group_any false
    b[5] = 0.0
    out = probe_counts(handles(dtype=dtype), R.GROUP, 0, np.concatenate([v, b], axis=1)).reshape(n, 8, 10)
    bi = b.astype(np.uint64)
    for lane in range(8):
        np.testing.assert_array_equal(out[:, lane, 0], v.sum(axis=1))
        np.testing.assert_array_equal(out[:, lane, 1], v.min(axis=1))
        np.testing.assert_array_equal(out[:, lane, 2].astype(np.uint64), np.bitwise_or.reduce(bi, axis=1))
        np.testing.assert_array_equal(out[:, lane, 3], ((bi & 1) != 0).any(axis=1))
        np.testing.assert_array_equal(out[:, lane, 4], v[:, min(lane, 4)])
        np.testing.assert_array_equal(out[:, lane, 5:10], v[:, :5] + 1000.0 * np.arange(5))
    assert 0 < out[:, 0, 3].sum() < n
    for fn in ("group_sum", "group_min", "group_or", "group_any", "lane_pick5", "lane_act_scatter/gather"):
        record(fn, dtype, "8 lanes", "exact", "integers as doubles", f"equal on {n} groups x 8 lanes")


def test_philox_uniform_exact(handles, oracle):
    """Philox4x32-10 bit for bit against the oracle's, counters and keys with bit 31 set included; rng_uniform within 1 ulp of the
    literal lo + (hi - lo) * u (the kernel may contract it into one fma)."""
    rng = np.random.default_rng(32)
    n = 520
    w = rng.integers(0, 2 ** 32, (n, 6), dtype=np.uint64).astype(np.uint32)
    w[0], w[1], w[2] = 0, 0xFFFFFFFF, 0x80000000
    w[3] = [1, 2, 3, 4, 5, 6]
    out = probe_counts(handles(), R.RNG, R.RNG_PHILOX, w.astype(np.float64)).astype(np.uint32)
    np.testing.assert_array_equal(out, R.philox4x32_10(w[:, :4], w[:, 4:]))
    for i in range(0, n, 13):
        np.testing.assert_array_equal(out[i], oracle.philox(w[i, :4], w[i, 4:]))
    record("philox4x32_10", "uint32", "-", "exact", "oracle fwo_philox / numpy restatement", f"equal on {n} blocks")
    env = handles()
    rows = np.stack([rng.integers(0, 2 ** 32, n), rng.integers(0, 2 ** 31, n), rng.integers(0, 64, n), rng.uniform(-50, 0, n), rng.uniform(0, 50, n)], axis=1).astype(np.float64)
    rows[0, 0] = 2.0 ** 32 - 1
    got = probe_counts(env, R.RNG, R.RNG_UNIFORM, rows)[:, 0]
    u = np.array([oracle.rng_uniform01(env.seed_value, int(r[0]), int(r[1]), 0, int(r[2])) for r in rows])
    want = rows[:, 3].astype(LD) + (rows[:, 4].astype(LD) - rows[:, 3].astype(LD)) * u.astype(LD)
    # an ulp at the size of the operands: the product (hi - lo) * u is rounded at that size whatever the sum comes to
    ul = np.asarray(np.abs(got.astype(LD) - want) / np.spacing(np.maximum(np.abs(rows[:, 3]), rows[:, 4] - rows[:, 3])), dtype=np.float64)
    record("rng_uniform", "float64", "-", "1 ulp of the operands", "the literal formula; the ulp is taken at max(|lo|, hi - lo), not at the result: looser than an ulp of a result near zero",
           f"{ul.max():.3f} ulp")
    assert ul.max() <= 1.0 and (0 <= u).all() and (u < 1).all()
