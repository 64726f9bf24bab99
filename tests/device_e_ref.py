"""The E_ref constants of tests/test_device_functions_gpu.py (a plain data module: the CPU test that recomputes them imports it
without importing the GPU test)."""
# E_ref: device_reference.e_ref_table(oracle) on the CPU (x86-64 glibc libm, numpy 2); tests/test_device_functions_cpu.py
# recomputes every entry.  float32 surfaces at 20 rad/s: below 10 m/s the rate is about the axis through the surface's position (the
# rate's 20 m/s would otherwise cancel down to V and the plain float32 evaluation be lost), and V = 1e-3 is left to float64.
E_REF = {
    "surface:V=10,rate=0:float64": 5.055e-14, "surface:V=10,rate=20:float64": 1.820e-13, "surface:V=1,rate=0:float64": 5.305e-14,
    "surface:V=1,rate=20:float64": 1.167e-12, "surface:V=0.001,rate=0:float64": 6.924e-14, "surface:V=0.001,rate=20:float64": 1.316e-09,
    "surface_ax:float64": 1.321e-14,
    "rot_from_quat:float64": 6.603e-16, "rot_from_unit_quat:float64": 5.345e-16, "normalize_quat:float64": 2.379e-16,
    "two_over_norm2:float64": 1.110e-16, "euler:random:float64": 6.262e-16, "euler:near_guard:float64": 3.011e-14,
    "euler:locked:float64": 4.254e-16, "euler:wrap:float64": 2.614e-16, "quat_from_euler:float64": 2.121e-16,
    "quat_step:float64": 2.145e-16, "normal2:float64": 6.516e-16, "wind:float64": 2.660e-14, "log:float64": 1.097e-16,
    "surface:V=10,rate=0:float32": 1.166e-04, "surface:V=10,rate=20:float32": 1.049e-04, "surface:V=1,rate=0:float32": 9.154e-05,
    "surface:V=1,rate=20:float32": 1.911e-04, "surface:V=0.001,rate=0:float32": 7.518e-05,
    "rot_from_quat:float32": 3.549e-07, "rot_from_unit_quat:float32": 3.356e-07, "normalize_quat:float32": 1.043e-07,
    "two_over_norm2:float32": 5.960e-08, "euler:random:float32": 2.938e-07, "euler:near_guard:float32": 1.403e-05,
    "euler:locked:float32": 4.783e-07, "euler:wrap:float32": 1.874e-07, "quat_from_euler:float32": 1.121e-07,
    "quat_step:float32": 1.298e-07, "normal2:float32": 4.447e-07, "wind:float32": 1.355e-05,
    "rcp:float32": 5.894e-08, "sqrt:float32": 5.887e-08, "sin:float32": 5.568e-08, "sincos.sin:float32": 5.568e-08,
    "sincos.cos:float32": 5.652e-08, "sin.far:float32": 5.322e-08, "sincos.sin.far:float32": 5.322e-08,
    "sincos.cos.far:float32": 5.573e-08, "asin:float32": 1.699e-07, "log:float32": 9.418e-08, "div:float32": 5.938e-08,
    "atan2:float32": 2.787e-07,
}
