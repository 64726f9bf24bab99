"""Dev tool (CPU): how often does a wave of the 8-lane step kernel see a stalled lifting surface?

The axis-aligned tick (fwsim_device.hpp: surface_wrench_ax) skips the post-stall arithmetic when no lane of the wave is stalled,
so its gain depends on that fraction.  This estimate runs the CPU oracle on the headline config (train_waypoints_v3) with
U(-1, 1) actions, evaluates each surface's stall test (the same alpha / stall-angle arithmetic as the kernel) on the state at
every agent step, and groups envs by 8 as the step kernel's waves do.  It samples once per agent step rather than every
physics tick.      usage: python tools/stall_fraction.py
"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyflyt_drone_amd  # noqa: F401
from pyflyt_drone_amd import config as K
from oracle import fw_oracle as O
cfg = K.train_waypoints_v3_config()
n = 1024
env = O.OracleEnv(cfg, n, seed=42); env.reset()
rng = np.random.default_rng(0)
d2r = np.pi / 180
S = []
for s in range(5):
    sp = cfg.surfaces[s]
    area, AR = sp.chord * sp.span, sp.span / sp.chord
    Cl3 = sp.Cl_alpha_2D * (AR / (AR + ((2.0 * (AR + 4.0)) / (AR + 2.0))))
    th = np.arccos(2 * sp.flap_to_chord - 1); tau_f = 1 - (th - np.sin(th)) / np.pi
    a0b, asP, asN = sp.alpha_0_base_deg * d2r, sp.alpha_stall_P_base_deg * d2r, sp.alpha_stall_N_base_deg * d2r
    S.append(dict(lift=np.array(sp.lift_unit[:]), fwd=np.array(sp.forward_unit[:]), pos=np.array(sp.pos[:]), Cl3=Cl3,
                  k_dCl=Cl3 * tau_f * sp.eta * sp.deflection_limit_deg * d2r, ftc=sp.flap_to_chord, a0b=a0b,
                  Pb=Cl3 * (asP - a0b), Nb=Cl3 * (asN - a0b)))
def quat_R(q):
    x, y, z, w = q.T
    return np.stack([1 - 2*(y*y+z*z), 2*(x*y-w*z), 2*(x*z+w*y), 2*(x*y+w*z), 1-2*(x*x+z*z), 2*(y*z-w*x),
                     2*(x*z-w*y), 2*(y*z+w*x), 1-2*(x*x+y*y)], -1).reshape(-1, 3, 3)
anyw, anys, cnt = 0, 0, 0
per = np.zeros(5)
for it in range(400):
    st = env.get_state()
    R = quat_R(st[:, 3:7]); v = st[:, 7:10]; w = st[:, 10:13]; act = st[:, 13:18]
    vb = np.einsum('nji,nj->ni', R, v); wb = np.einsum('nji,nj->ni', R, w)
    stall = np.zeros((n, 5), bool)
    for s, c in enumerate(S):
        vl = vb + np.cross(wb, c['pos'])
        vlift, vf = vl @ c['lift'], vl @ c['fwd']
        alpha = np.arctan2(-vlift, vf)
        dCl = c['k_dCl'] * act[:, s]
        a0 = c['a0b'] - dCl / c['Cl3']
        aP = a0 + (c['Pb'] + c['ftc'] * dCl) / c['Cl3']; aN = a0 + (c['Nb'] + c['ftc'] * dCl) / c['Cl3']
        stall[:, s] = ~((aN < alpha) & (alpha < aP))
    if it >= 20:
        per += stall.mean(0)
        wav = stall.reshape(-1, 8, 5).any(axis=(1, 2))
        anyw += wav.mean(); anys += stall.any(1).mean(); cnt += 1
    env.step(rng.uniform(-1, 1, size=(n, 4)))
print(f"per surface stalled: {per / cnt}; env with any stall {anys / cnt:.3f}; 8-env wave with any stall {anyw / cnt:.3f}")
