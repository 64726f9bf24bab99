"""Seeded corner-case states for tests/test_directed_states_gpu.py (a plain module, like helpers.py): rigid states that enter the
branches of the physics tick which no flown trace reaches, laid over the canonical state records of freshly reset envs.

Only position, attitude and the two velocities are written, so the same call serves the state records of every task.  Env i gets
branch BRANCHES[i % len(BRANCHES)]; the draws come from ``default_rng(seed)``.  tests/test_device_functions_cpu.py holds on the
oracle alone that every state made here is finite and well conditioned over the agent step that the GPU test flies (a 1e-13
perturbation changes no flag and moves observation, reward and state by at most 1e-9); ranges that failed that were narrowed
HERE -- nothing is filtered at run time.
"""
import numpy as np

from pyflyt_drone_amd import config as K

BRANCHES = (
    "fast_spin",          # |w| dt > pi/4 (above 188 rad/s at 240 Hz): quat_integrate's angular-motion clamp
    "backward",           # reverse flow on every surface (|alpha| near pi)
    "reverse_exact",      # level attitude, velocity exactly -x: v_l = +0, v_f < 0 -- alpha = atan2(-0, v_f < 0) = -pi by the sign bit
    "sideways",           # the fin at |alpha| near pi/2, the wings without forward speed
    "zero_velocity",      # V = 0 on every surface: atan2_(0, 0), hra * V = 0
    "deep_stall",         # every surface far beyond both stall angles
    "guard_inside",       # pitch beyond the gimbal guard (|sarg| >= 0.99999)
    "guard_outside",      # pitch within 1e-3 rad of it on the other side
    "quat_near_unit",     # |q| = 1 +- 2e-4: beyond the series of two_over_norm2 / 1/sqrt(1+e), the exact-reciprocal paths
    "quat_far",           # |q| = 3
)
NUM_ENVS = 64 + 1
# reverse_exact sits ON the model's discontinuity at alpha = +-pi (that is its point: the side is chosen by a sign bit), so a
# perturbation legitimately moves it to the other side; the CPU test asserts exactly that instead of the 1e-9 amplification
ON_A_DISCONTINUITY = ("reverse_exact",)
HEIGHT = 50.0             # inside every task's bounds, far from the ground


def _quat_from_euler(e):
    hr, hp, hy = 0.5 * e[0], 0.5 * e[1], 0.5 * e[2]
    cr, sr, cp, sp, cy, sy = np.cos(hr), np.sin(hr), np.cos(hp), np.sin(hp), np.cos(hy), np.sin(hy)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


def _rot(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def apply(state, seed=2024):
    """Overwrite the rigid part of the state records [n, FW_STATE_DIM] in place; returns the branch name of every env."""
    rng = np.random.default_rng(seed)
    names = []
    edge = np.arccos(0.99999)
    for i, s in enumerate(state):
        name = BRANCHES[i % len(BRANCHES)]
        names.append(name)
        e = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), rng.uniform(-3.0, 3.0)])
        v_body = np.array([rng.uniform(14.0, 24.0), rng.uniform(-1.0, 1.0), rng.uniform(-1.5, 1.5)])
        w = rng.uniform(-0.5, 0.5, 3)
        scale = 1.0
        if name == "fast_spin":
            axis = rng.normal(size=3)
            w = axis / np.linalg.norm(axis) * rng.uniform(195.0, 400.0)
        elif name == "backward":
            v_body = np.array([-rng.uniform(8.0, 20.0), rng.uniform(-1.0, 1.0), rng.uniform(-1.5, 1.5)])
        elif name == "reverse_exact":
            e[:] = 0.0
            v_body = np.array([-rng.uniform(8.0, 20.0), 0.0, 0.0])
            w[:] = 0.0
        elif name == "sideways":
            v_body = np.array([rng.uniform(-0.5, 0.5), rng.choice([-1.0, 1.0]) * rng.uniform(8.0, 18.0), rng.uniform(-1.0, 1.0)])
        elif name == "zero_velocity":
            v_body[:] = 0.0
            w[:] = 0.0
        elif name == "deep_stall":
            v_body = np.array([rng.uniform(3.0, 6.0), rng.choice([-1.0, 1.0]) * rng.uniform(6.0, 10.0), rng.choice([-1.0, 1.0]) * rng.uniform(6.0, 10.0)])
        elif name == "guard_inside":
            e[1] = rng.choice([-1.0, 1.0]) * (np.pi / 2 - edge * rng.uniform(0.0, 0.9))
        elif name == "guard_outside":
            e[1] = rng.choice([-1.0, 1.0]) * (np.pi / 2 - edge - 10.0 ** rng.uniform(-5.0, -3.0))
        elif name == "quat_near_unit":
            scale = 1.0 + rng.choice([-1.0, 1.0]) * 2e-4
        elif name == "quat_far":
            scale = 3.0
        q = _quat_from_euler(e)
        s[K.S_POS:K.S_POS + 3] = [rng.uniform(-5.0, 5.0), rng.uniform(-5.0, 5.0), HEIGHT]
        s[K.S_QUAT:K.S_QUAT + 4] = q * scale
        s[K.S_VEL:K.S_VEL + 3] = _rot(q) @ v_body if name != "reverse_exact" else v_body
        s[K.S_OMEGA:K.S_OMEGA + 3] = w
    return names


# ---- the legs: (kernel config, oracle config, kind, routing triple) -- every kernel family of the physics tick
GUST_FORCE = dict(enabled=True, mode="gust_sine", randomize_on_reset=True, randomize_gust_phase=True,
                  wind_enu_mps_range=[[-10, 10], [-10, 10], [-0.1, 0.1]], gust_amp_enu_mps_range=[[0, 3], [0, 3], [0, 0.3]], gust_freq_hz=0.2)
DIRECT_TRIPLE, LOWLEVEL_TRIPLE = (0, 2, 3), (1, 2, 4)


def legs():
    from helpers import set_routing_mixer
    wp_kw = dict(sparse_reward=False, num_targets=3, angle_representation="euler")
    legs = {"waypoints": (K.waypoints_config(**wp_kw), K.waypoints_config(**wp_kw), "waypoints", None),
            "waypoints_gust": (K.waypoints_config(wind_config=GUST_FORCE, **wp_kw), K.waypoints_config(wind_config=GUST_FORCE, **wp_kw), "waypoints", None)}
    base = dict(flight_dome_size=200.0, max_duration_seconds=120.0, agent_hz=30, context_length=2, angle_representation="euler")
    legs["direct"] = (K.waypoints_direct_config(**base), set_routing_mixer(K.waypoints_config(**base), DIRECT_TRIPLE), "direct", DIRECT_TRIPLE)
    wp = K.waypoints_config(num_targets=1, goal_reach_distance=1e-9, flight_dome_size=1e7, max_duration_seconds=1e5,
                            angle_representation="euler", agent_hz=120, context_length=1)
    wp.warmup_aviary_steps = 0
    K._set_vec(wp.start_vel, (15.0, 0.0, 0.0))
    legs["lowlevel"] = (K.lowlevel_config(), set_routing_mixer(wp, LOWLEVEL_TRIPLE), "lowlevel", LOWLEVEL_TRIPLE)
    return legs


def actions(n, seed=7):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, 4))
