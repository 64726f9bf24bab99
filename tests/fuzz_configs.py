"""A seeded generator of valid configs off the shipped airframe, rates and start pose (a plain module, like helpers.py).

Every oracle comparison elsewhere in the suite runs the vehicle of config._fill_vehicle at 240 / 120 Hz from [0, 0, 10] at
20 m/s after 10 warm-up steps.  The kernels never read fw_config: build_params (csrc/fwsim.hip) folds it into Params<T>, and
every kernel family reads those constants its own way.  The configs made here move every folded field at once, so that a
fold or a read path that is only right for the shipped numbers shows up against the CPU oracle.

``vehicle(i, cfg)`` mutates the vehicle, rate and start-state fields of a config from ``np.random.default_rng(1000 + i)``.
Every fourth ``i`` (``i % 4 == 3``) is the axis-aligned family: the same scalar mutations, but forward stays e_x, lift is
drawn per surface from {e_y, e_z} and the inertia stays diagonal -- the only configs that reach surface_wrench_ax with
constants other than the shipped ones.

The task wrappers (``waypoints``, ``objlock``, ``combined``, ``direct_pair``, ``lowlevel_pair``) lay such a vehicle over the
task configs of pyflyt_drone_amd.config; their task fields come from ``default_rng(2000 + i)``.  Half of the configs are
wind-free (the cached warm-up, the pre-sampled waypoints and the axis-aligned tick exist only there); the other half is
split evenly over gust + force coupling, constant + airspeed coupling, and constant randomised on reset.

The streams are numpy's: tests/golden/fuzz_*.npz store the config bytes made at the time the traces were recorded, and
tests/test_fuzz_configs_cpu.py compares, so that a change of the stream shows up as such and not as a parity failure.
"""
import ctypes as C
import math

import numpy as np

from pyflyt_drone_amd import config as K

RATES = ((240, 120), (480, 120), (240, 60), (360, 120), (120, 120))          # (physics_hz, control_hz): 2, 4, 4, 3, 1 ticks per Aviary step
AGENT_HZ = (30, 10, 40, 60, 120, 24, 15)                                     # 4, 12, 3, 2, 1, 5, 8 Aviary steps per agent step
MAIN_WING = K.SURFACE_ORDER.index("main_wing")
ZERO_COLLISION_POINTS = 5                                                    # the one vehicle without collision points

GUST_FORCE = dict(enabled=True, mode="gust_sine", randomize_on_reset=True, randomize_gust_phase=True, coupling="force",
                  wind_enu_mps_range=[[-10, 10], [-10, 10], [-0.1, 0.1]],
                  gust_amp_enu_mps_range=[[0, 3], [0, 3], [0, 0.3]], gust_freq_hz=0.2)
CONST_AIRSPEED = dict(enabled=True, mode="constant", wind_enu_mps=[2.0, -3.0, 0.25], coupling="airspeed")
CONST_RANDOM = dict(enabled=True, mode="constant", randomize_on_reset=True,
                    wind_enu_mps_range=[[-5, 5], [-5, 5], [-0.5, 0.5]])
WINDS = (None, GUST_FORCE, CONST_AIRSPEED, None, CONST_RANDOM, None)         # by i % 6


def is_axis_aligned_family(i):
    return i % 4 == 3


def wind_of(i):
    return WINDS[i % 6]


def _rotation(rng, max_deg):
    """Rotation matrix of a uniform angle in [0, max_deg] about a uniformly drawn axis (Rodrigues)."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = math.radians(rng.uniform(0.0, max_deg))
    kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(a) * kx + (1.0 - math.cos(a)) * (kx @ kx)


def vehicle(i, cfg, lowlevel=False):
    """Mutate the vehicle, rate and start-state fields of `cfg` in place (and return it).  `lowlevel`: keep what the low-level
    task fixes by definition -- 240 / 120 / 120 Hz and no warm-up; the draws are made all the same, so vehicle i is the same
    airframe under every task."""
    rng = np.random.default_rng(1000 + i)
    axis = is_axis_aligned_family(i)
    # ---- mass, inertia, environment
    cfg.mass *= rng.uniform(0.7, 1.4)
    for k in range(3):
        cfg.inertia[k] *= rng.uniform(0.7, 1.4)
    products = rng.uniform(-0.03, 0.03, 3)
    for k in range(3):
        cfg.inertia[3 + k] = 0.0 if axis else float(products[k])
    cfg.gravity = rng.uniform(3.0, 10.5)
    cfg.air_density = rng.uniform(0.9, 1.3)
    # ---- lifting surfaces
    for s in range(K.FW_NUM_SURFACES):
        sp = cfg.surfaces[s]
        sp.Cl_alpha_2D *= rng.uniform(0.85, 1.1)
        sp.chord *= rng.uniform(0.75, 1.25)
        sp.span *= rng.uniform(0.75, 1.25)
        sp.flap_to_chord = rng.uniform(0.15, 0.45)
        sp.eta = rng.uniform(0.5, 0.8)
        sp.alpha_0_base_deg = rng.uniform(-4.0, 2.0)
        sp.alpha_stall_P_base_deg = rng.uniform(7.0, 16.0)
        sp.alpha_stall_N_base_deg = rng.uniform(-12.0, -6.0)
        sp.Cd_0 = rng.uniform(0.005, 0.03)
        limit = rng.uniform(8.0, 35.0)
        sp.deflection_limit_deg = 0.0 if (s == MAIN_WING and i % 3 != 0) else limit
        sp.tau = rng.uniform(0.02, 0.1)
        for k in range(3):
            sp.pos[k] += rng.uniform(-0.05, 0.05)
        rot = _rotation(rng, 8.0)
        pick = int(rng.integers(0, 2))
        if axis:
            lift, fwd = np.eye(3)[1 + pick], np.eye(3)[0]
        else:                                   # rotated together: the pair stays orthonormal
            lift, fwd = rot @ np.array(sp.lift_unit[:]), rot @ np.array(sp.forward_unit[:])
        for k in range(3):
            sp.lift_unit[k], sp.forward_unit[k] = float(lift[k]), float(fwd[k])
    # ---- motor
    m = cfg.motor
    noisy = m.noise_ratio != 0.0
    m.total_thrust = rng.uniform(10.0, 26.0)
    m.thrust_coef *= rng.uniform(0.7, 1.4)
    m.torque_coef *= rng.uniform(0.7, 1.4)
    ratio = rng.uniform(0.0, 0.06)
    m.noise_ratio = ratio if noisy else 0.0
    m.tau = rng.uniform(0.005, 0.03)
    unit = _rotation(rng, 6.0) @ np.array(m.thrust_unit[:])
    for k in range(3):
        m.thrust_unit[k] = float(unit[k])
        m.pos[k] += rng.uniform(-0.05, 0.05)
    # ---- collision points
    npts = int(rng.integers(1, K.FW_MAX_COLLISION_PTS + 1))
    pts = rng.uniform(-1.0, 1.0, (K.FW_MAX_COLLISION_PTS, 3)) * [1.0, 1.2, 0.35]
    cfg.n_collision_pts = 0 if i == ZERO_COLLISION_POINTS else npts
    for p in range(K.FW_MAX_COLLISION_PTS):
        for k in range(3):
            cfg.collision_pts[p][k] = float(pts[p, k]) if p < cfg.n_collision_pts else 0.0
    # ---- mode-0 mixer: a random sign on every entry plus cross-coupling
    signs = rng.choice([-1.0, 1.0], (K.FW_NUM_ACTUATORS, 4))
    cross = rng.uniform(-0.2, 0.2, (K.FW_NUM_ACTUATORS, 4))
    for a in range(K.FW_NUM_ACTUATORS):
        for k in range(4):
            cfg.mixer[a][k] = cfg.mixer[a][k] * signs[a, k] + cross[a, k]
    # ---- rates
    warmup = int(rng.integers(0, 14))
    if lowlevel:
        cfg.warmup_aviary_steps = 0
    else:
        cfg.physics_hz, cfg.control_hz = RATES[i % len(RATES)]
        cfg.agent_hz = AGENT_HZ[i % len(AGENT_HZ)]
        cfg.warmup_aviary_steps = warmup
    # ---- start state
    cfg.gyroscopic = int(rng.integers(0, 2))
    cfg.start_pos[2] = rng.uniform(6.0, 20.0)
    cfg.start_vel[0], cfg.start_vel[2] = rng.uniform(14.0, 26.0), rng.uniform(-2.0, 2.0)
    cfg.start_orn[0], cfg.start_orn[1], cfg.start_orn[2] = rng.uniform(-0.2, 0.2), rng.uniform(-0.15, 0.15), rng.uniform(-3.0, 3.0)
    return cfg


def _short_episodes(cfg, rng):
    """max_duration_seconds such that int(agent_hz * max_duration_seconds) is 12 ... 40: truncations and the auto-resets after
    them fall inside a 45-step trace whatever the aircraft does."""
    cfg.max_duration_seconds = (int(rng.integers(12, 41)) + 0.5) / cfg.agent_hz
    return cfg


def waypoints(i):
    rng = np.random.default_rng(2000 + i)
    cfg = K.waypoints_config(sparse_reward=bool((i // 2) % 2), num_targets=i % 9, goal_reach_distance=rng.uniform(2.0, 30.0),
                             angle_representation=("euler", "quaternion")[i % 2], context_length=(3 * i + 1) % 10,
                             wind_config=wind_of(i))
    return _short_episodes(vehicle(i, cfg), rng)


def _camera_fields(cfg, rng):
    for k in range(3):
        cfg.camera_offset[k] += rng.uniform(-0.2, 0.2)
    cfg.camera_angle_deg = rng.uniform(-25.0, 10.0)
    cfg.camera_fov_deg = rng.uniform(50.0, 110.0)
    return cfg


def _camera_kwargs(i, rng, aimed):
    scale = rng.uniform(20.0, 80.0)
    return dict(camera_resolution=(32, 64, 100, 128)[i % 4], duck_camera_capture_interval_steps=int(rng.integers(1, 13)),
                num_obstacles=int(rng.integers(0, K.FW_MAX_OBSTACLES + 1)), duck_global_scaling=max(scale, 30.0) if aimed else scale,
                wind_config=None if aimed else wind_of(i), angle_representation=("euler", "quaternion")[(i // 2) % 2],
                sparse_reward=bool(i % 2))


def objlock(i, aimed=False):
    """`aimed`: the variant of config i that the aimed-start traces fly -- no wind, and a duck of scale 30 at the least, so that
    the duck fills enough pixels of the smallest camera to be seen."""
    rng = np.random.default_rng(2000 + i)
    cfg = K.objlock_config(flight_dome_size=rng.uniform(120.0, 200.0), duck_strike_distance_m=rng.uniform(2.0, 10.0),
                           duck_lock_hold_steps=int(rng.integers(2, 8)), **_camera_kwargs(i, rng, aimed))
    return _short_episodes(_camera_fields(vehicle(i, cfg), rng), rng)


def combined(i, aimed=False):
    rng = np.random.default_rng(2000 + i)
    cfg = K.waypoint_objlock_config(num_targets=1 + i % 8, goal_reach_distance=rng.uniform(2.0, 30.0), context_length=(3 * i + 1) % 10,
                                    duck_strike_distance_m=rng.uniform(2.0, 10.0), duck_lock_hold_steps=int(rng.integers(2, 8)),
                                    **_camera_kwargs(i, rng, aimed))
    return _short_episodes(_camera_fields(vehicle(i, cfg), rng), rng)


def direct_pair(i, triple):
    """(direct-command config, oracle config) of vehicle i: the waypoints task under six actuator commands, and the oracle's
    mode-0 waypoints task behind the routing mixer of `triple` (helpers.set_routing_mixer)."""
    from helpers import set_routing_mixer
    rng = np.random.default_rng(2000 + i)
    kw = dict(sparse_reward=bool(i % 2), num_targets=1 + i % 8, goal_reach_distance=rng.uniform(2.0, 30.0),
              angle_representation=("euler", "quaternion")[(i // 2) % 2], context_length=(3 * i + 1) % 10, wind_config=wind_of(i))
    wd = _short_episodes(vehicle(i, K.waypoints_direct_config(**kw)), rng)
    wp = vehicle(i, K.waypoints_config(**kw))
    wp.max_duration_seconds = wd.max_duration_seconds
    return wd, set_routing_mixer(wp, triple)


def lowlevel_pair(i, triple):
    """(low-level config, oracle config) of vehicle i at the task's own rates: the oracle flies the waypoints task from the same
    start with nothing that ends an episode, as tests/test_lowlevel_gpu.py does for the shipped vehicle."""
    from helpers import set_routing_mixer
    ll = vehicle(i, K.lowlevel_config(wind_config=wind_of(i)), lowlevel=True)
    wp = K.waypoints_config(num_targets=1, goal_reach_distance=1e-9, flight_dome_size=1e7, max_duration_seconds=1e5,
                            angle_representation="euler", agent_hz=120, context_length=1, wind_config=wind_of(i))
    wp.warmup_aviary_steps = 0
    K._set_vec(wp.start_vel, (15.0, 0.0, 0.0))
    vehicle(i, wp, lowlevel=True)
    return ll, set_routing_mixer(wp, triple)


def config_bytes(cfg):
    return np.frombuffer(C.string_at(C.byref(cfg), C.sizeof(cfg)), dtype=np.uint8).copy()


# ---- the sets the tests run (tests/test_fuzz_configs_cpu.py checks the conditions on every one of them, none left out)
N_WAYPOINTS, N_CAMERA, N_DIRECT = 32, 9, 6            # (camera vehicle 8: no warm-up steps, so its hand-off is the closing pass alone)
TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 4), (1, 3, 4), (2, 3, 4), (0, 2, 3))    # routing mixers of the six direct / low-level vehicles
DIRECT_VEHICLES = (0, 1, 2, 3, 4, 7)                                            # two of them of the axis-aligned family
NUM_ENVS, SEED, ACTION_SEED = 199, 1234, 5                                      # 199: not a multiple of 64, of 8 or of the tile
WAYPOINT_STEPS, CAMERA_STEPS, AIMED_STEPS, DIRECT_STEPS = 60, 45, 60, 60
AIMED_MIN_VISIBLE = 300
# Waypoint configs that fly again with the hand-off of pre-built episode starts switched off: four wind-free (3, 11: axis-aligned
# family; 11: no warm-up steps), four windy (7: axis-aligned family), and 8 -- windy without warm-up steps, the pre-simulated start
# whose closing pass (first compute_state, first observation) was once left out, so that the episode began with an all-zero observation
RESET_PATH_CONFIGS = (0, 3, 5, 11) + (1, 2, 4, 7) + (8,)
# Camera configs that fly again with the captures on a second wave (which is the builder of the pre-simulated starts as well)
CAPTURE_WAVE_CONFIGS = (("objlock", 1), ("objlock", 3), ("combined", 2), ("combined", 6), ("objlock", 8))


def actions_of(mode, rng, n):
    """The four mode-0 actions of one step of a leg (the direct / low-level kernels get them through helpers.route)."""
    from helpers import seeded_actions
    if mode == "uniform":
        return seeded_actions(rng, n, "uniform")
    if mode == "gentle":
        return seeded_actions(rng, n, "gentle")
    if mode == "aimed":
        return seeded_actions(rng, n, "gentle") * 0.3
    a = rng.uniform(-1.0, 1.0, size=(n, 4))
    if mode == "lowlevel":
        a[:, :3] *= 0.3
    return a


def aim_at_the_duck(oracle, state, rng):
    """Aircraft aimed at their duck from 60-200 m along a glide slope (tests/test_parity_gpu.py:_aimed_flights), in place on the
    canonical state records of a camera task after its reset; each keeps the speed it had."""
    T0 = K.S_TASK
    for s in state:
        rng_d, yaw, height = rng.uniform(60.0, 200.0), rng.uniform(-np.pi, np.pi), rng.uniform(8.0, 30.0)
        duck = s[T0:T0 + 3]
        pitch = np.arctan2(height, rng_d) * rng.uniform(0.6, 1.1)              # positive pitch = nose down
        speed = np.linalg.norm(s[K.S_VEL:K.S_VEL + 3])
        s[K.S_POS:K.S_POS + 3] = [duck[0] - rng_d * np.cos(yaw), duck[1] - rng_d * np.sin(yaw), height]
        s[K.S_QUAT:K.S_QUAT + 4] = oracle.quat_from_euler([0.0, pitch, yaw])
        s[K.S_VEL:K.S_VEL + 3] = oracle.mat_from_quat(s[K.S_QUAT:K.S_QUAT + 4]) @ np.array([speed, 0.0, 0.0])
        s[K.S_OMEGA:K.S_OMEGA + 3] = 0.0
    return state


def legs():
    """Every trace the GPU tests fly, as (id, mode, steps, oracle config): what tests/test_fuzz_configs_cpu.py holds its
    conditions over.  Nothing is filtered: the generator's ranges are what keeps every one of them well conditioned."""
    for i in range(N_WAYPOINTS):
        yield f"waypoints-{i}", "uniform", WAYPOINT_STEPS, waypoints(i)
    for i in range(N_CAMERA):
        yield f"objlock-{i}", "gentle", CAMERA_STEPS, objlock(i)
        yield f"objlock-aimed-{i}", "aimed", AIMED_STEPS, objlock(i, aimed=True)
        yield f"combined-{i}", "gentle", CAMERA_STEPS, combined(i)
        yield f"combined-aimed-{i}", "aimed", AIMED_STEPS, combined(i, aimed=True)
    for i, t in zip(DIRECT_VEHICLES, TRIPLES):
        yield f"direct-{i}", "direct", DIRECT_STEPS, direct_pair(i, t)[1]
        yield f"lowlevel-{i}", "lowlevel", DIRECT_STEPS, lowlevel_pair(i, t)[1]
