"""The fixed-shape step kernel whose second wave stays to the end of the launch (fwsim.hip: fw_step_kernel_g8xo, step_body OBSW).
Behind the noise draw that wave is the scenario worker of its own tile -- the grid has no worker workgroups -- and behind a second
workgroup barrier it runs the observation pass from a hand-off block in LDS, copies terminal observations out, takes the first row
the worker left (mode 1) and flushes the tile, while the step wave stores state and counters and, on the in-kernel fallback (mode 2),
the new episode's row straight to memory.  Only where the arithmetic runs changes, so every output must be bit-identical.

Twins: the same config, seed and actions on a handle created under FWSIM_OBS_WAVE=0 (fw_step_kernel_g8xs: worker workgroups, the
step wave writes its own rows) and on one created under FWSIM_STEP_SHAPE=0 (fw_step_kernel_g8x: the phase machine).  All six outputs
are compared after every step, state and counters at the end.  Sizes: 8 envs = one full tile, 11 = a ragged second tile with five
inactive rows, 64 = 8 tiles (the XCD block map is active).

What each trace covers was chosen on the CPU oracle alone and is asserted there, before a handle is created:
  * 14 m dome, seed 7, uniform actions of default_rng(5), 40 steps: every episode lasts 8 steps or more and envs end beside envs of
    the same tile that fly on -- at 11 envs in the ragged tile as well.  An env asks for its next scenario in the first launch of an
    episode, the worker serves it in the second, and a reset may take it from the third on: these resets are all hits (mode 1).
  * the same with goal_reach_distance 12 m: episodes of two steps (all waypoints within reach at the start) beside episodes of three
    and more in one tile.  A reset that follows a reset within two launches cannot have its scenario yet and must fall back
    (mode 2); the longer episodes hit.  Both modes, and mode-0 rows, share tiles -- the flush must skip exactly the mode-2 rows.
  * FWSIM_NO_SHADOW=1: no worker, every reset is mode 2.
  * auto_reset off: tiles hold envs that are done at entry (stale action view, pre-loaded by the second wave) beside stepping ones.
"""
import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
import directed_states as D
from helpers import run_lockstep, seeded_actions

pytestmark = pytest.mark.gpu

SEED = 7
OUTPUTS = ("obs", "rewards", "terminated", "truncated", "terminal_obs", "info")
SIZES = (8, 11, 64)
STEPS = 40
DOME = dict(flight_dome_size=14.0)
SHORT = dict(flight_dome_size=14.0, goal_reach_distance=12.0)
STALE_STEPS = 25
# one field of the row changed at a time: (config overrides, envs), as tests/test_step_shape_gpu.py lists them for the shape
OFF_ROW = {
    "agent_hz_60": (dict(agent_hz=60), 4096),
    "context_3": (dict(context_length=3), 4096),
    "targets_4": (dict(num_targets=4), 4096),
    "dense_reward": (dict(sparse_reward=False), 4096),
    "quaternion": (dict(angle_representation="quaternion"), 4096),
    "no_motor_noise": (dict(motor_noise=False), 4096),
    "float32": (dict(dtype="float32"), 4096),
    "wind": (dict(wind_config=K.TRAIN_OBJLOCK_WIND), 4096),
    "envs_4097": (dict(), 4097),
}


def _cfg(**kw):
    return K.train_waypoints_v3_config(**kw)


def _sel(env):
    L = _lib.lib()
    return int(L.fw_obs_wave(env._h)), int(L.fw_step_shape(env._h)), int(L.fw_aux_wave(env._h))


def _make(monkeypatch, n, env_vars, seed=SEED, **kw):
    for name in ("FWSIM_OBS_WAVE", "FWSIM_STEP_SHAPE", "FWSIM_AUX_WAVE"):
        monkeypatch.delenv(name, raising=False)
    for name, v in env_vars.items():
        monkeypatch.setenv(name, v)
    env = P.FixedwingVecEnv(_cfg(**kw), n, device=0, seed=seed)
    for name in env_vars:
        monkeypatch.delenv(name)
    return env


def _trio(monkeypatch, n, seed=SEED, **kw):
    """(handle on the observation-wave kernel, its twin on fw_step_kernel_g8xs, its twin on fw_step_kernel_g8x)"""
    new = _make(monkeypatch, n, {"FWSIM_OBS_WAVE": "1"}, seed, **kw)
    xs = _make(monkeypatch, n, {"FWSIM_OBS_WAVE": "0"}, seed, **kw)
    x = _make(monkeypatch, n, {"FWSIM_OBS_WAVE": "1", "FWSIM_STEP_SHAPE": "0"}, seed, **kw)     # (the shape switch wins)
    assert _sel(new) == (1, 1, 1) and _sel(xs) == (0, 1, 1) and _sel(x) == (0, 0, 1)
    assert new.obs_wave and not xs.obs_wave and not x.obs_wave
    return new, xs, x


def _same_outputs(new, old, tag):
    n = new.num_envs
    for name in OUTPUTS:
        x, y = getattr(new, name).cpu().numpy(), getattr(old, name).cpu().numpy()
        assert np.array_equal(x, y), f"{name} differs at {tag}: rows {np.nonzero((x != y).reshape(n, -1).any(1))[0][:8]}"


def _step_all(envs, a, t):
    a = torch.as_tensor(a, device=envs[0].device)
    for e in envs:
        e.step_tensor(a)
    for k, old in enumerate(envs[1:]):
        _same_outputs(envs[0], old, f"step {t}, twin {k}")


def _same_at_the_end(envs):
    s, c = envs[0].get_state(), envs[0].get_counters()
    for old in envs[1:]:
        assert np.array_equal(s, old.get_state())
        assert c == old.get_counters(), (c, old.get_counters())
    return c


def _reset_all(envs):
    o = envs[0].reset_tensor().cpu().numpy()
    for old in envs[1:]:
        assert np.array_equal(o, old.reset_tensor().cpu().numpy())


_FACTS = {}


def _trace_facts(oracle, n, steps, **kw):
    """On the CPU oracle under the seeded actions: the lengths of the episodes that end within the trace, the number of (step, tile)
    pairs in which an env ends beside one that flies on (all tiles / the ragged tile), and the number with a done-at-entry env
    beside a stepping one.  Computed once per (config, size) and shared."""
    key = (n, steps, tuple(sorted(kw.items())))
    if key not in _FACTS:
        ora = oracle.OracleEnv(_cfg(**kw), n, seed=SEED)
        ora.reset()
        rng = np.random.default_rng(5)
        born, at_entry = np.zeros(n, dtype=int), np.zeros(n, dtype=bool)
        lengths, mixed, mixed_ragged, mixed_entry = [], 0, 0, 0
        for t in range(steps):
            out = ora.step(seeded_actions(rng, n))
            done = (out[2] | out[3]).astype(bool)
            for i in np.nonzero(done & ~at_entry)[0]:
                lengths.append(t + 1 - born[i]); born[i] = t + 1
            for first in range(0, n, 8):
                sl = slice(first, min(first + 8, n))
                ended = done[sl] & ~at_entry[sl]
                if ended.any() and (~done[sl]).any():
                    mixed += 1
                    mixed_ragged += int(sl.stop - sl.start < 8)
                mixed_entry += int(at_entry[sl].any() and (~at_entry[sl]).any())
            at_entry = done if not kw.get("auto_reset", True) else at_entry
        _FACTS[key] = dict(lengths=np.array(lengths), mixed=mixed, mixed_ragged=mixed_ragged, mixed_entry=mixed_entry)
    return _FACTS[key]


def _run(envs, n, steps):
    _reset_all(envs)
    rng = np.random.default_rng(5)
    dones = 0
    for t in range(steps):
        _step_all(envs, seeded_actions(rng, n), t)
        dones += int((envs[0].terminated | envs[0].truncated).sum())
    return dones, _same_at_the_end(envs)


def test_selection_one_field_at_a_time(monkeypatch):
    full = dict(FWSIM_OBS_WAVE="1")
    assert _sel(_make(monkeypatch, 4096, full)) == (1, 1, 1)
    assert _sel(_make(monkeypatch, 2048, full)) == (1, 1, 1)
    assert _sel(_make(monkeypatch, 8, full)) == (1, 1, 1)
    assert _sel(_make(monkeypatch, 4096, {})) == (1, 1, 1) and _sel(_make(monkeypatch, 2048, {})) == (1, 1, 1)      # on by default (profiles/r24_obs_wave_ab.txt)
    assert _sel(_make(monkeypatch, 4096, dict(FWSIM_OBS_WAVE="0"))) == (0, 1, 1)
    assert _sel(_make(monkeypatch, 4096, dict(FWSIM_OBS_WAVE="1", FWSIM_STEP_SHAPE="0"))) == (0, 0, 1)      # fw_step_kernel_g8x, as before
    assert _sel(_make(monkeypatch, 4096, dict(FWSIM_OBS_WAVE="1", FWSIM_AUX_WAVE="0"))) == (0, 0, 0)
    # above 4096 envs never, even where the noise-wave row is forced
    assert _sel(_make(monkeypatch, 8192, dict(FWSIM_OBS_WAVE="1", FWSIM_AUX_WAVE="1"))) == (0, 1, 1)
    for name, (kw, n) in OFF_ROW.items():
        assert _sel(_make(monkeypatch, n, full, **kw))[0] == 0, name


@pytest.mark.parametrize("n", SIZES)
def test_resets_beside_stepping_envs_take_the_worker_row(oracle, monkeypatch, n):
    f = _trace_facts(oracle, n, STEPS, **DOME)
    assert len(f["lengths"]) >= n and f["lengths"].min() >= 3, "an episode of the dome trace is too short to have its scenario"
    assert f["mixed"] > 0 and (n % 8 == 0 or f["mixed_ragged"] > 0), "no env ends beside a flying env of its tile"
    dones, c = _run(_trio(monkeypatch, n, **DOME), n, STEPS)
    assert dones == len(f["lengths"]) == c["resets"]
    assert c["scenario_hits"] == c["resets"] and c["fallbacks"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_back_to_back_resets_fall_back_beside_hits(oracle, monkeypatch, n):
    f = _trace_facts(oracle, n, STEPS, **SHORT)
    short, long_ = int((f["lengths"] <= 2).sum()), int((f["lengths"] >= 3).sum())
    assert short > 0 and long_ > 0, "the trace needs episodes of two steps beside longer ones"
    assert f["mixed"] > 0 and (n % 8 == 0 or f["mixed_ragged"] > 0)
    dones, c = _run(_trio(monkeypatch, n, **SHORT), n, STEPS)
    assert dones == len(f["lengths"]) == c["resets"]
    assert c["fallbacks"] >= short and c["scenario_hits"] > 0 and c["scenario_hits"] + c["fallbacks"] == c["resets"]


@pytest.mark.parametrize("kw", [DOME, SHORT], ids=["dome", "dome_reach12"])
@pytest.mark.parametrize("n", SIZES)
def test_every_reset_falls_back_without_the_worker(oracle, monkeypatch, n, kw):
    f = _trace_facts(oracle, n, STEPS, **kw)
    assert f["mixed"] > 0
    monkeypatch.setenv("FWSIM_NO_SHADOW", "1")
    dones, c = _run(_trio(monkeypatch, n, **kw), n, STEPS)
    assert dones == len(f["lengths"]) == c["resets"] == c["fallbacks"] and c["scenario_hits"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_stale_view_of_envs_done_at_entry(oracle, monkeypatch, n):
    f = _trace_facts(oracle, n, STALE_STEPS, auto_reset=False, **DOME)
    assert f["mixed_entry"] > 0, "no tile holds a done-at-entry env beside a stepping one"
    envs = _trio(monkeypatch, n, auto_reset=False, **DOME)
    _reset_all(envs)
    rng = np.random.default_rng(5)
    for t in range(STALE_STEPS):
        _step_all(envs, seeded_actions(rng, n), t)
        s = envs[0].get_state()
        for old in envs[1:]:
            assert np.array_equal(s, old.get_state()), f"state differs at step {t}"
    assert (envs[0].terminated | envs[0].truncated).cpu().numpy().astype(bool).all()
    assert _same_at_the_end(envs)["resets"] == 0


def test_directed_states(monkeypatch):
    """Stall on both sides, reverse flow, V = 0, the gimbal guard of the observation's Euler angles and both renormalisation paths
    of the quaternion: the 65 states of tests/directed_states.py over three agent steps."""
    n = D.NUM_ENVS
    envs = _trio(monkeypatch, n)
    _reset_all(envs)
    states = [e.get_state() for e in envs]
    names = [D.apply(s) for s in states]
    assert names[0] == names[1] == names[2] and set(names[0]) == set(D.BRANCHES)
    assert np.array_equal(states[0], states[1]) and np.array_equal(states[0], states[2])
    for e, s in zip(envs, states):
        e.set_state(s)
    for t in range(3):
        _step_all(envs, D.actions(n, seed=7 + t), t)
    assert np.isfinite(envs[0].obs.cpu().numpy()).all()
    _same_at_the_end(envs)


@pytest.mark.parametrize("n", SIZES)
def test_launch_numbering_eager_and_replayed(oracle, monkeypatch, n):
    """25 steps: 1 eager launch + 3 replays of a captured graph of 8 launches on one handle, 25 eager launches on another and on
    the twins.  Which resets take the worker's row depends on the launch indices alone; here the worker reads the counter of the step
    workgroup it belongs to, which the step wave advances behind barrier 2."""
    warm, graph_len, replays = 1, 8, 3
    rng = np.random.default_rng(5)
    acts = [seeded_actions(rng, n) for _ in range(warm + graph_len)]
    order = acts[:warm] + acts[warm:] * replays
    assert len(order) == 25
    ora = oracle.OracleEnv(_cfg(**SHORT), n, seed=SEED)
    ora.reset()
    born, lengths = np.zeros(n, dtype=int), []
    for t, a in enumerate(order):
        out = ora.step(a)
        for i in np.nonzero(out[2] | out[3])[0]:
            lengths.append(t + 1 - born[i]); born[i] = t + 1
    ends, lengths = len(lengths), np.array(lengths)
    assert (lengths <= 2).any() and (lengths >= 3).any(), "the trace needs resets that must fall back beside resets that can hit"
    eager, xs, x = _trio(monkeypatch, n, **SHORT)
    replayed = _make(monkeypatch, n, {"FWSIM_OBS_WAVE": "1"}, **SHORT)
    assert _sel(replayed) == (1, 1, 1)
    for e in (eager, xs, x, replayed):
        e.reset_tensor()
    dev = [torch.as_tensor(a, device=replayed.device) for a in acts]
    s = torch.cuda.Stream()                                    # (capture as bench.Stepper does: warm up on a side stream first)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for a in dev[:warm]:
            replayed.step_tensor(a)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for a in dev[warm:]:
            replayed.step_tensor(a)
    for t, a in enumerate(acts[:warm]):
        _step_all((eager, xs, x), a, t)
    for r in range(replays):
        g.replay()
        for j, a in enumerate(acts[warm:]):
            _step_all((eager, xs, x), a, warm + r * graph_len + j)
        torch.cuda.synchronize()
        _same_outputs(replayed, eager, f"replay {r}")
        assert np.array_equal(replayed.get_state(), eager.get_state()), r
    c = _same_at_the_end((replayed, eager, xs, x))
    assert c["launches"] == 25 and c["resets"] == ends
    assert c["scenario_hits"] > 0 and c["fallbacks"] > 0 and c["scenario_hits"] + c["fallbacks"] == c["resets"]


def test_two_handles_stepped_alternately(monkeypatch):
    """Each handle has its own launch counters, hand-off words and LDS: two of them interleaved on one stream."""
    n, steps = 11, 30
    a_envs = _trio(monkeypatch, n, seed=SEED, **SHORT)
    b_envs = _trio(monkeypatch, n, seed=SEED + 1, **DOME)
    _reset_all(a_envs); _reset_all(b_envs)
    rng_a, rng_b = np.random.default_rng(5), np.random.default_rng(6)
    for t in range(steps):
        _step_all(a_envs, seeded_actions(rng_a, n), t)
        if t % 3 != 2:                                          # (and not in lockstep: the launch indices of the two drift apart)
            _step_all(b_envs, seeded_actions(rng_b, n), t)
    assert _same_at_the_end(a_envs)["resets"] > 0
    assert _same_at_the_end(b_envs)["resets"] > 0


def test_seed_and_set_state_followed_by_steps(monkeypatch):
    n = 11
    envs = _trio(monkeypatch, n, **SHORT)
    dones, c = _run(envs, n, 10)
    assert c["resets"] > 0
    for e in envs:                                              # a new seed invalidates what the worker has sampled
        e.seed(SEED + 100)
    dones, c2 = _run(envs, n, 10)
    assert c2["resets"] > c["resets"]
    s = envs[0].get_state()
    for e in envs:                                              # ... and so does a state set from outside
        e.set_state(s[::-1].copy())
    rng = np.random.default_rng(9)
    for t in range(10):
        _step_all(envs, seeded_actions(rng, n), t)
    assert _same_at_the_end(envs)["resets"] > c2["resets"]


@pytest.mark.parametrize("shadow", [True, False], ids=["worker", "no_shadow"])
@pytest.mark.parametrize("kw", [DOME, SHORT], ids=["dome", "dome_reach12"])
@pytest.mark.parametrize("n", SIZES)
def test_dome_traces_track_the_oracle(oracle, monkeypatch, n, kw, shadow):
    f = _trace_facts(oracle, n, STEPS, **kw)
    short, long_ = int((f["lengths"] <= 2).sum()), int((f["lengths"] >= 3).sum())
    assert len(f["lengths"]) > 0 and f["mixed"] > 0, "the trace resets nobody beside a flying env of its tile"
    if shadow:          # with the worker: the dome trace is all hits, the 12 m reach adds resets that must fall back
        assert long_ > 0 and (short > 0) == (kw == SHORT)
    if not shadow:
        monkeypatch.setenv("FWSIM_NO_SHADOW", "1")
    env = _make(monkeypatch, n, {"FWSIM_OBS_WAVE": "1"}, **kw)
    assert _sel(env) == (1, 1, 1)
    worst = run_lockstep(env, oracle.OracleEnv(_cfg(**kw), n, seed=SEED), STEPS, np.random.default_rng(5), atol=1e-7)
    assert worst["dones"] == len(f["lengths"]) > 0
