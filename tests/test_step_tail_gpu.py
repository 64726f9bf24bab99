"""The end of a launch of fw_step_kernel_g8xo (fwsim.hip: step_body OBSW; fwsim_device.hpp: flush_obs_tile_fixed).  The observation wave
flushes its tile in one trip: each lane's at most four words (e = lane + 64 j, row = e / 28) and their rows' mode words are read
unconditionally, the wave waits once, and the stores are predicated on e < rows * 28 and mode != 2.  Only the order in which the same
words are read and stored changed, so every output must be bit-identical to the twins': the same config, seed and actions on a handle
created under FWSIM_OBS_WAVE=0 (fw_step_kernel_g8xs) and on one created under FWSIM_STEP_SHAPE=0 (fw_step_kernel_g8x).  All six
outputs are compared after every step, state and counters at the end.

Sizes, the smallest at which the new flush can go wrong: 1 env (28 words: every j > 0 is out of range), 3 (84
words: the second word of 20 lanes is in range, of 44 out), 8 (a full tile), 9 and 11 (a second tile of one row and of three), 64
(8 tiles, the XCD block map).

What each trace covers is computed on the CPU oracle alone and asserted there before a handle exists (tests/test_obs_wave_gpu.py
says why an episode of two steps must fall back and one of three or more takes the worker's row):
  * 14 m dome with 12 m reach: rows of mode 0 (no reset), 1 (the worker's row) and 2 (the step wave's own row, which the flush
    must skip) -- from 3 envs on, all three in one tile in one launch;
  * the 14 m dome alone: every reset is mode 1;  FWSIM_NO_SHADOW=1: every reset is mode 2;
  * auto_reset off: envs done at entry beside stepping ones;
  * a handle stepped without `terminal_obs` and `info` buffers (the kernel takes null for both): the observation wave copies no terminal row out;
  * 1 eager launch + 3 replays of a captured graph of 8 launches against 25 eager launches.
"""
import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from helpers import seeded_actions

pytestmark = pytest.mark.gpu

SEED = 7
OUTPUTS = ("obs", "rewards", "terminated", "truncated", "terminal_obs", "info")
SIZES = (1, 3, 8, 9, 11, 64)
STEPS = 40
STALE_STEPS = 25
DOME = dict(flight_dome_size=14.0)
SHORT = dict(flight_dome_size=14.0, goal_reach_distance=12.0)
TILE = 8


def _cfg(**kw):
    return K.train_waypoints_v3_config(**kw)


def _sel(env):
    L = _lib.lib()
    return int(L.fw_obs_wave(env._h)), int(L.fw_step_shape(env._h)), int(L.fw_aux_wave(env._h))


def _make(monkeypatch, n, env_vars, **kw):
    for name in ("FWSIM_OBS_WAVE", "FWSIM_STEP_SHAPE", "FWSIM_AUX_WAVE"):
        monkeypatch.delenv(name, raising=False)
    for name, v in env_vars.items():
        monkeypatch.setenv(name, v)
    env = P.FixedwingVecEnv(_cfg(**kw), n, device=0, seed=SEED)
    for name in env_vars:
        monkeypatch.delenv(name)
    return env


def _trio(monkeypatch, n, **kw):
    """(handle on fw_step_kernel_g8xo, its twin on fw_step_kernel_g8xs, its twin on fw_step_kernel_g8x)"""
    new = _make(monkeypatch, n, {"FWSIM_OBS_WAVE": "1"}, **kw)
    xs = _make(monkeypatch, n, {"FWSIM_OBS_WAVE": "0"}, **kw)
    x = _make(monkeypatch, n, {"FWSIM_OBS_WAVE": "1", "FWSIM_STEP_SHAPE": "0"}, **kw)
    assert _sel(new) == (1, 1, 1) and _sel(xs) == (0, 1, 1) and _sel(x) == (0, 0, 1)
    return new, xs, x


def _same_outputs(new, old, tag, names=OUTPUTS):
    n = new.num_envs
    for name in names:
        x, y = getattr(new, name).cpu().numpy(), getattr(old, name).cpu().numpy()
        assert np.array_equal(x, y), f"{name} differs at {tag}: rows {np.nonzero((x != y).reshape(n, -1).any(1))[0][:8]}"


def _step_all(envs, a, t, names=OUTPUTS):
    a = torch.as_tensor(a, device=envs[0].device)
    for e in envs:
        e.step_tensor(a)
    for k, old in enumerate(envs[1:]):
        _same_outputs(envs[0], old, f"step {t}, twin {k}", names)


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


def _trace_facts(oracle, n, actions, **kw):
    """On the CPU oracle under `actions` (one array per step): the lengths of the episodes that end, and the number of (step, tile)
    pairs that hold an env flying on (mode 0) beside one ending an episode of three steps or more (mode 1) / beside one ending an
    episode of one or two (mode 2) / all three; and the number with a done-at-entry env beside a stepping one.  Computed once per
    (config, size, trace length) -- the action sequences of this file are functions of the size and the length -- and shared."""
    key = (n, len(actions), tuple(sorted(kw.items())))
    if key not in _FACTS:
        ora = oracle.OracleEnv(_cfg(**kw), n, seed=SEED)
        ora.reset()
        born, at_entry = np.zeros(n, dtype=int), np.zeros(n, dtype=bool)
        f = dict(lengths=[], with_1=0, with_2=0, all_three=0, mixed_entry=0)
        for t, a in enumerate(actions):
            out = ora.step(a)
            done = (out[2] | out[3]).astype(bool)
            mode = np.zeros(n, dtype=int)
            for i in np.nonzero(done & ~at_entry)[0]:
                length = t + 1 - born[i]
                f["lengths"].append(length); born[i] = t + 1
                mode[i] = 1 if length >= 3 else 2
            for first in range(0, n, TILE):
                m, e = mode[first:first + TILE], at_entry[first:first + TILE]
                has = [(m == k).any() for k in range(3)]
                f["with_1"] += int(has[0] and has[1]); f["with_2"] += int(has[0] and has[2]); f["all_three"] += int(all(has))
                f["mixed_entry"] += int(e.any() and (~e).any())
            at_entry = done if not kw.get("auto_reset", True) else at_entry
        f["lengths"] = np.array(f["lengths"])
        _FACTS[key] = f
    return _FACTS[key]


def _actions(n, steps):
    rng = np.random.default_rng(5)
    return [seeded_actions(rng, n) for _ in range(steps)]


def _run(envs, actions, names=OUTPUTS):
    _reset_all(envs)
    dones = 0
    for t, a in enumerate(actions):
        _step_all(envs, a, t, names)
        dones += int((envs[0].terminated | envs[0].truncated).sum())
    return dones, _same_at_the_end(envs)


@pytest.mark.parametrize("n", SIZES)
def test_three_modes_in_one_tile(oracle, monkeypatch, n):
    acts = _actions(n, STEPS)
    f = _trace_facts(oracle, n, acts, **SHORT)
    short, long_ = int((f["lengths"] <= 2).sum()), int((f["lengths"] >= 3).sum())
    assert short > 0 and long_ > 0, "the trace needs resets that must fall back and resets that can take the worker's row"
    if n > 1:
        assert f["all_three"] > 0, "no tile holds a flying env, a worker's row and a fallback row in one launch"
        assert f["with_2"] > 0, "no skipped (mode 2) row lies beside a flushed one"
    dones, c = _run(_trio(monkeypatch, n, **SHORT), acts)
    assert dones == len(f["lengths"]) == c["resets"]
    assert c["fallbacks"] >= short and c["scenario_hits"] > 0 and c["scenario_hits"] + c["fallbacks"] == c["resets"]


@pytest.mark.parametrize("n", SIZES)
def test_every_reset_takes_the_worker_row(oracle, monkeypatch, n):
    acts = _actions(n, STEPS)
    f = _trace_facts(oracle, n, acts, **DOME)
    assert len(f["lengths"]) >= n and f["lengths"].min() >= 3, "an episode of the dome trace is too short to have its scenario"
    assert n == 1 or f["with_1"] > 0, "no env ends beside a flying env of its tile"
    dones, c = _run(_trio(monkeypatch, n, **DOME), acts)
    assert dones == len(f["lengths"]) == c["resets"] == c["scenario_hits"] and c["fallbacks"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_every_reset_falls_back_without_the_worker(oracle, monkeypatch, n):
    acts = _actions(n, STEPS)
    f = _trace_facts(oracle, n, acts, **SHORT)
    assert len(f["lengths"]) > 0 and (n == 1 or f["with_1"] + f["with_2"] > 0)
    monkeypatch.setenv("FWSIM_NO_SHADOW", "1")
    dones, c = _run(_trio(monkeypatch, n, **SHORT), acts)
    assert dones == len(f["lengths"]) == c["resets"] == c["fallbacks"] and c["scenario_hits"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_envs_done_at_entry_beside_stepping_ones(oracle, monkeypatch, n):
    acts = _actions(n, STALE_STEPS)
    f = _trace_facts(oracle, n, acts, auto_reset=False, **DOME)
    assert n < TILE or f["mixed_entry"] > 0, "no tile holds a done-at-entry env beside a stepping one"      # (1 and 3 envs: all end in one step)
    assert len(f["lengths"]) == n, "every env ends within the trace and is stepped on, done at entry"
    envs = _trio(monkeypatch, n, auto_reset=False, **DOME)
    _reset_all(envs)
    for t, a in enumerate(acts):
        _step_all(envs, a, t)
        s = envs[0].get_state()
        for old in envs[1:]:
            assert np.array_equal(s, old.get_state()), f"state differs at step {t}"
    assert (envs[0].terminated | envs[0].truncated).cpu().numpy().astype(bool).all()
    assert _same_at_the_end(envs)["resets"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_without_terminal_obs_and_info_buffers(oracle, monkeypatch, n):
    """fw_step takes null for `terminal_obs` and `info`: the step wave then stores two outputs fewer and the observation wave copies no
    terminal row out in front of its flush.  The other four outputs, state and counters are those of the full call."""
    acts = _actions(n, STEPS)
    f = _trace_facts(oracle, n, acts, **SHORT)
    assert (f["lengths"] <= 2).any() and (f["lengths"] >= 3).any()
    full = _make(monkeypatch, n, {"FWSIM_OBS_WAVE": "1"}, **SHORT)
    bare = _make(monkeypatch, n, {"FWSIM_OBS_WAVE": "1"}, **SHORT)
    xs = _make(monkeypatch, n, {"FWSIM_OBS_WAVE": "0"}, **SHORT)
    assert _sel(full) == _sel(bare) == (1, 1, 1) and _sel(xs) == (0, 1, 1)
    for e in (bare, xs):
        e.terminal_obs = None; e.info = None
    dones, c = _run((full, bare, xs), acts, names=("obs", "rewards", "terminated", "truncated"))
    assert dones == len(f["lengths"]) == c["resets"] and c["scenario_hits"] > 0 and c["fallbacks"] > 0


@pytest.mark.parametrize("n", SIZES)
def test_eager_and_replayed_launches(oracle, monkeypatch, n):
    warm, graph_len, replays = 1, 8, 3
    acts = _actions(n, warm + graph_len)
    order = acts[:warm] + acts[warm:] * replays
    assert len(order) == 25
    f = _trace_facts(oracle, n, order, **SHORT)
    assert (f["lengths"] <= 2).any() and (f["lengths"] >= 3).any(), "the trace needs resets that must fall back beside resets that can hit"
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
    _same_outputs(replayed, eager, "the last step")
    c = _same_at_the_end((replayed, eager, xs, x))
    assert c["launches"] == 25 and c["resets"] == len(f["lengths"])
    assert c["scenario_hits"] > 0 and c["fallbacks"] > 0 and c["scenario_hits"] + c["fallbacks"] == c["resets"]
