"""The fixed-shape step kernel (fw_step_kernel_g8xs) with the agent step as a counted loop: step_ratio sub-steps over one per-lane
`stepping` bit instead of the phase machine of the run-time shapes, one wave-uniform exit test per sub-step, and the end-of-step
latch (step_count, ep_return, the stores of reward / terminated / truncated / info, the auto-reset decision) once, behind the
loop, for every env of the wave at once.

Twins as in tests/test_step_unroll_gpu.py: the same config, seed and actions on a second handle created under FWSIM_STEP_SHAPE=0,
which runs the phase machine (fw_step_kernel_g8x).  All six outputs must be equal after every step, state and counters at the end.
Sizes: 8 envs = one full tile, 11 = a ragged second tile with five inactive rows, 64 = 8 tiles (the XCD block map is active).

What each trace covers was chosen on the CPU oracle alone and is asserted there, before a handle is created:
  * 14 m dome, seed 7, uniform actions of default_rng(5): envs finish after sub-step 0, 1, 2 AND 3 of a step (tick advances 2, 4, 6
    and a full 8 with the env done) beside envs of the same tile that step on, at 11 envs in the ragged tile as well; tiles hold envs
    that are done at entry beside stepping ones (without auto-reset the done ones keep the stale view and their outputs); behind step
    15 every env is done at entry, so every wave leaves at the exit test of sub-step 0;
  * max_steps: step_count is compared in every sub-step and incremented by the latch alone, so the limit strikes in the FIRST
    sub-step of the step that is entered with step_count = max_steps + 1 (tick advance 2), and the step before it -- entered with
    step_count = max_steps -- runs all four sub-steps untruncated: a latch that ran ahead of a sub-step would end it a step early.
    (A limit that falls in a later sub-step cannot be made with max_steps: step_count does not change within a step.)
  * goal_reach_distance 62 m: num_reached advances in every sub-step of a step (by 4), and the last waypoint is reached in the
    middle of a step (tick advance 4: FL_TRUNC | FL_COMPLETE from sub-step 1); 80 m with auto-reset: completions and resets in
    nearly every step.
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
DOME = dict(flight_dome_size=14.0)
MID_STEPS, STALE_STEPS = 15, 10          # every env of the oracle's dome trace is done within 15 steps; then ten steps done at entry
TICKS_PER_STEP = 8                       # step_ratio 4 x 2 ticks per Aviary step
LIMIT = dict(max_duration_seconds=0.2)
REACH_MID, REACH_BUSY = 62.0, 80.0
WP_STEPS = 8
INFO_REACHED, INFO_COMPLETE = 0, 3


def _cfg(**kw):
    return K.train_waypoints_v3_config(**kw)


def _shape(env):
    return int(_lib.lib().fw_step_shape(env._h))


def _twins(monkeypatch, n, **kw):
    """(fixed-shape handle, run-time-shape handle) of the same config and seed"""
    monkeypatch.delenv("FWSIM_STEP_SHAPE", raising=False)
    new = P.FixedwingVecEnv(_cfg(**kw), n, device=0, seed=SEED)
    monkeypatch.setenv("FWSIM_STEP_SHAPE", "0")
    old = P.FixedwingVecEnv(_cfg(**kw), n, device=0, seed=SEED)
    monkeypatch.delenv("FWSIM_STEP_SHAPE")
    assert _shape(new) == 1 and _shape(old) == 0
    return new, old


def _same_outputs(new, old, tag):
    n = new.num_envs
    for name in OUTPUTS:
        x, y = getattr(new, name).cpu().numpy(), getattr(old, name).cpu().numpy()
        assert np.array_equal(x, y), f"{name} differs at {tag}: rows {np.nonzero((x != y).reshape(n, -1).any(1))[0][:8]}"


def _step_both(new, old, a, t, state=False):
    a = torch.as_tensor(a, device=new.device)
    new.step_tensor(a); old.step_tensor(a)
    _same_outputs(new, old, f"step {t}")
    if state:
        assert np.array_equal(new.get_state(), old.get_state()), f"state differs at step {t}"


def _same_at_the_end(new, old):
    assert np.array_equal(new.get_state(), old.get_state())
    assert new.get_counters() == old.get_counters()


def _reset_both(new, old):
    assert np.array_equal(new.reset_tensor().cpu().numpy(), old.reset_tensor().cpu().numpy())


_TRACES = {}


def _oracle_trace(oracle, n, steps, **kw):
    """Per step of the CPU oracle under the seeded actions: tick advance, done at entry, done, truncated, info, step_count at
    entry.  Computed once per (config, size) and shared."""
    key = (n, steps, tuple(sorted(kw.items())))
    if key not in _TRACES:
        ora = oracle.OracleEnv(_cfg(**kw), n, seed=SEED)
        ora.reset()
        rng = np.random.default_rng(5)
        s = ora.get_state()
        tick, done = s[:, K.S_TICK_COUNT].copy(), np.zeros(n, dtype=bool)
        rows = []
        for _ in range(steps):
            entry_count = ora.get_state()[:, K.S_STEP_COUNT].astype(int)
            out = ora.step(seeded_actions(rng, n))
            now = ora.get_state()[:, K.S_TICK_COUNT]
            d = (out[2] | out[3]).astype(bool)
            rows.append(dict(adv=(now - tick).astype(int), at_entry=done.copy(), done=d, trunc=out[3].astype(bool), info=out[5].astype(int),
                             entry_count=entry_count))
            tick, done = now.copy(), d
        _TRACES[key] = rows
    return _TRACES[key]


def _dome_trace_facts(oracle, n):
    """What the dome trace without auto-reset holds, on the oracle: {sub-step after which an env finished beside a stepping env of
    its tile}, the same for the ragged tile alone, and the number of (step, tile) pairs with done-at-entry envs beside stepping ones."""
    rows = _oracle_trace(oracle, n, MID_STEPS + STALE_STEPS, auto_reset=False, **DOME)
    finished, finished_ragged, mixed_entry = set(), set(), 0
    for r in rows:
        for first in range(0, n, 8):
            sl = slice(first, min(first + 8, n))
            adv, at_entry, done = r["adv"][sl], r["at_entry"][sl], r["done"][sl]
            assert ((adv >= 0) & (adv <= TICKS_PER_STEP) & (adv % 2 == 0)).all() and (adv[at_entry] == 0).all()
            ended = done & ~at_entry
            for a in adv[ended]:
                if (adv > a).any() or (a == TICKS_PER_STEP and (~done).any()):      # somebody of the tile ran a later sub-step
                    finished.add(a // 2 - 1)
                    if sl.stop - sl.start < 8:
                        finished_ragged.add(a // 2 - 1)
            mixed_entry += int(at_entry.any() and (adv > 0).any())
    assert all(r["at_entry"].all() for r in rows[MID_STEPS:]), "an env of the trace is still flying behind step 15"
    return finished, finished_ragged, mixed_entry


@pytest.mark.parametrize("n", SIZES)
def test_envs_finish_after_every_sub_step_without_auto_reset(oracle, monkeypatch, n):
    """Cases 1 and 2: finishes after sub-steps 0 to 3 beside stepping envs; done-at-entry envs beside stepping ones keep the stale
    observation, their outputs and their step_count (the state is compared after every step); then ten steps with every wave
    leaving at the exit test of sub-step 0."""
    finished, finished_ragged, mixed_entry = _dome_trace_facts(oracle, n)
    if n % 8:
        assert finished_ragged, "no env of the ragged tile finished beside a stepping one"
    assert finished == {0, 1, 2, 3}, f"the trace ends agent steps after sub-steps {sorted(finished)} only"
    assert mixed_entry > 0, "no tile held a done-at-entry env beside a stepping one"
    new, old = _twins(monkeypatch, n, auto_reset=False, **DOME)
    _reset_both(new, old)
    rng = np.random.default_rng(5)
    rows = _oracle_trace(oracle, n, MID_STEPS + STALE_STEPS, auto_reset=False, **DOME)
    tick = new.get_state()[:, K.S_TICK_COUNT].copy()
    for t in range(MID_STEPS + STALE_STEPS):
        _step_both(new, old, seeded_actions(rng, n), t, state=True)
        s = new.get_state()
        assert np.array_equal((s[:, K.S_TICK_COUNT] - tick).astype(int), rows[t]["adv"]), f"tick advance differs from the oracle's at step {t}"
        assert np.array_equal(s[:, K.S_STEP_COUNT].astype(int), rows[t]["entry_count"] + 1), t       # the latch counts every env, done at entry or not
        tick = s[:, K.S_TICK_COUNT].copy()
    assert (new.terminated | new.truncated).cpu().numpy().astype(bool).all()
    _same_at_the_end(new, old)
    assert new.get_counters()["resets"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_envs_finish_after_every_sub_step_with_auto_reset(monkeypatch, n):
    new, old = _twins(monkeypatch, n, **DOME)
    _reset_both(new, old)
    rng = np.random.default_rng(5)
    dones = 0
    for t in range(MID_STEPS + STALE_STEPS):
        _step_both(new, old, seeded_actions(rng, n), t)
        dones += int((new.terminated | new.truncated).sum())
    assert dones >= n
    _same_at_the_end(new, old)
    assert new.get_counters()["resets"] > 0


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_dome_traces_track_the_oracle(oracle, monkeypatch, n, auto_reset):
    monkeypatch.delenv("FWSIM_STEP_SHAPE", raising=False)
    cfg = _cfg(auto_reset=auto_reset, **DOME)
    env = P.FixedwingVecEnv(cfg, n, device=0, seed=SEED)
    assert _shape(env) == 1
    worst = run_lockstep(env, oracle.OracleEnv(cfg, n, seed=SEED), MID_STEPS + STALE_STEPS, np.random.default_rng(5), atol=1e-7)
    assert worst["dones"] >= n


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_truncation_by_max_steps(oracle, monkeypatch, n, auto_reset):
    """Case 3.  On the oracle: max_steps of the config is small, the step entered with step_count = max_steps runs its four sub-steps
    untruncated, the next one is truncated in its first sub-step."""
    max_steps = int(round(LIMIT["max_duration_seconds"] * _cfg().agent_hz))
    steps = max_steps + 5
    rows = _oracle_trace(oracle, n, steps, auto_reset=False, **LIMIT)
    first = next(t for t, r in enumerate(rows) if r["trunc"].any())
    assert first == max_steps + 1 and rows[first]["trunc"].all() and (rows[first]["adv"] == 2).all()
    assert (rows[first]["entry_count"] == max_steps + 1).all()
    before = rows[first - 1]
    assert (before["entry_count"] == max_steps).all() and not before["done"].any() and (before["adv"] == TICKS_PER_STEP).all()
    new, old = _twins(monkeypatch, n, auto_reset=auto_reset, **LIMIT)
    _reset_both(new, old)
    rng = np.random.default_rng(5)
    for t in range(steps):
        _step_both(new, old, seeded_actions(rng, n), t, state=True)
        trunc = new.truncated.cpu().numpy().astype(bool)
        if t <= first:
            assert np.array_equal(trunc, rows[t]["trunc"]), f"truncation differs from the oracle's at step {t}"
    _same_at_the_end(new, old)
    assert (new.get_counters()["resets"] > 0) == auto_reset


@pytest.mark.parametrize("n", SIZES)
def test_waypoints_reached_in_the_middle_of_a_step(oracle, monkeypatch, n):
    """Case 4.  On the oracle (no auto-reset, so that the tick advance of the completing step stays visible): num_reached advances
    by four in one step -- in sub-steps 0 to 2 among them -- and an env reaches its last waypoint after sub-step 1."""
    rows = _oracle_trace(oracle, n, WP_STEPS, auto_reset=False, goal_reach_distance=REACH_MID)
    reached = np.zeros(n, dtype=int)
    jump, mid_complete = 0, 0
    for r in rows:
        now = r["info"][:, INFO_REACHED]
        jump = max(jump, int((now - reached).max()))
        complete = r["info"][:, INFO_COMPLETE].astype(bool) & ~r["at_entry"]
        assert r["trunc"][complete].all()
        mid_complete += int((complete & (r["adv"] < TICKS_PER_STEP)).sum())
        reached = now
    assert jump == 4, "no env reached a waypoint in every sub-step of a step"
    assert mid_complete > 0, "no env reached its last waypoint in the middle of a step"
    new, old = _twins(monkeypatch, n, auto_reset=False, goal_reach_distance=REACH_MID)
    _reset_both(new, old)
    rng = np.random.default_rng(5)
    for t in range(WP_STEPS):
        _step_both(new, old, seeded_actions(rng, n), t, state=True)
        assert np.array_equal(new.info.cpu().numpy().astype(int), rows[t]["info"]), f"info differs from the oracle's at step {t}"
    _same_at_the_end(new, old)


@pytest.mark.parametrize("n", SIZES)
def test_waypoint_completions_with_auto_reset(monkeypatch, n):
    new, old = _twins(monkeypatch, n, goal_reach_distance=REACH_BUSY)
    _reset_both(new, old)
    rng = np.random.default_rng(5)
    complete = 0
    for t in range(12):
        _step_both(new, old, seeded_actions(rng, n), t)
        complete += int(new.info.cpu().numpy()[:, INFO_COMPLETE].sum())
    assert complete >= n
    _same_at_the_end(new, old)
    assert new.get_counters()["resets"] >= n


@pytest.mark.parametrize("reach,auto_reset,steps", [(REACH_MID, False, WP_STEPS), (REACH_BUSY, True, 12)])
@pytest.mark.parametrize("n", SIZES)
def test_waypoint_traces_track_the_oracle(oracle, monkeypatch, n, reach, auto_reset, steps):
    monkeypatch.delenv("FWSIM_STEP_SHAPE", raising=False)
    cfg = _cfg(goal_reach_distance=reach, auto_reset=auto_reset)
    env = P.FixedwingVecEnv(cfg, n, device=0, seed=SEED)
    assert _shape(env) == 1
    worst = run_lockstep(env, oracle.OracleEnv(cfg, n, seed=SEED), steps, np.random.default_rng(5), atol=1e-7, rtol=0)
    assert worst["dones"] > 0


def test_directed_states_twins(monkeypatch):
    """Case 5: stall on both sides, reverse flow, V = 0, the clamp and both renormalisation paths of the quaternion -- the 65
    states of tests/directed_states.py over three agent steps."""
    n = D.NUM_ENVS
    new, old = _twins(monkeypatch, n)
    _reset_both(new, old)
    sn, so = new.get_state(), old.get_state()
    names = D.apply(sn)
    assert D.apply(so) == names and set(names) == set(D.BRANCHES)
    assert np.array_equal(sn, so)
    new.set_state(sn); old.set_state(so)
    for t in range(3):
        _step_both(new, old, D.actions(n, seed=7 + t), t)
    assert np.isfinite(new.obs.cpu().numpy()).all()
    _same_at_the_end(new, old)


@pytest.mark.parametrize("n", SIZES)
def test_launch_numbering_eager_and_replayed(oracle, monkeypatch, n):
    """Case 6: 25 steps on the 14 m dome -- 1 eager launch + 3 replays of a captured graph of 8 launches on one handle, 25 eager
    launches on another and on the run-time-shape twin.  Which resets take the scenario hand-off depends on the launch indices
    alone, and the kernel must reach launch_done on every path of the counted loop."""
    warm, graph_len, replays = 1, 8, 3
    rng = np.random.default_rng(5)
    acts = [seeded_actions(rng, n) for _ in range(warm + graph_len)]
    order = acts[:warm] + acts[warm:] * replays
    assert len(order) == 25
    ora = oracle.OracleEnv(_cfg(**DOME), n, seed=SEED)
    ora.reset()
    ends = 0
    for a in order:
        out = ora.step(a)
        ends += int((out[2] | out[3]).sum())
    assert ends > 0, "the trace resets nobody within 25 steps"
    eager, old = _twins(monkeypatch, n, **DOME)
    replayed = P.FixedwingVecEnv(_cfg(**DOME), n, device=0, seed=SEED)
    assert _shape(replayed) == 1
    for e in (eager, old, replayed):
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
        _step_both(eager, old, a, t)
    for r in range(replays):
        g.replay()
        for j, a in enumerate(acts[warm:]):
            _step_both(eager, old, a, warm + r * graph_len + j)
        torch.cuda.synchronize()
        _same_outputs(replayed, eager, f"replay {r}")
        assert np.array_equal(replayed.get_state(), eager.get_state()), r
    c = replayed.get_counters()
    assert c == eager.get_counters() == old.get_counters(), (c, eager.get_counters(), old.get_counters())
    assert c["launches"] == 25 and c["resets"] == ends
    assert c["scenario_hits"] + c["fallbacks"] == c["resets"]
