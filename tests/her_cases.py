"""Shared pieces of the hindsight-relabelling tests (tests/test_sac_her_cpu.py, tests/test_sac_her_gpu.py): a scripted run of 4
low-level-task envs (rows of 50 floats: 21 observations, 6 actions) over 16 vec-steps with hand-placed episode ends, its per-env
trajectory lists, a check of relabelled rows against those lists that knows nothing of ring arithmetic, and the kernel's two Philox
draws restated in numpy."""
import numpy as np

import device_reference as R

N_ENVS, D, A, ROW = 4, 21, 6, 50
STEPS, RING_STEPS, HALF = 16, 10, 5          # the ring holds 10 vec-steps: 16 stores wrap it; 5 stores leave it half full
HORIZONS = (1, 2, 5, 64)
RCOL, NOBS = D + A, D + A + 1                # the reward column; where next_obs starts
SAMPLE_TAG = 0x5AC0C000                      # kSacTagSample (csrc/fwsim_sac.hpp)
# (vec-step, env): (terminated, truncated).  Steps 0-4 are what the half-full ring holds, steps 6-15 what the wrapped one holds.  Both
# windows hold ends of both kinds and an end in their newest step (4 and 15); the episodes are 2 to 10 rows long, and env 3 of the half
# window flies through all of it.
ENDS = {(1, 0): (1, 0), (2, 2): (0, 1), (4, 1): (1, 0),
        (7, 3): (1, 1), (8, 3): (0, 1), (10, 0): (1, 0), (12, 1): (0, 1), (15, 2): (1, 0)}
DOME, MIN_SPEED = 250.0, 14.0                # the variant-1 settings of the scripted rows: both penalties occur among them


def _obs(rng, goal):
    """A row of the low-level task's observation with values of the task's size: attitude beyond the 35 / 20 degree bounds in some rows,
    positions beyond DOME in some, airspeeds on both sides of MIN_SPEED."""
    o = np.empty((N_ENVS, D), dtype=np.float32)
    o[:, 0:3] = rng.standard_normal((N_ENVS, 3))
    o[:, 3:5] = 0.6 * rng.standard_normal((N_ENVS, 2))
    o[:, 5] = rng.uniform(-np.pi, np.pi, N_ENVS)
    o[:, 6:9] = np.array([18.0, 0.0, 0.0]) + 6.0 * rng.standard_normal((N_ENVS, 3))
    o[:, 9:11] = 200.0 * rng.standard_normal((N_ENVS, 2))
    o[:, 11] = rng.uniform(2.0, 98.0, N_ENVS)
    o[:, 12:18] = rng.uniform(-1, 1, (N_ENVS, 6))
    o[:, 18:21] = goal
    return o


def _goal(rng):
    return np.stack([rng.uniform(-np.pi, np.pi, N_ENVS), rng.uniform(10.0, 90.0, N_ENVS), rng.uniform(15.0, 30.0, N_ENVS)], axis=1).astype(np.float32)


def script(seed=0):
    """STEPS store() argument tuples (obs, act, rew, next_obs, terminal_obs, terminated, truncated) of float32 / uint8 arrays.  Inside
    an episode a step's next_obs is the next step's obs and the goal columns stay; at an end the env hands over the terminal observation
    (the old goal) and next_obs is the first observation of the new episode, with a new goal."""
    rng = np.random.default_rng(seed)
    goal = _goal(rng)
    obs, out = _obs(rng, goal), []
    for t in range(STEPS):
        term, trunc = np.zeros(N_ENVS, dtype=np.uint8), np.zeros(N_ENVS, dtype=np.uint8)
        for (tt, e), (a, b) in ENDS.items():
            if tt == t:
                term[e], trunc[e] = a, b
        tobs = _obs(rng, goal)
        ended = (term | trunc) != 0
        goal = np.where(ended[:, None], _goal(rng), goal)
        nxt = _obs(rng, goal)
        nxt[~ended] = tobs[~ended]           # (tobs is only read where the episode ended)
        out.append((obs, rng.uniform(-1, 1, (N_ENVS, A)).astype(np.float32), (10.0 * rng.standard_normal(N_ENVS)).astype(np.float32),
                    nxt, tobs, term, trunc))
        obs = nxt
    return out


def numpy_ends(stores):
    """The `ends` side ring after these stores, by the rule 'the byte of the row the store writes'."""
    ends, cursor = np.zeros(RING_STEPS * N_ENVS, dtype=np.uint8), 0
    for s in stores:
        ends[cursor:cursor + N_ENVS] = (s[5] != 0) * 1 + (s[6] != 0) * 2
        cursor = (cursor + N_ENVS) % len(ends)
    return ends


def numpy_ring(stores):
    """(ring [capacity, 50] float32, cursor, size) after these stores: fw_replay_store's rows in plain numpy."""
    cap = RING_STEPS * N_ENVS
    ring, cursor, size = np.zeros((cap, ROW), dtype=np.float32), 0, 0
    for obs, act, rew, nxt, tobs, term, trunc in stores:
        ended = (term | trunc) != 0
        rows = np.concatenate([obs, act, rew[:, None], np.where(ended[:, None], tobs, nxt), (term != 0).astype(np.float32)[:, None]], axis=1)
        ring[cursor:cursor + N_ENVS] = rows
        cursor = (cursor + N_ENVS) % cap
        size = min(size + N_ENVS, cap)
    return ring, cursor, size


def trajectories(stores):
    """Per env, the list of its transitions in time order, of the steps a ring of RING_STEPS vec-steps still holds; `episode` numbers
    the env's episodes."""
    first = max(0, len(stores) - RING_STEPS)
    traj, episode = [[] for _ in range(N_ENVS)], [0] * N_ENVS
    for t, s in enumerate(stores):
        obs, act, rew, nxt, tobs, term, trunc = s
        for e in range(N_ENVS):
            ended = bool(term[e] or trunc[e])
            if t >= first:
                traj[e].append(dict(obs=obs[e], act=act[e], rew=rew[e], next=(tobs if ended else nxt)[e], done=float(term[e] != 0),
                                    ended=ended, episode=episode[e]))
            episode[e] += ended
    return traj


def find(traj, row):
    """(env, position in its list) of the transition a (possibly relabelled) row started from: obs[0:18] and the action identify it."""
    hits = [(e, t) for e in range(N_ENVS) for t, s in enumerate(traj[e])
            if np.array_equal(s["obs"][:18], row[:18]) and np.array_equal(s["act"], row[D:D + A])]
    assert len(hits) == 1
    return hits[0]


def candidates(traj, e, t, horizon):
    """How many entries of env e's list, from entry t on, may give the goal: at most `horizon`, none behind the episode's end, none
    beyond the list."""
    k = 0
    for s in traj[e][t:t + horizon]:
        k += 1
        if s["ended"]:
            break
    return k


def check_rows(rows, js, draws, traj, horizon, what=""):
    """Relabelled rows (js >= 0) against the lists: j is (draw k) >> 32 with k counted from the list, the goal columns are the goal
    entry t + j achieved, which lies in the same episode, inside the list and fewer than `horizon` steps ahead; every other column but
    the reward is the entry's own.  Rows with js == -1 are the entry itself.  Returns the (env, t, j) triples."""
    out = []
    for b in range(len(rows)):
        e, t = find(traj, rows[b])
        s, tag = traj[e][t], f"{what} row {b} (env {e}, entry {t}, horizon {horizon})"
        assert np.array_equal(rows[b, :18], s["obs"][:18]) and np.array_equal(rows[b, D:D + A], s["act"]), tag
        assert np.array_equal(rows[b, NOBS:NOBS + 18], s["next"][:18]) and rows[b, -1] == s["done"], tag
        if js[b] < 0:
            assert np.array_equal(rows[b, 18:21], s["obs"][18:]) and np.array_equal(rows[b, NOBS + 18:NOBS + 21], s["next"][18:]), tag
            assert rows[b, RCOL] == s["rew"], tag
        else:
            k = candidates(traj, e, t, horizon)
            j = (int(draws[b]) * k) >> 32
            assert js[b] == j and 0 <= j < k <= horizon and t + j < len(traj[e]), tag
            src = traj[e][t + j]
            assert src["episode"] == s["episode"], tag
            v = src["next"][6:9].astype(np.float64)
            goal = np.array([src["next"][5], src["next"][11], np.float32(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))], dtype=np.float32)
            assert np.array_equal(rows[b, 18:21], goal) and np.array_equal(rows[b, NOBS + 18:NOBS + 21], goal), tag
        out.append((e, t, int(js[b])))
    return out


def draws(seed, grad_step, batch, size):
    """What the gather kernels draw for the rows of a batch at gradient step `grad_step`: (idx [B] of fw_replay_sample, o0 [B] and o1
    [B] of fw_replay_sample_her's second block), from the numpy Philox of tests/device_reference.py."""
    b = np.arange(batch, dtype=np.uint64)
    key = np.tile(np.array([[seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]], dtype=np.uint64), (batch, 1))

    def block(tag):
        ctr = np.stack([b, np.zeros_like(b), np.full_like(b, grad_step & 0xFFFFFFFF), np.full_like(b, ((grad_step >> 32) & 0xFFFFFFFF) ^ tag)], axis=1)
        return R.philox4x32_10(ctr, key).astype(np.uint64)

    s, h = block(SAMPLE_TAG), block(0x5AC0E000)
    idx = (s[:, 0] * np.uint64(max(int(size), 1))) >> np.uint64(32)
    return idx.astype(np.int64), h[:, 0], h[:, 1]
