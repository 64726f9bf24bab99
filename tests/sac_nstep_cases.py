"""Shared pieces of the n-step tests (tests/test_sac_nstep_cpu.py, tests/test_sac_nstep_gpu.py): a scripted run of 4 envs over 9
vec-steps with hand-placed episode ends, its per-env trajectory lists, and a computation of the n-step transition from those lists that
knows nothing of ring arithmetic."""
import numpy as np

N_ENVS, STEPS, RING_STEPS = 4, 9, 6          # the ring holds 6 vec-steps: 9 stores wrap it
HALF = 3                                     # stores before the "half full" check
N_STEPS = (1, 2, 3, 5, 8, 16)
U = 2.0 ** -24                               # unit roundoff of float32
# (vec-step, env): which flags end the episode there.  Steps 0-2 are what the half-full ring holds, steps 3-8 what the wrapped one holds;
# both windows hold a terminated-only, a truncated-only and a both-flags end, and an end in their newest step (2 and 8).
ENDS = {(0, 2): (1, 1), (1, 0): (1, 0), (2, 1): (0, 1),                 # half full: both, terminated only, truncated only (newest step)
        (3, 2): (1, 1), (4, 3): (1, 0), (5, 3): (0, 1),                 # wrapped: both; two in consecutive steps of env 3
        (6, 1): (1, 0), (7, 2): (0, 1), (8, 0): (1, 0)}                 # terminated only, truncated only, one in the newest step


def script(d, A, seed=0):
    """STEPS store() argument tuples (obs, act, rew, next_obs, terminal_obs, terminated, truncated) of float32 / uint8 arrays: inside an
    episode a step's next_obs is the next step's obs; at an end the env hands over the terminal observation and next_obs is the first
    observation of the new episode."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    obs, out = f(N_ENVS, d), []
    for t in range(STEPS):
        term, trunc = np.zeros(N_ENVS, dtype=np.uint8), np.zeros(N_ENVS, dtype=np.uint8)
        for (tt, e), (a, b) in ENDS.items():
            if tt == t:
                term[e], trunc[e] = a, b
        nxt, tobs = f(N_ENVS, d), f(N_ENVS, d)
        out.append((obs, rng.uniform(-1, 1, (N_ENVS, A)).astype(np.float32), f(N_ENVS), nxt, tobs, term, trunc))
        obs = nxt
    return out


def numpy_ends(stores):
    """The `ends` side ring after these stores, by the rule 'the byte of the row the store writes'."""
    ends, cursor = np.zeros(RING_STEPS * N_ENVS, dtype=np.uint8), 0
    for s in stores:
        ends[cursor:cursor + N_ENVS] = (s[5] != 0) * 1 + (s[6] != 0) * 2
        cursor = (cursor + N_ENVS) % len(ends)
    return ends


def trajectories(stores):
    """Per env, the list of its transitions in time order, of the steps a ring of RING_STEPS vec-steps still holds."""
    first = max(0, len(stores) - RING_STEPS)
    traj = [[] for _ in range(N_ENVS)]
    for s in stores[first:]:
        obs, act, rew, nxt, tobs, term, trunc = s
        for e in range(N_ENVS):
            ended = bool(term[e] or trunc[e])
            traj[e].append(dict(obs=obs[e], act=act[e], rew=rew[e], next=(tobs if ended else nxt)[e], done=float(term[e] != 0), ended=ended))
    return traj


def find(traj, obs):
    """(env, position in its list) of the transition that starts at this observation."""
    hits = [(e, t) for e in range(N_ENVS) for t, s in enumerate(traj[e]) if np.array_equal(s["obs"], obs)]
    assert len(hits) == 1
    return hits[0]


def brute(traj, e, t, n_steps, gamma):
    """The n-step transition from env e's list, starting at its entry t: collect entries until n_steps are used, the episode ended, or
    the list is exhausted.  float64 throughout, gamma the float32 value the kernel receives.  Returns a dict with obs, act, next, k, the
    return `ret`, the sum of |gamma^j r_j| `mag` and the last column 1 - (1 - done) gamma^(k-1)."""
    g, steps = float(np.float32(gamma)), traj[e][t:t + n_steps]
    used = []
    for s in steps:
        used.append(s)
        if s["ended"]:
            break
    k = len(used)
    terms = [g ** j * float(s["rew"]) for j, s in enumerate(used)]
    return dict(obs=used[0]["obs"], act=used[0]["act"], next=used[-1]["next"], k=k, ret=sum(terms), mag=sum(abs(x) for x in terms),
                last=1.0 - (1.0 - used[-1]["done"]) * g ** (k - 1))


def check_rows(rows, ks, traj, d, A, n_steps, gamma, what=""):
    """Every row of `rows` / `ks` (an n-step batch) against brute(): obs, action, next_obs and k exactly, the reward within
    (2n + 1) u sum|gamma^j r_j| (k - 1 roundings in g_j, one per product, one per sum -- an fma has fewer), the last column within
    (n + 1) u (k - 2 roundings in g, one product, one difference, all of values <= 1)."""
    for b in range(len(rows)):
        e, t = find(traj, rows[b, :d])
        w = brute(traj, e, t, n_steps, gamma)
        tag = f"{what} row {b} (env {e}, entry {t}, n_steps {n_steps})"
        assert ks[b] == w["k"], tag
        assert np.array_equal(rows[b, :d], w["obs"]) and np.array_equal(rows[b, d:d + A], w["act"]), tag
        assert np.array_equal(rows[b, d + A + 1:2 * d + A + 1], w["next"]), tag
        assert abs(float(rows[b, d + A]) - w["ret"]) <= (2 * n_steps + 1) * U * w["mag"], tag
        assert abs(float(rows[b, -1]) - w["last"]) <= (n_steps + 1) * U, tag
