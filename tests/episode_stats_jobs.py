"""Shared pieces of tests/test_episode_stats_cpu.py and tests/test_episode_stats_gpu.py: the synthetic step streams, SB3's
Monitor + ep_info_buffer written out literally, a CPU toy env with the device env's output buffers, and the rank of the
world_size-2 ``gloo`` job (started with the ``spawn`` context by the test itself)."""
import collections
import math
import os

import numpy as np

INFO_DIM = 8
SHAPES = [(199, 7), (1500, 100), (1, 1), (5, 100)]          # (N, W)


def make_stream(N, W, f64, seed=0):
    """A list of vec-steps ``(reward [N], terminated u8 [N], truncated u8 [N], info i32 [N, 8])`` as numpy arrays.  Among random
    steps (a tenth of the envs done) it holds: a step with every env done (twice), one with exactly min(W, N) done, one with none
    done, and one whose only dones are the last N mod 64 envs (the part of the last wave that is in use)."""
    rng = np.random.default_rng(1000 * seed + 7 * N + W)
    kinds = ["rand", "rand", "all", "rand", "exact", "none", "tail", "rand", "all", "rand", "rand"]
    out = []
    for kind in kinds:
        rew = (rng.normal(size=N) * 3.0 + 0.5).astype(np.float64 if f64 else np.float32)
        done = np.zeros(N, dtype=bool)
        if kind == "rand":
            done = rng.random(N) < 0.1
        elif kind == "all":
            done[:] = True
        elif kind == "exact":
            done[rng.permutation(N)[:min(W, N)]] = True
        elif kind == "tail":
            done[N - (N % 64):] = True
        trunc = done & (rng.random(N) < 0.5)
        term = done & ~trunc
        both = done & (rng.random(N) < 0.1)                  # (an env may raise both flags)
        term |= both
        info = np.zeros((N, INFO_DIM), dtype=np.int32)
        info[:, 0] = rng.integers(0, 6, N)
        info[:, 1:6] = rng.integers(0, 2, (N, 5))
        info[:, 6] = rng.integers(1, 500, N)
        out.append((rew, term.astype(np.uint8), trunc.astype(np.uint8), info))
    assert any(d[1].any() or d[2].any() for d in out)
    return out


class Sb3Statement:
    """stable_baselines3's bookkeeping, literally: ``Monitor`` keeps a running return and length per env and emits an episode record
    when the env is done; ``OnPolicyAlgorithm._update_info_buffer`` extends ``deque(maxlen=stats_window_size)`` with the step's
    records in env order.  Every finished episode is kept too (``all``) for the totals."""

    def __init__(self, N, W):
        self.N, self.W = N, W
        self.cur_r, self.cur_l = [0.0] * N, [0] * N
        self.buffer = collections.deque(maxlen=W)
        self.all = []
        self.steps = 0

    def step(self, rew, term, trunc, info=None):
        self.steps += 1
        finished = []
        for i in range(self.N):
            self.cur_r[i] += float(rew[i])
            self.cur_l[i] += 1
            if term[i] or trunc[i]:
                row = np.zeros(INFO_DIM, dtype=np.int32) if info is None else np.asarray(info[i], dtype=np.int32).copy()
                finished.append({"r": self.cur_r[i], "l": self.cur_l[i], "step": self.steps, "env": i,
                                 "truncated": int(trunc[i] != 0), "info": row})
                self.cur_r[i], self.cur_l[i] = 0.0, 0
        self.buffer.extend(finished)
        self.all.extend(finished)

    def window(self):
        b = list(self.buffer)
        return {"r": np.array([e["r"] for e in b], dtype=np.float64), "l": np.array([e["l"] for e in b], dtype=np.int64),
                "step": np.array([e["step"] for e in b], dtype=np.int64), "env": np.array([e["env"] for e in b], dtype=np.int64),
                "truncated": np.array([e["truncated"] for e in b], dtype=np.int64),
                "info": np.array([e["info"] for e in b], dtype=np.int32).reshape(len(b), INFO_DIM)}

    def int_totals(self):
        names = ("targets_reached", "collision", "out_of_bounds", "env_complete", "duck_strike", "is_success")
        out = {"episodes": len(self.all), "steps": self.steps, "truncated": sum(e["truncated"] for e in self.all),
               "sum_len": sum(e["l"] for e in self.all)}
        out.update({"sum_" + k: sum(int(e["info"][c]) for e in self.all) for c, k in enumerate(names)})
        return out

    def window_scalars(self):
        """``safe_mean`` over the buffer, as SB3's logger records them (NaN when it is empty)."""
        b = list(self.buffer)

        def safe_mean(xs):
            return float("nan") if len(xs) == 0 else float(np.mean(xs))
        return {"rollout/ep_rew_mean": safe_mean([e["r"] for e in b]), "rollout/ep_len_mean": safe_mean([e["l"] for e in b]),
                "rollout/success_rate": safe_mean([int(e["info"][5]) for e in b]),
                "rollout/targets_reached_mean": safe_mean([int(e["info"][0]) for e in b]),
                "rollout/collision_rate": safe_mean([int(e["info"][1]) for e in b]),
                "rollout/out_of_bounds_rate": safe_mean([int(e["info"][2]) for e in b]),
                "rollout/duck_strike_rate": safe_mean([int(e["info"][4]) for e in b]),
                "rollout/timeout_rate": safe_mean([e["truncated"] for e in b]),
                "rollout/episodes": float(len(self.all))}

    def check_double_totals(self, sum_ret, sum_ret2):
        """|sum - exact| <= n 2^-52 sum |x_i| for n summed terms: the rounding bound of a sum taken in any order."""
        r = [e["r"] for e in self.all]
        n = len(r)
        for got, xs in ((sum_ret, r), (sum_ret2, [x * x for x in r])):
            exact = math.fsum(xs)
            bound = n * 2.0 ** -52 * math.fsum(abs(x) for x in xs)
            assert abs(got - exact) <= bound, (got, exact, bound)


def assert_window_equal(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def same_scalars(a, b, keys=None):
    keys = list(b) if keys is None else keys
    return all((math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k] for k in keys)


class ToyVenv:
    """CPU stand-in with the device env's surface as VecNormalizeDevice and PPOConfig.episode_stats consume it: ``step_tensor`` and
    the output buffers ``rewards`` / ``terminated`` / ``truncated`` / ``info`` that hold the last step.  Env i meets its time limit
    after ``horizon + i % 3`` steps; an observation above a threshold terminates it."""

    def __init__(self, n=16, d=6, seed=0, horizon=5):
        import torch
        self.device = torch.device("cpu"); self.num_envs, self.obs_dim = n, d
        self.torch_dtype = torch.float64
        self.g = torch.Generator().manual_seed(seed)
        self.t = torch.zeros(n, dtype=torch.long); self.horizon = horizon
        self.terminal_obs = torch.zeros((n, d), dtype=torch.float64)
        self.obs = torch.zeros((n, d), dtype=torch.float64)
        self.rewards = torch.zeros(n, dtype=torch.float64)
        self.terminated = torch.zeros(n, dtype=torch.uint8)
        self.truncated = torch.zeros(n, dtype=torch.uint8)
        self.info = torch.zeros((n, INFO_DIM), dtype=torch.int32)
        self.record = []

    def _draw(self):
        import torch
        return torch.randn((self.num_envs, self.obs_dim), generator=self.g, dtype=torch.float64) * 3.0 + 1.5

    def reset_tensor(self):
        self.t.zero_(); self.obs = self._draw(); return self.obs

    def step_tensor(self, actions):
        import torch
        self.t += 1
        nxt = self._draw()
        rew = -(actions.to(torch.float64) ** 2).sum(-1) + 0.1 * nxt[:, 0]
        trunc = (self.t >= self.horizon + (torch.arange(self.num_envs) % 3))
        term = (nxt[:, 1] > 6.0) & ~trunc
        done = term | trunc
        self.terminal_obs = torch.where(done[:, None], nxt, self.terminal_obs)
        self.obs = torch.where(done[:, None], self._draw(), nxt)
        self.info.zero_()
        self.info[:, 0] = (nxt[:, 2] > 3.0).to(torch.int32) * 2
        self.info[:, 5] = (done & (nxt[:, 3] > 1.5)).to(torch.int32)
        self.info[:, 6] = torch.where(done, self.t, torch.zeros_like(self.t)).to(torch.int32)
        self.t = torch.where(done, torch.zeros_like(self.t), self.t)
        self.rewards.copy_(rew); self.terminated.copy_(term.to(torch.uint8)); self.truncated.copy_(trunc.to(torch.uint8))
        self.record.append((self.rewards.numpy().copy(), self.terminated.numpy().copy(), self.truncated.numpy().copy(),
                            self.info.numpy().copy()))
        return self.obs, self.rewards, self.terminated, self.truncated


def monitor_rank(rank, world, port, q):
    """One rank of the gloo job: a monitor over its own stream, its figures summed over the ranks with one all-reduce."""
    import torch
    import torch.distributed as td
    from pyflyt_drone_amd import monitor as M
    from pyflyt_drone_amd import rollout as R
    torch.set_num_threads(1)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    try:
        N, W = 37, 5
        m = M.EpisodeMonitor(N, W)
        calls = [0]
        reduce_ = R.all_reduce_sum_

        def spy(t):
            calls[0] += 1
            return reduce_(t)
        stream = make_stream(N, W, True, seed=11 + rank)
        out = []
        for part in (stream[:6], stream[6:]):
            for rew, te, tr, info in part:
                m.fold(torch.from_numpy(rew), torch.from_numpy(te), torch.from_numpy(tr), torch.from_numpy(info))
            out.append(m.scalars(reduce=spy))
        q.put((rank, dict(scalars=out, reduces=calls[0], local=m.totals(), window=m.window())))
    finally:
        td.destroy_process_group()
