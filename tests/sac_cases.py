"""Shared pieces of the SAC tests (tests/test_sac_cpu.py, tests/test_sac_gpu.py): the pinned inputs of the update-parity cases, the
comparison of two learners under the project's learner tolerances, and a numpy model of the replay ring."""
import copy

import numpy as np
import torch

from pyflyt_drone_amd import sac as S

# (obs_dim, act_dim, hidden, batch) x seeds of the update-parity cases
SHAPES = [(21, 6, 256, 64), (21, 6, 64, 32), (30, 3, 64, 16), (28, 4, 256, 256)]
SEEDS = [5, 6]
# (rtol, atol) of tests/test_wide_action_learner_gpu.py
TOL = {"param": (2e-3, 2e-5), "exp_avg": (5e-3, 1e-6), "exp_avg_sq": (5e-3, 1e-9)}
NETS = ("actor", "q1", "q2", "q1_target", "q2_target")


def make_policy(d, A, H, seed, perturb=0.0):
    """torch's default initialisation under `seed` (the global generator is left alone); `perturb` adds perturb x N(0, 1)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        pol = S.SacPolicy(d, A, H)
        if perturb:
            with torch.no_grad():
                for net in (pol.actor, pol.q1, pol.q2):
                    for q in net.parameters():
                        q.add_(perturb * torch.randn_like(q))
                pol.q1_target.load_state_dict(pol.q1.state_dict()); pol.q2_target.load_state_dict(pol.q2.state_dict())
    return pol


def make_batch(d, A, B, seed):
    """Rows [B, 2d + A + 2]: obs ~ N(0, 1) clamped to +-5, actions uniform in [-1, 1), rewards ~ N(0, 1), next_obs = obs + 0.1 N(0, 1),
    done with probability 0.1 (float32, CPU)."""
    g = torch.Generator().manual_seed(1000 + seed)
    obs = torch.randn((B, d), generator=g).clamp(-5, 5)
    act = torch.rand((B, A), generator=g) * 2.0 - 1.0
    rew = torch.randn((B, 1), generator=g)
    nxt = obs + 0.1 * torch.randn((B, d), generator=g)
    done = (torch.rand((B, 1), generator=g) < 0.1).float()
    return torch.cat([obs, act, rew, nxt, done], dim=1).contiguous()


def make_noise(A, B, seed, step):
    g = torch.Generator().manual_seed(2000 + 17 * seed + step)
    return torch.randn((2, B, A), generator=g)


def learner(pol, cfg, dtype=None, device=None):
    """A deep copy of `pol` in `dtype` on `device` and its three optimisers."""
    p = copy.deepcopy(pol)
    if dtype is not None:
        p = p.to(dtype)
    if device is not None:
        p = p.to(device)
    return p, S.make_optimizers(p, cfg)


def _close(name, x, y, rtol, atol):
    x, y = x.detach().double().cpu(), y.detach().double().cpu()
    bad = (x - y).abs() > atol + rtol * y.abs()
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {bad.numel()} elements outside rtol {rtol} atol {atol}, worst "
                                 f"|diff| {float((x - y).abs().max()):.3e}")


def compare(pa, oa, pb, ob, moments=True):
    """Every parameter of all five networks, log_ent_coef, every Adam moment and the step counts of learner a against learner b,
    with no element left out."""
    assert pa.n_updates == pb.n_updates
    for net in NETS:
        for (n, x), (_, y) in zip(getattr(pa, net).named_parameters(), getattr(pb, net).named_parameters()):
            _close(f"{net}.{n}", x, y, *TOL["param"])
    _close("log_ent_coef", pa.log_ent_coef, pb.log_ent_coef, *TOL["param"])
    if not moments:
        return
    for key in ("actor", "critic", "ent"):
        if oa[key] is None:
            assert ob[key] is None
            continue
        for ga, gb in zip(oa[key].param_groups, ob[key].param_groups):
            for x, y in zip(ga["params"], gb["params"]):
                sa, sb = oa[key].state[x], ob[key].state[y]
                assert float(sa["step"]) == float(sb["step"]) == pa.n_updates
                _close(f"{key} exp_avg", sa["exp_avg"], sb["exp_avg"], *TOL["exp_avg"])
                _close(f"{key} exp_avg_sq", sa["exp_avg_sq"], sb["exp_avg_sq"], *TOL["exp_avg_sq"])


class NumpyRing:
    """The replay ring as plain numpy: capacity (buffer_size // N) N rows of [obs | action | reward | next_obs | done]; a store
    appends N rows at the cursor, next_obs is the terminal observation where the episode ended, done is `terminated` alone."""

    def __init__(self, buffer_size, n, d, a):
        self.n, self.d, self.a = n, d, a
        self.capacity = (buffer_size // n) * n
        self.ring = np.zeros((self.capacity, 2 * d + a + 2), dtype=np.float32)
        self.cursor = self.size = self.steps = 0

    def store(self, obs, act, rew, next_obs, terminal_obs, terminated, truncated):
        ended = (np.asarray(terminated) | np.asarray(truncated)).astype(bool)
        nxt = np.where(ended[:, None], terminal_obs, next_obs)
        rows = np.concatenate([obs, act, np.asarray(rew)[:, None], nxt, np.asarray(terminated, dtype=bool)[:, None]], axis=1)
        self.ring[self.cursor:self.cursor + self.n] = rows.astype(np.float32)
        self.cursor = (self.cursor + self.n) % self.capacity
        self.size = min(self.size + self.n, self.capacity)
        self.steps += 1

    @property
    def counters(self):
        return [self.cursor, self.size, self.steps]
