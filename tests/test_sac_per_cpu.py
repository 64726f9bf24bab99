"""Prioritized replay on the replay ring, without a GPU: the exported symbols, the config, buffer and checkpoint rules, and the numpy
statements of the contract (sac.per_sums_reference, per_draw_reference, per_update_reference and their helpers), which
tests/test_sac_per_gpu.py holds the kernels to: the sums against float64, the draw's guarantees, its statistics on the scripted ring L
(tests/per_cases.py), the clamp rule, the exponents' edge values, the schedule of beta and the write-back's rules."""
import os
import re

import numpy as np
import pytest
import torch

from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import sac as S

import per_cases as PC
import sac_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fw_replay_per_mark_new", "fw_replay_per_rebuild", "fw_replay_sample_per", "fw_replay_per_update", "fw_sac_update_weighted")
DRAW_SEED, DRAWS = 9, 20000


@pytest.fixture(scope="module")
def rings():
    """name -> (leaves, hot rows, per_sums_reference of the leaves): computed once, never written."""
    out = {}
    for name in PC.RINGS:
        prio, hot = PC.leaves(name)
        sums = S.per_sums_reference(prio)
        for a in (prio, hot) + tuple(v for v in sums.values() if isinstance(v, np.ndarray)):
            a.setflags(write=False)
        out[name] = (prio, hot, sums)
    return out


def test_the_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "fwsim.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", header), name
    assert K.FW_ABI_VERSION == 7                                 # functions were added, none changed
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert S.PER_GROUP == 256 and S.PER_MAX_CAPACITY == 2 ** 22


# ------------------------------------------------------------------------------------------------ the sums
@pytest.mark.parametrize("name", list(PC.RINGS))
def test_sums_against_float64(rings, name):
    """A sum of 256 float32 terms in any fixed order lies within gamma_255 sum|x| of the exact one (255 roundings at most on any
    path): sum1 against the leaves, sum2 against the float32 sum1 it is made of, the total against sum2."""
    prio, _, r = rings[name]
    cap = prio.size
    n1, n2 = -(-cap // 256), -(-(-(-cap // 256)) // 256)
    assert r["sum1"].shape == r["min1"].shape == (n1,) and r["sum2"].shape == r["min2"].shape == (n2,)
    assert all(r[k].dtype == np.float32 for k in ("sum1", "min1", "sum2", "min2"))
    bound = 255 * PC.U / (1 - 255 * PC.U)

    def exact(v, groups):
        return np.pad(v.astype(np.float64), (0, groups * 256 - v.size)).reshape(groups, 256).sum(1)

    for got, want in ((r["sum1"], exact(prio, n1)), (r["sum2"], exact(r["sum1"], n2)), (np.array([r["total"]]), exact(r["sum2"], 1))):
        assert (np.abs(got.astype(np.float64) - want) <= bound * want).all()
    # mins: the smallest positive entry below, +inf where there is none
    g = np.pad(prio, (0, n1 * 256 - cap)).reshape(n1, 256)
    for k in range(n1):
        pos = g[k][g[k] > 0]
        assert r["min1"][k] == (pos.min() if pos.size else np.inf)
    assert r["pmin"] == prio[prio > 0].min() == r["min2"].min()
    if name == "L":
        assert n1 == 258 and n2 == 2 and r["sum2"][1] > 0         # the second level-2 entry holds two level-1 groups


def test_sums_of_an_empty_ring_and_the_capacity_limit():
    r = S.per_sums_reference(np.zeros(300, dtype=np.float32))
    assert r["total"] == 0 and np.isinf(r["pmin"]) and np.isinf(r["min1"]).all() and not r["sum1"].any()
    for bad in (np.zeros(0), np.zeros(2 ** 22 + 1, dtype=np.float32)):
        with pytest.raises(ValueError):
            S.per_sums_reference(bad)


def test_the_order_of_a_group_by_hand():
    x = np.zeros(256, dtype=np.float32)
    x[[0, 1, 5, 255]] = [1.0, 2.0 ** -24, 3.0, 2.0 ** -24]
    Sm, F, total = S.per_group_sums(x)
    assert Sm[0] == 1.0 and Sm[1] == 1.0                         # 1 + 2^-24 rounds to 1 in float32: the chain of four adds in float32
    assert F[0] == 0.0 and F[1] == 1.0 and F[4] == 1.0 and Sm[5] == 4.0 and F[6] == 4.0 and Sm[254] == 4.0
    assert total == Sm[255] == 4.0 and (np.diff(Sm) >= 0).all() and np.array_equal(F[1:], Sm[:-1])


# ------------------------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize("name", list(PC.RINGS))
def test_the_draw_returns_filled_rows_with_positive_leaves(rings, name):
    prio, _, sums = rings[name]
    for gs in range(3):
        idx = S.per_draw_reference(prio, sums, PC.words(DRAW_SEED, gs, 4096))
        assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < PC.RINGS[name]["filled"]
        assert (prio[idx] > 0).all()
    if name == "S":                                               # 12 288 draws over 38 positive rows reach every one of them
        seen = np.unique(np.concatenate([S.per_draw_reference(prio, sums, PC.words(DRAW_SEED, gs, 4096)) for gs in range(3)]))
        assert np.array_equal(seen, np.flatnonzero(prio > 0))


def test_the_draw_is_proportional_on_the_large_ring(rings):
    """20 000 draws on L from the numpy Philox: the count of every hot row, and the count every level-1 group's remaining rows
    collect, lies within 5 binomial standard deviations of M q.  (A prototype with numpy's random words and a 24-bit u had worst z of
    2.0 and 3.04; with the Philox words of seed 9 at gradient step 0, as drawn here: 2.51 over the hot rows, 2.95 over the groups.)"""
    prio, hot, sums = rings["L"]
    idx = S.per_draw_reference(prio, sums, PC.words(DRAW_SEED, 0, DRAWS))
    assert (prio[idx] > 0).all() and idx.max() < 66000
    z_hot, z_group = PC.worst_z(idx, prio, hot)
    share = float((prio[idx] == PC.HOT_LEAF).mean())
    print(f"worst z: hot rows {z_hot:.2f}, level-1 groups {z_group:.2f}; the hot rows took {share:.3f} of the draws")
    assert z_hot <= 5.0 and z_group <= 5.0
    assert abs(share - 0.43) < 0.02                               # "about 43 % of the mass"


def test_the_clamp_rule(rings):
    """t forced at and above the total: no running sum exceeds it, so every level takes its last positive entry -- the last row with a
    positive leaf.  Just below the first positive leaf: the first such row."""
    for name in PC.RINGS:
        prio, _, sums = rings[name]
        last, first = np.flatnonzero(prio > 0)[-1], np.flatnonzero(prio > 0)[0]
        tot = sums["total"]
        t = np.array([tot, np.nextafter(tot, np.float32(np.inf)), 2 * tot, np.float32(np.inf), 0.0, prio[first] * 0.5], dtype=np.float32)
        idx = S.per_draw_reference(prio, sums, None, t=t)
        assert idx.tolist() == [last] * 4 + [first] * 2, name
    # a zero leaf at the end of a group, and a whole group of zeros, are never the clamp's choice
    prio = np.zeros(1024, dtype=np.float32)
    prio[[5, 300, 301]] = [1.0, 2.0, 3.0]
    sums = S.per_sums_reference(prio)
    assert S.per_draw_reference(prio, sums, None, t=np.array([6.0, 5.9, 2.9, 3.0, 0.99, 1.0], dtype=np.float32)).tolist() == [301, 301, 300, 301, 5, 300]
    # sums nobody rebuilt (a positive sum over leaves of zero): the index still stays inside the ring
    stale = dict(sums)
    assert S.per_draw_reference(np.zeros(1024, dtype=np.float32), stale, None, t=np.array([4.0], dtype=np.float32)).tolist() == [256]
    empty = S.per_sums_reference(np.zeros(1024, dtype=np.float32))
    assert S.per_draw_reference(np.zeros(1024, dtype=np.float32), empty, PC.words(1, 0, 8)).tolist() == [0] * 8


# ------------------------------------------------------------------------------------------------ exponents, weights, write-back
def test_alpha_zero_makes_all_positive_leaves_equal_and_beta_zero_all_weights_one(rings):
    prio, _, sums = rings["S"]
    idx = np.arange(40)
    td = np.random.default_rng(0).uniform(0, 5, 40).astype(np.float32)
    out, pmax = S.per_update_reference(prio, idx, td, 0.0, 1e-6, 1.0)
    assert (out[:40] == 1.0).all() and (out[40:] == 0.0).all() and pmax == 1.0
    pos = np.flatnonzero(prio > 0)
    assert (S.per_weights_reference(prio, pos, sums["pmin"], 0.0) == 1.0).all()
    w = S.per_weights_reference(prio, pos, sums["pmin"], 0.5)
    assert w.max() == 1.0 and w.argmax() == prio[pos].argmin() and (w > 0).all()
    # (N P(row))^-beta over its maximum, in float64
    P = prio[pos].astype(np.float64) / prio[pos].astype(np.float64).sum()
    full = (len(pos) * P) ** -0.5
    np.testing.assert_allclose(w, full / full.max(), rtol=1e-12)


def test_the_schedule_of_beta():
    f = S.per_beta_reference
    assert f(0.4, 0, 10 ** 6) == np.float32(0.4) and f(0.4, 1000, 0) == np.float32(0.4)
    assert abs(float(f(0.4, 1000, 500)) - 0.7) < 1e-6 and f(0.4, 1000, 1000) == 1.0 and f(0.4, 1000, 5000) == 1.0
    assert f(1.0, 10, 3) == 1.0 and f(0.0, 4, 1) == np.float32(0.25)
    assert isinstance(f(0.4, 1000, 500), np.float32)


def test_the_write_back_takes_the_largest_duplicate_and_tracks_the_max(rings):
    prio, _, _ = rings["S"]
    idx = np.array([7, 2, 7, 30, 7, 2], dtype=np.int32)
    td = np.array([0.5, 3.0, 2.0, 0.0, 1.0, 0.25], dtype=np.float32)
    out, pmax = S.per_update_reference(prio, idx, td, 0.6, 1e-6, 1.0)
    leaf = lambda x: np.float32((np.float64(np.float32(x) + np.float32(1e-6))) ** np.float64(np.float32(0.6)))
    assert out[7] == leaf(2.0) and out[2] == leaf(3.0) and out[30] == leaf(0.0) and out[30] > 0
    untouched = np.setdiff1d(np.arange(64), [2, 7, 30])
    assert np.array_equal(out[untouched], prio[untouched]) and out.dtype == np.float32
    assert pmax == leaf(3.0) and S.per_update_reference(prio, idx, td, 0.6, 1e-6, 7.5)[1] == np.float32(7.5)
    assert S.per_update_reference(prio, idx, -td, 0.6, 1e-6, 1.0)[0].tolist() == out.tolist()           # |td|
    # skipped: an index outside the ring; a td that is not finite leaves 0
    out2, pmax2 = S.per_update_reference(prio, np.array([64, -1, 9]), np.array([1.0, 1.0, np.nan], dtype=np.float32), 0.6, 1e-6, 1.0)
    assert out2[9] == 0.0 and pmax2 == 1.0 and np.array_equal(np.delete(out2, 9), np.delete(prio, 9))


# ------------------------------------------------------------------------------------------------ config, buffer, checkpoints, torch step
def test_config_validation():
    c = S.SACConfig()
    assert (c.prioritized, c.per_alpha, c.per_beta, c.per_beta_steps, c.per_eps) == (False, 0.6, 0.4, 0, 1e-6)
    ok = S.SACConfig(prioritized=True, per_alpha=0.0, per_beta=1.0, per_beta_steps=1000, per_eps=1e-3)
    assert ok.prioritized and ok.per_beta_steps == 1000
    for bad in (dict(per_alpha=-0.1), dict(per_alpha=1.1), dict(per_beta=-0.1), dict(per_beta=1.5), dict(per_beta_steps=-1),
                dict(per_beta_steps=2.5), dict(per_eps=0.0), dict(per_eps=-1e-6), dict(per_alpha=float("nan"))):
        with pytest.raises(ValueError):
            S.SACConfig(prioritized=True, **bad)
    with pytest.raises(ValueError, match="not built"):
        S.SACConfig(prioritized=True, n_steps=3)
    with pytest.raises(ValueError, match="not built"):
        S.SACConfig(prioritized=True, her_goals=4)
    assert S.SACConfig(n_steps=3).prioritized is False


def test_buffer_and_checkpoint_rules():
    off = S.ReplayBufferDevice(40, 4, 21, 6, "cpu")
    assert off.prio is None and off.per_state is None and not off.prioritized
    on = S.ReplayBufferDevice(600, 4, 21, 6, "cpu", prioritized=True)
    assert on.prio.shape == (600,) and on.sum1.shape == on.min1.shape == (3,) and on.sum2.shape == on.min2.shape == (1,)
    assert on.per_state.tolist() == [1.0, 0.0, float("inf"), 0.0] and not on.prio.any() and torch.isinf(on.min1).all()
    for kw in (dict(n_steps=3), dict(per_alpha=1.5), dict(per_beta=-1.0), dict(per_eps=0.0), dict(per_beta_steps=-2)):
        with pytest.raises(ValueError):
            S.ReplayBufferDevice(40, 4, 21, 6, "cpu", prioritized=True, **kw)
    with pytest.raises(ValueError, match="2\\^22"):
        S.ReplayBufferDevice(2 ** 22 + 4, 4, 1, 1, "cpu", prioritized=True)
    with pytest.raises(ValueError):
        off.sample(1, torch.zeros((16, 50)), w_out=torch.zeros(16))
    # priorities travel with the rows
    on.ring.normal_(); on.counters.copy_(torch.tensor([80, 80, 20, 5]))
    on.prio[:80] = torch.rand(80) + 0.1; on.per_state[0] = 2.5
    on.rebuild()
    ref = S.per_sums_reference(on.prio.numpy())
    assert np.array_equal(on.sum1.numpy(), ref["sum1"]) and on.per_state[1] == float(ref["total"]) and on.per_state[2] == float(ref["pmin"])
    sd = on.state_dict(include_buffer=True)
    assert torch.equal(sd["prio"], on.prio) and torch.equal(sd["per_state"], on.per_state)
    assert "prio" not in on.state_dict() and "prio" not in off.state_dict(include_buffer=True)
    other = S.ReplayBufferDevice(600, 4, 21, 6, "cpu", prioritized=True)
    other.load_state_dict(sd)
    for k in ("prio", "sum1", "min1", "sum2", "min2", "per_state", "ring"):
        assert torch.equal(getattr(other, k), getattr(on, k)), k
    # rows without priorities: every filled row gets a leaf of 1.0
    plain = S.ReplayBufferDevice(600, 4, 21, 6, "cpu")
    plain.ring.copy_(on.ring); plain.counters.copy_(on.counters)
    other.load_state_dict(plain.state_dict(include_buffer=True))
    assert (other.prio[:80] == 1.0).all() and not other.prio[80:].any()
    assert other.per_state.tolist() == [1.0, 80.0, 1.0, 0.0] and other.sum1.tolist() == [80.0, 0.0, 0.0]
    # no rows: no leaves
    other.load_state_dict(on.state_dict())
    assert not other.prio.any() and other.per_state.tolist() == [1.0, 0.0, float("inf"), 0.0] and other.counters.tolist() == [0, 0, 20, 5]
    # a plain buffer takes a prioritized checkpoint's rows and ignores the leaves
    plain.load_state_dict(sd)
    assert torch.equal(plain.ring, on.ring) and plain.prio is None


def test_the_torch_step_weights_the_critic_loss_alone():
    d, A, H, B, seed = 21, 6, 64, 32, 5
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), seed=seed)
    pol, rows, eps = SC.make_policy(d, A, H, seed), SC.make_batch(d, A, B, seed), SC.make_noise(A, B, seed, 0)
    runs = {}
    for name, w in (("none", None), ("ones", torch.ones(B)), ("half", torch.full((B,), 0.5)), ("rand", torch.rand(B, generator=torch.Generator().manual_seed(1)) * 0.95 + 0.05)):
        p, o = SC.learner(pol, cfg)
        runs[name] = (p, S.sac_update_torch(p, o, rows, eps[0], eps[1], cfg, weights=w))
    (p0, s0), (p1, s1), (ph, sh), (pr, sr) = (runs[k] for k in ("none", "ones", "half", "rand"))
    for (n, x), (_, y) in zip(p0.named_parameters(), p1.named_parameters()):
        assert torch.equal(x, y), n                                # weights of one: the step itself
    # td is the mean absolute error of the two critics against the target, the same whatever the weights
    s, a, r, s2, done = S.split_rows(rows, d, A)
    with torch.no_grad():
        a2, lp2 = pol.sample(s2, eps[1])
        y = r + (1 - done) * cfg.gamma * (pol.q_min(s2, a2, target=True) - 1.0 * lp2)
        x = torch.cat([s, a], -1)
        td = 0.5 * ((pol.q1(x).squeeze(-1) - y).abs() + (pol.q2(x).squeeze(-1) - y).abs())
    for st in (s0, s1, sh, sr):
        torch.testing.assert_close(st["td"], td, rtol=1e-5, atol=1e-6)
        assert st["critic_loss"] == s0["critic_loss"]             # the unweighted loss is what is logged
        assert st["ent_coef_loss"] == s0["ent_coef_loss"]         # the entropy loss is not weighted
    assert not torch.equal(pr.q1[0].weight, p0.q1[0].weight) and not torch.equal(ph.q1[0].weight, p0.q1[0].weight)
