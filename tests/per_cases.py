"""Shared pieces of the prioritized-replay tests (tests/test_sac_per_cpu.py, tests/test_sac_per_gpu.py): three scripted rings of 4
envs and rows of 50 floats with their priority leaves, the first Philox word of every batch row as the gather kernels draw it, and the
statistics of a set of draws against the probabilities the leaves state.

  S   64 rows, 40 filled (one ragged level-1 group; the rows behind the fill have leaves of 0)
  M   1024 rows, wrapped, the cursor in mid-ring (four full level-1 groups)
  L   66 048 rows = 258 level-1 groups, so level 2 has two entries, the second one ragged; 66 000 filled; leaves uniform in [0.01, 1],
      2000 random ones set to 0 and 48 random ones to 500: those 48 hold about 43 % of the mass
"""
import numpy as np

import device_reference as R

N_ENVS, D, A, ROW = 4, 21, 6, 50
SAMPLE_TAG = 0x5AC0C000                      # kSacTagSample (csrc/fwsim_sac.hpp)
RINGS = {"S": dict(capacity=64, filled=40, cursor=40), "M": dict(capacity=1024, filled=1024, cursor=512),
         "L": dict(capacity=66048, filled=66000, cursor=66000)}
L_ZEROS, L_HOT, HOT_LEAF = 2000, 48, 500.0
U = 2.0 ** -24                               # unit roundoff of float32

# The weighted update-parity cases: the shapes and seeds of tests/sac_cases.py and the smallest wide shape, each with weights uniform in
# [0.05, 1] from torch's generator under WEIGHT_SEED_BASE + seed.  The rule of tests/sac_wide_cases.py holds here too: an input on which
# a float32 step can take the other side of a ReLU mask, of min(Q1, Q2) or of the log_std clamp tells nothing about the kernel, its seed
# is replaced by the next integer, the change is recorded here, and the tolerance is never touched.
# Replaced so far: (21, 6, 256, 64) seed 5 with weight seed 305.  In its second step the actor's second hidden layer has, in row 58,
# unit 227, a pre-activation of -7.8e-7 in float64 (-3.0e-6 in the float32 torch step): a 256-term float32 dot product in another
# summation order lands on either side of zero, and the product kernel gets +2.1e-6, so that unit's ReLU passes in one step and not in
# the other.  Every other mask, every min(Q1, Q2) choice and every clamp side agree in all three steps, and so do the critics (worst
# |diff| / bound 0.001); the one unit moves two elements of actor.0.weight out of the parameter tolerance after the third step (worst
# |diff| 8.5e-5) and an Adam moment to 191 bounds.  With weight seed 306 the same shape and seed agree at 0.036 of the bounds.  On an
# MI355X, over the five shapes, both seeds and weight seeds 300 to 305 (+ seed), the worst |diff| / bound of the kernel against the
# float64 torch step is at most 0.38 after 1 and 3 steps in 58 of 60 combinations; the other two are this one and one (weight seed
# 302 + 5 at (28, 4, 256, 256): 4.3 bounds) on which the float32 torch step sides with the kernel (0.04) and leaves the float64 step
# by the same 4.3 bounds.  That one is not among the cases.
WEIGHT_SEED_BASE = 300
WEIGHT_SEEDS_REPLACED = {(21, 6, 256, 64, 5): 306}


def weights(d, A, H, B, seed):
    """The case's importance weights [B] float32 (CPU), uniform in [0.05, 1]."""
    import torch
    ws = WEIGHT_SEEDS_REPLACED.get((d, A, H, B, seed), WEIGHT_SEED_BASE + seed)
    return torch.rand(B, generator=torch.Generator().manual_seed(ws)) * 0.95 + 0.05


def leaves(name):
    """The leaves [capacity] float32 of a scripted ring (and, for L, the indices of its hot rows)."""
    c = RINGS[name]
    rng = np.random.default_rng({"S": 11, "M": 12, "L": 13}[name])
    prio = np.zeros(c["capacity"], dtype=np.float32)
    prio[:c["filled"]] = rng.uniform(0.01, 1.0, c["filled"]).astype(np.float32)
    hot = np.zeros(0, dtype=np.int64)
    if name == "S":
        prio[[3, 17]] = 0.0                  # (a zero leaf inside the fill: a row whose update was skipped)
    if name == "L":
        pick = rng.permutation(c["filled"])[:L_ZEROS + L_HOT]
        prio[pick[:L_ZEROS]] = 0.0
        hot = np.sort(pick[L_ZEROS:])
        prio[hot] = HOT_LEAF
    return prio, hot


def rows(name, row=ROW):
    """Ring rows [capacity, row] float32 that tell their own index: column 0 is the row number, the rest is noise."""
    c = RINGS[name]
    rng = np.random.default_rng(100 + c["capacity"] + row)
    ring = rng.standard_normal((c["capacity"], row)).astype(np.float32)
    ring[:, 0] = np.arange(c["capacity"], dtype=np.float32)
    return ring


def counters(name, grad=0):
    c = RINGS[name]
    return [c["cursor"] % c["capacity"], c["filled"], max(c["filled"] // N_ENVS, 1), grad]


def words(seed, grad_step, batch):
    """o[0] [batch] (uint64 holding uint32 values) of the batch rows' Philox block at gradient step `grad_step`: fw_replay_sample's
    block, which fw_replay_sample_per shares.  From the numpy Philox of tests/device_reference.py."""
    b = np.arange(batch, dtype=np.uint64)
    key = np.tile(np.array([[seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]], dtype=np.uint64), (batch, 1))
    ctr = np.stack([b, np.zeros_like(b), np.full_like(b, grad_step & 0xFFFFFFFF),
                    np.full_like(b, ((grad_step >> 32) & 0xFFFFFFFF) ^ SAMPLE_TAG)], axis=1)
    return R.philox4x32_10(ctr, key).astype(np.uint64)[:, 0]


def worst_z(idx, prio, hot):
    """(worst |z| over the hot rows, worst |z| over the level-1 groups' counts of the remaining rows) of the draws `idx` against the
    probabilities q = leaf / sum(leaves) in float64: z = (count - M q) / sqrt(M q (1 - q))."""
    M = len(idx)
    p = prio.astype(np.float64)
    total = p.sum()
    count = np.bincount(idx, minlength=prio.size).astype(np.float64)

    def z(c, q):
        keep = q > 0
        return np.abs((c[keep] - M * q[keep]) / np.sqrt(M * q[keep] * (1.0 - q[keep])))

    z_hot = z(count[hot], p[hot] / total) if len(hot) else np.zeros(1)
    rest_p, rest_c = p.copy(), count.copy()
    rest_p[hot] = 0.0; rest_c[hot] = 0.0
    n1 = -(-prio.size // 256)
    pad = n1 * 256 - prio.size
    gp = np.pad(rest_p, (0, pad)).reshape(n1, 256).sum(1) / total
    gc = np.pad(rest_c, (0, pad)).reshape(n1, 256).sum(1)
    return float(z_hot.max()), float(z(gc, gp).max())
