"""Shared pieces of the SAC normalisation tests (tests/test_sac_norm_cpu.py, tests/test_sac_norm_gpu.py): statistics that are not the
initial ones, raw observations and batch rows at their scale, and the hand-computed three-row batch."""
import torch

from pyflyt_drone_amd import sac as S

CLIP_OBS, CLIP_REW, EPS = 10.0, 10.0, 1e-8
ACT_NS = (1, 16, 17, 33)                                         # 17 and 33: a ragged last workgroup of 16 rows
ACT_SHAPES = ((21, 6, 256), (30, 3, 64), (64, 8, 64))            # (d, A, H): d = 21 and 30 pad K to 24 and 32
NORM_BS = (16, 272, 576)                                         # rows: one workgroup of 64 partly filled, 4.25 and 9 workgroups
NORM_SHAPES = ((1, 1), (21, 6), (30, 3), (64, 8))                # (d, A)
RET_VAR = 4.0


def stats(d, seed=0):
    """(mean, var) [d] float64 on the CPU: means of order 100, variances in [0.25, 9], and -- for d > 1 -- column 1 with variance 0 (and a
    mean that float32 holds exactly)."""
    g = torch.Generator().manual_seed(500 + seed)
    mean = 100.0 * torch.randn(d, generator=g, dtype=torch.float64)
    var = 0.25 + 8.75 * torch.rand(d, generator=g, dtype=torch.float64)
    if d > 1:
        var[1] = 0.0
        mean[1] = float(mean[1].float())                         # a float32 value: a float32 env can hold exactly its mean
    return mean, var


def raw_obs(n, d, mean, var, seed, dtype=torch.float64, scale=4.0):
    """[n, d] raw observations: mean + scale sqrt(var) N(0, 1) -- with scale 4 about 1 % of the values lie beyond 10 sigma and clip.  The
    zero-variance column holds its mean in the even rows (0 after normalisation) and mean + 1 in the odd ones (the clip)."""
    g = torch.Generator().manual_seed(900 + seed)
    x = mean + scale * torch.sqrt(var) * torch.randn((n, d), generator=g, dtype=torch.float64)
    if d > 1:
        x[1::2, 1] += 1.0
    return x.to(dtype)


def rows(B, d, A, mean, var, seed):
    """[B, 2d + A + 2] float32 batch rows at raw scale: both observation blocks by :func:`raw_obs`, actions uniform in [-1, 1), rewards
    8 N(0, 1) (std of the return 2: about 1 % clip at 10), done with probability 0.2."""
    g = torch.Generator().manual_seed(1300 + seed)
    act = torch.rand((B, A), generator=g) * 2.0 - 1.0
    rew = 8.0 * torch.randn((B, 1), generator=g)
    done = (torch.rand((B, 1), generator=g) < 0.2).float()
    return torch.cat([raw_obs(B, d, mean, var, seed, torch.float32), act, rew, raw_obs(B, d, mean, var, seed + 1, torch.float32), done],
                     dim=1).contiguous()


# ---- the hand-computed batch: d = 3, A = 1, rows [o0 o1 o2 | a | r | n0 n1 n2 | done] ----
# mean (100, 2, 5), var (4, 0, 1): std (2, 1e-4, 1) up to an epsilon of 1e-8 under the root, which moves no float32 result below;
# std of the return sqrt(0.25) = 0.5.
HAND_MEAN, HAND_VAR, HAND_RET_VAR = (100.0, 2.0, 5.0), (4.0, 0.0, 1.0), 0.25
HAND_ROWS = (
    # (102 - 100) / 2 = 1; column 1 at its mean: 0 / 1e-4 = 0; 0.5 / 1 = 0.5 | 1.5 / 0.5 = 3 | -1; 0.5 / 1e-4 = 5000 -> clip 10; -1
    (102.0, 2.0, 5.5, 0.3, 1.5, 98.0, 2.5, 4.0, 0.0),
    # 30 / 2 = 15: beyond 10 sigma -> 10; -0.5 / 1e-4 -> -10; 0 | 7 / 0.5 = 14 -> the reward clips at 10 | 0; 0; 0
    (130.0, 1.5, 5.0, -0.7, 7.0, 100.0, 2.0, 5.0, 1.0),
    # -0.5; 0; -12 -> -10 | -0.25 / 0.5 = -0.5 | 0.5; 0; 1
    (99.0, 2.0, -7.0, 1.0, -0.25, 101.0, 2.0, 6.0, 0.0),
)
HAND_WANT = (
    (1.0, 0.0, 0.5, 0.3, 3.0, -1.0, 10.0, -1.0, 0.0),
    (10.0, -10.0, 0.0, -0.7, 10.0, 0.0, 0.0, 0.0, 1.0),
    (-0.5, 0.0, -10.0, 1.0, -0.5, 0.5, 0.0, 1.0, 0.0),
)


class StubEnv:
    """What sac.SAC reads of an env at construction, on the CPU: enough to build a learner without a device."""

    def __init__(self, num_envs=4, obs_dim=21, act_dim=6):
        self.num_envs, self.obs_dim, self.act_dim = num_envs, obs_dim, act_dim
        self.device, self.torch_dtype = torch.device("cpu"), torch.float64
        self.obs = torch.zeros((num_envs, obs_dim), dtype=torch.float64)
        self.rewards = torch.zeros(num_envs, dtype=torch.float64)
        self.terminated = torch.zeros(num_envs, dtype=torch.uint8)
        self.truncated = torch.zeros(num_envs, dtype=torch.uint8)


def stub_sac(**kw):
    return S.SAC(StubEnv(), S.SACConfig(batch_size=32, net_arch=(64, 64), buffer_size=64, **kw))
