"""Running observation / reward normalisation for SAC (SACConfig.normalize_obs / normalize_reward) without a GPU: the config rules, the
pure-torch restatements of fw_replay_normalize and of the statistics launch, the exported symbols, and what a learner constructs."""
import os
import re

import pytest
import torch

from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R
from pyflyt_drone_amd import sac as S

import sac_norm_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fw_sac_act_norm", "fw_replay_normalize")


def test_the_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "fwsim.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", header), name
    assert K.FW_ABI_VERSION == 7                                 # functions were added, none changed
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name


def test_config_validation():
    c = S.SACConfig()
    assert (c.normalize_obs, c.normalize_reward, c.clip_obs, c.clip_reward, c.norm_epsilon) == (False, False, 10.0, 10.0, 1e-8)
    assert not c.normalizes
    ok = S.SACConfig(normalize_obs=1, normalize_reward=True, clip_obs=5, clip_reward=2.5, norm_epsilon=1e-6)
    assert ok.normalize_obs is True and ok.normalizes and (ok.clip_obs, ok.clip_reward, ok.norm_epsilon) == (5.0, 2.5, 1e-6)
    assert isinstance(ok.clip_obs, float)
    assert S.SACConfig(normalize_reward=True).normalizes and not S.SACConfig(normalize_reward=True).normalize_obs
    for bad in (dict(clip_obs=0.0), dict(clip_obs=-1.0), dict(clip_reward=0.0), dict(clip_reward=float("inf")), dict(norm_epsilon=0.0),
                dict(norm_epsilon=-1e-8), dict(clip_obs=float("nan")), dict(clip_obs="10"), dict(clip_reward=None), dict(norm_epsilon=True)):
        with pytest.raises(ValueError):
            S.SACConfig(**bad)
    # it composes with the three gathers (their own exclusions stay)
    for kw in (dict(prioritized=True), dict(n_steps=3), dict(her_goals=4)):
        assert S.SACConfig(normalize_obs=True, normalize_reward=True, **kw).normalizes


def test_normalize_rows_reference_on_the_hand_computed_batch():
    rows = torch.tensor(NC.HAND_ROWS, dtype=torch.float32)
    mean, var = torch.tensor(NC.HAND_MEAN, dtype=torch.float64), torch.tensor(NC.HAND_VAR, dtype=torch.float64)
    want = torch.tensor(NC.HAND_WANT, dtype=torch.float32)
    got = S.normalize_rows_reference(rows, 3, 1, mean, var, 10.0, 1e-8, torch.tensor(NC.HAND_RET_VAR, dtype=torch.float64), 10.0, 1e-8)
    assert got.dtype == torch.float32 and got is not rows
    torch.testing.assert_close(got, want, rtol=1e-6, atol=0.0)
    assert torch.equal(got[:, 3], rows[:, 3]) and torch.equal(got[:, 8], rows[:, 8])                     # action and done: the input's bits
    for r, c in ((0, 6), (1, 0), (1, 1), (1, 4), (2, 2)):                                                 # the clipped ones sit ON the clip
        assert abs(float(got[r, c])) == 10.0
    assert float(got[0, 1]) == 0.0 and float(got[1, 6]) == 0.0                                            # variance 0 at the mean: exactly 0
    # either half alone leaves the other half's columns as they were
    obs_only = S.normalize_rows_reference(rows, 3, 1, mean, var)
    assert torch.equal(obs_only[:, 4], rows[:, 4]) and torch.equal(obs_only[:, :3], got[:, :3]) and torch.equal(obs_only[:, 5:8], got[:, 5:8])
    rew_only = S.normalize_rows_reference(rows, 3, 1, ret_var=NC.HAND_RET_VAR)
    assert torch.equal(rew_only[:, 4], got[:, 4]) and torch.equal(rew_only[:, :4], rows[:, :4]) and torch.equal(rew_only[:, 5:], rows[:, 5:])
    # a tighter clip
    tight = S.normalize_rows_reference(rows, 3, 1, mean, var, 0.75, 1e-8, NC.HAND_RET_VAR, 2.0, 1e-8)
    assert float(tight[:, :3].abs().max()) == 0.75 and float(tight[:, 4].abs().max()) == 2.0 and float(tight[2, 4]) == -0.5
    with pytest.raises(ValueError):
        S.normalize_rows_reference(rows, 3, 1)
    with pytest.raises(ValueError):
        S.normalize_rows_reference(rows, 3, 1, obs_mean=mean)
    with pytest.raises(ValueError):
        S.normalize_rows_reference(rows, 4, 1, mean, var)
    # the observation expression is VecNormalizeDevice's
    class _Holder:
        obs_rms, epsilon, clip_obs = R.RunningMeanStd((3,), "cpu"), 1e-8, 10.0
    _Holder.obs_rms.mean.copy_(mean); _Holder.obs_rms.var.copy_(var)
    torch.testing.assert_close(R.VecNormalizeDevice._norm_obs_torch(_Holder, rows[:, :3], torch.zeros(3, 3)), got[:, :3], rtol=1e-6, atol=0.0)


def test_the_statistics_reference_against_running_mean_std():
    g = torch.Generator().manual_seed(3)
    d, n = 21, 16
    rms, ret = R.RunningMeanStd((d,), "cpu"), R.RunningMeanStd((), "cpu")
    obs_stats = (rms.mean.clone(), rms.var.clone(), rms.count.clone())
    ret_stats = (ret.mean.clone(), ret.var.clone(), ret.count.clone())
    returns, want_returns = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for k in range(5):
        obs = 100.0 + 30.0 * torch.randn((n, d), generator=g, dtype=torch.float64)
        obs[:, 1] = 7.0                                          # a column that never varies
        rew = torch.randn(n, generator=g, dtype=torch.float64) - 2.0
        ended = torch.rand(n, generator=g) < 0.25
        rms.update(obs)
        want_returns = want_returns * 0.99 + rew
        ret.update(want_returns)
        want_returns = want_returns.masked_fill(ended, 0.0)
        obs_stats, ret_stats, returns = S.stats_step_reference(obs_stats, ret_stats, returns, obs, rew, ended.to(torch.uint8), 0.99)
        for got, ref in zip(obs_stats + ret_stats, (rms.mean, rms.var, rms.count, ret.mean, ret.var, ret.count)):
            torch.testing.assert_close(got.reshape(ref.shape), ref, rtol=1e-12, atol=1e-12)
        assert abs(float(obs_stats[2]) - (1e-4 + n * (k + 1))) < 1e-9 and abs(float(ret_stats[2]) - (1e-4 + n * (k + 1))) < 1e-9
        torch.testing.assert_close(returns, want_returns, rtol=1e-12, atol=0.0)
        assert bool((returns[ended] == 0).all())
    assert float(obs_stats[1][1]) < 1e-3 and abs(float(obs_stats[0][1]) - 7.0) < 1e-3
    # the flags: a half that is off does not move, the returns are still zeroed where an episode ended
    o2, r2, ret2 = S.stats_step_reference(obs_stats, ret_stats, returns + 1.0, obs, rew, torch.ones(n, dtype=torch.uint8), 0.99,
                                          update_obs=False, update_ret=False)
    assert all(torch.equal(a, b) for a, b in zip(o2 + r2, obs_stats + ret_stats)) and not ret2.any()


def test_both_flags_off_construct_nothing_new():
    off = NC.stub_sac()
    assert off.normalizer is None and "normalizer" not in off.state_dict()
    assert off.normalize_batch(off.batch) is off.batch                                    # no launch, the rows untouched
    ev = off.eval_env(NC.StubEnv())
    assert isinstance(ev, R.VecNormalizeDevice) and not ev.norm_obs and not ev.norm_reward and not ev.training
    on = NC.stub_sac(normalize_obs=True, normalize_reward=True, clip_obs=5.0)
    nz = on.normalizer
    assert isinstance(nz, R.VecNormalizeDevice) and nz.venv is on.env and nz.norm_obs and nz.norm_reward and nz.clip_obs == 5.0
    assert nz.obs_rms.mean.dtype == torch.float64 and nz.obs_rms.mean.shape == (21,) and nz.returns.shape == (4,) and nz.gamma == on.cfg.gamma
    assert float(nz.obs_rms.count) == 1e-4 and float(nz.ret_rms.count) == 1e-4
    only_r = NC.stub_sac(normalize_reward=True)
    assert only_r.normalizer is not None and not only_r.normalizer.norm_obs and not only_r.eval_env(NC.StubEnv()).norm_obs
    # the evaluation wrapper reads the learner's own tensors
    ev = on.eval_env(NC.StubEnv())
    assert ev.obs_rms is nz.obs_rms and ev.norm_obs and not ev.norm_reward and not ev.training and ev.clip_obs == 5.0
    with pytest.raises(ValueError):
        on.eval_env(NC.StubEnv(obs_dim=20))


def test_checkpoints_carry_the_statistics_in_place():
    a, b = NC.stub_sac(normalize_obs=True, normalize_reward=True), NC.stub_sac(normalize_obs=True, normalize_reward=True)
    nz = a.normalizer
    nz.obs_rms.mean.normal_(); nz.obs_rms.var.uniform_(0.5, 2.0); nz.obs_rms.count.fill_(48.0001)
    nz.ret_rms.mean.fill_(-3.0); nz.ret_rms.var.fill_(2.5); nz.ret_rms.count.fill_(32.0001); nz.returns.normal_()
    sd = a.state_dict()
    assert set(sd["normalizer"]) == {"obs_rms", "ret_rms", "returns"} and sd["config"]["normalize_obs"] is True
    ptrs = [t.data_ptr() for t in (b.normalizer.obs_rms.mean, b.normalizer.obs_rms.var, b.normalizer.obs_rms.count, b.normalizer.returns)]
    b.load_state_dict(sd)
    m = b.normalizer
    assert ptrs == [t.data_ptr() for t in (m.obs_rms.mean, m.obs_rms.var, m.obs_rms.count, m.returns)]       # copied in place
    for x, y in ((m.obs_rms.mean, nz.obs_rms.mean), (m.obs_rms.var, nz.obs_rms.var), (m.obs_rms.count, nz.obs_rms.count),
                 (m.ret_rms.mean, nz.ret_rms.mean), (m.ret_rms.var, nz.ret_rms.var), (m.ret_rms.count, nz.ret_rms.count), (m.returns, nz.returns)):
        assert torch.equal(x, y)
    # a checkpoint without statistics still loads and leaves them as they are; a plain learner ignores a checkpoint's statistics
    before = m.obs_rms.mean.clone()
    b.load_state_dict(NC.stub_sac().state_dict())
    assert torch.equal(m.obs_rms.mean, before)
    NC.stub_sac().load_state_dict(sd)
