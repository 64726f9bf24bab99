"""PPO training diagnostics (PPOConfig.diagnostics) without a device: the torch path against a plain re-statement of SB3's
PPO.train() figures, the flag-off twin, the two multi-process modes over gloo, and the argument errors of fw_ppo_update_diag /
fw_ppo_diag_floats through the C ABI."""
import copy
import ctypes as C
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mp_diag_jobs as J  # noqa: E402

from pyflyt_drone_amd import config as K  # noqa: E402
from pyflyt_drone_amd import rollout as R  # noqa: E402

SERIES = ("approx_kl", "clip_fraction", "policy_loss", "value_loss", "entropy_loss")
SCALARS = ("train/approx_kl", "train/clip_fraction", "train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/loss",
           "train/explained_variance", "train/std", "train/n_updates", "train/clip_range", "train/learning_rate")


def _sb3_train(policy, opt, cfg, obs, act, old_logp, adv, ret, perm_gen):
    """SB3's PPO.train() on a copy of the policy: its losses and logger records, minibatch by minibatch (the formulas of
    stable_baselines3/ppo/ppo.py, written out), with an optimiser and a permutation stream of its own."""
    B = obs.shape[0]
    out = {k: [] for k in SERIES}
    loss = None
    for _ in range(cfg.n_epochs):
        perm = torch.randperm(B, generator=perm_gen)
        for s in range(0, B, cfg.batch_size):
            idx = perm[s:s + cfg.batch_size]
            advantages = adv[idx]
            advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
            values, log_prob, entropy = policy.evaluate_actions(obs[idx], act[idx])
            ratio = torch.exp(log_prob - old_logp[idx])
            policy_loss_1 = advantages * ratio
            policy_loss_2 = advantages * torch.clamp(ratio, 1 - cfg.clip_range, 1 + cfg.clip_range)
            policy_loss = -torch.min(policy_loss_1, policy_loss_2).mean()
            clip_fraction = torch.mean((torch.abs(ratio - 1) > cfg.clip_range).float()).item()
            value_loss = torch.nn.functional.mse_loss(ret[idx], values)
            entropy_loss = -torch.mean(entropy)
            loss = policy_loss + cfg.ent_coef * entropy_loss + cfg.vf_coef * value_loss
            with torch.no_grad():
                log_ratio = log_prob - old_logp[idx]
                approx_kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio).item()
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(policy.parameters(), cfg.max_grad_norm)
            opt.step()
            for k, v in zip(SERIES, (approx_kl, clip_fraction, policy_loss.item(), value_loss.item(), entropy_loss.item())):
                out[k].append(v)
    return {k: np.array(v, dtype=np.float64) for k, v in out.items()}, float(loss.item())


@pytest.mark.parametrize("d,a,bs", [(28, 4, 128), (21, 6, 64), (30, 3, 256)])
def test_torch_path_series_and_scalars_equal_the_sb3_restatement(d, a, bs):
    ppo = J.filled_ppo(d, a, bs, 2, diagnostics=True)
    cfg = ppo.cfg
    twin = copy.deepcopy(ppo.policy)
    opt = torch.optim.Adam(twin.parameters(), lr=cfg.learning_rate, eps=1e-5)
    B = 4 * 256
    bufs = (ppo.buf_obs.reshape(B, -1).clone(), ppo.buf_act.reshape(B, -1).clone(), ppo.buf_logp.reshape(B).clone(),
            ppo.adv.reshape(B).clone(), ppo.ret.reshape(B).clone())
    perm_gen = torch.Generator().manual_seed(cfg.seed)          # the twin of PPO.gen, which draws the permutations
    n_mb = 2 * B // bs
    for call in range(2):                                       # the second call: the buffers are re-zeroed, the counters go on
        want, last_loss = _sb3_train(twin, opt, cfg, *bufs, perm_gen)
        ppo.train()
        assert set(ppo.diagnostic_series) == set(SERIES) and set(ppo.diagnostics) == set(SCALARS)
        for k in SERIES:
            got = ppo.diagnostic_series[k]
            assert got.dtype == np.float64 and got.shape == (n_mb,)
            np.testing.assert_allclose(got, want[k], rtol=1e-6, atol=0, err_msg=f"{k}, call {call}")
        s = ppo.diagnostics
        assert s["train/approx_kl"] == pytest.approx(want["approx_kl"].mean(), rel=1e-6)
        assert s["train/clip_fraction"] == pytest.approx(want["clip_fraction"].mean(), rel=1e-6)
        assert s["train/policy_gradient_loss"] == pytest.approx(want["policy_loss"].mean(), rel=1e-6)
        assert s["train/value_loss"] == pytest.approx(want["value_loss"].mean(), rel=1e-6)
        assert s["train/entropy_loss"] == pytest.approx(want["entropy_loss"].mean(), rel=1e-6)
        assert s["train/loss"] == pytest.approx(last_loss, rel=1e-6)
        assert s["train/std"] == pytest.approx(float(torch.exp(twin.log_std.detach()).mean()), rel=1e-6)
        assert s["train/n_updates"] == 2 * (call + 1) and s["train/clip_range"] == cfg.clip_range
        assert s["train/learning_rate"] == cfg.learning_rate
        y, v = bufs[4].numpy().astype(np.float64), ppo.buf_val.reshape(-1).numpy().astype(np.float64)
        assert s["train/explained_variance"] == pytest.approx(1.0 - np.var(y - v) / np.var(y), rel=1e-12, abs=1e-12)
        # about a third of the samples sit outside the clip range: the figures are not trivially zero
        assert 0.1 < want["clip_fraction"][0] < 0.6 and want["approx_kl"][0] > 1e-3
        # the five keys of PPO.logs are what they were
        assert set(ppo.logs) == {"policy_loss", "value_loss", "entropy_loss", "adv_mean", "adv_std"}
        assert ppo.logs["policy_loss"] == pytest.approx(want["policy_loss"].mean(), rel=1e-5, abs=1e-7)
    for p, q in zip(ppo.policy.parameters(), twin.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-8)
    pe = R.per_epoch(ppo.diagnostic_series, 2)
    assert pe["approx_kl"].shape == (2,)
    np.testing.assert_allclose(pe["approx_kl"][1], ppo.diagnostic_series["approx_kl"][n_mb // 2:].mean(), rtol=1e-12)
    with pytest.raises(ValueError):
        R.per_epoch(ppo.diagnostic_series, n_mb + 1)


def test_explained_variance_definition_and_nan():
    rng = np.random.default_rng(0)
    y, v = rng.normal(size=1000) * 3, rng.normal(size=1000)
    assert R.explained_variance(v.astype(np.float32), y.astype(np.float32)) == pytest.approx(
        1.0 - np.var(y.astype(np.float32).astype(np.float64) - v.astype(np.float32).astype(np.float64)) / np.var(y.astype(np.float32).astype(np.float64)),
        rel=1e-12)
    assert R.explained_variance(y, y) == 1.0
    assert math.isnan(R.explained_variance(v, np.full(1000, 2.5)))
    # ... and through train(): constant returns give NaN, everything else stays finite
    ppo = J.filled_ppo(12, 4, 64, 1, T=2, n=64, diagnostics=True)
    ppo.ret = torch.full_like(ppo.ret, 1.25)
    ppo.train()
    assert math.isnan(ppo.diagnostics["train/explained_variance"])
    assert all(math.isfinite(x) for k, x in ppo.diagnostics.items() if k != "train/explained_variance")


def _state(ppo):
    out = [p.detach().clone() for p in ppo.policy.parameters()]
    for p in ppo.policy.parameters():
        st = ppo.optimizer.state[p]
        out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone(), torch.as_tensor(float(st["step"]))]
    return out


def test_flag_off_is_the_learner_of_before_and_flag_on_moves_nothing_else():
    never = J.filled_ppo(28, 4, 128, 2)                                   # a twin that never heard of the flag
    off = J.filled_ppo(28, 4, 128, 2, diagnostics=False)
    on = J.filled_ppo(28, 4, 128, 2, diagnostics=True)
    assert R.PPOConfig().diagnostics is False
    for _ in range(2):
        for p in (never, off, on):
            p.train()
        assert off.diagnostics == {} and off.diagnostic_series == {} and never.diagnostics == {}
        assert off._diag_buf is None
        assert never.logs == off.logs == on.logs and list(off.logs) == ["policy_loss", "value_loss", "entropy_loss", "adv_mean", "adv_std"]
    for x, y, z in zip(_state(never), _state(off), _state(on)):
        assert torch.equal(x, y) and torch.equal(x, z)


def _two_ranks(dist_update):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = [ctx.Process(target=J.diag_rank, args=(r, 2, port, q, dist_update)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60); assert p.exitcode == 0
    return [r[1] for r in res]


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


def test_replicated_ranks_report_identical_diagnostics_without_a_collective():
    a, b = _two_ranks("replicated")
    assert a["replicated"] and b["replicated"]
    assert a["reduces"] == b["reduces"] == 0                             # no collective was added
    assert _same(a["scalars"], b["scalars"]) and _same(a["series"], b["series"]) and _same(a["first"], b["first"])
    assert np.array_equal(a["weights"], b["weights"])
    assert set(a["scalars"]) == set(SCALARS) and a["series"]["approx_kl"].shape == (2 * (2 * 2 * 64) // 32,)
    assert a["scalars"]["train/n_updates"] == 4 and a["first"]["train/n_updates"] == 2
    # the explained variance is that of the gathered rollout (ret - adv of both shards), not of a rank's own
    ret = np.concatenate([a["ret"], b["ret"]]); adv = np.concatenate([a["adv"], b["adv"]])
    y, v = ret.astype(np.float64), (ret - adv).astype(np.float64)
    assert a["scalars"]["train/explained_variance"] == pytest.approx(1.0 - np.var(y - v) / np.var(y), rel=1e-9)
    assert a["scalars"]["train/explained_variance"] != pytest.approx(a["local_ev"], rel=1e-6)


def test_allreduce_ranks_report_the_rank_mean_from_one_all_reduce():
    a, b = _two_ranks("allreduce")
    assert not a["replicated"] and not b["replicated"]
    assert a["reduces"] == b["reduces"] == 2 and len(a["sent"]) == 2     # one all-reduce per train()
    assert _same(a["scalars"], b["scalars"]) and _same(a["series"], b["series"])
    n = 2 * (2 * 64) // 32
    mean = (a["sent"][1] + b["sent"][1]) / 2
    assert not np.array_equal(a["sent"][1], b["sent"][1])                # the ranks walked different minibatches
    for i, k in enumerate(SERIES):
        assert a["series"][k].shape == (n,)
        np.testing.assert_allclose(a["series"][k], mean[i * n:(i + 1) * n], rtol=1e-15)
    assert a["scalars"]["train/approx_kl"] == pytest.approx(mean[:n].mean(), rel=1e-12)
    assert a["scalars"]["train/explained_variance"] == pytest.approx((a["local_ev"] + b["local_ev"]) / 2, rel=1e-12)
    assert np.array_equal(a["weights"], b["weights"])


def test_diag_floats_and_argument_errors_through_the_c_abi():
    from pyflyt_drone_amd import _lib
    L = _lib.lib()                              # (loads without a device; a missing or stale library is a failure, not a skip)
    assert L.fw_ppo_diag_floats(1) == 2 * 8 * 4 * 4
    assert L.fw_ppo_diag_floats(10240) == 10240 * 256
    for bad in (0, -3):
        assert L.fw_ppo_diag_floats(bad) == K.FW_EINVAL
    one = C.c_void_p(16)                        # (a non-NULL address: the checks below return before anything is read)
    H = R._PpoHyper()
    ok_tail = (C.byref(H), None, one, 1 << 40, None)

    def call(act_dim, diag, diag_floats, n_mb=4, ptr=one):
        return L.fw_ppo_update_diag(*([ptr] * 9), n_mb, 64, 21, act_dim, *ok_tail, diag, diag_floats)
    for a in (0, 1, 2, 5, 7, 8, -4):
        assert call(a, one, 1 << 30) == K.FW_EINVAL
        assert "act_dim must be 3, 4 or 6" in L.fw_last_error(None).decode()
    for a in (3, 4, 6):
        assert call(a, None, 1 << 30) == K.FW_EINVAL and "diag is NULL" in L.fw_last_error(None).decode()
        assert call(a, one, 4 * 256 - 1) == K.FW_EINVAL and "fw_ppo_diag_floats" in L.fw_last_error(None).decode()
        assert call(a, one, 0) == K.FW_EINVAL
        for n_mb in (0, -1):
            assert call(a, one, 1 << 30, n_mb=n_mb) == K.FW_EINVAL and "n_minibatches must be positive" in L.fw_last_error(None).decode()
        # with a good diagnostics buffer the call goes on to the checks of the plain entry point
        assert call(a, one, 4 * 256, ptr=None) == K.FW_EINVAL and "fw_ppo_update_diag: bad arguments" in L.fw_last_error(None).decode()
