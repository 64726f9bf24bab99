"""PPO training diagnostics on the device: fw_ppo_update_diag against the plain entry points (nothing else moves), its arithmetic
against a float64 reference with the learning rate pinned to zero, the fused learner against the torch path, the three collectors
end to end, and what a second or a failed train() leaves behind.

Tolerances.  Losses and approx_kl: the project's fused-against-torch tolerance for logged losses (rel 2e-3, abs 1e-5:
tests/test_rollout_gpu.py).  Clip fraction: a bracket, not a tolerance -- DELTA below is 8 x the largest difference between the
log-ratio of a float32 torch forward and of a float64 one over the test buffers (measured by the test itself and printed)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mp_diag_jobs as J  # noqa: E402

import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import rollout as R  # noqa: E402

pytestmark = pytest.mark.gpu

SERIES = ("approx_kl", "clip_fraction", "policy_loss", "value_loss", "entropy_loss")
REL, ABS = 2e-3, 1e-5                     # fused against torch, logged losses
# the means over an update, fused against torch: both paths move their parameters (they agree to rtol 2e-3 after an update,
# tests/test_rollout_gpu.py), so later minibatches see slightly different policies; see test 7 and DESIGN section 4b
MEAN_REL, MEAN_ABS = 2e-3, 1e-5
# entropy_loss, the whole series, fused against torch with a real learning rate.  The entry is -sum_k (0.5 + 0.5 ln 2 pi + log_std_k),
# 4.3 to 8.5 here, where one float32 ulp is 4.8e-7 to 9.5e-7.  Both paths start from the same log_std and move it by Adam steps of
# about lr = 3e-4 each, whose inputs differ by the summation order of a float32 gradient; 1e-5 leaves ten to twenty ulps for that.
# A kernel that read log_std one Adam step late would be off by about lr on every log_std that moved: thirty times this tolerance.
ENT_ABS = 1e-5
BAND_MAX = 4                              # samples of the 1024 allowed inside the clip band (the precondition of the bracket)

CUTS = [(16, None), (32, None), (64, None), (128, None), (256, None), (512, "64x8"), (128, "all-to-all"), (128, "32x4")]
CASES = [(d, a, bs, split) for bs, split in CUTS for d, a in ((28, 4), (21, 6), (30, 3))] + [(5, 4, 64, None), (64, 4, 64, None)]
IDS = [f"{d}-{a}-{bs}-{split or 'default'}" for d, a, bs, split in CASES]


def _set_cut(monkeypatch, split):
    if split == "all-to-all":
        monkeypatch.setenv("FWSIM_PPO_RS", "0")
    elif split is not None:
        monkeypatch.setenv("FWSIM_PPO_SPLIT", split)


def _nsplit(bs, split):
    """blocks per network of the cut the library chooses (ppo_split in csrc/fwsim_ppo.hpp), or of the forced one"""
    if split not in (None, "all-to-all"):
        return int(split.split("x")[1])
    max_blocks = 4 if split == "all-to-all" else 8

    def cut(ch):
        c = bs // ch
        return ch, (8 if c >= 8 and max_blocks >= 8 else 4 if c >= 4 else 2 if c >= 2 else 1)

    def cost(s):
        ch, ns = s
        return ((bs // ch + ns - 1) // ns) * {64: 10, 32: 6, 16: 4}[ch] + (1 if ns == 2 else 0)
    best = cut(16)
    if bs % 32 == 0 and cost(cut(32)) <= cost(best):
        best = cut(32)
    if bs % 64 == 0 and cost(cut(64)) <= cost(best):
        best = cut(64)
    return best[1]


def _ppo(d, a, bs, fused=True, diag=True, **cfg):
    return J.filled_ppo(d, a, bs, 2, device="cuda", fused_update=fused, fused_six_actions=True, fused_three_actions=True,
                        diagnostics=diag, **cfg)


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("d,a,bs,split", CASES, ids=IDS)
def test_the_diagnostics_kernel_moves_nothing_else(d, a, bs, split, monkeypatch):
    """fw_ppo_update_diag and the plain entry point of the width on identical inputs: parameters, both moment images and loss_acc
    bit for bit, status 0 (a non-zero status raises)."""
    _set_cut(monkeypatch, split)
    x, y = _ppo(d, a, bs, diag=True), _ppo(d, a, bs, diag=False)
    for call in range(2):
        x.train(); y.train()
        torch.cuda.synchronize()
        assert x._fused is not None and y._fused is not None and x._fused.A == a
        assert x._fused.diag_series is not None and y._fused.diag_series is None and y._fused._diag is None
        for name in ("flat", "mom_m", "mom_v", "loss"):
            assert torch.equal(getattr(x._fused, name), getattr(y._fused, name)), f"{name}, call {call}"
        assert x.logs == y.logs and y.diagnostics == {}
    for p, q in zip(x.policy.parameters(), y.policy.parameters()):
        assert torch.equal(p, q)


# ---------------------------------------------------------------------------------------------------------------- 6
def _reference_lr0(ppo, perm, bs):
    """Per-minibatch figures in float64 from the initial weights alone (the learning rate is zero), and the per-sample |ratio - 1|
    with the measured float32-against-float64 difference of the log-ratio."""
    cfg = ppo.cfg
    B = perm.numel() // cfg.n_epochs
    obs, act = ppo.buf_obs.reshape(B, -1), ppo.buf_act.reshape(B, -1)
    old, adv, ret = ppo.buf_logp.reshape(B), ppo.adv.reshape(B), ppo.ret.reshape(B)
    import copy
    p64 = copy.deepcopy(ppo.policy).double()
    with torch.no_grad():
        v64, lp64, ent64 = p64.evaluate_actions(obs.double(), act.double())
        _, lp32, _ = ppo.policy.evaluate_actions(obs, act)
        lr64 = lp64 - old.double()
        measured = float(((lp32 - old).double() - lr64).abs().max())
        ratio = torch.exp(lr64)
        out = {k: [] for k in SERIES}
        for m in range(perm.numel() // bs):
            idx = perm[m * bs:(m + 1) * bs].long()
            A = adv[idx].double()
            A = (A - A.mean()) / (A.std() + 1e-8)
            r = ratio[idx]
            out["approx_kl"].append(float(((r - 1) - lr64[idx]).mean()))
            out["policy_loss"].append(float(-torch.min(A * r, A * r.clamp(1 - cfg.clip_range, 1 + cfg.clip_range)).mean()))
            out["value_loss"].append(float(((ret[idx].double() - v64[idx]) ** 2).mean()))
            out["entropy_loss"].append(float(-ent64[idx].mean()))
    return {k: np.array(v) for k, v in out.items()}, (ratio - 1).abs().cpu().numpy(), measured


@pytest.mark.parametrize("d,a,bs,split", CASES, ids=IDS)
def test_the_arithmetic_with_the_learning_rate_pinned_to_zero(d, a, bs, split, monkeypatch):
    _set_cut(monkeypatch, split)
    ppo = _ppo(d, a, bs, learning_rate=0.0)
    clip = ppo.cfg.clip_range
    B = 4 * 256
    g = torch.Generator(device="cuda"); g.manual_seed(ppo.cfg.seed)             # the twin of PPO.gen
    perm = torch.cat([torch.randperm(B, device="cuda", generator=g) for _ in range(2)])
    before = [p.detach().clone() for p in ppo.policy.parameters()]
    want, dist, measured = _reference_lr0(ppo, perm, bs)
    delta = 8.0 * measured
    band = int((np.abs(dist - clip) <= delta).sum())
    print(f"\n[diag lr0] case {d}-{a}-{bs}-{split}: max |log-ratio f32 - f64| = {measured:.3e}, delta = {delta:.3e}, samples in the band: {band}")
    assert band <= BAND_MAX, "the bracket of the clip fraction is not tight for these buffers (choose another seed)"
    ppo.train()
    torch.cuda.synchronize()
    for p, q in zip(ppo.policy.parameters(), before):
        assert torch.equal(p, q)                                                 # (nothing moved: the reference holds for every minibatch)
    got = ppo.diagnostic_series
    n_mb = 2 * B // bs
    for k in ("approx_kl", "policy_loss", "value_loss", "entropy_loss"):
        err = np.abs(got[k] - want[k])
        print(f"[diag lr0]   {k}: max abs diff {err.max():.3e}, max rel diff {(err / np.maximum(np.abs(want[k]), 1e-30)).max():.3e}")
        assert got[k].shape == (n_mb,)
        np.testing.assert_allclose(got[k], want[k], rtol=REL, atol=ABS, err_msg=k)
    pm = perm.cpu().numpy()
    for m in range(n_mb):
        dm = dist[pm[m * bs:(m + 1) * bs]]
        lo, hi = int((dm > clip + delta).sum()), int((dm > clip - delta).sum())
        count = got["clip_fraction"][m] * bs
        assert abs(count - round(count)) < 1e-3 and lo <= round(count) <= hi, (m, lo, count, hi)
    # the buffer itself: rows of the parts this cut does not use are as the caller zeroed them, every wave of the others wrote
    ns = _nsplit(bs, split)
    raw = ppo._fused._diag[:n_mb * 256].view(n_mb, 2, 8, 4, 4).cpu().numpy()
    assert (raw[:, :, ns:] == 0).all()
    assert (raw[:, 1, :ns, :, 0] > 0).all() and (raw[:, 1, :, :, 1:] == 0).all()       # value rows: the squared error of every wave's samples
    ent = raw[:, 0, :, :, 3]
    assert (ent[:, 0, 0] != 0).all() and np.count_nonzero(ent) == n_mb                # the entropy loss: part 0, wave 0 only
    assert (raw[:, 0, :ns, :, 2] * bs == np.round(raw[:, 0, :ns, :, 2] * bs)).all()    # clipped counts are whole numbers


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("d,a,bs,split", CASES, ids=IDS)
def test_fused_diagnostics_against_the_torch_path(d, a, bs, split, monkeypatch):
    _set_cut(monkeypatch, split)
    x, y = _ppo(d, a, bs, fused=True), _ppo(d, a, bs, fused=False)
    x.train(); y.train()
    torch.cuda.synchronize()
    assert x._fused is not None and y._fused is None
    sx, sy = x.diagnostic_series, y.diagnostic_series
    for k in SERIES:
        if k == "clip_fraction":              # at most BAND_MAX samples of the buffer sit where float32 rounding decides (test 6)
            assert abs(sx[k][0] - sy[k][0]) * bs <= BAND_MAX
        else:
            assert sx[k][0] == pytest.approx(sy[k][0], rel=REL, abs=ABS), k
    # the entropy loss of every minibatch is taken at the log_std its forward used, before its Adam step
    ent = np.abs(sx["entropy_loss"] - sy["entropy_loss"])
    print(f"\n[diag fused-vs-torch] case {d}-{a}-{bs}-{split}: entropy_loss series, max abs diff {ent.max():.3e} (at minibatch {int(ent.argmax())})")
    assert sx["entropy_loss"].shape == sy["entropy_loss"].shape == (2 * 4 * 256 // bs,)
    assert not np.array_equal(sy["entropy_loss"][1:], sy["entropy_loss"][:-1])          # (log_std moves: a late read would show)
    np.testing.assert_allclose(sx["entropy_loss"], sy["entropy_loss"], rtol=0, atol=ENT_ABS)
    worst = {}
    for k in ("train/approx_kl", "train/clip_fraction", "train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/loss",
              "train/std"):
        worst[k] = (abs(x.diagnostics[k] - y.diagnostics[k]), abs(x.diagnostics[k] - y.diagnostics[k]) / max(abs(y.diagnostics[k]), 1e-30))
    print(f"\n[diag fused-vs-torch] case {d}-{a}-{bs}-{split}: " + ", ".join(f"{k[6:]} abs {v[0]:.3e} rel {v[1]:.3e}" for k, v in worst.items()))
    for k in worst:
        assert x.diagnostics[k] == pytest.approx(y.diagnostics[k], rel=MEAN_REL, abs=MEAN_ABS), k
    assert x.diagnostics["train/explained_variance"] == y.diagnostics["train/explained_variance"]
    for k in ("train/n_updates", "train/clip_range", "train/learning_rate"):
        assert x.diagnostics[k] == y.diagnostics[k]
    assert set(x.logs) == {"policy_loss", "value_loss", "entropy_loss", "adv_mean", "adv_std"}


def test_torch_path_under_the_captured_update_graph():
    """The torch path books its rows through a device-side counter: the replayed graph fills the same series as the eager loop.
    (The two differ in Adam's implementation -- capturable or not -- so later minibatches agree to fp32 rounding accumulated over
    the steps, the first one exactly.)"""
    x, y = _ppo(28, 4, 256, fused=False, use_graphs=True), _ppo(28, 4, 256, fused=False, use_graphs=False)
    for call in range(2):
        x.train(); y.train()
        torch.cuda.synchronize()
        assert x._g_update is not None and y._g_update is None
        for k in SERIES:
            assert x.diagnostic_series[k].shape == (8,)
            if call == 0:
                assert x.diagnostic_series[k][0] == pytest.approx(y.diagnostic_series[k][0], rel=1e-6, abs=1e-9), k
            np.testing.assert_allclose(x.diagnostic_series[k], y.diagnostic_series[k], rtol=1e-4, atol=1e-6, err_msg=k)
        assert x.diagnostics["train/n_updates"] == 2 * (call + 1)


def test_the_captured_update_graph_follows_the_flag_when_it_changes():
    """The captured step books a row or not as the flag stood at capture: switching the flag captures anew.  On, off, on again: the
    off update writes no row (and nothing past the buffer's end), and every update is the one of a twin whose flag never changed."""
    x, on, off = (_ppo(28, 4, 256, fused=False, use_graphs=True, diag=f) for f in (True, True, False))
    for call, flag in enumerate((True, False, True)):
        x.cfg.diagnostics = flag
        for p in (x, on, off):
            p.train()
        torch.cuda.synchronize()
        assert x._g_update is not None and x._g_update_diag == flag
        assert x.logs == on.logs == off.logs
        if flag:
            assert int(x._diag_i) == 8 and x.diagnostics == on.diagnostics
            for k in SERIES:
                assert np.array_equal(x.diagnostic_series[k], on.diagnostic_series[k]), (call, k)
        else:
            assert int(x._diag_i) == 8 and x.diagnostics == off.diagnostics == {}      # (the counter stands where the last booked update left it)
            assert x.diagnostic_series == {}
    for p, q in zip(x.policy.parameters(), off.policy.parameters()):
        assert torch.equal(p, q)


def test_cnn_detector_policy_books_its_rows_through_the_captured_graph():
    from pyflyt_drone_amd import config as K
    env = R.VecNormalizeDevice(P.FixedwingVecEnv(K.train_waypoint_objlock_config(), 64, seed=11))
    ppo = R.PPO(env, R.PPOConfig(n_steps=8, batch_size=128, n_epochs=2, detector="cnn", image_res=32, seed=5, diagnostics=True))
    assert isinstance(ppo.policy, R.CnnDetectorPolicy) and ppo._fused is None and ppo._graphs
    for call in range(2):
        ppo.collect_rollouts(); ppo.train()
        torch.cuda.synchronize()
        assert ppo._g_update is not None
        s, series = ppo.diagnostics, ppo.diagnostic_series
        assert all(v.shape == (8,) and np.isfinite(v).all() for v in series.values()) and set(series) == set(SERIES)
        assert all(math.isfinite(v) for v in s.values()), s
        # a fresh rollout's first minibatch: the policy is the one that sampled it (torch collector and torch update: fp32 rounding)
        assert abs(series["approx_kl"][0]) < 1e-6 and series["clip_fraction"][0] == 0.0
        assert (series["approx_kl"][1:] > 0).all() and s["train/n_updates"] == 2 * (call + 1)
        yv, v = ppo.ret.reshape(-1).double().cpu().numpy(), ppo.buf_val.reshape(-1).double().cpu().numpy()
        assert s["train/explained_variance"] == pytest.approx(1.0 - np.var(yv - v) / np.var(yv), rel=1e-6, abs=1e-6)
        assert s["train/policy_gradient_loss"] == pytest.approx(ppo.logs["policy_loss"], rel=1e-5, abs=1e-7)
        assert s["train/value_loss"] == pytest.approx(ppo.logs["value_loss"], rel=1e-5, abs=1e-7)
    env.venv.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def _waypoints(diag):
    env = R.VecNormalizeDevice(P.FixedwingWaypointsVecEnv(64, angle_representation="euler", seed=11))
    return R.PPO(env, R.PPOConfig(n_steps=8, batch_size=128, n_epochs=2, seed=11, diagnostics=diag))


def _lowlevel(diag):
    env = R.VecNormalizeDevice(P.FixedwingLowLevelVecEnv(num_envs=32, seed=12, device=0), norm_obs=True, norm_reward=True, clip_obs=10.0)
    return R.PPO(env, R.PPOConfig(n_steps=8, batch_size=64, n_epochs=2, seed=12, fused_six_actions=True, diagnostics=diag))


def _highlevel(diag):
    from pyflyt_drone_amd.highlevel import HighLevelCmdVecEnv
    torch.manual_seed(21)
    pol = R.MlpPolicy(21, 6)
    with torch.no_grad():
        for q in pol.parameters():
            q.add_(0.1 * torch.randn_like(q))
    g = np.random.default_rng(21)
    mean = g.normal(0.0, 1.0, 21) * np.array([1] * 6 + [10] * 6 + [0.3] * 6 + [1, 50, 10], dtype=np.float64)
    var = g.uniform(0.2, 4.0, 21) * np.array([1] * 6 + [100] * 6 + [0.1] * 6 + [3, 2500, 80], dtype=np.float64)
    env = R.VecNormalizeDevice(HighLevelCmdVecEnv(16, pol, (mean, var), seed=13), norm_obs=True, norm_reward=True, clip_obs=10.0, gamma=0.995)
    return R.PPO(env, R.PPOConfig(n_steps=8, batch_size=64, n_epochs=2, gamma=0.995, seed=13, fused_three_actions=True, diagnostics=diag))


@pytest.mark.parametrize("make,act_dim,one_launch", [(_waypoints, 4, True), (_lowlevel, 6, False), (_highlevel, 3, False)],
                         ids=["waypoints", "lowlevel", "highlevel"])
def test_end_to_end_through_the_collectors(make, act_dim, one_launch):
    x, y = make(True), make(False)
    assert x.act_dim == act_dim and x._collect_fused and bool(x._one_launch) == one_launch
    for p in (x, y):
        p.collect_rollouts()
        p.train()
    torch.cuda.synchronize()
    assert x._fused is not None and x._fused.A == act_dim and x._fused.diag_series is not None
    s, series = x.diagnostics, x.diagnostic_series
    assert all(math.isfinite(v) for v in s.values()), s
    n_mb = len(series["approx_kl"])
    assert n_mb == 2 * (8 * x.env.num_envs) // x.cfg.batch_size
    first_epoch = slice(0, n_mb // 2)
    assert (series["approx_kl"][first_epoch] >= 0).all() and (series["clip_fraction"][first_epoch] >= 0).all()
    # collector and update share the log-prob function: a fresh sample's ratio is exactly 1
    assert series["approx_kl"][0] == 0.0 and series["clip_fraction"][0] == 0.0
    yv, v = x.ret.reshape(-1).double().cpu().numpy(), x.buf_val.reshape(-1).double().cpu().numpy()
    assert s["train/explained_variance"] == pytest.approx(1.0 - np.var(yv - v) / np.var(yv), rel=1e-6, abs=1e-6)
    assert y.diagnostics == {}
    for p, q in zip(x.policy.parameters(), y.policy.parameters()):
        assert torch.equal(p, q)
    for p in (x, y):
        p.env.venv.close()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_a_second_update_starts_from_zeroed_rows_and_a_failed_one_clears_the_figures(monkeypatch):
    monkeypatch.setenv("FWSIM_PPO_SPLIT", "64x2")                      # two workgroups per network
    x, twin = _ppo(28, 4, 128), _ppo(28, 4, 128, diag=False)
    x.train(); twin.train()
    first = {k: v.copy() for k, v in x.diagnostic_series.items()}
    twin.cfg.diagnostics = True                                         # the twin's diagnostics buffer is born for the second call
    x.train(); twin.train()
    torch.cuda.synchronize()
    raw = x._fused._diag[:16 * 256].view(16, 2, 8, 4, 4)
    assert (raw[:, :, 2:] == 0).all()
    for k in SERIES:
        assert np.array_equal(x.diagnostic_series[k], twin.diagnostic_series[k]), k      # nothing of the first call's rows is in the second's
    assert not np.array_equal(first["approx_kl"], x.diagnostic_series["approx_kl"])
    assert x.diagnostics["train/n_updates"] == 4
    monkeypatch.setenv("FWSIM_SPIN_LOG2", "0")                          # every bounded wait: one poll
    with pytest.raises(RuntimeError, match="fw_ppo_update gave up"):
        x.train()
    torch.cuda.synchronize()
    assert x.diagnostics == {} and x.diagnostic_series == {}
    monkeypatch.delenv("FWSIM_SPIN_LOG2")
    x.train()
    assert set(x.diagnostic_series) == set(SERIES) and all(math.isfinite(v) for v in x.diagnostics.values())
