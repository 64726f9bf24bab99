"""PPOConfig.target_kl on the device: fw_ppo_update_kl against the plain and the diagnostics entry points bit for bit (the stop decided
inside the launch, under every cut and both exchange forms), its argument errors, and the fused learner against the torch path end to
end on the three action widths.

The pinned inputs, the float64 restatement that says where each case must stop and the condition that makes that verdict independent
of float32 rounding are in tests/ppo_kl_cases.py (checked by tests/test_ppo_target_kl_cpu.py).

The cuts.  16x8, 32x4 and 64x2 need 128 samples per minibatch; the (21, 6, 64) shape takes 64x1, 16x4 and -- both batch sizes -- 16x4
with FWSIM_PPO_RS=0 (the all-to-all exchange with four workgroups).  A cut a batch size does not admit is refused by the library
(FW_EINVAL: fewer chunks than workgroups) and is not a case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_kl_cases as KC  # noqa: E402

import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import _lib  # noqa: E402
from pyflyt_drone_amd import config as K  # noqa: E402
from pyflyt_drone_amd import rollout as R  # noqa: E402
from pyflyt_drone_amd._lib import devptr as _p  # noqa: E402

pytestmark = pytest.mark.gpu

CUTS_128 = [("16x8", None), ("32x4", None), ("64x2", None), ("16x4", "0")]
CUTS_64 = [("64x1", None), ("16x4", None), ("16x4", "0")]
GRID = [(s, cut, rs) for s in KC.SHAPES for cut, rs in (CUTS_128 if s[2] == 128 else CUTS_64)]
GRID_IDS = [f"{d}-{a}-{bs}-{cut}{'-a2a' if rs else ''}" for (d, a, bs), cut, rs in GRID]


@pytest.fixture(scope="module")
def reference():
    """Per shape, computed once on the CPU and left alone: the minibatch order, the no-stop KL series of the float64 restatement over
    it, from which every case takes its ``target_kl``, and the stop index the restatement reaches with it."""
    torch.set_num_threads(min(torch.get_num_threads(), 4))
    out = {}
    for d, a, bs in KC.SHAPES:
        ppo = KC.make_ppo(d, a, bs)
        perm = KC.permutation(ppo)
        series = KC.Restated(ppo).train(perm, bs)["kl"]
        per_case = {}
        for case, j in KC.CASES.items():
            t = KC.pick_target_kl(series, j)
            m = KC.Restated(ppo).train(perm, bs, target_kl=t)["stepped"]
            assert m == (KC.N_MB if j is None else j)
            per_case[case] = (t, m)
        per_case["perm"] = perm
        out[(d, a, bs)] = per_case
    return out


class Inputs:
    """The device buffers of one shape as the entry points take them, and the calls themselves on fresh copies of the images."""

    def __init__(self, d, a, bs, perm):
        self.d, self.a, self.bs = d, a, bs
        ppo = KC.make_ppo(d, a, bs, device="cuda")             # (the CPU reference's buffers and initial weights, on the device)
        self.ppo = ppo
        B = 2 * bs
        self.bufs = [x.contiguous() for x in (ppo.buf_obs.reshape(B, -1), ppo.buf_act.reshape(B, -1), ppo.buf_logp.reshape(B),
                                              ppo.adv.reshape(B), ppo.ret.reshape(B))]
        self.perm = perm.to(device="cuda", dtype=torch.int32)    # (... and its minibatch order)
        self.f = R.FusedPpoUpdate(ppo.policy, ppo.optimizer, d)
        self.step0 = self.f.load_from_torch()
        cfg, pg = ppo.cfg, ppo.optimizer.param_groups[0]
        self.H = R._PpoHyper(lr=pg["lr"], clip_range=cfg.clip_range, ent_coef=cfg.ent_coef, vf_coef=cfg.vf_coef, max_grad_norm=cfg.max_grad_norm,
                             beta1=pg["betas"][0], beta2=pg["betas"][1], eps=pg["eps"], adv_mean=0.0, adv_std=1.0, norm_adv=1, step0=self.step0)
        self.ws = self.f._workspace(KC.N_MB, bs)

    def call(self, entry, n_mb, target_kl=None, diag=True):
        """entry: 'plain' (the width's own entry point), 'diag', 'kl'.  Returns dict(flat, mom_m, mom_v, loss, diag, stepped, status)."""
        L, f = _lib.lib(), self.f
        flat, mm, mv = f.flat.clone(), f.mom_m.clone(), f.mom_v.clone()
        loss = torch.zeros(16, dtype=torch.float32, device="cuda")
        dg = torch.zeros(KC.N_MB * 256, dtype=torch.float32, device="cuda")
        stepped = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        st = _lib.stream(flat.device)
        head = (_p(flat), _p(mm), _p(mv), *(_p(x) for x in self.bufs), _p(self.perm), n_mb, self.bs, self.d)
        tail = (C.byref(self.H), _p(loss), _p(self.ws), self.ws.numel(), st)
        if entry == "plain":
            rc = (L.fw_ppo_update_a3(*head, *tail) if self.a == 3 else L.fw_ppo_update_a(*head, self.a, *tail))
        elif entry == "diag":
            rc = L.fw_ppo_update_diag(*head, self.a, *tail, _p(dg), dg.numel())
        else:
            rc = L.fw_ppo_update_kl(*head, self.a, *tail, _p(dg) if diag else None, dg.numel() if diag else 0, float(target_kl), _p(stepped))
        _lib.check(rc)
        status, paths = C.c_uint32(0), C.c_uint32(0)
        _lib.check(L.fw_ppo_update_status(_p(self.ws), self.ws.numel(), C.byref(status), C.byref(paths), st))
        torch.cuda.synchronize()
        return dict(flat=flat, mom_m=mm, mom_v=mv, loss=loss[:3].clone(), diag=dg.view(KC.N_MB, 256), stepped=int(stepped.item()),
                    status=int(status.value))


@pytest.fixture(scope="module")
def inputs(reference):
    return {s: Inputs(*s, reference[s]["perm"]) for s in KC.SHAPES}


def _set_cut(monkeypatch, cut, rs):
    monkeypatch.setenv("FWSIM_PPO_SPLIT", cut)
    if rs is not None:
        monkeypatch.setenv("FWSIM_PPO_RS", rs)


def _same(x, y, names=("flat", "mom_m", "mom_v")):
    for n in names:
        assert torch.equal(x[n], y[n]), n


# ---------------------------------------------------------------------------------------------------------------- 1, 2, 3
@pytest.mark.parametrize("case", list(KC.CASES))
@pytest.mark.parametrize("shape,cut,rs", GRID, ids=GRID_IDS)
def test_stop_inside_the_launch_against_the_plain_and_diagnostics_entry_points(shape, cut, rs, case, reference, inputs, monkeypatch):
    _set_cut(monkeypatch, cut, rs)
    inp = inputs[shape]
    t, m = reference[shape][case]
    got = inp.call("kl", KC.N_MB, target_kl=t)
    kl = R.fused_diag_series(got["diag"].cpu().numpy(), KC.N_MB)["approx_kl"]
    print(f"\n[kl gpu] {shape} {cut} rs={rs} {case}: limit {np.float32(1.5 * t):.6g}, stepped {got['stepped']} (reference {m}), KL rows {np.round(kl, 6).tolist()}")
    assert got["status"] == 0 and got["stepped"] == m
    computed = min(m + 1, KC.N_MB)
    if m == 0:
        _same(got, dict(flat=inp.f.flat, mom_m=inp.f.mom_m, mom_v=inp.f.mom_v))
    else:
        want = inp.call("plain", m)                            # the same permutation prefix, the same step0
        assert want["status"] == 0
        _same(got, want)
    losses = inp.call("plain", computed)
    assert torch.equal(got["loss"], losses["loss"]), (got["loss"].tolist(), losses["loss"].tolist())
    # diagnostics rows: those of fw_ppo_update_diag up to the stop, later ones as the caller zeroed them; diag = NULL: the same images
    rows = inp.call("diag", KC.N_MB)
    assert torch.equal(got["diag"][:computed], rows["diag"][:computed])
    assert int(got["diag"][:computed, :].ne(0).sum()) > 0 and not bool(got["diag"][computed:].ne(0).any())
    null = inp.call("kl", KC.N_MB, target_kl=t, diag=False)
    assert null["status"] == 0 and null["stepped"] == m and not bool(null["diag"].ne(0).any())
    _same(null, got, ("flat", "mom_m", "mom_v", "loss"))
    if case == "never":
        assert m == KC.N_MB
        _same(got, rows, ("flat", "mom_m", "mom_v", "loss"))


# ---------------------------------------------------------------------------------------------------------------- 4, 5
@pytest.mark.parametrize("case", ["mid_epoch_2", "never"])
@pytest.mark.parametrize("shape,cut,rs", GRID, ids=GRID_IDS)
def test_every_workgroup_reaches_the_same_verdict_and_two_runs_the_same_bits(shape, cut, rs, case, reference, inputs, monkeypatch):
    """The switches change which workgroup writes the results back and which path the exchanges take: the same bits under each of
    them means every workgroup stopped at the same minibatch with the same state."""
    _set_cut(monkeypatch, cut, rs)
    inp = inputs[shape]
    t, m = reference[shape][case]
    base = inp.call("kl", KC.N_MB, target_kl=t)
    again = inp.call("kl", KC.N_MB, target_kl=t)
    assert base["status"] == again["status"] == 0 and base["stepped"] == again["stepped"] == m
    _same(again, base, ("flat", "mom_m", "mom_v", "loss", "diag"))
    for name, value in (("FWSIM_PPO_NO_L2_SWAP", "1"), ("FWSIM_PPO_WRITER", "last")):
        with monkeypatch.context() as mp:
            mp.setenv(name, value)
            other = inp.call("kl", KC.N_MB, target_kl=t)
        assert other["status"] == 0 and other["stepped"] == m, name
        _same(other, base, ("flat", "mom_m", "mom_v", "loss", "diag"))


# ---------------------------------------------------------------------------------------------------------------- 6
def test_argument_errors_run_nothing(inputs):
    inp = inputs[KC.SHAPES[0]]
    L, f = _lib.lib(), inp.f
    flat, mm, mv = f.flat.clone(), f.mom_m.clone(), f.mom_v.clone()
    loss = torch.zeros(16, dtype=torch.float32, device="cuda")
    stepped = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    st = _lib.stream(flat.device)

    def call(act_dim=4, target_kl=0.01, count=stepped):
        return L.fw_ppo_update_kl(_p(flat), _p(mm), _p(mv), *(_p(x) for x in inp.bufs), _p(inp.perm), KC.N_MB, inp.bs, inp.d, act_dim,
                                  C.byref(inp.H), _p(loss), _p(inp.ws), inp.ws.numel(), st, None, 0, target_kl, _p(count))
    for t in (0.0, -0.5, float("nan"), float("inf")):
        assert call(target_kl=t) == K.FW_EINVAL
    assert call(count=None) == K.FW_EINVAL
    assert call(act_dim=5) == K.FW_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(flat, f.flat) and torch.equal(mm, f.mom_m) and torch.equal(mv, f.mom_v)
    assert int(stepped.item()) == -7 and not bool(loss.ne(0).any())
    # the existing entry points refuse what they refused: a three-action call through the *_a family, a NULL diagnostics buffer
    assert L.fw_ppo_update_a(_p(flat), _p(mm), _p(mv), *(_p(x) for x in inp.bufs), _p(inp.perm), KC.N_MB, inp.bs, inp.d, 3, C.byref(inp.H),
                             _p(loss), _p(inp.ws), inp.ws.numel(), st) == K.FW_EINVAL
    assert L.fw_ppo_update_diag(_p(flat), _p(mm), _p(mv), *(_p(x) for x in inp.bufs), _p(inp.perm), KC.N_MB, inp.bs, inp.d, 4, C.byref(inp.H),
                                _p(loss), _p(inp.ws), inp.ws.numel(), st, None, 0) == K.FW_EINVAL


# ---------------------------------------------------------------------------------------------------------------- the learner
@pytest.mark.parametrize("diagnostics", [False, True], ids=["plain", "diagnostics"])
@pytest.mark.parametrize("shape", KC.SHAPES, ids=[f"{d}-{a}-{bs}" for d, a, bs in KC.SHAPES])
def test_fused_learner_on_the_pinned_inputs(shape, diagnostics):
    """PPO.train() through FusedPpoUpdate.run: counts, logs, series and the optimiser's step follow the stop."""
    d, a, bs = shape
    ppo = KC.make_ppo(d, a, bs, device="cuda", target_kl=1.0, diagnostics=diagnostics)
    # (the learner draws its minibatch order from the device's generator: the restatement walks that order, on the same buffers)
    perm = KC.permutation(ppo).cpu()
    series = KC.Restated(ppo).train(perm, bs)["kl"]            # (float64, on the CPU)
    j, t = KC.first_clear_stop(series)                         # (this order is not the pinned one: the first stop the condition admits)
    m = KC.Restated(ppo).train(perm, bs, target_kl=t)["stepped"]
    print(f"\n[kl gpu learner] {shape}: stop at {j}, target_kl {t:.6g}, smallest margin {KC.margins(series, j, t)[0].min():.3f}")
    assert m == j
    ppo.cfg.target_kl = t
    ppo.train()
    assert ppo._fused is not None and ppo._fused.A == a
    assert (ppo.logs["minibatches_stepped"], ppo.logs["epochs_run"], ppo.logs["kl_stopped"]) == (m, m // KC.MB_PER_EPOCH + 1, True)
    assert ppo._n_updates == m // KC.MB_PER_EPOCH + 1
    assert {float(st["step"]) for st in ppo.optimizer.state.values()} == {float(m)}
    assert ppo.stop_kl > ppo.cfg.kl_stop and ppo.early_stop_message().startswith(f"Early stopping at step {m // KC.MB_PER_EPOCH} due to")
    if diagnostics:
        s = ppo.diagnostic_series
        assert all(v.shape == (m + 1,) for v in s.values()) and s["approx_kl"][-1] == ppo.stop_kl
        assert (s["approx_kl"][:-1] <= ppo.cfg.kl_stop).all() and ppo.diagnostics["train/n_updates"] == ppo._n_updates
        assert ppo.diagnostics["train/policy_gradient_loss"] == pytest.approx(ppo.logs["policy_loss"], rel=1e-5, abs=1e-7)
    else:
        assert ppo.diagnostics == {}
    twin = KC.make_ppo(d, a, bs, device="cuda", target_kl=t, diagnostics=diagnostics, fused_update=False)
    twin.train()
    assert {k: twin.logs[k] for k in ("minibatches_stepped", "epochs_run", "kl_stopped")} == {k: ppo.logs[k] for k in ("minibatches_stepped", "epochs_run", "kl_stopped")}
    for (n, x), (_, y) in zip(ppo.policy.named_parameters(), twin.policy.named_parameters()):
        KC.SC._close(n, x, y, *KC.TOL["param"])
    assert torch.equal(ppo.perm_gen.get_state(), twin.perm_gen.get_state())


# ---------------------------------------------------------------------------------------------------------------- 7
def _waypoints(fused):
    env = R.VecNormalizeDevice(P.FixedwingVecEnv(K.train_waypoints_v3_config(), 16, device=0, seed=11), norm_obs=True, norm_reward=True, clip_obs=10.0)
    return lambda **kw: R.PPO(env, R.PPOConfig(n_steps=16, batch_size=64, n_epochs=3, seed=11, use_graphs=False, diagnostics=True,
                                               fused_update=fused, **kw))


def _lowlevel(fused):
    env = R.VecNormalizeDevice(P.FixedwingLowLevelVecEnv(num_envs=16, seed=11, device=0), norm_obs=True, norm_reward=True, clip_obs=10.0)
    return lambda **kw: R.PPO(env, R.PPOConfig(n_steps=16, batch_size=64, n_epochs=3, seed=11, use_graphs=False, diagnostics=True,
                                               fused_update=fused, fused_six_actions=True, **kw))


def _highlevel(fused):
    from pyflyt_drone_amd.highlevel import HighLevelCmdVecEnv
    torch.manual_seed(21)
    pol = R.MlpPolicy(21, 6)
    with torch.no_grad():
        for q in pol.parameters():
            q.add_(0.1 * torch.randn_like(q))
    g = np.random.default_rng(21)
    mean, var = g.normal(0.0, 1.0, 21), g.uniform(0.2, 4.0, 21)
    env = R.VecNormalizeDevice(HighLevelCmdVecEnv(16, pol, (mean, var), seed=11), norm_obs=True, norm_reward=True, clip_obs=10.0, gamma=0.995)
    return lambda **kw: R.PPO(env, R.PPOConfig(n_steps=16, batch_size=64, n_epochs=3, gamma=0.995, seed=11, use_graphs=False, diagnostics=True,
                                               fused_update=fused, fused_three_actions=True, **kw))


@pytest.mark.parametrize("make", [_waypoints, _lowlevel, _highlevel], ids=["fused-four-actions", "fused_six_actions", "fused_three_actions"])
def test_end_to_end_against_the_torch_path(make):
    """Two updates on a 16-env handle, the fused learner against the torch path with the same ``target_kl``.  The limit of the first
    update comes from a no-stop look at the very same rollout (a third learner) by tests/ppo_kl_cases.py's helper -- the first
    minibatch, from the third on, that its 5 % condition admits -- so both paths must stop there; the second update runs under a
    limit above every KL of the first and must not stop on either path."""
    look = make(False)()
    look.collect_rollouts(); look.train()
    series = look.diagnostic_series["approx_kl"]
    j, t = KC.first_clear_stop(series)
    x, y = make(True)(target_kl=t), make(False)(target_kl=t)
    assert x._collect_fused == y._collect_fused
    for update in range(2):
        x.collect_rollouts(); y.collect_rollouts()
        x.train(); y.train()
        torch.cuda.synchronize()
        want = (j, j // 4 + 1, True) if update == 0 else (12, 3, False)
        assert x._fused is not None and x._fused.last_stepped == want[0] and x._fused.last_computed == min(want[0] + 1, 12)
        for p in (x, y):
            assert (p.logs["minibatches_stepped"], p.logs["epochs_run"], p.logs["kl_stopped"]) == want, (update, p.logs)
        assert x._n_updates == y._n_updates
        steps = float(j if update == 0 else j + 12)
        for p in (x, y):
            assert {float(st["step"]) for st in p.optimizer.state.values()} == {steps}
        for (n, a), (_, b) in zip(x.policy.named_parameters(), y.policy.named_parameters()):
            KC.SC._close(n, a, b, *KC.TOL["param"])
        x.cfg.target_kl = y.cfg.target_kl = KC.pick_target_kl(series, None)
