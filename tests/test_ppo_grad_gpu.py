"""The gradients of the fused PPO update (fw_ppo_update and its _a / _a3 / _diag / _kl forms), one minibatch at a time, against the
float64 restatement of tests/ppo_grad_cases.py: every tensor of both networks and log_std, in every cut of a minibatch over 1 to 8
blocks per network, for four-, six- and three-action policies.  Each test is ONE single-minibatch launch per learner it builds; the
gradient the kernel applied is read back from the Adam moments of a step taken from zero state (the handle: ppo_grad_cases).

Tolerances (ppo_grad_cases.tolerance).  A tensor's recovered gradient may be K = 8 x E32 from the float64 one, plus 4 float32 epsilons
of the tensor's largest gradient; E32 is the error of the float32 torch path on the same case and tensor, measured on the CPU when the
test runs (tests/test_ppo_grad_cpu.py asserts it and prints it).  The 8 pays for the kernel's other summation order over the samples
(per thread, per wave, per block, across blocks) and its ``expf``; profiles/ppo_grad_margin.txt has the measured kernel error over
E32 per case family (worst 2.57; written by a session of this module with FWSIM_PPO_GRAD_MARGIN_OUT=<file>).  What the comparison catches: a flipped branch of the
surrogate (``A < 0`` with the ratio above the range treated as clipped, say) removes or adds a whole sample's share of the policy
gradient -- 1 / bs of it or more, 2e-3 at 512 samples, against a tolerance of about 5e-6 of the scale; a mis-scaled tensor, a dropped
term of dlog_std or dbo likewise.

The clip scalar: ``g_clipped / g_raw`` is one number for every element of every tensor of both networks (spread: 4 epsilons -- two
float32 products and two moments, half an ulp each), and equals ``max_grad_norm / (N64 + 1e-6)`` to K x the relative float32 error of
the torch path's ``clip_grad_norm_`` total on the case plus 4 epsilons (the float32 roundings of the norm, the quotient and
max_grad_norm itself).  A per-thread element (bo, log_std, Wo) missing from or doubled in the exchanged norm moves that scalar by
ten times this or more (tests/test_ppo_grad_cpu.py asserts that on the restatement and prints the factor: 40 to 1e5).

The warm Adam step: the float64 Adam formula with the hyper-parameters as the C ABI carries them (float32: beta2 is 0.99900001287) fed
the clipped gradient of a cold twin; tolerance K x the error of torch.optim.Adam in float32 on the same inputs against the same
formula with the double hyper-parameters, plus the 4-epsilon floor.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_grad_cases as G  # noqa: E402
from test_learner_diag_gpu import CUTS, _set_cut  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = G.EPS32
SHAPES = [(28, 4), (21, 6), (30, 3)]
GRID = [(d, a, bs, split) for bs, split in CUTS for d, a in SHAPES] + [(5, 4, 64, None), (27, 4, 64, None), (64, 4, 64, None)]
IDS = [f"{d}-{a}-{bs}-{split or 'default'}" for d, a, bs, split in GRID]
CLIP_GRID = [(28, 4, bs, split) for bs, split in CUTS] + [(21, 6, 128, None), (30, 3, 128, None)]
CLIP_IDS = [f"{d}-{a}-{bs}-{split or 'default'}" for d, a, bs, split in CLIP_GRID]
WARM_GRID = [(28, 4, 16, None), (28, 4, 128, None), (28, 4, 128, "all-to-all"), (28, 4, 512, "64x8"), (21, 6, 64, None), (30, 3, 128, None)]
WARM_IDS = [f"{d}-{a}-{bs}-{split or 'default'}" for d, a, bs, split in WARM_GRID]

_WORST = {}


def _book(family, ratio, where):
    print(f"[ppo grad] {family}: {where}: kernel error / float32 torch error = {ratio:.3f}")
    if ratio > _WORST.get(family, (-1.0, ""))[0]:
        _WORST[family] = (ratio, where)


@pytest.fixture(scope="module", autouse=True)
def margin_file():
    yield
    path = os.environ.get("FWSIM_PPO_GRAD_MARGIN_OUT")
    if path and _WORST:
        with open(path, "a") as f:
            for family in sorted(_WORST):
                f.write(f"{family:44s} worst kernel error / E32 {_WORST[family][0]:8.3f}   at {_WORST[family][1]}\n")


def _run(c, **over):
    """One single-minibatch launch on the case; returns the learner and its recovered (g, g squared) per tensor."""
    ppo = c.make("cuda", **over)
    ppo.train()
    torch.cuda.synchronize()
    # (what only FusedPpoUpdate.run sets: the torch path on the device would leave these as they were born)
    assert ppo._fused is not None and ppo._fused.A == c.a and ppo._fused.last_stepped == 1 and ppo._fused.synced, \
        "the fused learner did not take the update"
    got, step = G.recovered(ppo, "kernel")
    assert step == 1.0
    for n, (g1, g2) in got.items():
        assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(g2).all()), n
    assert all(bool(torch.isfinite(q).all()) for q in ppo.policy.parameters())
    return ppo, got


def _compare(got, m, family, where):
    """Every tensor against the restatement: prints the figures, books the worst, then asserts."""
    bad = []
    for n, (g1, _) in got.items():
        err = float((g1 - m["ref"]["grads"][n]).abs().max())
        floor = G.FLOOR_EPS * EPS * m["scale"][n]
        tol = G.tolerance(m, n)
        ratio = err / max(m["e32"][n], floor) if err > 0 else 0.0
        print(f"[ppo grad] {where} {n:20s} |kernel - g64| {err:.3e}  E32 {m['e32'][n]:.3e}  tolerance {tol:.3e}  max|g64| {m['scale'][n]:.3e}")
        _book(family, ratio, f"{where} {n}")
        if not err <= tol:
            bad.append((n, err, tol))
    assert not bad, bad


def _moments_agree(got):
    """exp_avg_sq / (1 - beta2) is the square of exp_avg / (1 - beta1): both moments come from one gradient (two float32 products
    each: 4 epsilons)."""
    for n, (g1, g2) in got.items():
        sq = g1 * g1
        assert bool(((g2 - sq).abs() <= 4 * EPS * sq + 1e-35).all()), n


def _padding_rows_zero(ppo):
    f = ppo._fused
    if f.D == f.Dp:
        return
    slots = f._slots()
    per_net = [slots[0][1], slots[6][1]]                        # W1 is the first of the six slots of each network
    assert slots[0][2] == slots[6][2] == (f.Dp, 64)
    for off in per_net:
        for image in (f.flat, f.m, f.v):                       # (m, v: the moments in flat order, as store_to_torch staged them)
            row = image[off + f.D * 64: off + f.Dp * 64]
            assert row.numel() == 64 and bool((row == 0).all())


# ------------------------------------------------------------------------------------------------------ raw gradients
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("d,a,bs,split", GRID, ids=IDS)
def test_raw_gradient_of_every_tensor_against_float64(d, a, bs, split, kind, monkeypatch):
    """``max_grad_norm = 1e30``: the moments give the raw gradient.  ``mixed`` holds every branch of the surrogate by construction
    (and A == +-0.0), ``live`` only samples outside the range whose gradient flows, ``dead`` only samples that pass none; a flipped
    branch changes the policy gradient by whole samples' shares.  Odd obs_dim: the padding row of W1 stays zero, moments too."""
    _set_cut(monkeypatch, split)
    c, m = G.case(d, a, bs, kind), G.measure(d, a, bs, kind)
    ppo, got = _run(c)
    print()
    _compare(got, m, f"gradient {kind} A={a}", f"{d}-{a}-{bs}-{split or 'default'} {kind}")
    _moments_agree(got)
    _padding_rows_zero(ppo)
    if kind == "dead":
        # the surrogate passes nothing: the policy network's gradient is exactly zero, dlog_std_k is the entropy term alone
        for n, (g1, g2) in got.items():
            if n.startswith("pi_net") or n.startswith("action_net"):
                assert float(g1.abs().max()) == 0.0 and float(g2.abs().max()) == 0.0, n
        want = G.ONE_MINUS["kernel"][0] * float(np.float32(-0.01))
        m1 = ppo.optimizer.state[ppo.policy.log_std]["exp_avg"].double().cpu()
        assert m1.shape == (a,) and bool(((m1 - want).abs() <= EPS * abs(want)).all()), m1


@pytest.mark.parametrize("d,a,bs,split", GRID, ids=IDS)
def test_a_minibatch_without_gradient_moves_nothing(d, a, bs, split, monkeypatch):
    """``dead`` with ent_coef = 0 and vf_coef = 0: the whole gradient is zero and so is the norm.  Parameters bit for bit, zero
    moments, step 1, everything finite (0 / (0 + eps) in Adam, max_grad_norm / 1e-6 in the clip)."""
    _set_cut(monkeypatch, split)
    c = G.case(d, a, bs, "dead")
    for mgn in (0.5, G.BIG):
        ppo = c.make("cuda", ent_coef=0.0, vf_coef=0.0, max_grad_norm=mgn)
        before = [q.detach().clone() for q in ppo.policy.parameters()]
        ppo.train()
        torch.cuda.synchronize()
        assert ppo._fused is not None
        for q, q0 in zip(ppo.policy.parameters(), before):
            assert torch.equal(q, q0)
            st = ppo.optimizer.state[q]
            assert float(st["step"]) == 1.0
            assert bool((st["exp_avg"] == 0).all()) and bool((st["exp_avg_sq"] == 0).all())
        assert bool(torch.isfinite(ppo._fused.flat).all()) and all(math.isfinite(v) for v in ppo.logs.values())
        _padding_rows_zero(ppo)


# ------------------------------------------------------------------------------------------------------ clipping
@pytest.mark.parametrize("kind", ("mixed", "random"))
@pytest.mark.parametrize("d,a,bs,split", CLIP_GRID, ids=CLIP_IDS)
def test_the_clip_scalar_is_one_number_and_the_right_one(d, a, bs, split, kind, monkeypatch):
    _set_cut(monkeypatch, split)
    c, m = G.case(d, a, bs, kind), G.measure(d, a, bs, kind)
    N = m["ref"]["norm"]
    raw, g = _run(c)
    # inactive: 4 N64 -- the same bits as without clipping
    off, _ = _run(c, max_grad_norm=4.0 * N)
    for (n, q), q_off in zip(raw.policy.named_parameters(), off.policy.parameters()):
        assert torch.equal(q, q_off), n
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(raw.optimizer.state[q][k], off.optimizer.state[q_off][k]), (n, k)
    # active: 0.25 N64
    mgn = 0.25 * N
    _, gc = _run(c, max_grad_norm=mgn)
    num = sum(float((gc[n][0] * g[n][0]).sum()) for n in g)
    den = sum(float((g[n][0] * g[n][0]).sum()) for n in g)
    s = num / den                                                       # the least-squares scalar over every element of both networks
    want = float(np.float32(mgn)) / (N + 1e-6)                          # (max_grad_norm crosses the ABI as float32)
    spread = 0.0
    for n in g:
        big = g[n][0].abs() > 1e-20                                     # (float32 normal range after the (1 - beta1) product, nothing more)
        if bool(big.any()):
            spread = max(spread, float(((gc[n][0][big] / g[n][0][big]) / s - 1.0).abs().max()))
    tol = G.K * m["norm_err"] + G.FLOOR_EPS * EPS
    where = f"{d}-{a}-{bs}-{split or 'default'} {kind}"
    print(f"\n[ppo grad] {where}: clip scalar {s:.9g} want {want:.9g} rel diff {abs(s / want - 1):.3e} tolerance {tol:.3e} "
          f"(torch total rel error {m['norm_err']:.3e}); spread {spread:.3e}")
    _book(f"clip scalar {kind} A={a}", abs(s / want - 1.0) / max(m["norm_err"], G.FLOOR_EPS * EPS), where)
    assert spread <= 4 * EPS
    assert abs(s / want - 1.0) <= tol
    _moments_agree(gc)


# ------------------------------------------------------------------------------------------------------ hyper-parameters
@pytest.mark.parametrize("kind,over", G.HYPER, ids=G.HYPER_IDS)
@pytest.mark.parametrize("d,a,bs", G.HYPER_SHAPES, ids=["28-4-128", "21-6-64"])
def test_raw_gradient_under_other_hyper_parameters(d, a, bs, kind, over):
    """clip_range, vf_coef, ent_coef (0 too) and the three advantage normalisations (norm_adv 0 / 1 / 2) on the device; that each of
    them reaches the restated gradient is asserted in tests/test_ppo_grad_cpu.py."""
    c, m = G.case(d, a, bs, kind), G.measure(d, a, bs, kind, **over)
    _, got = _run(c, **over)
    print()
    _compare(got, m, f"gradient hyper A={a}", f"{d}-{a}-{bs} {kind} {over}")
    _moments_agree(got)


# ------------------------------------------------------------------------------------------------------ one warm Adam step
def _adam64(p0, m0, v0, g, t, lr, b1, b2, eps):
    m1 = b1 * m0 + (1.0 - b1) * g
    v1 = b2 * v0 + (1.0 - b2) * g * g
    p1 = p0 - (lr / (1.0 - b1 ** t)) * m1 / (v1.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
    return p1, m1, v1


def _preload(ppo, state, step):
    for q, (m0, v0) in zip(ppo.policy.parameters(), state):
        ppo.optimizer.state[q] = {"step": torch.tensor(float(step)), "exp_avg": m0.to(q.device).clone(), "exp_avg_sq": v0.to(q.device).clone()}


@pytest.mark.parametrize("d,a,bs,split", WARM_GRID, ids=WARM_IDS)
def test_one_warm_adam_step_against_the_float64_formula(d, a, bs, split, monkeypatch):
    _set_cut(monkeypatch, split)
    c = G.case(d, a, bs, "random")
    cold, got = _run(c, max_grad_norm=0.5)                              # the clipped gradient the warm twin will apply as well
    gen = torch.Generator(); gen.manual_seed(77)
    state = [(1e-3 * torch.randn(q.shape, generator=gen), 1e-6 * (0.5 + torch.rand(q.shape, generator=gen))) for q in cold.policy.parameters()]
    STEP = 1000
    warm = c.make("cuda", max_grad_norm=0.5)
    p0 = [q.detach().cpu().clone() for q in warm.policy.parameters()]
    _preload(warm, state, STEP)
    warm.train()
    torch.cuda.synchronize()
    assert warm._fused is not None
    # float32 torch.optim.Adam on the same inputs
    tw = [q.clone().requires_grad_(True) for q in p0]
    opt = torch.optim.Adam(tw, lr=warm.cfg.learning_rate, eps=1e-5)
    for q, (m0, v0), n in zip(tw, state, got):
        opt.state[q] = {"step": torch.tensor(float(STEP)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        q.grad = got[n][0].float()
    opt.step()
    lr, eps = warm.cfg.learning_rate, 1e-5
    f32 = lambda x: float(np.float32(x))      # noqa: E731
    where = f"{d}-{a}-{bs}-{split or 'default'}"
    print()
    bad = []
    for (n, q), q0, (m0, v0), qt in zip(warm.policy.named_parameters(), p0, state, tw):
        g = got[n][0]
        exact = _adam64(q0.double(), m0.double(), v0.double(), g, STEP + 1, lr, 0.9, 0.999, eps)
        abi = _adam64(q0.double(), m0.double(), v0.double(), g, STEP + 1, f32(lr), f32(0.9), f32(0.999), f32(eps))
        st, stt = warm.optimizer.state[q], opt.state[qt]
        assert float(st["step"]) == STEP + 1
        rows = (("param", q.detach().double().cpu(), qt.detach().double(), 0, float((abi[0] - q0.double()).abs().max())),
                ("exp_avg", st["exp_avg"].double().cpu(), stt["exp_avg"].double(), 1, float(abi[1].abs().max())),
                ("exp_avg_sq", st["exp_avg_sq"].double().cpu(), stt["exp_avg_sq"].double(), 2, float(abi[2].abs().max())))
        for what, kernel, torch32, i, scale in rows:
            e_t = float((torch32 - exact[i]).abs().max())
            e_k = float((kernel - abi[i]).abs().max())
            tol = G.K * e_t + G.FLOOR_EPS * EPS * scale
            print(f"[ppo grad] warm {where} {n:20s} {what:10s} |kernel - f64| {e_k:.3e}  torch float32 error {e_t:.3e}  tolerance {tol:.3e}")
            _book(f"warm Adam step {what} A={a}", e_k / max(e_t, G.FLOOR_EPS * EPS * scale), f"{where} {n}")
            if not e_k <= tol:
                bad.append((n, what, e_k, tol))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------ entry points
@pytest.mark.parametrize("d,a,bs", [(28, 4, 128), (21, 6, 64), (30, 3, 128)], ids=["28-4-128", "21-6-64", "30-3-128"])
def test_the_diag_and_kl_entry_points_apply_the_same_gradient(d, a, bs):
    """fw_ppo_update_diag and fw_ppo_update_kl (a target_kl far above any KL of the buffers) are instantiations of the same kernel
    row: moments and parameters after the one step are the plain entry point's bit for bit."""
    c = G.case(d, a, bs, "mixed")
    plain, _ = _run(c)
    for over in (dict(diagnostics=True), dict(target_kl=1e6), dict(diagnostics=True, target_kl=1e6)):
        other, _ = _run(c, **over)
        if "target_kl" in over:
            assert other.logs["minibatches_stepped"] == 1 and not other.logs["kl_stopped"]
        if "diagnostics" in over:
            assert other._fused.diag_series is not None
        for (n, q), q2 in zip(plain.policy.named_parameters(), other.policy.parameters()):
            assert torch.equal(q, q2), (n, over)
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(plain.optimizer.state[q][k], other.optimizer.state[q2][k]), (n, k, over)
