"""The per-gradient tests of the PPO learner without a device (tests/ppo_grad_cases.py has the inputs and the float64 restatement):
the restatement against the float32 torch path per tensor, the read-back of a gradient from the Adam moments, the precondition of
the ``random`` inputs (no sample where float32 rounding decides the branch), the side of ``max_grad_norm`` every clipping case is on,
and the float32-against-float64 figures the tolerances of tests/test_ppo_grad_gpu.py are built from.

Tolerance of the torch path against the restatement.  Both differentiate the same formulas; they differ by float32 rounding.  A
gradient element is a sum over the minibatch of products of O(1) factors: torch's float32 evaluation is good to a few epsilons of the
tensor's largest element unless the formulas differ.  REL = 64 epsilons (7.6e-6) of the largest |g64| of the tensor: the worst figure
printed below is about 30 (value_net.bias, a sum of signed terms that cancels to a hundredth of its terms); a wrong term, sign,
normalisation mode or coefficient moves a tensor by 1e-2 of its scale or more.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_grad_cases as G  # noqa: E402

REL = 64 * G.EPS32
SHAPES = [(28, 4), (21, 6), (30, 3)]
# every batch size of the GPU grid: the reference and the figures are per case
GRID = [(d, a, bs) for bs in (16, 32, 64, 128, 256, 512) for d, a in SHAPES] + [(5, 4, 64), (27, 4, 64), (64, 4, 64)]
IDS = [f"{d}-{a}-{bs}" for d, a, bs in GRID]
HYPER, HYPER_IDS = G.HYPER, G.HYPER_IDS


def _check(m, label):
    worst = 0.0
    for n, e in m["e32"].items():
        s = m["scale"][n]
        print(f"[ppo grad cpu] {label} {n:20s} max|g32 - g64| {e:.3e}  max|g64| {s:.3e}  in eps of the scale {e / (G.EPS32 * s) if s else 0.0:.2f}")
        assert e <= REL * s, (label, n, e, s)
        worst = max(worst, e / (G.EPS32 * s) if s else 0.0)
    return worst


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("d,a,bs", GRID, ids=IDS)
def test_the_restatement_is_what_the_torch_path_computes_and_the_moments_give_the_gradient_back(d, a, bs, kind):
    m = G.measure(d, a, bs, kind)
    print()
    _check(m, f"{d}-{a}-{bs} {kind}")
    # the read-back: exp_avg / (1 - beta1) is the gradient the optimiser was handed (p.grad still holds it), exp_avg_sq its square
    for g32, (n, (g1, g2)) in zip(m["grads32"], m["got"].items()):
        g32 = g32.double()
        assert float((g1 - g32).abs().max()) <= G.EPS32 * float(g32.abs().max()), n
        assert float((g2 - g32 * g32).abs().max()) <= 2 * G.EPS32 * float((g32 * g32).max()), n
    assert m["norm_err"] <= 8 * G.EPS32
    if kind == "dead":                   # the surrogate passes nothing: the policy network's gradient is zero in both, log_std's is the entropy term
        for n, gr in m["ref"]["grads"].items():
            if n.startswith("pi_net") or n.startswith("action_net"):
                assert float(gr.abs().max()) == 0.0 and m["e32"][n] == 0.0, n
        assert torch.equal(m["ref"]["grads"]["log_std"], torch.full((a,), -0.01, dtype=torch.float64))


@pytest.mark.parametrize("d,a,bs", GRID, ids=IDS)
def test_the_inputs_decide_their_branch(d, a, bs):
    """``random``: no sample of the chosen seed sits in the band.  Directed kinds: every sample is where it was put -- the ratio at
    least 0.05 from the edge of each clip range the tests use, the advantage with the sign it was given or exactly zero."""
    band, measured = G.case(d, a, bs, "random").band_count()
    print(f"\n[ppo grad cpu] {d}-{a}-{bs} random: max |log-ratio f32 - f64| = {measured:.3e}, samples in the band: {band}")
    assert band == 0, "choose another seed for this shape (ppo_grad_cases.SEEDS)"
    assert measured < 1e-4
    for kind in ("mixed", "dead", "live"):
        c = G.case(d, a, bs, kind)
        r = torch.exp(c.reference()["log_ratio"])
        assert float((torch.log(r) - c.l).abs().max()) < 1e-5                    # float32 rounding of old_logp, nothing more
        for clip in (0.1, 0.2, 0.3):
            assert float(((r - 1.0).abs() - clip).abs().min()) > 0.045
        A = c.adv.double()
        if kind == "mixed":
            assert int((A == 0).sum()) == G.ZEROS and bool(torch.signbit(c.adv[c.zeros]).any()) and not bool(torch.signbit(c.adv[c.zeros]).all())
            live = torch.ones(bs, dtype=torch.bool); live[c.zeros] = False
            counts = torch.bincount(c.combo[live], minlength=8)
            assert counts.tolist() == [(bs - G.ZEROS) // 8] * 8
            assert float(A[live].abs().min()) >= 0.5
        elif kind == "dead":
            assert bool(((A > 0) & (c.l == 0.5) | (A < 0) & (c.l == -0.5)).all())
        else:
            assert bool(((A > 0) & (c.l == -0.5) | (A < 0) & (c.l == 0.5)).all())


@pytest.mark.parametrize("d,a,bs", GRID, ids=IDS)
def test_every_clipping_case_lies_on_its_side_of_the_threshold(d, a, bs):
    """The clipping test runs ``max_grad_norm`` = 0.25 N64 (active) and 4 N64 (inactive), N64 the restated norm: with the float32
    norm of the torch path within 8 epsilons of N64 (asserted above) and N64 itself far above the 1e-6 of the formula, both verdicts
    hold with a factor of almost 4 to spare; the raw runs (1e30) never clip.  Also prints where the default 0.5 falls."""
    for kind in ("mixed", "random"):
        m = G.measure(d, a, bs, kind)
        N = m["ref"]["norm"]
        print(f"\n[ppo grad cpu] {d}-{a}-{bs} {kind}: N64 = {N:.6g}, torch float32 total {m['norm32']:.6g} (rel {m['norm_err']:.2e}); "
              f"the default max_grad_norm 0.5 would {'clip' if N + 1e-6 > 0.5 else 'not clip'}")
        assert N > 1e-2 and N < G.BIG / 1e10
        for n32 in (N, m["norm32"]):
            assert 0.25 * N / (n32 + 1e-6) < 0.26 and 4.0 * N / (n32 + 1e-6) > 3.9
        # what a contribution missing from (or doubled in) the exchanged norm would do to the clip scalar, per tensor of the heads and
        # log_std -- the per-thread elements the exchange carries apart from the tiles: at least ten times the tolerance
        tol = G.K * m["norm_err"] + G.FLOOR_EPS * G.EPS32
        for n in ("log_std", "action_net.weight", "action_net.bias", "value_net.weight"):
            share = float((m["ref"]["grads"][n] ** 2).sum()) / N ** 2
            effect = abs(1.0 / (1.0 - share) ** 0.5 - 1.0)
            print(f"[ppo grad cpu]     without {n:18s} the clip scalar moves by {effect:.3e} = {effect / tol:.0f} x the tolerance")
            assert effect > 10 * tol, (n, share, tol)


@pytest.mark.parametrize("kind,over", HYPER, ids=HYPER_IDS)
@pytest.mark.parametrize("d,a,bs", G.HYPER_SHAPES, ids=["28-4-128", "21-6-64"])
def test_the_restatement_follows_the_hyper_parameters(d, a, bs, kind, over):
    m = G.measure(d, a, bs, kind, **over)
    print()
    _check(m, f"{d}-{a}-{bs} {kind} {over}")
    base = G.measure(d, a, bs, kind)
    moved = max(float((m["ref"]["grads"][n] - base["ref"]["grads"][n]).abs().max()) / base["scale"][n] for n in base["scale"])
    if "clip_range" in over and kind == "mixed":
        assert moved == 0.0                      # every ratio is clear of all three ranges: the same branches, the same gradient
    elif over != dict(normalize_advantage=False):                                # (that one is the case's own setting)
        assert moved > 1e-2, "the hyper-parameter does not reach the gradient"
    if "clip_range" in over and kind == "random":
        band, measured = G.case(d, a, bs, kind).band_count(over["clip_range"])
        assert band == 0, "choose another seed for this shape (ppo_grad_cases.SEEDS)"
    # normalised advantages: no sample so close to zero that its sign (and so its branch) hangs on rounding
    if kind == "mixed" and over.get("normalize_advantage", False):
        assert float(m["ref"]["adv_used"].abs().min()) > 1e-3
