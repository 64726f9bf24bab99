"""TD3 without a GPU: the exported symbols, TD3Config and the options it refuses, the layout of the flat image and its pack -> unpack
round trip, and td3_update_torch against the restatement of tests/td3_cases.py (torch.autograd.grad and a hand-written Adam)."""
import ctypes as C
import os
import re

import pytest
import torch

from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import sac as S
from pyflyt_drone_amd import td3 as T

import td3_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fw_sizeof_td3_hyper", "fw_td3_param_count", "fw_td3_update_workspace_bytes", "fw_td3_act", "fw_td3_update")


def test_symbols_are_exported_and_declared_and_the_abi_stays_at_7():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fwsim.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b" + name + r"\s*\(", text), name
    assert K.FW_ABI_VERSION == 7 and L.fw_abi_version() == 7 and "#define FW_ABI_VERSION 7" in open(os.path.join(ROOT, "include", "fwsim.h")).read()
    assert L.fw_sizeof_td3_hyper() == C.sizeof(T._Td3Hyper) == 40
    assert (T.ACT_EXPLORE, T.ACT_DETERMINISTIC, T.ACT_WARMUP) == (S.ACT_STOCHASTIC, S.ACT_DETERMINISTIC, S.ACT_WARMUP)


def test_config_defaults_validation_and_refused_options():
    cfg = T.TD3Config()
    assert (cfg.learning_rate, cfg.buffer_size, cfg.batch_size, cfg.gamma, cfg.tau) == (1e-3, 1_000_000, 256, 0.99, 0.005)
    assert (cfg.policy_delay, cfg.target_policy_noise, cfg.target_noise_clip, cfg.learning_starts, cfg.gradient_steps) == (2, 0.2, 0.5, 100, 1)
    assert cfg.net_arch == (256, 256) and cfg.action_noise_sigma == 0.1 and cfg.hidden == 256          # the two departures from SB3
    assert "(400, 300)" in T.TD3Config.__doc__ and "action_noise" in T.TD3Config.__doc__
    assert T.TD3Config(gradient_steps=-1).resolved_gradient_steps(16) == 16 and T.TD3Config(her_goals=4).her_relabel_prob == 0.8
    for bad in (dict(policy_delay=0), dict(policy_delay=9), dict(policy_delay=2.5), dict(policy_delay=True), dict(net_arch=(256, 64)),
                dict(batch_size=0), dict(tau=0.0), dict(gamma=1.5), dict(gradient_steps=-2), dict(target_policy_noise=-0.1),
                dict(action_noise_sigma=float("nan")), dict(n_steps=17), dict(n_steps=3, her_goals=2), dict(her_horizon=65),
                dict(episode_fold="two"), dict(stats_window_size=0)):
        with pytest.raises(ValueError):
            T.TD3Config(**bad)
    for refused in (dict(prioritized=True), dict(normalize_obs=True), dict(normalize_reward=True)):
        with pytest.raises(ValueError, match="not built"):
            T.TD3Config(**refused)
    assert T.TD3Config(policy_delay=8).policy_delay == 8 and T.TD3Config(policy_delay=1.0).policy_delay == 1
    assert T.fits(21, 6, 256, 256) and T.fits(64, 8, 64, 16) and T.fits(21, 6, 64, 512)
    for d, a, h, b in ((65, 6, 256, 256), (21, 9, 256, 256), (21, 6, 128, 256), (21, 6, 256, 24), (21, 6, 256, 8), (21, 6, 256, 528), (21, 6, 256, 1024)):
        assert not T.fits(d, a, h, b)


@pytest.mark.parametrize("d,A,H", [(21, 6, 256), (30, 3, 64), (2, 1, 64)])
def test_the_python_layout_is_the_librarys(d, A, H):
    L = _lib.lib()
    lay = T.image_layout(d, A, H)
    na, nc = S.net_floats(d, H, A), S.net_floats(d + A, H, 1)
    assert L.fw_td3_param_count(d, A, H) == lay["total"] == 4 * (na + 2 * nc) + 4
    assert [lay[k] for k in T.NETS] == [0, na, na + nc, na + 2 * nc, 2 * na + 2 * nc, 2 * na + 3 * nc]
    assert lay["exp_avg"] == 2 * lay["trained"] and lay["exp_avg_sq"] == 3 * lay["trained"] and lay["tail"] == 4 * lay["trained"]
    assert L.fw_td3_param_count(d, A, 128) == K.FW_EUNSUPPORTED and L.fw_td3_param_count(d, 9, H) == K.FW_EUNSUPPORTED
    assert L.fw_td3_param_count(0, A, H) == K.FW_EINVAL
    assert L.fw_td3_update_workspace_bytes(d, A, H, 24) == K.FW_EUNSUPPORTED and L.fw_td3_update_workspace_bytes(d, A, H, 528) == K.FW_EUNSUPPORTED
    assert L.fw_td3_update_workspace_bytes(d, A, H, 8) == K.FW_EUNSUPPORTED and L.fw_td3_update_workspace_bytes(d, A, H, 0) == K.FW_EINVAL
    assert L.fw_td3_update_workspace_bytes(d, A, H, 512) > L.fw_td3_update_workspace_bytes(d, A, H, 16) > 0


def _three_steps(d, A, H, B, seed, dtype=torch.float32):
    cfg = T.TD3Config(batch_size=B, net_arch=(H, H), policy_delay=2)
    pol, opts = TC.learner(TC.make_policy(d, A, H, seed), cfg, dtype=dtype)
    rows = TC.make_batch(d, A, B, seed).to(dtype)
    for step in range(3):
        T.td3_update_torch(pol, opts, rows, TC.make_noise(A, B, seed, step).to(dtype), cfg)
    return cfg, pol, opts, rows


def test_pack_unpack_round_trip_on_cpu_tensors():
    d, A, H, B = 21, 6, 64, 32
    cfg, pa, oa, rows = _three_steps(d, A, H, B, 1)
    assert (pa.n_updates, pa.n_actor_updates) == (3, 1)
    fa = T.FusedTd3Update(pa, oa, cfg)
    fa.pack()
    assert fa.current()
    L = fa.L
    assert fa.image[L["tail"]:].view(torch.int32).tolist() == [3, 1, 0, 0]
    # W[in][out] = weight^T, biases behind their weights, the moments and the target at the parameter's offset of their blocks
    w1, q2b = pa.actor[0].weight, pa.q2[4].bias
    assert torch.equal(fa.image[:d * H].view(d, H), w1.t())
    assert torch.equal(fa.image[L["actor_target"]:L["actor_target"] + d * H].view(d, H), pa.actor_target[0].weight.t())
    assert torch.equal(fa.image[L["exp_avg"]:L["exp_avg"] + d * H].view(d, H), oa["actor"].state[w1]["exp_avg"].t())
    assert float(fa.image[L["q1_target"] - 1]) == float(pa.actor_target[4].bias.detach()[-1]) and float(fa.image[L["trained"] - 1]) == float(q2b.detach()[0])
    assert float(fa.image[L["exp_avg_sq"] + L["trained"] - 1]) == float(oa["critic"].state[q2b]["exp_avg_sq"][0])
    pb, ob = TC.learner(TC.make_policy(d, A, H, 2), cfg)
    fb = T.FusedTd3Update(pb, ob, cfg)
    fb.image.copy_(fa.image)
    fb.unpack()
    assert (pb.n_updates, pb.n_actor_updates) == (3, 1) and fb.current()
    for x, y in zip(pa.parameters(), pb.parameters()):
        assert torch.equal(x, y)
    for key, steps in (("actor", 1.0), ("critic", 3.0)):
        for x, y in zip(oa[key].param_groups[0]["params"], ob[key].param_groups[0]["params"]):
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(oa[key].state[x][k], ob[key].state[y][k])
            assert float(ob[key].state[y]["step"]) == steps          # the actor's Adam counts its own steps
    # the guard: an in-place write to a parameter, a target or a moment is seen
    with torch.no_grad():
        pb.actor_target[0].bias.add_(1.0)
    assert not fb.current()
    fb.pack()
    assert fb.current()
    ob["critic"].state[pb.q1[0].weight]["exp_avg"].mul_(2.0)
    assert not fb.current()
    # ... and the torch path goes on from the unpacked state exactly as from the original (a step with the actor part)
    pc, oc = TC.learner(TC.make_policy(d, A, H, 2), cfg)
    fc = T.FusedTd3Update(pc, oc, cfg)
    fc.image.copy_(fa.image); fc.unpack()
    eps = TC.make_noise(A, B, 1, 3)
    T.td3_update_torch(pa, oa, rows, eps, cfg); T.td3_update_torch(pc, oc, rows, eps, cfg)
    assert (pc.n_updates, pc.n_actor_updates) == (4, 2)
    for x, y in zip(pa.parameters(), pc.parameters()):
        assert torch.equal(x, y)


def _state(pol, opts):
    """Clones of what a step without the actor part must leave alone: the actor, its moments, all three targets."""
    keep = [q.detach().clone() for name in ("actor", "actor_target", "q1_target", "q2_target") for q in getattr(pol, name).parameters()]
    for q in pol.actor.parameters():
        st = opts["actor"].state.get(q)
        if st:
            keep += [st["exp_avg"].clone(), st["exp_avg_sq"].clone(), torch.as_tensor(float(st["step"]))]
    return keep


@pytest.mark.parametrize("d,A,H,B", [(21, 6, 64, 32), (30, 3, 64, 16)])
def test_torch_update_against_the_restatement(d, A, H, B):
    """Three steps with policy_delay 2 in float64, both sides: step 2 carries the actor part, steps 1 and 3 do not.  The noise is
    1.5 x N(0, 1), so with target_policy_noise 0.2 the smoothing clip (0.5) holds the elements with |eps| > 1.67, and the actor's output
    bias of +-1 puts tanh near +-0.76, so the action clamp holds part of the smoothed actions: both are conditions of the test."""
    seed = 5
    cfg = T.TD3Config(batch_size=B, net_arch=(H, H), policy_delay=2)
    pol, opts = TC.learner(TC.make_policy(d, A, H, seed), cfg, dtype=torch.float64)
    ref = TC.Restated(pol, cfg.learning_rate)
    rows = TC.make_batch(d, A, B, seed).double()
    for step in range(3):
        eps = TC.make_noise(A, B, seed, step, scale=1.5).double()
        before = _state(pol, opts)
        got = T.td3_update_torch(pol, opts, rows, eps, cfg)
        with_actor = step == 1
        want_c, want_a, clipped, clamped = ref.step(rows, eps, cfg, with_actor, d, A)
        print(f"step {step + 1}: smoothing clip holds {clipped:.3f} of the noise, the action clamp {clamped:.3f} of the target actions")
        assert clipped > 0.0 and clamped > 0.0, "the pinned inputs do not reach both clamps"
        assert clipped < 0.5 and clamped < 0.5, "the pinned inputs sit in the clamps almost everywhere"
        assert ("actor_loss" in got) == with_actor
        assert float(got["critic_loss"]) == pytest.approx(float(want_c), rel=1e-10)
        if with_actor:
            assert float(got["actor_loss"]) == pytest.approx(float(want_a), rel=1e-10)
        else:                  # the actor, its moments and all three targets: bit-identical to before
            after = _state(pol, opts)
            assert len(after) == len(before) and all(torch.equal(x, y) for x, y in zip(before, after))
        assert (pol.n_updates, pol.n_actor_updates) == (ref.n_updates, ref.n_actor_updates) == (step + 1, int(step >= 1))
        for name in T.NETS:
            for (n, x), y in zip(getattr(pol, name).named_parameters(), ref.p[name]):
                torch.testing.assert_close(x.detach(), y, rtol=1e-9, atol=1e-12, msg=lambda m: f"step {step + 1} {name}.{n}: {m}")
        for key, names in (("actor", ("actor",)), ("critic", ("q1", "q2"))):
            if key == "actor" and step == 0:
                assert not opts["actor"].state
                continue
            qs = [q for name in names for q in getattr(pol, name).parameters()]
            ms = [m for name in names for m in ref.m[name]]
            vs = [v for name in names for v in ref.v[name]]
            for q, m, v in zip(qs, ms, vs):
                torch.testing.assert_close(opts[key].state[q]["exp_avg"], m, rtol=1e-9, atol=1e-15)
                torch.testing.assert_close(opts[key].state[q]["exp_avg_sq"], v, rtol=1e-9, atol=1e-20)
    # the targets did move on step 2, and by tau
    fresh = TC.make_policy(d, A, H, seed).double()
    moved = max(float((x - y).abs().max()) for x, y in zip(pol.q1_target.parameters(), fresh.q1_target.parameters()))
    # two critic steps, scaled by tau; an Adam step is at most lr (1 - beta1) / sqrt(1 - beta2) = 3.17 lr
    assert 0.0 < moved <= cfg.tau * 2 * cfg.learning_rate * 3.17


@pytest.mark.parametrize("seed", TC.SEEDS)
@pytest.mark.parametrize("d,A,H,B", TC.SHAPES)
def test_update_in_float32_matches_float64(d, A, H, B, seed):
    """The pinned inputs of the GPU parity test (tests/test_td3_gpu.py): no element of any parameter or Adam moment may leave the learner
    tolerances after four steps with policy_delay 2, so the GPU test's bound is one the arithmetic itself keeps."""
    cfg = T.TD3Config(batch_size=B, net_arch=(H, H), policy_delay=2)
    pol = TC.make_policy(d, A, H, seed)
    rows = TC.make_batch(d, A, B, seed)
    p32, o32 = TC.learner(pol, cfg)
    p64, o64 = TC.learner(pol, cfg, dtype=torch.float64)
    for step in range(4):
        eps = TC.make_noise(A, B, seed, step)
        T.td3_update_torch(p32, o32, rows, eps, cfg)
        T.td3_update_torch(p64, o64, rows.double(), eps.double(), cfg)
        TC.compare(p32, o32, p64, o64)
    assert (p32.n_updates, p32.n_actor_updates) == (4, 2)


def test_policy_forward_has_the_evaluators_shape():
    pol = TC.make_policy(21, 6, 64, 3)
    a, v, lp = pol(torch.randn(5, 21, dtype=torch.float64), deterministic=True)
    assert a.shape == (5, 6) and v.shape == (5,) and lp.shape == (5,) and float(lp.abs().sum()) == 0.0 and float(a.detach().abs().max()) <= 1.0
    assert torch.equal(pol(torch.zeros(2, 21), deterministic=False)[0], pol(torch.zeros(2, 21))[0])
