"""SAC without a GPU: sac_update_torch in float32 against float64, one hand-computed gradient step, the numpy model of the replay
ring, SACConfig / fits, and the pack -> unpack round trip of the flat image."""
import math

import numpy as np
import pytest
import torch

from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import sac as S

import sac_cases as SC


# ------------------------------------------------------------------------------------------------ 1. float32 against float64
@pytest.mark.parametrize("seed", SC.SEEDS)
@pytest.mark.parametrize("d,A,H,B", SC.SHAPES)
def test_update_in_float32_matches_float64(d, A, H, B, seed):
    """The pinned inputs of the GPU parity test (tests/test_sac_gpu.py): no element of any parameter or Adam moment may leave the
    learner tolerances after 1 and after 3 gradient steps."""
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), seed=seed)
    pol = SC.make_policy(d, A, H, seed)
    rows = SC.make_batch(d, A, B, seed)
    p32, o32 = SC.learner(pol, cfg)
    p64, o64 = SC.learner(pol, cfg, dtype=torch.float64)
    for step in range(3):
        eps = SC.make_noise(A, B, seed, step)
        s32 = S.sac_update_torch(p32, o32, rows, eps[0], eps[1], cfg)
        s64 = S.sac_update_torch(p64, o64, rows.double(), eps[0].double(), eps[1].double(), cfg)
        if step in (0, 2):
            SC.compare(p32, o32, p64, o64)
            for k in S.SCALARS:
                assert float(s32[k]) == pytest.approx(float(s64[k]), rel=2e-3, abs=1e-5), k
    assert p32.n_updates == 3


# ------------------------------------------------------------------------------------------------ 2. one step by hand
def _np_net(net):
    return [(l.weight.detach().double().numpy().copy(), l.bias.detach().double().numpy().copy()) for l in (net[0], net[2], net[4])]


def _np_forward(params, x):
    (w1, b1), (w2, b2), (w3, b3) = params
    h1 = np.maximum(x @ w1.T + b1, 0.0)
    h2 = np.maximum(h1 @ w2.T + b2, 0.0)
    return h2 @ w3.T + b3, h1, h2


def _np_critic_first_adam_step(params, x, y, lr, eps=1e-8):
    """The critic after ONE Adam step from zero moments on 0.5 mse(Q(x), y): back-propagation by hand, p -= lr g / (|g| + eps)."""
    (w1, b1), (w2, b2), (w3, b3) = params
    q, h1, h2 = _np_forward(params, x)
    n = x.shape[0]
    g3 = (q[:, 0] - y)[:, None] / n                       # d(0.5 mean (q - y)^2) / dq
    gw3, gb3 = g3.T @ h2, g3.sum(0)
    g2 = (g3 @ w3) * (h2 > 0)
    gw2, gb2 = g2.T @ h1, g2.sum(0)
    g1 = (g2 @ w2) * (h1 > 0)
    gw1, gb1 = g1.T @ x, g1.sum(0)
    step = lambda p, g: p - lr * g / (np.abs(g) + eps)
    return [(step(w1, gw1), step(b1, gb1)), (step(w2, gw2), step(b2, gb2)), (step(w3, gw3), step(b3, gb3))]


def test_one_step_by_hand_pins_the_order():
    """Two samples, d = 2, A = 1, H = 64, float64, a large learning rate: the target uses alpha of BEFORE the ent-coef step, the actor
    loss the critics of AFTER theirs -- either order the other way round moves the checked figures by far more than the bound."""
    d, A, H, lr, gamma = 2, 1, 64, 0.05, 0.99
    cfg = S.SACConfig(batch_size=16, net_arch=(H, H), learning_rate=lr, gamma=gamma)
    pol = SC.make_policy(d, A, H, 3).double()
    with torch.no_grad():
        pol.log_ent_coef.fill_(0.5)
    opts = S.make_optimizers(pol, cfg)
    s = np.array([[0.3, -1.2], [1.1, 0.4]]); a = np.array([[0.5], [-0.7]]); r = np.array([1.0, -2.0])
    s2 = np.array([[0.2, -1.0], [1.3, 0.1]]); done = np.array([0.0, 1.0])
    eps = np.array([[0.4], [-1.1]]); eps2 = np.array([[-0.6], [0.9]])
    actor, q1, q2 = _np_net(pol.actor), _np_net(pol.q1), _np_net(pol.q2)

    def sample(obs, e):
        out = _np_forward(actor, obs)[0]
        mean, ls = out[:, :A], np.clip(out[:, A:], -20.0, 2.0)
        act = np.tanh(mean + np.exp(ls) * e)
        logp = (-0.5 * e * e - ls - 0.5 * math.log(2 * math.pi)).sum(1) - np.log(1.0 - act * act + 1e-6).sum(1)
        return act, logp

    a_pi, logp = sample(s, eps)
    alpha = math.exp(0.5)
    g_lec = -(logp.mean() - A)
    lec_new = 0.5 - lr * g_lec / (abs(g_lec) + 1e-8)
    a2, logp2 = sample(s2, eps2)
    x2 = np.concatenate([s2, a2], 1)
    qmin2 = np.minimum(_np_forward(q1, x2)[0][:, 0], _np_forward(q2, x2)[0][:, 0])
    y = r + (1.0 - done) * gamma * (qmin2 - alpha * logp2)
    x = np.concatenate([s, a], 1)
    critic_loss = 0.5 * (((_np_forward(q1, x)[0][:, 0] - y) ** 2).mean() + ((_np_forward(q2, x)[0][:, 0] - y) ** 2).mean())
    q1n, q2n = _np_critic_first_adam_step(q1, x, y, lr), _np_critic_first_adam_step(q2, x, y, lr)
    xp = np.concatenate([s, a_pi], 1)
    actor_loss = (alpha * logp - np.minimum(_np_forward(q1n, xp)[0][:, 0], _np_forward(q2n, xp)[0][:, 0])).mean()
    actor_loss_old_critics = (alpha * logp - np.minimum(_np_forward(q1, xp)[0][:, 0], _np_forward(q2, xp)[0][:, 0])).mean()

    t = lambda v: torch.as_tensor(v, dtype=torch.float64)
    got = S.sac_update_torch(pol, opts, (t(s), t(a), t(r), t(s2), t(done)), t(eps), t(eps2), cfg)
    assert float(got["ent_coef"]) == pytest.approx(alpha, rel=1e-12)
    assert float(got["mean_logp"]) == pytest.approx(logp.mean(), rel=1e-10)
    assert float(got["critic_loss"]) == pytest.approx(critic_loss, rel=1e-10)
    assert float(got["actor_loss"]) == pytest.approx(actor_loss, rel=1e-9, abs=1e-10)
    assert abs(actor_loss - actor_loss_old_critics) > 1e-3, "the case does not tell the stepped critics from the old ones"
    y_new_alpha = r + (1.0 - done) * gamma * (qmin2 - math.exp(lec_new) * logp2)
    assert abs(y_new_alpha[0] - y[0]) > 1e-3, "the case does not tell the old alpha from the new one"
    # sign and size of the log_ent_coef step: one Adam step from zero moments moves it by lr against the gradient's sign
    assert pol.log_ent_coef.item() == pytest.approx(lec_new, rel=1e-12)
    assert abs(pol.log_ent_coef.item() - 0.5) == pytest.approx(lr, rel=1e-6) and (pol.log_ent_coef.item() - 0.5) * g_lec < 0
    for got_net, want in ((pol.q1, q1n), (pol.q2, q2n)):
        for (w, b), (gw, gb) in zip(want, _np_net(got_net)):
            np.testing.assert_allclose(gw, w, rtol=1e-9, atol=1e-12); np.testing.assert_allclose(gb, b, rtol=1e-9, atol=1e-12)
    # Polyak after the step: tau of the stepped critic
    for tgt, old, new in ((pol.q1_target, q1, q1n), (pol.q2_target, q2, q2n)):
        for (w, b), (ow, ob), (nw, nb) in zip(_np_net(tgt), old, new):
            np.testing.assert_allclose(w, (1 - cfg.tau) * ow + cfg.tau * nw, rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(b, (1 - cfg.tau) * ob + cfg.tau * nb, rtol=1e-12, atol=1e-15)


# ------------------------------------------------------------------------------------------------ 3. the ring model
def test_numpy_ring_against_hand_made_expectations():
    n, d, a = 2, 2, 1
    ring = SC.NumpyRing(7, n, d, a)                       # 7 // 2 * 2 = 6 rows
    assert ring.capacity == 6 and ring.ring.shape == (6, 7)
    f = lambda *v: np.array(v, dtype=np.float32)
    for k in range(4):
        obs = np.array([[10 * k + 1, 10 * k + 2], [10 * k + 3, 10 * k + 4]], dtype=np.float32)
        ring.store(obs, f([0.1 * k], [-0.1 * k]), f(k, -k), obs + 100, obs + 1000,
                   terminated=np.array([k == 1, 0], dtype=np.uint8), truncated=np.array([0, k == 2], dtype=np.uint8))
    assert ring.counters == [2, 6, 4]                     # four stores of 2 rows into 6: wrapped once
    # step 3 overwrote rows 0-1; rows 2-3 are step 1 (env 0 terminated: terminal obs, done 1); rows 4-5 step 2 (env 1 truncated only:
    # terminal obs, done 0 -- a time-limit end bootstraps)
    np.testing.assert_array_equal(ring.ring[0], f(31, 32, 0.3, 3, 131, 132, 0))
    np.testing.assert_array_equal(ring.ring[1], f(33, 34, -0.3, -3, 133, 134, 0))
    np.testing.assert_array_equal(ring.ring[2], f(11, 12, 0.1, 1, 1011, 1012, 1))
    np.testing.assert_array_equal(ring.ring[3], f(13, 14, -0.1, -1, 113, 114, 0))
    np.testing.assert_array_equal(ring.ring[4], f(21, 22, 0.2, 2, 121, 122, 0))
    np.testing.assert_array_equal(ring.ring[5], f(23, 24, -0.2, -2, 1023, 1024, 0))
    assert S.ring_capacity(7, 2) == 6 and S.ring_capacity(200_000, 16) == 200_000 and S.ring_capacity(100, 32) == 96
    with pytest.raises(ValueError):
        S.ring_capacity(3, 4)


# ------------------------------------------------------------------------------------------------ 4. config, limits, the image
def test_config_validation_and_limits():
    cfg = S.SACConfig()
    assert (cfg.learning_rate, cfg.buffer_size, cfg.batch_size, cfg.gamma, cfg.tau) == (3e-4, 200_000, 256, 0.99, 0.02)
    assert (cfg.gradient_steps, cfg.target_update_interval, cfg.learning_starts, cfg.ent_coef, cfg.net_arch) == (1, 1, 100, "auto", (256, 256))
    assert cfg.auto_ent and cfg.hidden == 256 and cfg.resolved_gradient_steps(16) == 1
    assert S.SACConfig(gradient_steps=-1).resolved_gradient_steps(16) == 16
    assert not S.SACConfig(ent_coef=0.2).auto_ent
    for bad in (dict(gradient_steps=-2), dict(net_arch=(256, 64)), dict(net_arch=(64,)), dict(batch_size=0), dict(tau=0.0),
                dict(target_update_interval=0), dict(ent_coef=-1.0), dict(gamma=1.5)):
        with pytest.raises(ValueError):
            S.SACConfig(**bad)
    assert S.fits(21, 6, 256, 256) and S.fits(64, 8, 64, 16) and S.fits(21, 6, 64, 512)
    for d, a, h, b in ((65, 6, 256, 256), (21, 9, 256, 256), (21, 6, 128, 256), (21, 6, 256, 24), (21, 6, 256, 8), (21, 6, 256, 528)):
        assert not S.fits(d, a, h, b)


@pytest.mark.parametrize("d,A,H", [(21, 6, 256), (30, 3, 64), (2, 1, 64)])
def test_the_python_layout_is_the_librarys(d, A, H):
    L = _lib.lib()
    assert L.fw_sac_param_count(d, A, H) == S.image_layout(d, A, H)["total"]
    assert L.fw_sizeof_sac_hyper() == __import__("ctypes").sizeof(S._SacHyper)
    from pyflyt_drone_amd import config as K
    assert L.fw_sac_param_count(d, A, 128) == K.FW_EUNSUPPORTED and L.fw_sac_param_count(d, 9, H) == K.FW_EUNSUPPORTED
    assert L.fw_sac_update_workspace_bytes(d, A, H, 24) == K.FW_EUNSUPPORTED and L.fw_sac_param_count(0, A, H) == K.FW_EINVAL


def test_pack_unpack_round_trip_on_cpu_tensors():
    d, A, H, B = 21, 6, 64, 32
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), target_update_interval=2)
    pa, oa = SC.learner(SC.make_policy(d, A, H, 1), cfg)
    rows = SC.make_batch(d, A, B, 1)
    for step in range(3):
        eps = SC.make_noise(A, B, 1, step)
        S.sac_update_torch(pa, oa, rows, eps[0], eps[1], cfg)
    fa = S.FusedSacUpdate(pa, oa, cfg)
    fa.pack()
    assert fa.current()
    L = fa.L
    assert int(fa.image[L["tail"]:].view(torch.int32)[0]) == 3
    # W[in][out] = weight^T, biases behind their weights, the moments at the parameter's offset of their blocks
    w1 = pa.actor[0].weight
    assert torch.equal(fa.image[:d * H].view(d, H), w1.t())
    assert torch.equal(fa.image[L["exp_avg"]:L["exp_avg"] + d * H].view(d, H), oa["actor"].state[w1]["exp_avg"].t())
    assert float(fa.image[L["log_ent_coef"]]) == pa.log_ent_coef.item()
    pb, ob = SC.learner(SC.make_policy(d, A, H, 2), cfg)
    fb = S.FusedSacUpdate(pb, ob, cfg)
    fb.image.copy_(fa.image)
    fb.unpack()
    assert pb.n_updates == 3 and fb.current()
    for x, y in zip(pa.parameters(), pb.parameters()):
        assert torch.equal(x, y)
    for key in ("actor", "critic", "ent"):
        for x, y in zip(oa[key].param_groups[0]["params"], ob[key].param_groups[0]["params"]):
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(oa[key].state[x][k], ob[key].state[y][k])
            assert float(ob[key].state[y]["step"]) == 3.0
    # the guard: an in-place write to a parameter or a moment is seen
    with torch.no_grad():
        pb.q1[0].bias.add_(1.0)
    assert not fb.current()
    fb.pack()
    assert fb.current()
    ob["actor"].state[pb.actor[0].weight]["exp_avg"].mul_(2.0)
    assert not fb.current()
    # ... and the torch path goes on from the unpacked state exactly as from the original
    pc, oc = SC.learner(SC.make_policy(d, A, H, 2), cfg)
    fc = S.FusedSacUpdate(pc, oc, cfg)
    fc.image.copy_(fa.image); fc.unpack()
    eps = SC.make_noise(A, B, 1, 3)
    S.sac_update_torch(pa, oa, rows, eps[0], eps[1], cfg); S.sac_update_torch(pc, oc, rows, eps[0], eps[1], cfg)
    for x, y in zip(pa.parameters(), pc.parameters()):
        assert torch.equal(x, y)
