"""The SAC kernels (fw_sac_act, fw_replay_store / _sample, fw_sac_noise, fw_sac_update) against torch and a numpy ring, and the
learner (sac.SAC) end to end on the low-level env."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib, evaluate
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R
from pyflyt_drone_amd import sac as S

import sac_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
_p = S._p


def _counters(cursor=0, size=0, steps=0, grad=0):
    return torch.tensor([cursor, size, steps, grad], dtype=torch.int64, device=DEV)


def _image(pol, cfg):
    f = S.FusedSacUpdate(pol, S.make_optimizers(pol, cfg), cfg)
    f.pack()
    return f.image


def _act(image, obs, A, H, mode, seed, ctr, env_offset=0):
    n, d = obs.shape
    out = dict(act=torch.full((n, A), 9.0, device=DEV), env=torch.full((n, A), 9.0, device=DEV, dtype=obs.dtype),
               stage=torch.full((n, d), 9.0, device=DEV), logp=torch.full((n,), 9.0, device=DEV), eps=torch.full((n, A), 9.0, device=DEV))
    _lib.check(_lib.lib().fw_sac_act(_p(image), _p(obs), int(obs.dtype == torch.float64), n, d, A, H, mode, seed, env_offset, _p(ctr),
                                     _p(out["act"]), _p(out["env"]), _p(out["stage"]), _p(out["logp"]), _p(out["eps"]), None))
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ 1. act
# The (seed, step counter) of the act parity case: with sigma near 1 and six components about 3 % of the rows have max|u| > 3 in torch
# alone, so of 64 rows a draw leaves out 0 to 5 (seeds 1 to 8 at this counter: 0-3 at H 64, 2-5 at H 256); this one leaves out 1 and 2.
ACT_SEED, ACT_STEP = 5, 7


@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_act_against_torch(H, dtype):
    n, d, A, seed = 64, 21, 6, ACT_SEED
    cfg = S.SACConfig(net_arch=(H, H), seed=seed)
    pol = SC.make_policy(d, A, H, 11, perturb=0.1).to(DEV)
    img = _image(pol, cfg)
    g = torch.Generator(device=DEV).manual_seed(21)
    # (perturbed by 0.1, a 256-wide layer's pre-activations have a standard deviation of 0.1 sqrt(256) rms(h): unit-scale rows drive the
    # head's log_std into its clamp and |u| past 3 on a third of the rows in torch alone; rows of scale 0.25 keep sigma near 1)
    obs = (0.25 * torch.randn((n, d), device=DEV, generator=g)).to(dtype)
    ctr = _counters(steps=ACT_STEP)
    det = _act(img, obs, A, H, S.ACT_DETERMINISTIC, seed, ctr)
    sto = _act(img, obs, A, H, S.ACT_STOCHASTIC, seed, ctr)
    with torch.no_grad():
        x = obs.float()
        mean, ls = pol.dist(x)
        torch.testing.assert_close(det["act"], torch.tanh(mean), rtol=2e-3, atol=2e-5)
        a, logp = pol.sample(x, sto["eps"])
        torch.testing.assert_close(sto["act"], a, rtol=2e-3, atol=2e-5)
        u = mean + torch.exp(ls) * sto["eps"]
        keep = u.abs().amax(1) <= 3.0
        print(f"H {H}: {int((~keep).sum())} of {n} rows have max|u| > 3; worst |logp - torch| on the others "
              f"{float((sto['logp'] - logp)[keep].abs().max()):.3e}")
        assert int((~keep).sum()) <= 0.05 * n
        torch.testing.assert_close(sto["logp"][keep], logp[keep], rtol=2e-3, atol=2e-3)
    for o in (det, sto):
        assert torch.equal(o["env"], o["act"].to(dtype)) and torch.equal(o["stage"], obs.float())
    assert torch.equal(det["eps"], sto["eps"])          # the deterministic form reports the draw it did not use
    # the same (seed, counter) gives the same bits, the next counter, another seed and other envs different ones
    again = _act(img, obs, A, H, S.ACT_STOCHASTIC, seed, ctr)
    assert all(torch.equal(again[k], sto[k]) for k in sto)
    for other in (_act(img, obs, A, H, S.ACT_STOCHASTIC, seed, _counters(steps=ACT_STEP + 1)), _act(img, obs, A, H, S.ACT_STOCHASTIC, seed + 1, ctr),
                  _act(img, obs, A, H, S.ACT_STOCHASTIC, seed, ctr, env_offset=n)):
        assert not torch.equal(other["eps"], sto["eps"]) and not (other["eps"] == sto["eps"]).any()


def test_act_noise_statistics_and_warm_up():
    n, d, A, H, seed = 4096, 21, 6, 64, 2
    cfg = S.SACConfig(net_arch=(H, H), seed=seed)
    img = _image(SC.make_policy(d, A, H, 11).to(DEV), cfg)
    obs = torch.zeros((n, d), device=DEV, dtype=torch.float64)
    eps = _act(img, obs, A, H, S.ACT_STOCHASTIC, seed, _counters(steps=3))["eps"]
    print(f"eps over {eps.numel()} draws: mean {float(eps.mean()):+.4f}, var {float(eps.var()):.4f}")
    assert abs(float(eps.mean())) < 0.032 and abs(float(eps.var()) - 1.0) < 0.045          # five standard errors at n = 24 576
    assert len(torch.unique(eps)) > 0.99 * eps.numel()
    warm = _act(img, obs, A, H, S.ACT_WARMUP, seed, _counters(steps=3))
    a = warm["act"]
    assert bool((a >= -1.0).all()) and bool((a < 1.0).all())
    assert abs(float(a.mean())) < 5 * 0.577 / math.sqrt(a.numel())
    assert abs(float(a.var()) - 1.0 / 3.0) < 0.02 and len(torch.unique(a)) > 0.99 * a.numel()
    assert torch.equal(warm["env"], a.double()) and torch.equal(warm["stage"], obs.float())
    assert torch.equal(_act(img, obs, A, H, S.ACT_WARMUP, seed, _counters(steps=3))["act"], a)
    assert not torch.equal(_act(img, obs, A, H, S.ACT_WARMUP, seed, _counters(steps=4))["act"], a)


# ------------------------------------------------------------------------------------------------ 2. store and sample
def test_store_and_sample_against_the_numpy_ring():
    n, d, A, seed = 32, 21, 6, 9
    buf = S.ReplayBufferDevice(3 * n + 5, n, d, A, DEV)              # capacity rounds down to 3 N rows
    ref = SC.NumpyRing(3 * n + 5, n, d, A)
    assert buf.capacity == ref.capacity == 3 * n
    rng = np.random.default_rng(0)
    batch, idx = torch.zeros((64, buf.row), device=DEV), torch.zeros(64, dtype=torch.int32, device=DEV)
    for k in range(5):
        obs, act = rng.standard_normal((n, d)).astype(np.float32), rng.uniform(-1, 1, (n, A)).astype(np.float32)
        rew, nxt, tobs = rng.standard_normal(n), rng.standard_normal((n, d)), rng.standard_normal((n, d))
        term, trunc = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        term[[1, 5 + k]] = 1; trunc[[2, 5 + k, 20]] = 1              # terminated only, truncated only, both, neither
        t = lambda x: torch.as_tensor(x, device=DEV)
        buf.store(t(obs), t(act), t(rew), t(nxt), t(tobs), t(term), t(trunc))
        ref.store(obs, act, rew.astype(np.float32), nxt.astype(np.float32), tobs.astype(np.float32), term, trunc)
        assert np.array_equal(buf.ring.cpu().numpy(), ref.ring), k
        assert buf.counters.tolist() == ref.counters + [0], k
        if k < 3:                                                    # size 32, 64, 96
            buf.sample(seed, batch, idx)
            i = idx.cpu().numpy()
            assert i.min() >= 0 and i.max() < ref.size and len(np.unique(i)) > 1
            assert np.array_equal(batch.cpu().numpy(), ref.ring[i])
    assert ref.counters == [2 * n, 3 * n, 5]
    # float32 env tensors take the same path
    buf32, t32 = S.ReplayBufferDevice(3 * n, n, d, A, DEV), lambda x: torch.as_tensor(x, device=DEV, dtype=torch.float32)
    buf32.store(t(obs), t(act), t32(rew), t32(nxt), t32(tobs), t(term), t(trunc))
    assert np.array_equal(buf32.ring.cpu().numpy()[:n], ref.ring[ref.capacity - 2 * n:ref.capacity - n])
    # 64 gradient-step counters at size 96, B = 256: every row is drawn (a miss has probability ~96 e^-170); a counter repeats itself
    big, bidx = torch.zeros((256, buf.row), device=DEV), torch.zeros(256, dtype=torch.int32, device=DEV)
    seen, draws = np.zeros(ref.capacity, dtype=bool), []
    for c in range(64):
        buf.counters[S.CTR_GRAD] = c
        buf.sample(seed, big, bidx)
        i = bidx.cpu().numpy()
        assert i.min() >= 0 and i.max() < ref.capacity and np.array_equal(big.cpu().numpy(), ref.ring[i])
        seen[i] = True; draws.append(i.copy())
    assert seen.all()
    assert not np.array_equal(draws[0], draws[1])
    buf.counters[S.CTR_GRAD] = 0
    buf.sample(seed, big, bidx)
    assert np.array_equal(bidx.cpu().numpy(), draws[0])
    buf.sample(seed + 1, big, bidx)
    assert not np.array_equal(bidx.cpu().numpy(), draws[0])


# ------------------------------------------------------------------------------------------------ 3. update parity
def _parity(d, A, H, B, seed, interval=1, steps=3, check=(0, 2)):
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), seed=seed, target_update_interval=interval)
    pol = SC.make_policy(d, A, H, seed)
    rows = SC.make_batch(d, A, B, seed).to(DEV)
    pt, ot = SC.learner(pol, cfg, device=DEV)            # the torch learner
    pf, of = SC.learner(pol, cfg, device=DEV)            # the modules the image is unpacked into
    fused = S.FusedSacUpdate(pf, of, cfg)
    fused.pack()
    ctr_t, ctr_f = _counters(grad=40), _counters(grad=40)
    for step in range(steps):
        eps = S.sac_noise(seed, ctr_t, B, A)
        st = S.sac_update_torch(pt, ot, rows, eps[0], eps[1], cfg)
        ctr_t[S.CTR_GRAD] += 1
        fused.run(rows, ctr_f)
        if step in check:
            fused.unpack()
            assert pf.n_updates == step + 1 and ctr_f.tolist() == ctr_t.tolist()
            SC.compare(pf, of, pt, ot)
            sf = fused.scalars()
            print(f"step {step + 1}: fused {sf}")
            for k in S.SCALARS:
                assert sf[k] == pytest.approx(float(st[k]), rel=2e-3, abs=1e-5), (k, step)


@pytest.mark.parametrize("seed", SC.SEEDS)
@pytest.mark.parametrize("d,A,H,B", SC.SHAPES)
def test_fused_update_matches_the_torch_update(d, A, H, B, seed):
    _parity(d, A, H, B, seed)


def test_fused_update_with_a_target_interval_of_two_and_a_fixed_coefficient():
    _parity(21, 6, 64, 32, 5, interval=2, steps=4, check=(0, 1, 2, 3))
    d, A, H, B, seed = 21, 6, 64, 32, 6
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), seed=seed, ent_coef=0.2)
    pol = SC.make_policy(d, A, H, seed)
    rows = SC.make_batch(d, A, B, seed).to(DEV)
    pt, ot = SC.learner(pol, cfg, device=DEV); pf, of = SC.learner(pol, cfg, device=DEV)
    fused = S.FusedSacUpdate(pf, of, cfg); fused.pack()
    ctr = _counters()
    eps = S.sac_noise(seed, ctr, B, A)
    st = S.sac_update_torch(pt, ot, rows, eps[0], eps[1], cfg)
    fused.run(rows, ctr); fused.unpack()
    SC.compare(pf, of, pt, ot)
    assert fused.scalars()["ent_coef"] == pytest.approx(0.2) and pf.log_ent_coef.item() == 0.0
    assert fused.scalars()["actor_loss"] == pytest.approx(float(st["actor_loss"]), rel=2e-3, abs=1e-5)


def test_update_noise_is_the_noise_entry_points():
    """fw_sac_update draws what fw_sac_noise writes: a step whose noise differs would miss the parity above; here the stream itself."""
    B, A = 64, 6
    a, b = S.sac_noise(3, _counters(grad=5), B, A), S.sac_noise(3, _counters(grad=5), B, A)
    assert torch.equal(a, b) and not (a[0] == a[1]).any()
    assert not (S.sac_noise(3, _counters(grad=6), B, A) == a).any() and not (S.sac_noise(4, _counters(grad=5), B, A) == a).any()
    assert torch.equal(S.sac_noise(3, _counters(grad=5), 16, A), a[:, :16])          # a row's noise does not depend on the batch size
    big = S.sac_noise(3, _counters(grad=5), 512, 8)
    assert abs(float(big.mean())) < 5 / math.sqrt(big.numel()) and abs(float(big.var()) - 1.0) < 5 * math.sqrt(2.0 / big.numel())


# ------------------------------------------------------------------------------------------------ 4. determinism and replay
def _ring_learner(H, B, seed=5, d=21, A=6, rows=96):
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), seed=seed)
    pol = SC.make_policy(d, A, H, seed).to(DEV)
    fused = S.FusedSacUpdate(pol, S.make_optimizers(pol, cfg), cfg)
    fused.pack()
    buf = S.ReplayBufferDevice(rows, 32, d, A, DEV)
    buf.ring.copy_(SC.make_batch(d, A, rows, seed))
    buf.counters.copy_(_counters(size=rows))
    return cfg, fused, buf


@pytest.mark.parametrize("H,B", [(256, 256), (64, 32)])
def test_update_is_deterministic(H, B):
    out = []
    for _ in range(2):
        cfg, fused, buf = _ring_learner(H, B)
        batch = buf.sample(cfg.seed, torch.zeros((B, buf.row), device=DEV))
        fused.run(batch, buf.counters)
        torch.cuda.synchronize()
        out.append((fused.image.clone(), fused.out.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.isfinite(out[0][0]).all()


def test_eight_replayed_gradient_steps_equal_eight_eager_ones():
    H, B = 64, 64
    res = []
    for graph in (False, True):
        cfg, fused, buf = _ring_learner(H, B)
        batch, idx = torch.zeros((B, buf.row), device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
        hist = []

        def step():
            buf.sample(cfg.seed, batch, idx)
            fused.run(batch, buf.counters)

        if graph:
            step()                                   # loads the kernels; counts as the first step
            hist.append(idx.clone())
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            for _ in range(7):
                g.replay()
                hist.append(idx.clone())
        else:
            for _ in range(8):
                step()
                hist.append(idx.clone())
        torch.cuda.synchronize()
        res.append((fused.image.clone(), fused.out.clone(), buf.counters.clone(), torch.stack(hist)))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert res[0][2].tolist() == [0, 96, 0, 8]
    assert int(res[0][0][-4:].view(torch.int32)[0]) == 8
    assert len(torch.unique(res[0][3], dim=0)) == 8          # every step drew its own batch


# ------------------------------------------------------------------------------------------------ 5. the learner end to end
def _env(seed=3):
    return P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=4), 16, seed=seed)      # episodes end inside the run: terminal rows


def _sac(fused=True, graphs=False, **kw):
    cfg = S.SACConfig(batch_size=32, net_arch=(64, 64), learning_starts=32, gradient_steps=-1, seed=7, use_graphs=graphs,
                      fused_update=fused, buffer_size=16 * 40, **kw)
    return S.SAC(_env(), cfg)


def _run(sac, n):
    for _ in range(n):
        sac.collect_step()
    torch.cuda.synchronize()
    return sac


@pytest.fixture(scope="module")
def fused_run():
    return _run(_sac(), 6)


def test_learner_counts_and_buffer(fused_run):
    sac = fused_run
    assert sac.num_timesteps == 96 and sac.n_updates == 4 * 16 and sac.buffer.counters.tolist() == [96, 96, 6, 64]
    assert sac.policy.n_updates == 64 and sac.fused.ahead == 0
    assert all(torch.isfinite(p).all() for p in sac.policy.parameters())
    logs = sac.read_logs()
    assert all(math.isfinite(logs[k]) for k in S.SCALARS) and logs["n_updates"] == 64
    s, a, r, s2, done = S.split_rows(sac.buffer.ring[:96], 21, 6)
    assert bool((a >= -1).all()) and bool((a <= 1).all()) and bool(((done == 0) | (done == 1)).all())
    # one more vec-step (of a learner of its own: the fixture stays at six), checked against the env's tensors around it
    sac = _run(_sac(), 6)
    env = sac.env
    before, cursor = env.obs.clone(), sac.buffer.cursor
    sac.collect_step(train=False)
    torch.cuda.synchronize()
    ended = (env.terminated | env.truncated).bool()
    want = torch.cat([before.float(), sac.act_f32, env.rewards.float()[:, None],
                      torch.where(ended[:, None], env.terminal_obs, env.obs).float(), env.terminated.float()[:, None]], dim=1)
    assert torch.equal(sac.buffer.ring[cursor:cursor + 16], want)
    assert torch.equal(sac.act_env, sac.act_f32.double()) and sac.buffer.counters.tolist() == [112, 112, 7, 64]


def test_truncated_episodes_bootstrap():
    sac = _run(_sac(), 5)
    ring = sac.buffer.ring[:80]
    # max_episode_steps = 4: the fourth vec-step ends every surviving episode by the time limit; its rows carry the terminal
    # observation (not the reset one) and done = 0
    third, fourth, fifth = ring[32:48], ring[48:64], ring[64:80]
    alive = third[:, -1] == 0                                    # (an env that crashed at step 3 is one step into a new episode at step 4)
    assert bool(alive.any())
    assert torch.equal(third[alive, 28:49], fourth[alive, :21])  # inside an episode next_obs is the next row's obs ...
    assert not bool((fourth[alive, 28:49] == fifth[alive, :21]).all(1).any())      # ... at its end it is the terminal row, not the reset one
    assert bool((fourth[alive, -1] <= third[alive, -1] + 1).all())


def test_fused_and_torch_learners_agree(fused_run):
    a, b = fused_run, _run(_sac(fused=False), 6)
    assert b.n_updates == 64 and b.buffer.counters.tolist() == [96, 96, 6, 64]
    SC.compare(a.policy, a.optimizers, b.policy, b.optimizers)


def test_graph_replay_equals_eager_bit_for_bit():
    a, b = _run(_sac(), 6), _run(_sac(graphs=True), 6)
    assert len(b._graphs) == 2 and all(isinstance(g, torch.cuda.CUDAGraph) for g in b._graphs.values())
    assert torch.equal(a.fused.image, b.fused.image) and torch.equal(a.buffer.ring, b.buffer.ring)
    assert torch.equal(a.buffer.counters, b.buffer.counters) and torch.equal(a.fused.out, b.fused.out)
    assert torch.equal(a.env.obs, b.env.obs)
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)


def test_state_dict_round_trip_continues_bit_identically():
    a = _run(_sac(), 4)
    sd = a.state_dict(include_buffer=True)
    b = _sac()
    b.env.reset_tensor(); b._started = True
    b.env.set_state(a.env.get_state()); b.env.obs.copy_(a.env.obs)
    b.load_state_dict(sd)
    _run(a, 2); _run(b, 2)
    assert torch.equal(a.fused.image, b.fused.image) and torch.equal(a.buffer.ring, b.buffer.ring)
    assert a.buffer.counters.tolist() == b.buffer.counters.tolist() == [96, 96, 6, 64] and a.num_timesteps == b.num_timesteps == 96
    for (k, p), q in zip(a.policy.named_parameters(), b.policy.parameters()):
        assert torch.equal(p, q), k
    for key in ("actor", "critic", "ent"):
        for x, y in zip(a.optimizers[key].param_groups[0]["params"], b.optimizers[key].param_groups[0]["params"]):
            assert torch.equal(a.optimizers[key].state[x]["exp_avg_sq"], b.optimizers[key].state[y]["exp_avg_sq"])


def test_evaluate_policy_takes_the_sac_actor(fused_run):
    venv = P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=30), 16, seed=5)
    r = evaluate.evaluate_policy(fused_run.policy, R.VecNormalizeDevice(venv, training=False, norm_obs=False, norm_reward=False), 4)
    trk = r.tracking_scalars()
    assert len(r.episode_rewards) == 4 and trk and all(math.isfinite(v) for v in trk.values())
    a, v, lp = fused_run.policy(venv.obs, deterministic=True)
    assert a.shape == (16, 6) and v.shape == (16,) and lp.shape == (16,) and float(a.abs().max()) <= 1.0


# ------------------------------------------------------------------------------------------------ 6. errors
def test_unsupported_shapes_and_bad_arguments():
    L = _lib.lib()
    img, rows, ctr, out = (torch.zeros(4_000_00, device=DEV), torch.zeros((512, 60), device=DEV), _counters(), torch.zeros(8, device=DEV))
    ws = torch.zeros(1 << 24, dtype=torch.uint8, device=DEV)
    H = S._SacHyper(lr=3e-4, gamma=0.99, tau=0.02, beta1=0.9, beta2=0.999, eps=1e-8, target_entropy=-6.0, ent_coef=0.0, auto_ent=1,
                    target_update_interval=1, seed=1)
    upd = lambda d, A, Hh, B, image=img: L.fw_sac_update(_p(image), _p(rows), d, A, Hh, B, C.byref(H), _p(ctr), _p(out), _p(ws), ws.numel(), None)
    assert upd(21, 6, 128, 32) == K.FW_EUNSUPPORTED and b"hidden" in L.fw_last_error(None)
    assert upd(21, 6, 64, 24) == K.FW_EUNSUPPORTED and upd(21, 9, 64, 32) == K.FW_EUNSUPPORTED and upd(65, 6, 64, 32) == K.FW_EUNSUPPORTED
    assert upd(21, 6, 64, 528) == K.FW_EUNSUPPORTED and upd(21, 6, 64, 0) == K.FW_EINVAL and upd(21, 6, 64, 32, image=None) == K.FW_EINVAL
    assert L.fw_sac_update(_p(img), _p(rows), 21, 6, 64, 32, C.byref(H), _p(ctr), _p(out), _p(ws), 16, None) == K.FW_EINVAL
    obs = torch.zeros((16, 21), device=DEV, dtype=torch.float64)
    a32, a64, st = torch.zeros((16, 9), device=DEV), torch.zeros((16, 9), device=DEV, dtype=torch.float64), torch.zeros((16, 21), device=DEV)
    act = lambda A, Hh, n=16, image=img: L.fw_sac_act(_p(image), _p(obs), 1, n, 21, A, Hh, 0, 1, 0, _p(ctr), _p(a32), _p(a64), _p(st), None, None, None)
    assert act(6, 128) == K.FW_EUNSUPPORTED and act(9, 64) == K.FW_EUNSUPPORTED and act(6, 64, n=0) == K.FW_EINVAL
    assert act(6, 64, image=None) == K.FW_EINVAL
    assert L.fw_sac_noise(1, _p(ctr), 32, 9, _p(out), None) == K.FW_EUNSUPPORTED and L.fw_sac_noise(1, None, 32, 6, _p(out), None) == K.FW_EINVAL
    assert L.fw_replay_sample(None, 96, _p(ctr), 1, 50, 32, _p(rows), None, None) == K.FW_EINVAL
    assert L.fw_replay_store(_p(img), 100, _p(ctr), _p(st), _p(a32), _p(obs), _p(obs), _p(obs), _p(ctr), _p(ctr), 1, 16, 21, 6, None) == K.FW_EINVAL      # 100 rows: no multiple of 16
    torch.cuda.synchronize()
    assert float(img.abs().sum()) == 0.0 and ctr.tolist() == [0, 0, 0, 0]          # nothing ran
    with pytest.raises(ValueError):
        S.SAC(_env(), S.SACConfig(batch_size=24, net_arch=(64, 64)))
    with pytest.raises(ValueError):
        S.SAC(_env(), S.SACConfig(batch_size=32, net_arch=(128, 128)))
