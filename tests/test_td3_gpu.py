"""The TD3 kernels (fw_td3_act, fw_td3_update) against torch, and the learner (td3.TD3) end to end on the low-level env, on the replay
ring and the samplers the SAC tests already check."""
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
from pyflyt_drone_amd import td3 as T

import her_cases as HC
import sac_nstep_cases as NC
import td3_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
_p = S._p


def _counters(cursor=0, size=0, steps=0, grad=0):
    return torch.tensor([cursor, size, steps, grad], dtype=torch.int64, device=DEV)


def _image(pol, cfg):
    f = T.FusedTd3Update(pol, T.make_optimizers(pol, cfg), cfg)
    f.pack()
    return f.image


def _act(image, obs, A, H, mode, seed, ctr, sigma=0.3, env_offset=0, guard=4):
    """fw_td3_act on `obs`; every output has `guard` rows behind the last env, which the launch must leave alone."""
    n, d = obs.shape
    out = dict(act=torch.full((n + guard, A), 9.0, device=DEV), env=torch.full((n + guard, A), 9.0, device=DEV, dtype=obs.dtype),
               stage=torch.full((n + guard, d), 9.0, device=DEV), eps=torch.full((n + guard, A), 9.0, device=DEV))
    _lib.check(_lib.lib().fw_td3_act(_p(image), _p(obs), int(obs.dtype == torch.float64), n, d, A, H, mode, seed, env_offset, _p(ctr),
                                     _p(out["act"]), _p(out["env"]), _p(out["stage"]), sigma, _p(out["eps"]), None))
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((v[n:] == 9.0).all()), f"{k}: rows behind the last env were written"
        out[k] = v[:n]
    return out


# ------------------------------------------------------------------------------------------------ 1. act
@pytest.mark.parametrize("n", [16, 20])
@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_act_against_torch(H, dtype, n):
    d, A, seed, sigma = 21, 6, 5, 0.3
    cfg = T.TD3Config(net_arch=(H, H), seed=seed)
    pol = TC.make_policy(d, A, H, 11, perturb=0.1).to(DEV)
    img = _image(pol, cfg)
    g = torch.Generator(device=DEV).manual_seed(21)
    obs = (0.25 * torch.randn((n, d), device=DEV, generator=g)).to(dtype)
    ctr = _counters(steps=7)
    det = _act(img, obs, A, H, T.ACT_DETERMINISTIC, seed, ctr, sigma)
    exp = _act(img, obs, A, H, T.ACT_EXPLORE, seed, ctr, sigma)
    with torch.no_grad():
        mean = pol.pi(obs.float())
        torch.testing.assert_close(det["act"], mean, rtol=2e-3, atol=2e-5)
        raw = mean + sigma * exp["eps"]
        torch.testing.assert_close(exp["act"], raw.clamp(-1.0, 1.0), rtol=2e-3, atol=2e-5)
        print(f"H {H} n {n}: the action clamp holds {int((raw.abs() > 1).sum())} of {raw.numel()} exploring actions")
        assert bool((raw.abs() > 1).any()) and bool((raw.abs() < 1).any())          # both sides of the clamp are in the case
        assert float(exp["act"].abs().max()) <= 1.0
    for o in (det, exp):
        assert torch.equal(o["env"], o["act"].to(dtype)) and torch.equal(o["stage"], obs.float())
    assert torch.equal(det["eps"], exp["eps"])          # the deterministic form reports the draw it did not use
    # the noise is fw_sac_act's for the same (seed, env, vec-step counter)
    sac_eps, sac_act, sac_env, sac_stage = (torch.zeros((n, A), device=DEV), torch.zeros((n, A), device=DEV), torch.zeros((n, A), device=DEV, dtype=dtype),
                                            torch.zeros((n, d), device=DEV))
    simg = torch.zeros(_lib.lib().fw_sac_param_count(d, A, H), device=DEV)
    _lib.check(_lib.lib().fw_sac_act(_p(simg), _p(obs), int(dtype == torch.float64), n, d, A, H, 0, seed, 0, _p(ctr), _p(sac_act), _p(sac_env),
                                     _p(sac_stage), None, _p(sac_eps), None))
    torch.cuda.synchronize()
    assert torch.equal(sac_eps, exp["eps"])
    # the same (seed, counter) gives the same bits, the next counter, another seed and other envs different ones
    again = _act(img, obs, A, H, T.ACT_EXPLORE, seed, ctr, sigma)
    assert all(torch.equal(again[k], exp[k]) for k in exp)
    for other in (_act(img, obs, A, H, T.ACT_EXPLORE, seed, _counters(steps=8), sigma), _act(img, obs, A, H, T.ACT_EXPLORE, seed + 1, ctr, sigma),
                  _act(img, obs, A, H, T.ACT_EXPLORE, seed, ctr, sigma, env_offset=n)):
        assert not (other["eps"] == exp["eps"]).any()
    # sigma 0: exploring is deterministic
    assert torch.equal(_act(img, obs, A, H, T.ACT_EXPLORE, seed, ctr, 0.0)["act"], det["act"])


def test_act_noise_statistics_and_warm_up():
    n, d, A, H, seed = 4096, 21, 6, 64, 2
    cfg = T.TD3Config(net_arch=(H, H), seed=seed)
    img = _image(TC.make_policy(d, A, H, 11).to(DEV), cfg)
    obs = torch.zeros((n, d), device=DEV, dtype=torch.float64)
    eps = _act(img, obs, A, H, T.ACT_EXPLORE, seed, _counters(steps=3))["eps"]
    print(f"eps over {eps.numel()} draws: mean {float(eps.mean()):+.4f}, var {float(eps.var()):.4f}")
    assert abs(float(eps.mean())) < 0.032 and abs(float(eps.var()) - 1.0) < 0.045          # five standard errors at n = 24 576
    assert len(torch.unique(eps)) > 0.99 * eps.numel()
    warm = _act(img, obs, A, H, T.ACT_WARMUP, seed, _counters(steps=3))
    a = warm["act"]
    assert bool((a >= -1.0).all()) and bool((a < 1.0).all())
    assert abs(float(a.mean())) < 5 * 0.577 / math.sqrt(a.numel())
    assert abs(float(a.var()) - 1.0 / 3.0) < 0.02 and len(torch.unique(a)) > 0.99 * a.numel()
    assert torch.equal(warm["env"], a.double()) and torch.equal(warm["stage"], obs.float())
    assert torch.equal(_act(img, obs, A, H, T.ACT_WARMUP, seed, _counters(steps=3))["act"], a)
    assert not torch.equal(_act(img, obs, A, H, T.ACT_WARMUP, seed, _counters(steps=4))["act"], a)


# ------------------------------------------------------------------------------------------------ 2. update parity
def _parity(d, A, H, B, seed, delay=2, steps=4):
    cfg = T.TD3Config(batch_size=B, net_arch=(H, H), seed=seed, policy_delay=delay)
    pol = TC.make_policy(d, A, H, seed)
    rows = TC.make_batch(d, A, B, seed).to(DEV)
    pt, ot = TC.learner(pol, cfg, device=DEV)            # the torch learner
    pf, of = TC.learner(pol, cfg, device=DEV)            # the modules the image is unpacked into
    fused = T.FusedTd3Update(pf, of, cfg)
    fused.pack()
    ctr_t, ctr_f = _counters(grad=40), _counters(grad=40)
    actor_steps = 0
    for step in range(steps):
        with_actor = (step + 1) % delay == 0
        actor_steps += int(with_actor)
        eps = S.sac_noise(seed, ctr_t, B, A)[0]          # both learners get the step's noise from fw_sac_noise
        st = T.td3_update_torch(pt, ot, rows, eps, cfg)
        ctr_t[S.CTR_GRAD] += 1
        fused.run(rows, ctr_f, with_actor)
        fused.unpack()
        assert (pf.n_updates, pf.n_actor_updates) == (step + 1, actor_steps) and ctr_f.tolist() == ctr_t.tolist()
        TC.compare(pf, of, pt, ot)
        sf = fused.scalars()
        print(f"step {step + 1} (actor part: {with_actor}): fused {sf}")
        assert ("actor_loss" in st) == with_actor
        for k in st:
            assert sf[k] == pytest.approx(float(st[k]), rel=2e-3, abs=1e-5), (k, step)
    assert actor_steps == steps // delay


@pytest.mark.parametrize("seed", TC.SEEDS)
@pytest.mark.parametrize("d,A,H,B", TC.SHAPES)
def test_fused_update_matches_the_torch_update(d, A, H, B, seed):
    _parity(d, A, H, B, seed)


@pytest.mark.parametrize("delay,steps", [(1, 3), (3, 6)])
def test_fused_update_with_other_policy_delays(delay, steps):
    _parity(21, 6, 64, 32, 5, delay=delay, steps=steps)


def test_consecutive_fused_steps_without_a_repack():
    """Four steps on the image alone (the learner's path: no unpack in between), then one comparison."""
    d, A, H, B, seed = 21, 6, 64, 32, 6
    cfg = T.TD3Config(batch_size=B, net_arch=(H, H), seed=seed)
    pol = TC.make_policy(d, A, H, seed)
    rows = TC.make_batch(d, A, B, seed).to(DEV)
    pt, ot = TC.learner(pol, cfg, device=DEV); pf, of = TC.learner(pol, cfg, device=DEV)
    fused = T.FusedTd3Update(pf, of, cfg); fused.pack()
    ctr_t, ctr_f = _counters(), _counters()
    for step in range(4):
        T.td3_update_torch(pt, ot, rows, S.sac_noise(seed, ctr_t, B, A)[0], cfg)
        ctr_t[S.CTR_GRAD] += 1
        fused.run(rows, ctr_f, (step + 1) % 2 == 0)
    fused.unpack()                                       # reads both counts from the image's tail
    assert (pf.n_updates, pf.n_actor_updates) == (4, 2) and ctr_f.tolist() == [0, 0, 0, 4]
    TC.compare(pf, of, pt, ot)


# ------------------------------------------------------------------------------------------------ 3. a step without the actor part
@pytest.mark.parametrize("H,B", [(64, 32), (256, 64)])
def test_a_step_without_the_actor_part_leaves_actor_and_targets_alone(H, B):
    d, A, seed = 21, 6, 5
    cfg = T.TD3Config(batch_size=B, net_arch=(H, H), seed=seed)
    pol, opts = TC.learner(TC.make_policy(d, A, H, seed), cfg, device=DEV)
    rows = TC.make_batch(d, A, B, seed).to(DEV)
    fused = T.FusedTd3Update(pol, opts, cfg); fused.pack()
    ctr = _counters()
    fused.run(rows, ctr, False); fused.run(rows, ctr, True)          # moments and targets that are not zeros and copies
    torch.cuda.synchronize()
    before, L = fused.image.clone(), fused.L
    fused.out[1] = 123.0
    fused.run(rows, ctr, False)
    torch.cuda.synchronize()
    after = fused.image
    na = L["q1"]
    for name, lo, hi in (("actor", 0, na), ("the three targets", L["actor_target"], L["params"]), ("actor exp_avg", L["exp_avg"], L["exp_avg"] + na),
                         ("actor exp_avg_sq", L["exp_avg_sq"], L["exp_avg_sq"] + na)):
        assert torch.equal(before[lo:hi], after[lo:hi]), name
        assert float(before[lo:hi].abs().sum()) > 0.0, name
    assert not torch.equal(before[na:L["trained"]], after[na:L["trained"]])          # the critics did step
    assert before[L["tail"]:].view(torch.int32).tolist() == [2, 1, 0, 0] and after[L["tail"]:].view(torch.int32).tolist() == [3, 1, 0, 0]
    assert float(fused.out[1]) == 123.0 and ctr.tolist() == [0, 0, 0, 3]          # the actor loss is written with the actor part only


# ------------------------------------------------------------------------------------------------ 4. determinism and replay
def _ring_learner(H, B, seed=5, d=21, A=6, rows=96):
    cfg = T.TD3Config(batch_size=B, net_arch=(H, H), seed=seed)
    pol = TC.make_policy(d, A, H, seed).to(DEV)
    fused = T.FusedTd3Update(pol, T.make_optimizers(pol, cfg), cfg)
    fused.pack()
    buf = S.ReplayBufferDevice(rows, 32, d, A, DEV)
    buf.ring.copy_(TC.make_batch(d, A, rows, seed))
    buf.counters.copy_(_counters(size=rows))
    return cfg, fused, buf


@pytest.mark.parametrize("H,B", [(256, 256), (64, 32)])
def test_update_is_deterministic(H, B):
    out = []
    for _ in range(2):
        cfg, fused, buf = _ring_learner(H, B)
        batch = torch.zeros((B, buf.row), device=DEV)
        for with_actor in (False, True):
            buf.sample(cfg.seed, batch)
            fused.run(batch, buf.counters, with_actor)
        torch.cuda.synchronize()
        out.append((fused.image.clone(), fused.out.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.isfinite(out[0][0]).all()


def _env(seed=3):
    return P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=4), 16, seed=seed)      # episodes end inside the run: terminal rows


def _td3(fused=True, graphs=False, gradient_steps=4, batch_size=32, buffer_steps=40, **kw):
    cfg = T.TD3Config(batch_size=batch_size, net_arch=(64, 64), learning_starts=32, gradient_steps=gradient_steps, seed=7, use_graphs=graphs,
                      fused_update=fused, buffer_size=16 * buffer_steps, **kw)
    return T.TD3(_env(), cfg)


def _run(td3, n):
    for _ in range(n):
        td3.collect_step()
    torch.cuda.synchronize()
    return td3


def _same(a, b):
    assert torch.equal(a.fused.image, b.fused.image) and torch.equal(a.buffer.ring, b.buffer.ring)
    assert torch.equal(a.buffer.counters, b.buffer.counters) and torch.equal(a.fused.out, b.fused.out)
    assert torch.equal(a.env.obs, b.env.obs) and torch.equal(a.batch, b.batch)


def test_eight_replayed_vec_steps_equal_eight_eager_ones():
    """policy_delay 2 with three gradient steps per vec-step: the residue n_updates % 2 alternates, so two training graphs are in use.
    Two warm-up vec-steps, then ten trained ones: of each training form the first runs eagerly and the other four are replays."""
    a = _run(_td3(gradient_steps=3), 12)
    b = _run(_td3(gradient_steps=3, graphs=True), 12)
    assert sorted(b._graphs) == [(False, True, 0), (False, True, 1), (True, False, 0)]
    assert all(isinstance(g, torch.cuda.CUDAGraph) for g in b._graphs.values())
    _same(a, b)
    assert a.n_updates == b.n_updates == 30 and a.n_actor_updates == b.n_actor_updates == 15
    assert a.buffer.counters.tolist() == [192, 192, 12, 30]
    assert a.fused.image[a.fused.L["tail"]:].view(torch.int32).tolist() == [30, 15, 0, 0]
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)


# ------------------------------------------------------------------------------------------------ 5. the learner end to end
@pytest.fixture(scope="module")
def fused_run():
    return _run(_td3(), 6)


def test_learner_counts_and_buffer(fused_run):
    td3 = fused_run
    assert td3.num_timesteps == 96 and td3.n_updates == 16 and td3.n_actor_updates == 8 and td3.buffer.counters.tolist() == [96, 96, 6, 16]
    assert (td3.policy.n_updates, td3.policy.n_actor_updates) == (16, 8) and td3.fused.ahead == 0 and td3.fused.ahead_actor == 0
    assert all(torch.isfinite(p).all() for p in td3.policy.parameters())
    for opt, steps in ((td3.optimizers["actor"], 8.0), (td3.optimizers["critic"], 16.0)):
        assert all(float(st["step"]) == steps for st in opt.state.values()) and len(opt.state) > 0
    logs = td3.read_logs()
    assert set(logs) == {"critic_loss", "actor_loss", "n_updates", "num_timesteps"}
    assert all(math.isfinite(logs[k]) for k in T.SCALARS) and logs["n_updates"] == 16 and logs["num_timesteps"] == 96 and logs["critic_loss"] > 0.0
    s, a, r, s2, done = S.split_rows(td3.buffer.ring[:96], 21, 6)
    assert bool((a >= -1).all()) and bool((a <= 1).all()) and bool(((done == 0) | (done == 1)).all())
    # one more vec-step (of a learner of its own: the fixture stays at six), checked against the env's tensors around it
    td3 = _run(_td3(), 6)
    env = td3.env
    before, cursor = env.obs.clone(), td3.buffer.cursor
    td3.collect_step(train=False)
    torch.cuda.synchronize()
    ended = (env.terminated | env.truncated).bool()
    want = torch.cat([before.float(), td3.act_f32, env.rewards.float()[:, None],
                      torch.where(ended[:, None], env.terminal_obs, env.obs).float(), env.terminated.float()[:, None]], dim=1)
    assert torch.equal(td3.buffer.ring[cursor:cursor + 16], want)
    assert torch.equal(td3.act_env, td3.act_f32.double()) and td3.buffer.counters.tolist() == [112, 112, 7, 16]
    # the stored action is the exploring one: the actor's tanh plus sigma eps, clamped
    with torch.no_grad():
        eps = torch.zeros((16, 6), device=DEV)
        det = td3.policy.pi(before.float())
    td3.buffer.counters[S.CTR_STEPS] -= 1                 # the counter the act launch saw
    env.obs.copy_(before)
    td3.act(T.ACT_EXPLORE, eps=eps)
    torch.cuda.synchronize()
    torch.testing.assert_close(td3.act_f32, (det + td3.cfg.action_noise_sigma * eps).clamp(-1, 1), rtol=2e-3, atol=2e-5)
    assert torch.equal(td3.act_f32, want[:, 21:27])


def test_fused_and_torch_learners_agree(fused_run):
    """Both learners draw the same batch indices (they depend on the counters alone) and stay within the learner tolerances."""
    a, b = fused_run, _run(_td3(fused=False), 6)
    assert (b.n_updates, b.n_actor_updates) == (16, 8) and b.buffer.counters.tolist() == [96, 96, 6, 16]
    assert torch.equal(a.batch_idx, b.batch_idx)
    TC.compare(a.policy, a.optimizers, b.policy, b.optimizers)


def test_fused_and_torch_learners_sample_the_same_batches():
    """From a common checkpoint the next vec-step is identical in both: the rows stored, the counters and every batch drawn."""
    a = _run(_td3(), 5)
    b = _td3(fused=False)
    b.env.reset_tensor(); b._started = True
    b.env.set_state(a.env.get_state()); b.env.obs.copy_(a.env.obs)
    b.load_state_dict(a.state_dict(include_buffer=True))
    a.collect_step(train=False); b.collect_step(train=False)
    for _ in range(2):
        a.buffer.sample(a.cfg.seed, a.batch, a.batch_idx); b.buffer.sample(b.cfg.seed, b.batch, b.batch_idx)
        torch.cuda.synchronize()
        assert torch.equal(a.batch_idx, b.batch_idx) and torch.equal(a.batch, b.batch) and torch.equal(a.buffer.ring, b.buffer.ring)
        a.buffer.counters[S.CTR_GRAD] += 1; b.buffer.counters[S.CTR_GRAD] += 1
    assert a.buffer.counters.tolist() == b.buffer.counters.tolist() == [96, 96, 6, 14]


def test_state_dict_round_trip_continues_bit_identically():
    a = _run(_td3(gradient_steps=3), 4)                   # 6 gradient steps, 3 with the actor part: the next residue is 0 ...
    a.collect_step()                                      # ... and after this vec-step 1: the checkpoint sits inside a delay period
    sd = a.state_dict(include_buffer=True)
    assert (sd["n_updates"], sd["n_actor_updates"]) == (9, 4)
    b = _td3(gradient_steps=3)
    b.env.reset_tensor(); b._started = True
    b.env.set_state(a.env.get_state()); b.env.obs.copy_(a.env.obs)
    b.load_state_dict(sd)
    _run(a, 2); _run(b, 2)
    assert torch.equal(a.fused.image, b.fused.image) and torch.equal(a.buffer.ring, b.buffer.ring)
    assert a.buffer.counters.tolist() == b.buffer.counters.tolist() == [112, 112, 7, 15] and a.num_timesteps == b.num_timesteps == 112
    assert (a.n_updates, a.n_actor_updates) == (b.n_updates, b.n_actor_updates) == (15, 7)
    for (k, p), q in zip(a.policy.named_parameters(), b.policy.parameters()):
        assert torch.equal(p, q), k
    for key in ("actor", "critic"):
        for x, y in zip(a.optimizers[key].param_groups[0]["params"], b.optimizers[key].param_groups[0]["params"]):
            assert torch.equal(a.optimizers[key].state[x]["exp_avg_sq"], b.optimizers[key].state[y]["exp_avg_sq"])


def test_n_step_learner_trains_on_the_reference_batch():
    td3 = _run(_td3(gradient_steps=2, batch_size=64, buffer_steps=8, n_steps=3), 12)          # 8 vec-steps: the 12 of the run wrap the ring
    assert td3.buffer.n_steps == 3 and td3.buffer.counters.tolist() == [64, 128, 12, 20] and (td3.n_updates, td3.n_actor_updates) == (20, 10)
    assert all(torch.isfinite(q).all() for q in td3.policy.parameters())
    ends = td3.buffer.ends.cpu().numpy()
    assert (ends & S.END_TRUNCATED).any() and ends.max() <= 3
    idx = td3.batch_idx.cpu().numpy()
    ref_rows, ref_k = S.nstep_rows_reference(td3.buffer.ring.cpu().numpy(), ends, 64, 128, 16, idx, 3, td3.cfg.gamma, 21)
    got = td3.batch.cpu().numpy()
    assert np.array_equal(got[:, :27], ref_rows[:, :27]) and np.array_equal(got[:, 28:49], ref_rows[:, 28:49])
    assert ref_k.max() == 3 and np.abs(got[:, 49].astype(np.float64) - ref_rows[:, 49]).max() <= 4 * NC.U


def test_hindsight_learner_trains_on_the_reference_batch():
    td3 = _run(_td3(gradient_steps=2, batch_size=64, buffer_steps=6, her_goals=4), 8)          # 6 vec-steps: the 8 of the run wrap the ring
    assert td3.buffer.her_goals == 4 and td3.buffer.her_prob == 0.8 and td3.buffer.counters.tolist() == [32, 96, 8, 12] and td3.n_updates == 12
    assert all(torch.isfinite(q).all() for q in td3.policy.parameters())
    ends = td3.buffer.ends.cpu().numpy()
    idx, (want_idx, o0, o1) = td3.batch_idx.cpu().numpy(), HC.draws(td3.cfg.seed, 11, 64, 96)
    assert np.array_equal(idx, want_idx)
    relabel = o0 < np.uint64(int(float(np.float32(0.8)) * 2.0 ** 32))
    ref, ref_j = S.her_rows_reference(td3.buffer.ring.cpu().numpy(), ends, 32, 96, 16, idx, relabel, o1, 64, td3.buffer.her_task)
    got = td3.batch.cpu().numpy()
    keep = np.ones(50, dtype=bool); keep[27] = False
    assert np.array_equal(got[:, keep], ref[:, keep]) and 0.5 * 64 < relabel.sum() < 64
    assert (np.abs(got[:, 27].astype(np.float64) - ref[:, 27]) <= np.spacing(np.abs(ref[:, 27]))).all()
    assert not np.array_equal(got[:, 18:21], td3.buffer.ring.cpu().numpy()[idx, 18:21])        # goals did change


def test_evaluate_policy_takes_the_td3_actor(fused_run):
    venv = P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=30), 16, seed=5)
    r = evaluate.evaluate_policy(fused_run.policy, R.VecNormalizeDevice(venv, training=False, norm_obs=False, norm_reward=False), 4)
    trk = r.tracking_scalars()
    assert len(r.episode_rewards) == 4 and trk and all(math.isfinite(v) for v in trk.values())
    a, v, lp = fused_run.policy(venv.obs, deterministic=True)
    assert a.shape == (16, 6) and v.shape == (16,) and lp.shape == (16,) and float(a.detach().abs().max()) <= 1.0 and float(lp.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ 6. errors
def test_unsupported_shapes_and_bad_arguments():
    L = _lib.lib()
    img, rows, ctr, out = (torch.zeros(700_000, device=DEV), torch.zeros((528, 60), device=DEV), _counters(), torch.zeros(8, device=DEV))
    ws = torch.zeros(1 << 24, dtype=torch.uint8, device=DEV)
    H = T._Td3Hyper(lr=1e-3, gamma=0.99, tau=0.005, beta1=0.9, beta2=0.999, eps=1e-8, policy_noise=0.2, noise_clip=0.5, seed=1)
    upd = lambda d, A, Hh, B, image=img, ctrs=ctr, work=ws, hyper=C.byref(H): L.fw_td3_update(
        _p(image), _p(rows), d, A, Hh, B, hyper, 1, _p(ctrs), _p(out), _p(work), ws.numel(), None)
    assert upd(21, 6, 64, 528) == K.FW_EUNSUPPORTED and b"batch" in L.fw_last_error(None)
    assert upd(21, 6, 64, 8) == K.FW_EUNSUPPORTED and upd(21, 6, 64, 24) == K.FW_EUNSUPPORTED and upd(21, 6, 64, 1024) == K.FW_EUNSUPPORTED
    assert upd(21, 6, 128, 32) == K.FW_EUNSUPPORTED and b"hidden" in L.fw_last_error(None)
    assert upd(21, 9, 64, 32) == K.FW_EUNSUPPORTED and upd(65, 6, 64, 32) == K.FW_EUNSUPPORTED
    assert upd(21, 6, 64, 0) == K.FW_EINVAL and upd(0, 6, 64, 32) == K.FW_EINVAL
    assert upd(21, 6, 64, 32, image=None) == K.FW_EINVAL and upd(21, 6, 64, 32, ctrs=None) == K.FW_EINVAL
    assert upd(21, 6, 64, 32, work=None) == K.FW_EINVAL and upd(21, 6, 64, 32, hyper=None) == K.FW_EINVAL
    assert L.fw_td3_update(_p(img), None, 21, 6, 64, 32, C.byref(H), 1, _p(ctr), _p(out), _p(ws), ws.numel(), None) == K.FW_EINVAL
    assert L.fw_td3_update(_p(img), _p(rows), 21, 6, 64, 32, C.byref(H), 1, _p(ctr), _p(out), _p(ws), 16, None) == K.FW_EINVAL      # workspace too small
    obs = torch.zeros((16, 21), device=DEV, dtype=torch.float64)
    a32, a64, st = torch.zeros((16, 9), device=DEV), torch.zeros((16, 9), device=DEV, dtype=torch.float64), torch.zeros((16, 21), device=DEV)
    act = lambda A, Hh, n=16, image=img, mode=0, sigma=0.1, stage=st: L.fw_td3_act(
        _p(image), _p(obs), 1, n, 21, A, Hh, mode, 1, 0, _p(ctr), _p(a32), _p(a64), _p(stage), sigma, None, None)
    assert act(6, 128) == K.FW_EUNSUPPORTED and act(9, 64) == K.FW_EUNSUPPORTED
    assert act(6, 64, n=0) == K.FW_EINVAL and act(6, 64, mode=3) == K.FW_EINVAL and act(6, 64, sigma=-1.0) == K.FW_EINVAL
    assert act(6, 64, image=None) == K.FW_EINVAL and act(6, 64, stage=None) == K.FW_EINVAL
    torch.cuda.synchronize()
    assert float(img.abs().sum()) == 0.0 and ctr.tolist() == [0, 0, 0, 0] and float(a32.abs().sum()) == 0.0          # nothing ran
    with pytest.raises(ValueError):
        T.TD3(_env(), T.TD3Config(batch_size=24, net_arch=(64, 64)))
    with pytest.raises(ValueError):
        T.TD3(_env(), T.TD3Config(batch_size=1024, net_arch=(64, 64)))
    with pytest.raises(ValueError):
        T.TD3(_env(), T.TD3Config(batch_size=32, net_arch=(128, 128)))
