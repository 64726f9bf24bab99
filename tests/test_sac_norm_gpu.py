"""Running observation / reward normalisation for SAC on the GPU: fw_sac_act_norm against fw_normalize_obs followed by fw_sac_act (bit
for bit) and against the torch forward, fw_replay_normalize against fw_normalize_obs on the extracted blocks and the float64 reward
expression, and the learner (sac.SAC with normalize_obs / normalize_reward): counts, raw ring rows, graph replay, the torch learner,
checkpoints, flags off, the compositions with the three gathers, and evaluation through SAC.eval_env."""
import ctypes as C
import types

import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib, evaluate
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R
from pyflyt_drone_amd import sac as S

import sac_cases as SC
import sac_norm_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"
_p = S._p
CLIP, EPS = NC.CLIP_OBS, NC.EPS


def _counters(cursor=0, size=0, steps=0, grad=0):
    return torch.tensor([cursor, size, steps, grad], dtype=torch.int64, device=DEV)


def _image(pol, cfg):
    f = S.FusedSacUpdate(pol, S.make_optimizers(pol, cfg), cfg)
    f.pack()
    return f.image


def _outs(n, d, A, dtype):
    return dict(act=torch.full((n, A), 9.0, device=DEV), env=torch.full((n, A), 9.0, device=DEV, dtype=dtype),
                stage=torch.full((n, d), 9.0, device=DEV), logp=torch.full((n,), 9.0, device=DEV), eps=torch.full((n, A), 9.0, device=DEV))


def _act(image, obs, A, H, mode, seed, ctr):
    n, d = obs.shape
    out = _outs(n, d, A, obs.dtype)
    _lib.check(_lib.lib().fw_sac_act(_p(image), _p(obs), int(obs.dtype == torch.float64), n, d, A, H, mode, seed, 0, _p(ctr),
                                     _p(out["act"]), _p(out["env"]), _p(out["stage"]), _p(out["logp"]), _p(out["eps"]), None))
    torch.cuda.synchronize()
    return out


def _act_norm(image, obs, A, H, mode, seed, ctr, mean, var, clip=CLIP, eps=EPS):
    n, d = obs.shape
    out = _outs(n, d, A, obs.dtype)
    _lib.check(_lib.lib().fw_sac_act_norm(_p(image), _p(obs), int(obs.dtype == torch.float64), n, d, A, H, mode, seed, 0, _p(ctr),
                                          _p(out["act"]), _p(out["env"]), _p(out["stage"]), _p(out["logp"]), _p(out["eps"]),
                                          _p(mean), _p(var), clip, eps, None))
    torch.cuda.synchronize()
    return out


def _normalize_obs(raw, mean, var, clip=CLIP, eps=EPS):
    """fw_normalize_obs(update = 0) of raw [n, d] (float32 or float64) -> float32 [n, d]"""
    n, d = raw.shape
    raw = raw.contiguous()
    out, cnt = torch.full((n, d), 7.0, device=DEV), torch.full((1,), 1.0, dtype=torch.float64, device=DEV)
    _lib.check(_lib.lib().fw_normalize_obs(_p(raw), int(raw.dtype == torch.float64), n, d, _p(mean), _p(var), _p(cnt), 0, clip, eps, _p(out),
                                           None, None, None))
    torch.cuda.synchronize()
    return out


def _stats(d, seed=0):
    mean, var = NC.stats(d, seed)
    return mean.to(DEV), var.to(DEV)


# ------------------------------------------------------------------------------------------------ 1. act
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape", NC.ACT_SHAPES)
def test_act_norm_is_normalize_obs_then_act_bit_for_bit(shape, dtype):
    d, A, H = shape
    seed = 5
    img = _image(SC.make_policy(d, A, H, 11, perturb=0.1).to(DEV), S.SACConfig(net_arch=(H, H), seed=seed))
    mean, var = _stats(d)
    ctr = _counters(steps=7)
    for n in NC.ACT_NS:
        raw = NC.raw_obs(n, d, mean.cpu(), var.cpu(), n, dtype).to(DEV)
        obs_n = _normalize_obs(raw, mean, var)
        assert float(obs_n.abs().max()) <= CLIP
        if n >= 16:                                              # the inputs do what they are for: the clip and the eps path are taken
            assert bool((obs_n.abs() == CLIP).any()) and bool((obs_n[0::2, 1] == 0).all()) and bool((obs_n[1::2, 1] == CLIP).all())
        for mode in (S.ACT_STOCHASTIC, S.ACT_DETERMINISTIC):
            got, want = _act_norm(img, raw, A, H, mode, seed, ctr, mean, var), _act(img, obs_n, A, H, mode, seed, ctr)
            for k in ("act", "logp", "eps"):
                assert torch.equal(got[k], want[k]), (n, mode, k)
            assert torch.equal(got["env"], got["act"].to(dtype)), (n, mode)
            assert torch.equal(got["stage"], raw.float()), (n, mode)             # the ring stores raw rows
        # mode 2 needs no statistics and equals fw_sac_act's
        got, want = _act_norm(img, raw, A, H, S.ACT_WARMUP, seed, ctr, None, None), _act(img, raw, A, H, S.ACT_WARMUP, seed, ctr)
        assert all(torch.equal(got[k], want[k]) for k in got), n
        assert torch.equal(got["stage"], raw.float())


# the (seed, step counter) of tests/test_sac_gpu.py::test_act_against_torch and its observations, as z-scores: the normalised rows are
# that test's rows up to rounding, so the same one or two rows of 64 have max|u| > 3 in torch alone
ACT_SEED, ACT_STEP = 5, 7


@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_act_norm_against_the_torch_forward(H, dtype):
    n, d, A, seed = 64, 21, 6, ACT_SEED
    pol = SC.make_policy(d, A, H, 11, perturb=0.1).to(DEV)
    img = _image(pol, S.SACConfig(net_arch=(H, H), seed=seed))
    mean, var = _stats(d)
    g = torch.Generator(device=DEV).manual_seed(21)
    z = 0.25 * torch.randn((n, d), device=DEV, generator=g)
    raw = (mean + z.double() * torch.sqrt(var + EPS)).to(dtype)
    ctr = _counters(steps=ACT_STEP)
    det = _act_norm(img, raw, A, H, S.ACT_DETERMINISTIC, seed, ctr, mean, var)
    sto = _act_norm(img, raw, A, H, S.ACT_STOCHASTIC, seed, ctr, mean, var)
    holder = types.SimpleNamespace(obs_rms=types.SimpleNamespace(mean=mean, var=var), epsilon=EPS, clip_obs=CLIP)
    with torch.no_grad():
        x = R.VecNormalizeDevice._norm_obs_torch(holder, raw, torch.zeros((n, d), device=DEV))
        m, ls = pol.dist(x)
        torch.testing.assert_close(det["act"], torch.tanh(m), rtol=2e-3, atol=2e-5)
        a, logp = pol.sample(x, sto["eps"])
        torch.testing.assert_close(sto["act"], a, rtol=2e-3, atol=2e-5)
        keep = (m + torch.exp(ls) * sto["eps"]).abs().amax(1) <= 3.0
        print(f"H {H}: {int((~keep).sum())} of {n} rows have max|u| > 3; worst |logp - torch| on the others "
              f"{float((sto['logp'] - logp)[keep].abs().max()):.3e}")
        assert int((~keep).sum()) <= 0.05 * n
        torch.testing.assert_close(sto["logp"][keep], logp[keep], rtol=2e-3, atol=2e-3)
    assert torch.equal(det["stage"], raw.float()) and torch.equal(det["eps"], sto["eps"])


# ------------------------------------------------------------------------------------------------ 2. normalise
def _normalize(rows, d, A, mean, var, ret_var, clip_obs=CLIP, clip_rew=NC.CLIP_REW):
    out = rows.clone()
    rc = _lib.lib().fw_replay_normalize(_p(out), out.shape[0], d, A, _p(mean), _p(var), clip_obs, EPS, _p(ret_var), clip_rew, EPS, None)
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("B", NC.NORM_BS)
@pytest.mark.parametrize("shape", NC.NORM_SHAPES)
def test_replay_normalize(shape, B):
    d, A = shape
    mean, var = _stats(d)
    ret_var = torch.tensor([NC.RET_VAR], dtype=torch.float64, device=DEV)
    rows = NC.rows(B, d, A, mean.cpu(), var.cpu(), B + d).to(DEV)
    s, a, r, s2, done = S.split_rows(rows, d, A)
    want_s, want_s2 = _normalize_obs(s, mean, var), _normalize_obs(s2, mean, var)
    want_r = (r.double() / torch.sqrt(ret_var + EPS)).clamp(-NC.CLIP_REW, NC.CLIP_REW).float()
    rc, got = _normalize(rows, d, A, mean, var, ret_var)
    assert rc == K.FW_OK
    gs, ga, gr, gs2, gdone = S.split_rows(got, d, A)
    assert torch.equal(gs, want_s) and torch.equal(gs2, want_s2)                     # both observation blocks: fw_normalize_obs's bits
    assert torch.equal(ga, a) and torch.equal(gdone, done)                           # never written
    print(f"B {B} d {d}: reward bits equal the rounded float64 expression: {torch.equal(gr, want_r)}; "
          f"worst relative difference {float(((gr - want_r).abs() / want_r.abs().clamp_min(1e-30)).max()):.3e}")
    torch.testing.assert_close(gr, want_r, rtol=1e-6, atol=0.0)
    assert torch.equal(gr, want_r)                               # (the bits agree: both sides are one correctly rounded double division)
    assert float(gs.abs().max()) <= CLIP and float(gs2.abs().max()) <= CLIP and float(gr.abs().max()) <= NC.CLIP_REW
    if B * d >= 272:                                             # the inputs do what they are for: something clips in every block
        assert bool((gs.abs() == CLIP).any()) and bool((gs2.abs() == CLIP).any())
    if B >= 272:
        assert bool((gr.abs() == NC.CLIP_REW).any()) and bool((gr.abs() < NC.CLIP_REW).any())
    # the CPU restatement says the same
    ref = S.normalize_rows_reference(rows.cpu(), d, A, mean.cpu(), var.cpu(), CLIP, EPS, ret_var.cpu(), NC.CLIP_REW, EPS)
    rs, _, rr, rs2, _ = S.split_rows(ref, d, A)
    assert torch.equal(rs, gs.cpu()) and torch.equal(rs2, gs2.cpu())
    torch.testing.assert_close(rr, gr.cpu(), rtol=1e-6, atol=0.0)
    # ret_var NULL: the reward stays; obs_mean NULL: the observations stay
    rc, obs_only = _normalize(rows, d, A, mean, var, None)
    assert rc == K.FW_OK and torch.equal(obs_only[:, d + A], r) and torch.equal(obs_only[:, :d], want_s) and torch.equal(obs_only[:, d + A + 1:-1], want_s2)
    rc, rew_only = _normalize(rows, d, A, None, None, ret_var)
    assert rc == K.FW_OK and torch.equal(rew_only[:, d + A], gr)
    keep = [c for c in range(rows.shape[1]) if c != d + A]
    assert torch.equal(rew_only[:, keep], rows[:, keep])
    # a tighter clip holds too
    rc, tight = _normalize(rows, d, A, mean, var, ret_var, clip_obs=1.5, clip_rew=0.5)
    ts, _, tr, ts2, _ = S.split_rows(tight, d, A)
    assert rc == K.FW_OK and float(ts.abs().max()) <= 1.5 and float(ts2.abs().max()) <= 1.5 and float(tr.abs().max()) <= 0.5


def test_replay_normalize_error_codes():
    L = _lib.lib()
    mean, var = _stats(21)
    big_mean, big_var = torch.zeros(65, dtype=torch.float64, device=DEV), torch.ones(65, dtype=torch.float64, device=DEV)
    rv = torch.ones(1, dtype=torch.float64, device=DEV)
    rows = torch.full((16, 2 * 65 + 9 + 2), 3.0, device=DEV)
    call = lambda b=rows, B=16, d=21, A=6, m=mean, v=var, r=rv, co=10.0, cr=10.0: L.fw_replay_normalize(_p(b), B, d, A, _p(m), _p(v), co, 1e-8, _p(r), cr, 1e-8, None)
    assert call(m=None, v=None, r=None) == K.FW_EINVAL and b"fw_replay_normalize" in L.fw_last_error(None)
    assert call(b=None) == K.FW_EINVAL and call(v=None) == K.FW_EINVAL and call(m=None) == K.FW_EINVAL
    assert call(B=0) == K.FW_EINVAL and call(d=0) == K.FW_EINVAL and call(A=0) == K.FW_EINVAL and call(co=0.0) == K.FW_EINVAL and call(cr=-1.0) == K.FW_EINVAL
    assert call(d=65, m=big_mean, v=big_var) == K.FW_EUNSUPPORTED and b"obs_dim <= 64" in L.fw_last_error(None)
    assert call(A=9) == K.FW_EUNSUPPORTED
    # fw_sac_act_norm: modes 0 and 1 need the statistics
    img, obs, ctr = torch.zeros(400_000, device=DEV), torch.zeros((16, 21), device=DEV, dtype=torch.float64), _counters()
    a32, a64, st = torch.zeros((16, 9), device=DEV), torch.zeros((16, 9), device=DEV, dtype=torch.float64), torch.full((16, 21), 3.0, device=DEV)
    act = lambda A=6, H=64, mode=0, m=mean, v=var, clip=10.0, d=21: L.fw_sac_act_norm(_p(img), _p(obs), 1, 16, d, A, H, mode, 1, 0, _p(ctr), _p(a32), _p(a64), _p(st),
                                                                                  None, None, _p(m), _p(v), clip, 1e-8, None)
    assert act(m=None) == K.FW_EINVAL and act(mode=1, v=None) == K.FW_EINVAL and act(clip=0.0) == K.FW_EINVAL and act(mode=3) == K.FW_EINVAL
    assert act(H=128) == K.FW_EUNSUPPORTED and act(A=9) == K.FW_EUNSUPPORTED and act(d=65) == K.FW_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((rows == 3.0).all()) and bool((st == 3.0).all())                     # nothing ran


# ------------------------------------------------------------------------------------------------ 3. the learner
VEC_STEPS = 8            # 4 warm-up vec-steps (learning_starts 64 on 16 envs) and 4 trained ones


def _env(seed=3):
    return P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=4), 16, seed=seed)      # a short time limit: episodes end inside the run


def _sac(fused=True, graphs=False, **kw):
    kw.setdefault("normalize_obs", True)
    kw.setdefault("normalize_reward", True)
    kw.setdefault("gradient_steps", 1)
    kw.setdefault("buffer_size", 4096)
    cfg = S.SACConfig(batch_size=64, net_arch=(64, 64), learning_starts=64, seed=7, use_graphs=graphs, fused_update=fused, **kw)
    return S.SAC(_env(), cfg)


def _run(sac, n=VEC_STEPS):
    for _ in range(n):
        sac.collect_step()
    torch.cuda.synchronize()
    return sac


def _stat_tensors(sac):
    nz = sac.normalizer
    return [nz.obs_rms.mean, nz.obs_rms.var, nz.obs_rms.count, nz.ret_rms.mean, nz.ret_rms.var, nz.ret_rms.count, nz.returns]


def _same(a, b):
    assert torch.equal(a.fused.image, b.fused.image) and torch.equal(a.buffer.ring, b.buffer.ring)
    assert torch.equal(a.buffer.counters, b.buffer.counters) and torch.equal(a.fused.out, b.fused.out) and torch.equal(a.env.obs, b.env.obs)
    for (k, p), q in zip(a.policy.named_parameters(), b.policy.parameters()):
        assert torch.equal(p, q), k


@pytest.fixture(scope="module")
def fused_run():
    return _run(_sac())


def test_counts_raw_ring_rows_and_clipped_batches(fused_run):
    sac, k = fused_run, VEC_STEPS
    nz = sac.normalizer
    assert isinstance(nz, R.VecNormalizeDevice) and sac.buffer.counters.tolist() == [16 * k, 16 * k, k, 4] and sac.n_updates == 4
    assert float(nz.obs_rms.count) == pytest.approx(1e-4 + 16 * (k + 1), rel=0, abs=1e-9)       # the reset rows and every step's
    assert float(nz.ret_rms.count) == pytest.approx(1e-4 + 16 * k, rel=0, abs=1e-9)
    assert all(bool(torch.isfinite(t).all()) for t in _stat_tensors(sac)) and all(bool(torch.isfinite(p).all()) for p in sac.policy.parameters())
    assert float(nz.obs_rms.mean.abs().max()) > 10.0                                            # altitude: the statistics moved off (0, 1)
    assert float(sac.batch[:, :21].abs().max()) <= 10.0 and float(sac.batch[:, 28:49].abs().max()) <= 10.0 and float(sac.batch[:, 27].abs().max()) <= 10.0
    # reward normalisation off: the return statistics stay at their initial values, the observation ones still count
    only_obs = _run(_sac(normalize_reward=False), 5)
    m = only_obs.normalizer
    assert float(m.ret_rms.count) == 1e-4 and float(m.ret_rms.var) == 1.0 and float(m.ret_rms.mean) == 0.0
    assert float(m.obs_rms.count) == pytest.approx(1e-4 + 16 * 6, rel=0, abs=1e-9)
    # one more vec-step of a learner of its own, checked against the env's tensors around it: the ring row is raw, the batch is not
    sac = _run(_sac(), 7)                                        # (the eighth vec-step ends every episode by the time limit of 4)
    env = sac.env
    before, cursor = env.obs.clone(), sac.buffer.cursor
    stats_before = [t.clone() for t in _stat_tensors(sac)]
    sac.collect_step()
    torch.cuda.synchronize()
    ended = (env.terminated | env.truncated).bool()
    want = torch.cat([before.float(), sac.act_f32, env.rewards.float()[:, None],
                      torch.where(ended[:, None], env.terminal_obs, env.obs).float(), env.terminated.float()[:, None]], dim=1)
    assert torch.equal(sac.buffer.ring[cursor:cursor + 16], want) and torch.equal(sac.obs_stage, before.float())
    assert float(want[:, :21].abs().max()) > 10.0                                               # raw indeed
    # the statistics launch against its restatement: the env's new rows (never a terminal observation), returns zeroed at episode ends
    o, r, ret = S.stats_step_reference(tuple(stats_before[0:3]), tuple(stats_before[3:6]), stats_before[6], env.obs, env.rewards, ended, sac.cfg.gamma)
    # (float64 sums in another order: a variance is s2 / n - mean^2, so its error is a few roundings of the largest squared value)
    atol = 64.0 * 2.0 ** -52 * float((env.obs.double() ** 2).max())
    for got, ref in zip(_stat_tensors(sac), o + r + (ret,)):
        torch.testing.assert_close(got, ref.reshape(got.shape), rtol=1e-12, atol=atol)
    assert bool(ended.any()) and bool((sac.normalizer.returns[ended] == 0).all())
    # the batch of that step's gradient step: the sampled ring rows under the statistics of that moment
    idx = sac.batch_idx.long()
    nz = sac.normalizer
    ref = S.normalize_rows_reference(sac.buffer.ring[idx].cpu(), 21, 6, nz.obs_rms.mean.cpu(), nz.obs_rms.var.cpu(), 10.0, 1e-8,
                                     nz.ret_rms.var.cpu(), 10.0, 1e-8)
    torch.testing.assert_close(sac.batch.cpu(), ref, rtol=1e-6, atol=0.0)
    assert torch.equal(sac.batch[:, 21:27], sac.buffer.ring[idx][:, 21:27]) and torch.equal(sac.batch[:, -1], sac.buffer.ring[idx][:, -1])


def test_graph_replay_equals_eager_bit_for_bit(fused_run):
    a, b = fused_run, _run(_sac(graphs=True))
    assert len(b._graphs) == 2 and all(isinstance(g, torch.cuda.CUDAGraph) for g in b._graphs.values())
    _same(a, b)
    for x, y in zip(_stat_tensors(a), _stat_tensors(b)):
        assert torch.equal(x, y)


def test_fused_and_torch_learners_agree():
    # 8 vec-steps, 4 of them trained, one gradient step per env: 64 gradient steps, as tests/test_sac_gpu.py's pair takes
    a, b = _run(_sac(gradient_steps=-1)), _run(_sac(fused=False, gradient_steps=-1))
    assert a.n_updates == b.n_updates == 64 and b.buffer.counters.tolist() == [128, 128, 8, 64]
    SC.compare(a.policy, a.optimizers, b.policy, b.optimizers)
    assert torch.equal(a.normalizer.obs_rms.count, b.normalizer.obs_rms.count) and torch.equal(a.normalizer.ret_rms.count, b.normalizer.ret_rms.count)


def test_state_dict_round_trip_continues_bit_identically():
    a = _run(_sac(), 6)
    sd = a.state_dict(include_buffer=True)
    b = _sac()
    b.env.reset_tensor(); b._started = True
    b.env.set_state(a.env.get_state()); b.env.obs.copy_(a.env.obs)
    ptrs = [t.data_ptr() for t in _stat_tensors(b)]
    b.load_state_dict(sd)
    assert ptrs == [t.data_ptr() for t in _stat_tensors(b)]
    _run(a, 2); _run(b, 2)
    _same(a, b)
    for x, y in zip(_stat_tensors(a), _stat_tensors(b)):
        assert torch.equal(x, y)
    assert a.num_timesteps == b.num_timesteps == 128


def test_flags_off_is_the_default_learner_bit_for_bit():
    cfg = S.SACConfig(batch_size=64, net_arch=(64, 64), learning_starts=64, gradient_steps=1, seed=7, use_graphs=False, buffer_size=4096)
    a, b = _run(_sac(normalize_obs=False, normalize_reward=False)), _run(S.SAC(_env(), cfg))
    assert a.normalizer is None and b.normalizer is None
    _same(a, b)
    c = _run(_sac())                                             # and the feature does something: other parameters from the same seed
    assert not torch.equal(c.fused.image, b.fused.image)
    assert torch.equal(c.buffer.ring[:64], b.buffer.ring[:64])   # (the warm-up rows are the same raw rows)


@pytest.mark.parametrize("kw", [dict(prioritized=True), dict(n_steps=3), dict(her_goals=4)], ids=["prioritized", "n_steps", "her_goals"])
def test_compositions_with_the_three_gathers(kw):
    sac = _run(_sac(gradient_steps=2, **kw))
    assert sac.n_updates == 8 and all(bool(torch.isfinite(p).all()) for p in sac.policy.parameters())
    assert bool(torch.isfinite(sac.batch).all()) and float(sac.batch[:, :21].abs().max()) <= 10.0 and float(sac.batch[:, 28:49].abs().max()) <= 10.0
    assert all(bool(torch.isfinite(t).all()) for t in _stat_tensors(sac))
    if "prioritized" in kw:
        assert bool(torch.isfinite(sac.buffer.prio).all()) and bool((sac.batch_w > 0).all())
    if "her_goals" not in kw:
        return
    # hindsight: the relabelled reward is the task's reward of RAW values, scaled afterwards.  One more gather by hand: raw rows, the
    # reward of their (raw) relabelled goals by fw_her_reward, then the normalise launch
    raw, js = torch.zeros_like(sac.batch), torch.zeros(64, dtype=torch.int32, device=DEV)
    sac.buffer.sample(sac.cfg.seed, raw, sac.batch_idx, j_out=js)
    rew = torch.zeros(64, device=DEV)
    _lib.check(_lib.lib().fw_her_reward(_p(raw), 50, 64, 21, _p(raw[:, 46:49].contiguous()), C.byref(sac.buffer.her_task), _p(rew), None))
    torch.cuda.synchronize()
    rel = js >= 0
    assert bool(rel.any()) and bool((~rel).any())
    assert torch.equal(raw[rel, 27], rew[rel])                   # computed on the raw row, in front of the normalisation
    done = sac.normalize_batch(raw.clone())
    nz = sac.normalizer
    want = (rew.double() / torch.sqrt(nz.ret_rms.var + 1e-8)).clamp(-10.0, 10.0).float()
    torch.cuda.synchronize()
    torch.testing.assert_close(done[rel, 27], want[rel], rtol=1e-6, atol=0.0)
    # the goal columns of a relabelled row are normalised like any other column
    torch.testing.assert_close(done[:, 18:21].cpu(), S.normalize_obs_reference(raw[:, :21].cpu(), nz.obs_rms.mean.cpu(), nz.obs_rms.var.cpu())[:, 18:21],
                               rtol=1e-6, atol=0.0)


def test_evaluation_through_eval_env_sees_the_live_statistics(fused_run):
    sac = fused_run
    venv = P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=30), 16, seed=5)
    ev = sac.eval_env(venv)
    assert ev.obs_rms is sac.normalizer.obs_rms and not ev.training and ev.norm_obs and not ev.norm_reward
    count = float(sac.normalizer.obs_rms.count)
    # the actor under the wrapper's normalisation against SAC.act(mode = 1) on the same raw observations
    obs_n = ev.reset()
    kept = sac.env.obs.clone()
    sac.env.obs.copy_(venv.obs)
    with torch.no_grad():
        a_torch, _, _ = sac.policy(obs_n, deterministic=True)
    a_kernel = sac.act(S.ACT_DETERMINISTIC).clone()
    sac.env.obs.copy_(kept)                                      # (the fixture's env goes on where it was)
    torch.cuda.synchronize()
    torch.testing.assert_close(a_kernel.float(), a_torch, rtol=2e-3, atol=2e-5)
    with torch.no_grad():
        a_raw, _, _ = sac.policy(venv.obs, deterministic=True)
    assert float((a_raw - a_torch).abs().max()) > 1e-2           # (the bare observation gives other actions: the wrapper matters)
    r = evaluate.evaluate_policy(sac.policy, ev, 4)
    trk = r.tracking_scalars()
    assert len(r.episode_rewards) == 4 and trk and all(torch.isfinite(torch.tensor(v)) for v in trk.values())
    assert float(sac.normalizer.obs_rms.count) == count          # an evaluation moves no statistics
    venv.close()
