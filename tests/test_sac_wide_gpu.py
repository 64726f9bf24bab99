"""The wide form of the SAC gradient step (512 < B <= 8192, csrc/fwsim_sac.hpp) on the GPU: fw_sac_update against sac_update_torch on
the pinned wide cases, the boundary between the two forms, determinism, graph replay, fw_sac_noise / fw_replay_sample at the new
sizes and the learner end to end with a 1024-row batch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import sac as S

import sac_cases as SC
import sac_wide_cases as WC

pytestmark = pytest.mark.gpu
DEV = "cuda"
_p = S._p


def _counters(cursor=0, size=0, steps=0, grad=0):
    return torch.tensor([cursor, size, steps, grad], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------ 1. update parity
def _parity(d, A, H, B, seed, steps=3, check=(0, 2)):
    """fw_sac_update against the torch step in float32 on the same device and the same fw_sac_noise stream.  The noise is Philox, not
    sac_cases.make_noise, so the case also runs the torch step in float64 on the same inputs and noise: a reference pair that leaves
    the tolerances by itself fails the case as an invalid input (it is never skipped); a pair that agrees while the kernel does not is
    a kernel bug."""
    case = (d, A, H, B, seed)
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), seed=seed)
    pol = SC.make_policy(d, A, H, seed)
    rows = SC.make_batch(d, A, B, seed).to(DEV)
    pt, ot = SC.learner(pol, cfg, device=DEV)                                # the torch learner, float32
    pd, od = SC.learner(pol, cfg, dtype=torch.float64, device=DEV)          # the same in float64
    pf, of = SC.learner(pol, cfg, device=DEV)                                # the modules the image is unpacked into
    fused = S.FusedSacUpdate(pf, of, cfg)
    fused.pack()
    ctr_t, ctr_f = _counters(grad=40), _counters(grad=40)
    for step in range(steps):
        eps = S.sac_noise(seed, ctr_t, B, A)
        st = S.sac_update_torch(pt, ot, rows, eps[0], eps[1], cfg)
        sd = S.sac_update_torch(pd, od, rows.double(), eps[0].double(), eps[1].double(), cfg)
        ctr_t[S.CTR_GRAD] += 1
        fused.run(rows, ctr_f)
        if step in check:
            WC.check_reference_pair(pt, ot, st, pd, od, sd, case, step)
            fused.unpack()
            assert pf.n_updates == step + 1 and ctr_f.tolist() == ctr_t.tolist()
            SC.compare(pf, of, pt, ot)
            sf = fused.scalars()
            print(f"{case} step {step + 1}: fused {sf}")
            WC.compare_scalars(sf, st, "fused against torch")


@pytest.mark.parametrize("d,A,H,B,seed", WC.WIDE_CASES_GPU)
def test_wide_update_matches_the_torch_update(d, A, H, B, seed):
    _parity(d, A, H, B, seed)


# ------------------------------------------------------------------------------------------------ 2. the boundary between the forms
@pytest.mark.parametrize("B", [512, 576])
def test_either_side_of_the_dispatch_matches_torch(B):
    """512 rows take the 24-launch form, 576 the wide one: the same policy and seed through both."""
    _parity(21, 6, 64, B, 5)


def test_rejected_batches_keep_their_codes():
    L = _lib.lib()
    img, rows, ctr, out = torch.zeros(400_000, device=DEV), torch.zeros((8256, 50), device=DEV), _counters(), torch.zeros(8, device=DEV)
    ws = torch.zeros(1 << 24, dtype=torch.uint8, device=DEV)
    H = S._SacHyper(lr=3e-4, gamma=0.99, tau=0.02, beta1=0.9, beta2=0.999, eps=1e-8, target_entropy=-6.0, ent_coef=0.0, auto_ent=1,
                    target_update_interval=1, seed=1)
    upd = lambda B, n=ws.numel(): L.fw_sac_update(_p(img), _p(rows), 21, 6, 64, B, C.byref(H), _p(ctr), _p(out), _p(ws), n, None)
    assert upd(528) == K.FW_EUNSUPPORTED and b"multiples of 64 in (512, 8192]" in L.fw_last_error(None)
    assert upd(8256) == K.FW_EUNSUPPORTED and upd(520) == K.FW_EUNSUPPORTED and upd(24) == K.FW_EUNSUPPORTED and upd(0) == K.FW_EINVAL
    assert upd(576, n=L.fw_sac_update_workspace_bytes(21, 6, 64, 576) - 4) == K.FW_EINVAL          # a workspace of the old size is too small
    torch.cuda.synchronize()
    assert float(img.abs().sum()) == 0.0 and ctr.tolist() == [0, 0, 0, 0]          # nothing ran
    with pytest.raises(ValueError, match="multiples of 64"):
        S.SAC(P.FixedwingLowLevelVecEnv(16, seed=3), S.SACConfig(batch_size=528, net_arch=(64, 64)))


# ------------------------------------------------------------------------------------------------ 3. determinism, 4. graph replay
def _ring_learner(H, B, seed=5, d=21, A=6, rows=2048):
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), seed=seed)
    pol = SC.make_policy(d, A, H, seed).to(DEV)
    fused = S.FusedSacUpdate(pol, S.make_optimizers(pol, cfg), cfg)
    fused.pack()
    buf = S.ReplayBufferDevice(rows, 64, d, A, DEV)
    buf.ring.copy_(SC.make_batch(d, A, rows, seed))
    buf.counters.copy_(_counters(size=rows))
    return cfg, fused, buf


@pytest.mark.parametrize("H,B", [(256, 1024), (64, 576)])
def test_three_wide_steps_are_deterministic(H, B):
    out = []
    for _ in range(2):
        cfg, fused, buf = _ring_learner(H, B)
        batch = torch.zeros((B, buf.row), device=DEV)
        for _ in range(3):
            buf.sample(cfg.seed, batch)
            fused.run(batch, buf.counters)
        torch.cuda.synchronize()
        out.append((fused.image.clone(), fused.out.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.isfinite(out[0][0]).all() and int(out[0][0][-4:].view(torch.int32)[0]) == 3


def test_four_replayed_wide_steps_equal_four_eager_ones():
    H, B = 64, 576
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
            for _ in range(3):
                g.replay()
                hist.append(idx.clone())
        else:
            for _ in range(4):
                step()
                hist.append(idx.clone())
        torch.cuda.synchronize()
        res.append((fused.image.clone(), fused.out.clone(), buf.counters.clone(), torch.stack(hist)))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert res[0][2].tolist() == [0, 2048, 0, 4] and int(res[0][0][-4:].view(torch.int32)[0]) == 4
    assert len(torch.unique(res[0][3], dim=0)) == 4          # every step drew its own batch


# ------------------------------------------------------------------------------------------------ 5. noise and sampling
def test_noise_and_sampling_at_wide_batches():
    """fw_sac_noise keys a draw by (batch row, step counter), so the first 512 rows of a 1024-row draw are the 512-row draw; the largest
    shape (8192 x 8) has the statistics of N(0, 1); fw_replay_sample at 1024 and 8192 rows against the numpy ring, bit for bit.  The two
    entry points have no batch rule of their own (any positive size, as before): 528 rows, which fw_sac_update rejects, are drawn too."""
    a, b = S.sac_noise(3, _counters(grad=5), 1024, 6), S.sac_noise(3, _counters(grad=5), 512, 6)
    assert torch.equal(a[:, :512], b) and not (a[0] == a[1]).any()
    assert torch.equal(S.sac_noise(3, _counters(grad=5), 528, 6), a[:, :528])
    assert torch.equal(S.sac_noise(3, _counters(grad=5), 1024, 6), a) and not (S.sac_noise(3, _counters(grad=6), 1024, 6) == a).any()
    store = torch.full((2 * 8192 * 8 + 64,), 9.0, device=DEV)          # the draw and 64 floats behind it that must stay
    big = store[:2 * 8192 * 8].view(2, 8192, 8)
    S.sac_noise(3, _counters(grad=5), 8192, 8, out=big)
    assert abs(float(big.mean())) < 5 / math.sqrt(big.numel()) and abs(float(big.var()) - 1.0) < 5 * math.sqrt(2.0 / big.numel())
    assert not bool((big == 9.0).any()) and bool((store[-64:] == 9.0).all()) and len(torch.unique(big)) > 0.99 * big.numel()
    n, d, A, seed = 64, 21, 6, 9
    buf = S.ReplayBufferDevice(5 * n, n, d, A, DEV)
    ring = np.random.default_rng(0).standard_normal((5 * n, buf.row)).astype(np.float32)
    buf.ring.copy_(torch.as_tensor(ring)); buf.counters.copy_(_counters(size=5 * n, grad=3))
    for B in (528, 1024, 8192):
        batch, idx = torch.zeros((B, buf.row), device=DEV), torch.full((B,), -1, dtype=torch.int32, device=DEV)
        buf.sample(seed, batch, idx)
        i = idx.cpu().numpy()
        assert i.min() >= 0 and i.max() < 5 * n and np.array_equal(batch.cpu().numpy(), ring[i])
        if B == 528:
            small = i.copy()
        elif B == 1024:
            first = i.copy()
            assert len(np.unique(i)) > 0.9 * 5 * n and np.array_equal(i[:528], small)
        else:
            assert len(np.unique(i)) == 5 * n          # (8192 draws from 320 rows: a miss has probability ~320 e^-25.6)
            assert np.array_equal(i[:1024], first)          # a row's index does not depend on the batch size either


# ------------------------------------------------------------------------------------------------ 6. the learner end to end
N, VEC_STEPS = 64, 24          # learning_starts = 128: two warm-up vec-steps, 22 trained ones of one 1024-row gradient step each


def _sac(fused=True, graphs=False, stats=False):
    cfg = S.SACConfig(batch_size=1024, net_arch=(64, 64), learning_starts=2 * N, gradient_steps=1, seed=7, use_graphs=graphs,
                      fused_update=fused, buffer_size=N * 40, episode_stats=stats, stats_window_size=20)
    return S.SAC(P.FixedwingLowLevelVecEnv(N, seed=3), cfg)


def _run(sac, n):
    for _ in range(n):
        sac.collect_step()
    torch.cuda.synchronize()
    return sac


@pytest.fixture(scope="module")
def fused_run():
    return _run(_sac(), VEC_STEPS)


def test_learner_with_a_wide_batch_counts(fused_run):
    sac = fused_run
    assert sac.batch.shape == (1024, sac.buffer.row) and sac.noise.shape == (2, 1024, 6)
    assert sac.num_timesteps == N * VEC_STEPS and sac.n_updates == VEC_STEPS - 2
    assert sac.buffer.counters.tolist() == [N * VEC_STEPS, N * VEC_STEPS, VEC_STEPS, VEC_STEPS - 2]
    assert all(torch.isfinite(p).all() for p in sac.policy.parameters())
    assert all(math.isfinite(v) for v in sac.read_logs().values())


@pytest.mark.parametrize("stats", [False, True])
def test_fused_and_torch_learners_agree_at_a_wide_batch(fused_run, stats):
    a, b = (_run(_sac(stats=True), VEC_STEPS) if stats else fused_run), _run(_sac(fused=False, stats=stats), VEC_STEPS)
    assert (a.episode_monitor is not None) == (b.episode_monitor is not None) == stats
    assert b.n_updates == VEC_STEPS - 2 and b.buffer.counters.tolist() == a.buffer.counters.tolist()
    SC.compare(a.policy, a.optimizers, b.policy, b.optimizers, moments=False)


@pytest.mark.parametrize("stats", [False, True])
def test_graph_replay_equals_eager_bit_for_bit_at_a_wide_batch(fused_run, stats):
    a, b = fused_run, _run(_sac(graphs=True, stats=stats), VEC_STEPS)
    assert len(b._graphs) == 2 and all(isinstance(g, torch.cuda.CUDAGraph) for g in b._graphs.values())
    assert (b.episode_monitor is not None) == stats
    assert torch.equal(a.fused.image, b.fused.image) and torch.equal(a.buffer.ring, b.buffer.ring)
    assert torch.equal(a.buffer.counters, b.buffer.counters) and torch.equal(a.fused.out, b.fused.out)
    assert torch.equal(a.env.obs, b.env.obs)
    if stats:
        assert "episode_stats" in b.state_dict()


@pytest.mark.parametrize("stats", [False, True])
def test_state_dict_round_trip_continues_bit_identically_at_a_wide_batch(stats):
    a = _run(_sac(stats=stats), 6)
    sd = a.state_dict(include_buffer=True)
    b = _sac(stats=stats)
    b.env.reset_tensor(); b._started = True
    b.env.set_state(a.env.get_state()); b.env.obs.copy_(a.env.obs)
    b.load_state_dict(sd)
    _run(a, 3); _run(b, 3)
    assert torch.equal(a.fused.image, b.fused.image) and torch.equal(a.buffer.ring, b.buffer.ring)
    assert a.buffer.counters.tolist() == b.buffer.counters.tolist() == [9 * N, 9 * N, 9, 7] and a.num_timesteps == b.num_timesteps == 9 * N
    for (k, p), q in zip(a.policy.named_parameters(), b.policy.parameters()):
        assert torch.equal(p, q), k
    if stats:
        assert a.episode_monitor.totals()["episodes"] == b.episode_monitor.totals()["episodes"]
