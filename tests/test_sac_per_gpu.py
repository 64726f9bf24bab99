"""Prioritized replay on the device replay ring (fw_replay_per_mark_new / _rebuild / _update, fw_replay_sample_per,
fw_sac_update_weighted, SACConfig.prioritized) on the GPU: the kernels against the numpy statements of their contract in sac.py on the
scripted rings of tests/per_cases.py, the weighted gradient step against fw_sac_update and against sac_update_torch(weights=), their
reproducibility and graph replay, the learner end to end, and the error codes."""
import ctypes as C

import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import sac as S

import per_cases as PC
import sac_cases as SC
import sac_wide_cases as WC

pytestmark = pytest.mark.gpu
DEV = "cuda"
_p = S._p
SEED = 9
WIDE = WC.WIDE_SHAPES[0]                     # (21, 6, 64, 576): the smallest wide shape


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x.view(np.uint32)


def _counters(cursor=0, size=0, steps=0, grad=0):
    return torch.tensor([cursor, size, steps, grad], dtype=torch.int64, device=DEV)


@pytest.fixture(scope="module")
def rings():
    """name -> (leaves, hot rows, per_sums_reference of the leaves): computed once, never written."""
    out = {}
    for name in PC.RINGS:
        prio, hot = PC.leaves(name)
        sums = S.per_sums_reference(prio)
        for a in (prio, hot) + tuple(v for v in sums.values() if isinstance(v, np.ndarray)):
            a.setflags(write=False)
        out[name] = (prio, hot, sums)
    return out


def _buffer(name, prio, d=PC.D, A=PC.A, grad=0, **kw):
    """A prioritized device buffer holding the scripted ring `name`, its leaves and rebuilt sums."""
    c = PC.RINGS[name]
    buf = S.ReplayBufferDevice(c["capacity"], PC.N_ENVS, d, A, DEV, prioritized=True, **kw)
    assert buf.capacity == c["capacity"]
    buf.ring.copy_(torch.tensor(PC.rows(name, buf.row)))
    buf.prio.copy_(torch.tensor(prio))
    buf.counters.copy_(torch.tensor(PC.counters(name, grad)))
    buf.rebuild()
    return buf


# ------------------------------------------------------------------------------------------------ 1. rebuild and draw
@pytest.mark.parametrize("name", list(PC.RINGS))
def test_rebuild_against_the_reference_bit_for_bit(rings, name):
    prio, _, ref = rings[name]
    buf = _buffer(name, prio)
    buf.per_state[S.PER_MAX] = 3.25
    for k in ("sum1", "min1", "sum2", "min2"):                    # a rebuild recomputes everything: no stale value survives
        getattr(buf, k).fill_(7.0)
    buf.rebuild()
    for k in ("sum1", "min1", "sum2", "min2"):
        assert np.array_equal(_bits(getattr(buf, k)), _bits(ref[k])), k
    st = buf.per_state.cpu().numpy()
    assert st[S.PER_TOTAL].view(np.uint32) == ref["total"].view(np.uint32) and st[S.PER_MIN] == ref["pmin"]
    assert st[S.PER_MAX] == 3.25 and st[3] == 0.0                 # the running max and the spare are not the rebuild's
    assert np.array_equal(_bits(buf.prio), _bits(prio))


def test_rebuild_of_an_empty_ring():
    buf = S.ReplayBufferDevice(300, 4, 21, 6, DEV, prioritized=True)
    buf.sum1.fill_(5.0); buf.min2.fill_(5.0)
    buf.rebuild()
    assert buf.per_state.tolist() == [1.0, 0.0, float("inf"), 0.0] and not buf.sum1.any() and not buf.sum2.any()
    assert torch.isinf(buf.min1).all() and torch.isinf(buf.min2).all()
    # a draw from it reads nothing out of bounds: every index stays in the ring (the result is unspecified)
    out, idx = torch.zeros((64, buf.row), device=DEV), torch.full((64,), -1, dtype=torch.int32, device=DEV)
    buf.sample(SEED, out, idx)
    assert int(idx.min()) >= 0 and int(idx.max()) < buf.capacity


def _check_draw(buf, prio, ref, B, grad, beta0, beta_steps):
    out, idx = torch.full((B, buf.row), 9.0, device=DEV), torch.full((B,), -1, dtype=torch.int32, device=DEV)
    w = torch.full((B,), 9.0, device=DEV)
    buf.counters[S.CTR_GRAD] = grad
    keep = buf.counters.clone()
    buf.sample(SEED, out, idx, w_out=w)
    want = S.per_draw_reference(prio, ref, PC.words(SEED, grad, B))
    got = idx.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, want)
    assert (prio[got] > 0).all() and got.max() < int(buf.counters[S.CTR_SIZE])
    assert np.array_equal(_bits(out), _bits(buf.ring.cpu().numpy()[got]))                    # every gathered column
    beta = S.per_beta_reference(beta0, beta_steps, grad)
    w_ref = S.per_weights_reference(prio, want, ref["pmin"], beta).astype(np.float32)
    np.testing.assert_allclose(w.cpu().numpy(), w_ref, rtol=1e-5, atol=0)
    assert torch.equal(buf.counters, keep)                        # reads the counters, writes none
    return got, w.cpu().numpy()


@pytest.mark.parametrize("B", [16, 256, 4096])
@pytest.mark.parametrize("name", list(PC.RINGS))
def test_draw_against_the_reference_bit_for_bit(rings, name, B):
    prio, hot, ref = rings[name]
    buf = _buffer(name, prio, per_beta=0.4)
    got, w = _check_draw(buf, prio, ref, B, 3, 0.4, 0)
    assert w.max() <= 1.0 and w.min() > 0.0
    if name == "L" and B == 4096:
        share = np.isin(got, hot).mean()
        assert 0.38 < share < 0.48                                # the 48 hot rows hold about 43 % of the mass
    got2, _ = _check_draw(buf, prio, ref, B, 4, 0.4, 0)           # another gradient step, another batch
    assert not np.array_equal(got, got2)


def test_draw_of_wide_rows_and_the_schedule_of_beta(rings):
    """Rows of 138 floats (wider than one wave), and beta annealed from 0.4 to 1 over 1000 gradient steps, at step 0, 500 and beyond."""
    prio, _, ref = rings["M"]
    buf = _buffer("M", prio, d=64, A=8, per_beta=0.4, per_beta_steps=1000)
    assert buf.row == 138
    ws = [_check_draw(buf, prio, ref, 256, grad, 0.4, 1000)[1] for grad in (0, 500, 1000, 5000)]
    zero = _buffer("M", prio, per_beta=0.0)
    out, w = torch.zeros((64, 50), device=DEV), torch.zeros(64, device=DEV)
    zero.sample(SEED, out, None, w_out=w)
    assert (w == 1.0).all()                                       # beta = 0: no correction
    zero.sample(SEED, out)                                        # idx_out and w_out are optional
    assert ws[0].min() > ws[2].min()                              # a larger exponent pushes the small weights down


# ------------------------------------------------------------------------------------------------ 2. mark-new
def test_mark_new_writes_the_rows_the_next_store_writes():
    d, A, n = 21, 6, 4
    buf = S.ReplayBufferDevice(6 * n, n, d, A, DEV, prioritized=True)
    rng = np.random.default_rng(0)
    t = lambda x: torch.as_tensor(x, device=DEV)
    L = _lib.lib()
    for step in range(8):                                         # six stores fill the ring, the last two wrap it
        cursor = int(buf.counters[0])
        assert cursor == (step % 6) * n
        buf.per_state[S.PER_MAX] = 1.0 + step
        before, ctr = buf.prio.clone(), buf.counters.clone()
        _lib.check(L.fw_replay_per_mark_new(_p(buf.prio), buf.capacity, _p(buf.counters), _p(buf.per_state), n, None))
        want = before.clone(); want[cursor:cursor + n] = 1.0 + step
        assert torch.equal(buf.prio, want) and torch.equal(buf.counters, ctr)           # reads the cursor, writes no counter
        buf.prio.copy_(before)
        tag = rng.standard_normal((n, d)).astype(np.float32)
        buf.store(t(tag), t(rng.uniform(-1, 1, (n, A)).astype(np.float32)), t(rng.standard_normal(n)), t(rng.standard_normal((n, d))),
                  t(rng.standard_normal((n, d))), t(np.zeros(n, dtype=np.uint8)), t(np.zeros(n, dtype=np.uint8)))
        assert torch.equal(buf.prio, want)                        # store = mark-new, store, rebuild: the same leaves ...
        assert np.array_equal(buf.ring[cursor:cursor + n, :d].cpu().numpy(), tag)           # ... on the rows it wrote
        ref = S.per_sums_reference(buf.prio.cpu().numpy())
        assert np.array_equal(_bits(buf.sum1), _bits(ref["sum1"])) and float(buf.per_state[S.PER_TOTAL]) == float(ref["total"])
    assert buf.prio.tolist() == [7.0] * 4 + [8.0] * 4 + [3.0] * 4 + [4.0] * 4 + [5.0] * 4 + [6.0] * 4
    buf.counters[0] = 22                                          # a cursor no store left behind is normalised as the store does
    _lib.check(L.fw_replay_per_mark_new(_p(buf.prio), buf.capacity, _p(buf.counters), _p(buf.per_state), n, None))
    assert buf.prio[:4].tolist() == [8.0] * 4 and buf.prio[20:].tolist() == [6.0] * 4


# ------------------------------------------------------------------------------------------------ 3. priority update
def test_priority_update_against_the_reference(rings):
    prio, _, _ = rings["S"]
    buf = _buffer("S", prio, per_alpha=0.6, per_eps=1e-6)
    rng = np.random.default_rng(3)
    B = 64
    others = np.setdiff1d(np.arange(40), [7, 12, 33])
    idx = others[rng.integers(0, len(others), B)].astype(np.int32)          # (64 draws over 37 rows: more duplicates among them)
    td = rng.uniform(0.0, 4.0, B).astype(np.float32)
    idx[[2, 20, 41]] = 7; td[[2, 20, 41]] = [0.5, 3.5, 1.25]      # the same row three times: the middle one wins
    idx[5], td[5] = 33, 3.5                                        # (a row of its own with the winner's td)
    idx[9], td[9] = 12, 0.0                                        # td = 0: the leaf is eps^alpha, positive
    td[11] = 9.0                                                   # the batch's largest leaf: the new running max
    buf.update_priorities(torch.from_numpy(idx).to(DEV), torch.from_numpy(td).to(DEV))
    want, pmax = S.per_update_reference(prio, idx, td, 0.6, 1e-6, 1.0)
    got = buf.prio.cpu().numpy()
    touched = np.unique(idx)
    rest = np.setdiff1d(np.arange(64), touched)
    assert np.array_equal(_bits(got[rest]), _bits(prio[rest]))
    np.testing.assert_allclose(got[touched], want[touched], rtol=1e-5, atol=0)
    assert got[7].view(np.uint32) == got[33].view(np.uint32)      # the winner among duplicates, exactly
    assert got[12] > 0 and abs(got[12] - 1e-6 ** 0.6) < 1e-5 * 1e-6 ** 0.6
    st = buf.per_state.cpu().numpy()
    assert st[S.PER_MAX] == got[idx[11]] and abs(st[S.PER_MAX] - pmax) <= 1e-5 * pmax and st[S.PER_MAX] > 1.0
    ref = S.per_sums_reference(got)                               # ... followed by a rebuild
    for k in ("sum1", "min1", "sum2", "min2"):
        assert np.array_equal(_bits(getattr(buf, k)), _bits(ref[k])), k
    assert st[S.PER_TOTAL].view(np.uint32) == ref["total"].view(np.uint32) and st[S.PER_MIN] == ref["pmin"]
    # a smaller batch does not lower the running max; alpha = 0 makes every touched leaf 1
    flat = _buffer("S", prio, per_alpha=0.0)
    flat.per_state[S.PER_MAX] = 2.0
    flat.update_priorities(torch.from_numpy(idx).to(DEV), torch.from_numpy(td).to(DEV))
    assert (flat.prio.cpu().numpy()[touched] == 1.0).all() and float(flat.per_state[S.PER_MAX]) == 2.0


def test_priority_update_with_many_duplicates_does_not_depend_on_order(rings):
    """4096 rows drawn from L: the hot rows occur dozens of times each.  Two runs give the same bits, and they are the reference's max."""
    prio, hot, ref = rings["L"]
    idx = S.per_draw_reference(prio, ref, PC.words(SEED, 0, 4096)).astype(np.int32)
    assert np.bincount(idx).max() >= 20
    td = np.random.default_rng(5).uniform(0.0, 10.0, 4096).astype(np.float32)
    runs = []
    for _ in range(2):
        buf = _buffer("L", prio)
        buf.update_priorities(torch.from_numpy(idx).to(DEV), torch.from_numpy(td).to(DEV))
        runs.append((buf.prio.clone(), buf.sum1.clone(), buf.per_state.clone()))
    for x, y in zip(*runs):
        assert np.array_equal(_bits(x), _bits(y))
    want, pmax = S.per_update_reference(prio, idx, td, 0.6, 1e-6, 1.0)
    np.testing.assert_allclose(runs[0][0].cpu().numpy(), want, rtol=1e-5, atol=0)
    assert abs(float(runs[0][2][S.PER_MAX]) - pmax) <= 1e-5 * pmax


# ------------------------------------------------------------------------------------------------ 4. the weighted update
def _fused(pol, cfg):
    p, o = SC.learner(pol, cfg, device=DEV)
    f = S.FusedSacUpdate(p, o, cfg)
    f.pack()
    return p, o, f


@pytest.mark.parametrize("d,A,H,B", [SC.SHAPES[0], WIDE], ids=["512-row form", "wide form"])
def test_weights_of_one_leave_the_image_bit_identical(d, A, H, B):
    seed = 5
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), seed=seed)
    pol, rows = SC.make_policy(d, A, H, seed), SC.make_batch(d, A, B, seed).to(DEV)
    (_, _, plain), (_, _, weighted) = _fused(pol, cfg), _fused(pol, cfg)
    ca, cb = _counters(grad=40), _counters(grad=40)
    ones, td = torch.ones(B, device=DEV), torch.full((B,), -1.0, device=DEV)
    for step in range(3):
        plain.run(rows, ca)
        weighted.run(rows, cb, weights=ones, td_out=td)
        assert np.array_equal(_bits(plain.image), _bits(weighted.image)), step
        assert np.array_equal(_bits(plain.out), _bits(weighted.out)) and torch.equal(ca, cb)
        assert bool((td >= 0).all()) and float(td.max()) > 0
    weighted.run(rows, cb, weights=ones)                          # td_out is optional
    with pytest.raises(ValueError):
        plain.run(rows, ca, td_out=td)


@pytest.mark.parametrize("seed", SC.SEEDS)
@pytest.mark.parametrize("d,A,H,B", SC.SHAPES + [WIDE])
def test_weighted_update_matches_the_weighted_torch_update(d, A, H, B, seed):
    """Random weights in [0.05, 1]: fw_sac_update_weighted against sac_update_torch(weights=) on the same fw_sac_noise stream after 1
    and 3 steps under sac_cases.TOL, every element; td_out against the torch step's per-row value under TOL["param"].  The torch step
    runs in float64 beside it, as in tests/test_sac_wide_gpu.py: a reference pair that leaves the tolerances by itself fails the case as
    an invalid input (tests/per_cases.py records the one weight seed replaced so far)."""
    case = (d, A, H, B, seed)
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), seed=seed)
    pol, rows = SC.make_policy(d, A, H, seed), SC.make_batch(d, A, B, seed).to(DEV)
    w = PC.weights(*case).to(DEV)
    assert 0.05 <= float(w.min()) and float(w.max()) <= 1.0 and float(w.max() - w.min()) > 0.5
    pt, ot = SC.learner(pol, cfg, device=DEV)
    pd, od = SC.learner(pol, cfg, dtype=torch.float64, device=DEV)
    pf, of, fused = _fused(pol, cfg)
    ctr_t, ctr_f = _counters(grad=40), _counters(grad=40)
    td = torch.zeros(B, device=DEV)
    for step in range(3):
        eps = S.sac_noise(seed, ctr_t, B, A)
        st = S.sac_update_torch(pt, ot, rows, eps[0], eps[1], cfg, weights=w)
        sd = S.sac_update_torch(pd, od, rows.double(), eps[0].double(), eps[1].double(), cfg, weights=w.double())
        ctr_t[S.CTR_GRAD] += 1
        fused.run(rows, ctr_f, weights=w, td_out=td)
        if step in (0, 2):
            WC.check_reference_pair(pt, ot, st, pd, od, sd, case, step)
            fused.unpack()
            assert pf.n_updates == step + 1 and ctr_f.tolist() == ctr_t.tolist()
            SC.compare(pf, of, pt, ot)
            SC._close("td", td, st["td"], *SC.TOL["param"])
            sf = fused.scalars()
            print(f"step {step + 1}: fused {sf}, worst |td - torch| {float((td - st['td']).abs().max()):.3e}")
            WC.compare_scalars(sf, st, "weighted fused against torch")           # the critic loss logged is the unweighted one


# ------------------------------------------------------------------------------------------------ 5. determinism and replay
def _per_learner(H=64, B=64, seed=5, d=21, A=6, name="M", **kw):
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), seed=seed, prioritized=True)
    pol = SC.make_policy(d, A, H, seed).to(DEV)
    fused = S.FusedSacUpdate(pol, S.make_optimizers(pol, cfg), cfg)
    fused.pack()
    buf = _buffer(name, PC.leaves(name)[0], per_beta_steps=16, **kw)
    buf.ring.copy_(SC.make_batch(d, A, buf.capacity, seed))
    return cfg, fused, buf


def _per_step(cfg, fused, buf, batch, idx, w, td):
    buf.sample(cfg.seed, batch, idx, w_out=w)
    fused.run(batch, buf.counters, weights=w, td_out=td)
    buf.update_priorities(idx, td)


def _per_state_of(fused, buf):
    return [x.clone() for x in (fused.image, fused.out, buf.prio, buf.sum1, buf.min1, buf.sum2, buf.min2, buf.per_state, buf.counters)]


@pytest.mark.parametrize("B", [64, 576])
def test_two_runs_give_the_same_bits(B):
    out = []
    for _ in range(2):
        cfg, fused, buf = _per_learner(B=B)
        batch, idx = torch.zeros((B, buf.row), device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
        w, td = torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
        for _ in range(3):
            _per_step(cfg, fused, buf, batch, idx, w, td)
        torch.cuda.synchronize()
        out.append(_per_state_of(fused, buf) + [idx.clone(), w.clone(), td.clone()])
    for x, y in zip(*out):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    assert out[0][-4].tolist()[3] == 3 and torch.isfinite(out[0][0]).all()
    assert not np.array_equal(out[0][2].cpu().numpy(), PC.leaves("M")[0])          # the leaves did move


def test_eight_replayed_steps_equal_eight_eager_ones():
    B = 64
    res = []
    for graph in (False, True):
        cfg, fused, buf = _per_learner(B=B)
        batch, idx = torch.zeros((B, buf.row), device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
        w, td = torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
        step = lambda: _per_step(cfg, fused, buf, batch, idx, w, td)
        hist = []
        if graph:
            step()                                   # loads the kernels; counts as the first step
            hist.append((idx.clone(), w.clone()))
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
        for _ in range(7 if graph else 8):
            g.replay() if graph else step()
            hist.append((idx.clone(), w.clone()))
        torch.cuda.synchronize()
        res.append((_per_state_of(fused, buf), hist))
    for x, y in zip(res[0][0], res[1][0]):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    assert res[0][0][-1].tolist()[3] == 8
    for (i0, w0), (i1, w1) in zip(res[0][1], res[1][1]):
        assert torch.equal(i0, i1) and np.array_equal(_bits(w0), _bits(w1))


# ------------------------------------------------------------------------------------------------ 6. the learner
VEC_STEPS = 40


def _env(seed=3):
    return P.FixedwingVecEnv(K.lowlevel_config(), 16, seed=seed)


def _sac(fused=True, graphs=False, **kw):
    kw.setdefault("prioritized", True)
    cfg = S.SACConfig(batch_size=64, net_arch=(64, 64), learning_starts=64, gradient_steps=1, seed=7, use_graphs=graphs,
                      fused_update=fused, buffer_size=4096, per_beta_steps=100, **kw)
    return S.SAC(_env(), cfg)


def _run(sac, n=VEC_STEPS):
    for _ in range(n):
        sac.collect_step()
    torch.cuda.synchronize()
    return sac


@pytest.fixture(scope="module")
def eager_run():
    return _run(_sac())


def _same(a, b):
    assert torch.equal(a.fused.image, b.fused.image) and torch.equal(a.buffer.ring, b.buffer.ring)
    assert torch.equal(a.buffer.counters, b.buffer.counters) and torch.equal(a.env.obs, b.env.obs)
    for k in ("prio", "sum1", "min1", "sum2", "min2", "per_state"):
        assert np.array_equal(_bits(getattr(a.buffer, k)), _bits(getattr(b.buffer, k))), k


def test_learner_counts_and_the_structure_it_leaves(eager_run):
    sac = eager_run
    assert sac.buffer.prioritized and sac.buffer.counters.tolist() == [640, 640, 40, 36] and sac.n_updates == 36
    assert all(torch.isfinite(q).all() for q in sac.policy.parameters())
    prio = sac.buffer.prio.cpu().numpy()
    assert (prio[:640] > 0).all() and not prio[640:].any()
    ref = S.per_sums_reference(prio)
    for k in ("sum1", "min1", "sum2", "min2"):
        assert np.array_equal(_bits(getattr(sac.buffer, k)), _bits(ref[k])), k
    st = sac.buffer.per_state.cpu().numpy()
    assert st[S.PER_TOTAL] == ref["total"] and st[S.PER_MIN] == ref["pmin"] and st[S.PER_MAX] >= prio.max()
    assert len(np.unique(prio[:640])) > 100                       # the write-back did give rows leaves of their own
    td, w = sac.batch_td.cpu().numpy(), sac.batch_w.cpu().numpy()
    assert (td >= 0).all() and td.max() > 0 and (w > 0).all() and w.max() <= 1.0 and w.min() < 1.0
    logs = sac.read_logs()
    assert all(np.isfinite(v) for v in logs.values())


def test_graph_replay_equals_eager_bit_for_bit(eager_run):
    b = _run(_sac(graphs=True))
    assert len(b._graphs) == 2 and all(isinstance(g, torch.cuda.CUDAGraph) for g in b._graphs.values())      # warm-up and training
    _same(eager_run, b)
    assert torch.equal(eager_run.fused.out, b.fused.out) and torch.equal(eager_run.batch, b.batch)
    assert torch.equal(eager_run.batch_idx, b.batch_idx) and torch.equal(eager_run.batch_w, b.batch_w)


def test_fused_and_torch_learners_on_the_same_batches_stay_within_tolerance():
    """From a common checkpoint the next vec-step draws the same prioritized batch and weights in both learners; their gradient steps
    then agree under sac_cases.TOL, and so do the TD errors the new leaves are made of."""
    a = _run(_sac(), 10)
    b = _sac(fused=False)
    b.env.reset_tensor(); b._started = True
    b.env.set_state(a.env.get_state()); b.env.obs.copy_(a.env.obs)
    b.load_state_dict(a.state_dict(include_buffer=True))
    _ = a.policy
    assert torch.equal(a.buffer.prio, b.buffer.prio) and np.array_equal(_bits(a.buffer.per_state), _bits(b.buffer.per_state))
    a.collect_step(); b.collect_step()
    torch.cuda.synchronize()
    assert a.buffer.counters.tolist() == b.buffer.counters.tolist() == [176, 176, 11, 7]
    assert torch.equal(a.buffer.ring, b.buffer.ring) and torch.equal(a.batch_idx, b.batch_idx)
    assert np.array_equal(_bits(a.batch), _bits(b.batch)) and np.array_equal(_bits(a.batch_w), _bits(b.batch_w))
    SC.compare(a.policy, a.optimizers, b.policy, b.optimizers)
    SC._close("td", a.batch_td, b.batch_td, *SC.TOL["param"])


def test_state_dict_round_trip_continues_bit_identically():
    a = _run(_sac(), 12)
    sd = a.state_dict(include_buffer=True)
    assert sd["config"]["prioritized"] is True and torch.equal(sd["buffer"]["prio"], a.buffer.prio.cpu())
    assert torch.equal(sd["buffer"]["per_state"], a.buffer.per_state.cpu())
    b = _sac()
    b.env.reset_tensor(); b._started = True
    b.env.set_state(a.env.get_state()); b.env.obs.copy_(a.env.obs)
    b.load_state_dict(sd)
    _run(a, 4); _run(b, 4)
    _same(a, b)
    assert a.buffer.counters.tolist() == [256, 256, 16, 12] and a.num_timesteps == b.num_timesteps == 256
    for (name, p), q in zip(a.policy.named_parameters(), b.policy.parameters()):
        assert torch.equal(p, q), name
    # rows that come without priorities: every filled row enters with a leaf of 1.0; no rows: no leaves
    plain = _run(_sac(prioritized=False), 6)
    b.load_state_dict(plain.state_dict(include_buffer=True))
    assert (b.buffer.prio[:96] == 1.0).all() and not b.buffer.prio[96:].any() and float(b.buffer.per_state[S.PER_TOTAL]) == 96.0
    b.load_state_dict(plain.state_dict())
    assert not b.buffer.prio.any() and float(b.buffer.per_state[S.PER_TOTAL]) == 0.0 and b.buffer.counters.tolist()[:2] == [0, 0]


def test_prioritized_off_is_the_default_learner_bit_for_bit():
    a = _run(_sac(prioritized=False), 12)
    cfg = S.SACConfig(batch_size=64, net_arch=(64, 64), learning_starts=64, gradient_steps=1, seed=7, use_graphs=False, buffer_size=4096)
    b = _run(S.SAC(_env(), cfg), 12)
    assert a.buffer.prio is None and b.buffer.prio is None and a.batch_w is None and not b.cfg.prioritized
    assert torch.equal(a.fused.image, b.fused.image) and torch.equal(a.buffer.ring, b.buffer.ring)
    assert torch.equal(a.buffer.counters, b.buffer.counters) and torch.equal(a.fused.out, b.fused.out) and torch.equal(a.batch, b.batch)


# ------------------------------------------------------------------------------------------------ 7. errors
def test_bad_arguments(rings):
    L = _lib.lib()
    prio, _, _ = rings["S"]
    buf = _buffer("S", prio)
    before = [x.clone() for x in (buf.prio, buf.sum1, buf.min1, buf.sum2, buf.min2, buf.per_state, buf.counters)]
    out, idx, w = torch.zeros((32, 50), device=DEV), torch.zeros(32, dtype=torch.int32, device=DEV), torch.zeros(32, device=DEV)
    td = torch.zeros(32, device=DEV)
    BIG = 2 ** 22 + 4

    def sample(ring=buf.ring, cap=64, ctr=buf.counters, o=out, pr=buf.prio, s1=buf.sum1, s2=buf.sum2, st=buf.per_state, beta=0.4, steps=0, B=32, row=50):
        return L.fw_replay_sample_per(_p(ring), cap, _p(ctr), 1, row, B, _p(o), _p(idx), _p(w), _p(pr), _p(s1), _p(s2), _p(st), beta, steps, None)

    assert sample() == K.FW_OK
    for kw in (dict(ring=None), dict(ctr=None), dict(o=None), dict(pr=None), dict(s1=None), dict(s2=None), dict(st=None), dict(B=0),
               dict(row=0), dict(cap=0), dict(beta=-0.1), dict(beta=1.5), dict(beta=float("nan")), dict(steps=-1)):
        assert sample(**kw) == K.FW_EINVAL, kw
    assert sample(cap=BIG) == K.FW_EUNSUPPORTED and b"2^22" in L.fw_last_error(None)

    def rebuild(pr=buf.prio, cap=64, s1=buf.sum1, m1=buf.min1, s2=buf.sum2, m2=buf.min2, st=buf.per_state):
        return L.fw_replay_per_rebuild(_p(pr), cap, _p(s1), _p(m1), _p(s2), _p(m2), _p(st), None)

    assert rebuild() == K.FW_OK
    for kw in (dict(pr=None), dict(s1=None), dict(m1=None), dict(s2=None), dict(m2=None), dict(st=None), dict(cap=0), dict(cap=-4)):
        assert rebuild(**kw) == K.FW_EINVAL, kw
    assert rebuild(cap=BIG) == K.FW_EUNSUPPORTED

    def mark(pr=buf.prio, cap=64, ctr=buf.counters, st=buf.per_state, N=4):
        return L.fw_replay_per_mark_new(_p(pr), cap, _p(ctr), _p(st), N, None)

    for kw in (dict(pr=None), dict(ctr=None), dict(st=None), dict(N=0), dict(N=5), dict(cap=0)):
        assert mark(**kw) == K.FW_EINVAL, kw
    assert mark(cap=BIG) == K.FW_EUNSUPPORTED

    def update(pr=buf.prio, cap=64, i=idx, t=td, B=32, alpha=0.6, eps=1e-6, st=buf.per_state):
        return L.fw_replay_per_update(_p(pr), cap, _p(i), _p(t), B, alpha, eps, _p(st), None)

    for kw in (dict(pr=None), dict(i=None), dict(t=None), dict(st=None), dict(B=0), dict(alpha=-0.1), dict(alpha=1.01), dict(eps=0.0),
               dict(eps=-1.0), dict(cap=0)):
        assert update(**kw) == K.FW_EINVAL, kw
    assert update(cap=BIG) == K.FW_EUNSUPPORTED
    torch.cuda.synchronize()
    for x, y in zip(before, (buf.prio, buf.sum1, buf.min1, buf.sum2, buf.min2, buf.per_state, buf.counters)):
        assert torch.equal(x, y)                                  # the refused calls ran nothing (the accepted ones recompute the same)
    # an index outside the ring and a td that is not finite are skipped
    bad_idx = torch.tensor([64, -1, 2 ** 30, 9] + [1] * 28, dtype=torch.int32, device=DEV)
    bad_td = torch.tensor([1.0, 1.0, 1.0, float("nan")] + [0.5] * 28, device=DEV)
    assert update(i=bad_idx, t=bad_td) == K.FW_OK
    torch.cuda.synchronize()
    got = buf.prio.cpu().numpy()
    assert got[9] == 0.0 and np.array_equal(np.delete(got, [1, 9]), np.delete(prio, [1, 9])) and float(buf.per_state[S.PER_MAX]) == 1.0
    # the weighted step: NULL weights, the shape rules of fw_sac_update
    img, rows, ctr, o8 = torch.zeros(400_000, device=DEV), torch.zeros((64, 50), device=DEV), _counters(), torch.zeros(8, device=DEV)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
    H = S._SacHyper(lr=3e-4, gamma=0.99, tau=0.02, beta1=0.9, beta2=0.999, eps=1e-8, target_entropy=-6.0, ent_coef=0.0, auto_ent=1,
                    target_update_interval=1, seed=1)
    ones = torch.ones(64, device=DEV)
    upd = lambda B=64, wt=ones, im=img: L.fw_sac_update_weighted(_p(im), _p(rows), 21, 6, 64, B, C.byref(H), _p(ctr), _p(o8), _p(ws), ws.numel(),
                                                                 _p(wt), None, None)
    assert upd(wt=None) == K.FW_EINVAL and upd(im=None) == K.FW_EINVAL and upd(B=24) == K.FW_EUNSUPPORTED and upd(B=0) == K.FW_EINVAL
    torch.cuda.synchronize()
    assert float(img.abs().sum()) == 0.0 and ctr.tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="not built"):
        S.SAC(_env(), S.SACConfig(batch_size=32, net_arch=(64, 64), prioritized=True, n_steps=3))
