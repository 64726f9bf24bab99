"""n-step returns from the device replay ring (fw_replay_mark_ends, fw_replay_sample_nstep, SACConfig.n_steps) on the GPU: the kernel
against sac.nstep_rows_reference and against the per-env trajectory lists of tests/sac_nstep_cases.py, its reproducibility, the learner
with n_steps = 3, and a walk that crosses a time-limit end."""
import ctypes as C

import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import sac as S

import sac_nstep_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"
_p = S._p
GAMMA, SEED, B = 0.99, 9, 256


def _t(x):
    return torch.as_tensor(x, device=DEV)


def _push(buf, stores):
    for s in stores:
        buf.store(*(_t(x) for x in s))


def _nstep_raw(buf, ends, n, B, seed=SEED, gamma=GAMMA, k=True):
    """fw_replay_sample_nstep itself on buf's ring and counters: (rc, rows, idx, k)."""
    out, idx = torch.zeros((B, buf.row), device=DEV), torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ks = torch.zeros(B, dtype=torch.int32, device=DEV) if k else None
    rc = _lib.lib().fw_replay_sample_nstep(_p(buf.ring), buf.capacity, _p(buf.counters), seed, buf.row, B, _p(out), _p(idx), _p(ends),
                                           buf.obs_dim, buf.num_envs, n, gamma, _p(ks), None)
    return rc, out, idx, ks


def _one_step_raw(buf, B, seed=SEED):
    out, idx = torch.zeros((B, buf.row), device=DEV), torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().fw_replay_sample(_p(buf.ring), buf.capacity, _p(buf.counters), seed, buf.row, B, _p(out), _p(idx), None))
    return out, idx


def _bits(x):
    return x.detach().cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the kernel against the reference
@pytest.mark.parametrize("stored", [NC.HALF, NC.STEPS], ids=["half_full", "wrapped"])
@pytest.mark.parametrize("d,A", [(21, 6), (64, 8)], ids=["row50", "row138"])          # the second row is wider than one wave
def test_kernel_against_the_reference(d, A, stored):
    """Bounds (tests/sac_nstep_cases.check_rows): reward within (2n + 1) 2^-24 sum|gamma^j r_j| of the float64 sum of the stored fp32
    rewards, last column within (n + 1) 2^-24 of 1 - (1 - done) gamma^(k-1); everything else bit for bit."""
    stores = NC.script(d, A, seed=d)[:stored]
    traj, ends_np = NC.trajectories(stores), NC.numpy_ends(stores)
    n_env, cap = NC.N_ENVS, NC.RING_STEPS * NC.N_ENVS
    size = min(stored, NC.RING_STEPS) * n_env
    for n in NC.N_STEPS:
        buf = S.ReplayBufferDevice(cap + 3, n_env, d, A, DEV, n_steps=max(n, 2))      # (n = 1 owns no ends: it borrows a 2-step buffer's)
        assert buf.capacity == cap
        _push(buf, stores)
        assert np.array_equal(buf.ends.cpu().numpy(), ends_np)
        assert buf.counters.tolist() == [stored * n_env % cap, size, stored, 0]
        ring_np = buf.ring.cpu().numpy()
        seen = np.zeros(cap, dtype=bool)
        for c in range(8):
            buf.counters[S.CTR_GRAD] = c
            want_rows1, want_idx = _one_step_raw(buf, B)
            if n == 1:
                rc, rows, idx, ks = _nstep_raw(buf, buf.ends, 1, B)
                assert rc == K.FW_OK
                assert np.array_equal(_bits(rows), _bits(want_rows1))           # the whole batch is fw_replay_sample's
            else:
                rows, idx = torch.zeros((B, buf.row), device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
                ks = torch.zeros(B, dtype=torch.int32, device=DEV)
                buf.sample(SEED, rows, idx, gamma=GAMMA, k_out=ks)
            assert torch.equal(idx, want_idx)
            i = idx.cpu().numpy()
            assert i.min() >= 0 and i.max() < size
            seen[i] = True
            ref_rows, ref_k = S.nstep_rows_reference(ring_np, ends_np, buf.cursor, size, n_env, i, n, GAMMA, d)
            got, got_k = rows.cpu().numpy(), ks.cpu().numpy()
            assert np.array_equal(got_k, ref_k)
            rc_ = d + A
            assert np.array_equal(got[:, :rc_].view(np.uint32), ref_rows[:, :rc_].view(np.uint32))              # obs | action
            assert np.array_equal(got[:, rc_ + 1:-1].view(np.uint32), ref_rows[:, rc_ + 1:-1].view(np.uint32))  # next_obs
            NC.check_rows(got, got_k, traj, d, A, n, GAMMA, f"counter {c}")       # reward and last column, against float64
        assert seen[:size].all() and not seen[size:].any()       # a condition of the test: 2048 draws over at most 24 rows reach all
        with pytest.raises(ValueError):
            buf.sample(SEED, rows, idx)                          # an n-step buffer's sample needs gamma


# ------------------------------------------------------------------------------------------------ 2. reproducibility
def test_same_counters_same_bits():
    stores = NC.script(21, 6)
    buf = S.ReplayBufferDevice(24, 4, 21, 6, DEV, n_steps=5)
    _push(buf, stores)
    buf.counters[S.CTR_GRAD] = 3
    a, b = _nstep_raw(buf, buf.ends, 5, B), _nstep_raw(buf, buf.ends, 5, B)
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    buf.counters[S.CTR_GRAD] = 4
    assert not torch.equal(_nstep_raw(buf, buf.ends, 5, B)[2], a[2])
    rc, rows, idx, _ = _nstep_raw(buf, buf.ends, 5, B, k=False)                   # k_out is optional
    assert rc == K.FW_OK and int(idx.min()) >= 0


def test_a_replayed_mark_store_sample_equals_eager_calls():
    d, A, n = 21, 6, 3
    stores = NC.script(d, A)[:6]
    _push(S.ReplayBufferDevice(24, 4, d, A, DEV, n_steps=n), stores[:1])          # loads the kernels
    res = []
    for graph in (False, True):
        buf = S.ReplayBufferDevice(24, 4, d, A, DEV, n_steps=n)
        stage = [_t(x).clone() for x in stores[0]]
        rows, idx = torch.zeros((64, buf.row), device=DEV), torch.zeros(64, dtype=torch.int32, device=DEV)
        ks = torch.zeros(64, dtype=torch.int32, device=DEV)

        def step():
            buf.store(*stage)                                    # mark, store, advance
            buf.sample(SEED, rows, idx, gamma=GAMMA, k_out=ks)
            buf.counters[S.CTR_GRAD] += 1

        if graph:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
        hist = []
        for s in stores:
            for dst, src in zip(stage, s):
                dst.copy_(_t(src))
            g.replay() if graph else step()
            hist.append((rows.clone(), idx.clone(), ks.clone()))
        torch.cuda.synchronize()
        res.append((buf.ring.clone(), buf.ends.clone(), buf.counters.clone(), hist))
    for x, y in zip(res[0][:3], res[1][:3]):
        assert torch.equal(x, y)
    assert res[0][2].tolist() == [0, 24, 6, 6] and np.array_equal(res[0][1].cpu().numpy(), NC.numpy_ends(stores))
    for (r0, i0, k0), (r1, i1, k1) in zip(res[0][3], res[1][3]):
        assert np.array_equal(_bits(r0), _bits(r1)) and torch.equal(i0, i1) and torch.equal(k0, k1)
    assert int(res[0][3][-1][2].max()) == n                      # the later steps do span n rows


# ------------------------------------------------------------------------------------------------ 3. the learner
VEC_STEPS = 12


def _env(seed=3):
    return P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=4), 16, seed=seed)      # a short time limit: truncated ends inside the run


def _sac(fused=True, graphs=False, buffer_steps=8, **kw):
    kw.setdefault("n_steps", 3)
    cfg = S.SACConfig(batch_size=64, net_arch=(64, 64), learning_starts=32, gradient_steps=2, seed=7, use_graphs=graphs,
                      fused_update=fused, buffer_size=16 * buffer_steps, **kw)          # 8 vec-steps: the 12 of a run wrap the ring
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
    assert (a.buffer.ends is None) == (b.buffer.ends is None)
    if a.buffer.ends is not None:
        assert torch.equal(a.buffer.ends, b.buffer.ends)


def test_learner_counts_and_the_batch_it_trains_on(eager_run):
    sac = eager_run
    assert sac.buffer.n_steps == 3 and sac.buffer.counters.tolist() == [64, 128, 12, 20] and sac.n_updates == 20
    assert all(torch.isfinite(q).all() for q in sac.policy.parameters())
    ends = sac.buffer.ends.cpu().numpy()
    assert (ends & S.END_TRUNCATED).any() and ends.max() <= 3
    # the last gradient step's batch is the n-step batch of the reference at the counter it was drawn with
    idx = sac.batch_idx.cpu().numpy()
    ref_rows, ref_k = S.nstep_rows_reference(sac.buffer.ring.cpu().numpy(), ends, 64, 128, 16, idx, 3, sac.cfg.gamma, 21)
    got = sac.batch.cpu().numpy()
    assert np.array_equal(got[:, :27], ref_rows[:, :27]) and np.array_equal(got[:, 28:49], ref_rows[:, 28:49])
    assert ref_k.max() == 3 and np.abs(got[:, 49].astype(np.float64) - ref_rows[:, 49]).max() <= 4 * NC.U


def test_graph_replay_equals_eager_bit_for_bit(eager_run):
    b = _run(_sac(graphs=True))
    assert len(b._graphs) == 2 and all(isinstance(g, torch.cuda.CUDAGraph) for g in b._graphs.values())      # warm-up and training
    _same(eager_run, b)
    assert torch.equal(eager_run.fused.out, b.fused.out) and torch.equal(eager_run.batch, b.batch)


def test_fused_and_torch_learners_sample_the_same_batches(eager_run):
    """The two gradient steps differ in rounding (tests/test_sac_gpu.py compares them under tolerances), so two independent runs stop
    holding the same bits once a trained actor has acted.  From a common checkpoint the next vec-step is identical in both -- the rows
    stored, their ends, the counters and the batch drawn -- which is what this checks; the update itself is unchanged."""
    a = _run(_sac(), 6)
    b = _sac(fused=False)
    b.env.reset_tensor(); b._started = True
    b.env.set_state(a.env.get_state()); b.env.obs.copy_(a.env.obs)
    b.load_state_dict(a.state_dict(include_buffer=True))
    assert torch.equal(a.buffer.ends, b.buffer.ends) and torch.equal(a.buffer.ring, b.buffer.ring)
    a.collect_step(); b.collect_step()                          # (both gradient steps of it draw from the same ring at the same counters)
    torch.cuda.synchronize()
    assert torch.equal(a.buffer.ring, b.buffer.ring) and torch.equal(a.buffer.ends, b.buffer.ends)
    assert a.buffer.counters.tolist() == b.buffer.counters.tolist() == [112, 112, 7, 10]
    assert torch.equal(a.batch_idx, b.batch_idx) and np.array_equal(_bits(a.batch), _bits(b.batch))
    k = torch.zeros(64, dtype=torch.int32, device=DEV)
    a.buffer.counters[S.CTR_GRAD] = 9                           # the counter that batch was drawn at
    a.buffer.sample(a.cfg.seed, torch.zeros_like(a.batch), None, gamma=a.cfg.gamma, k_out=k)
    assert int(k.max()) == 3 and int(k.min()) == 1


def test_state_dict_round_trip_continues_bit_identically():
    a = _run(_sac(), 9)                                           # the ring has wrapped
    sd = a.state_dict(include_buffer=True)
    assert sd["config"]["n_steps"] == 3 and torch.equal(sd["buffer"]["ends"], a.buffer.ends.cpu())
    b = _sac()
    b.env.reset_tensor(); b._started = True
    b.env.set_state(a.env.get_state()); b.env.obs.copy_(a.env.obs)
    b.load_state_dict(sd)
    _run(a, 3); _run(b, 3)
    _same(a, b)
    assert a.buffer.counters.tolist() == [64, 128, 12, 20] and a.num_timesteps == b.num_timesteps == 192
    for (name, p), q in zip(a.policy.named_parameters(), b.policy.parameters()):
        assert torch.equal(p, q), name
    one = _sac(n_steps=1)
    with pytest.raises(ValueError):                               # rows without ends cannot serve an n-step learner
        b.load_state_dict(one.state_dict(include_buffer=True))


def test_one_step_is_the_default_learner_bit_for_bit():
    a = _run(_sac(n_steps=1), 8)
    cfg = S.SACConfig(batch_size=64, net_arch=(64, 64), learning_starts=32, gradient_steps=2, seed=7, use_graphs=False, buffer_size=16 * 8)
    b = _run(S.SAC(_env(), cfg), 8)
    assert a.buffer.ends is None and b.buffer.ends is None and b.cfg.n_steps == 1
    _same(a, b)
    assert torch.equal(a.fused.out, b.fused.out) and torch.equal(a.batch, b.batch)


# ------------------------------------------------------------------------------------------------ 4. a walk across a time-limit end
def test_a_walk_stops_at_a_truncated_end_and_bootstraps(eager_run):
    sac, n, g = eager_run, 3, float(np.float32(eager_run.cfg.gamma))
    buf = sac.buffer
    ring, ends = buf.ring.cpu().numpy(), buf.ends.cpu().numpy()
    cap, newest = buf.capacity, (buf.cursor - 16) % buf.capacity
    rows, idx = torch.zeros((256, buf.row), device=DEV), torch.zeros(256, dtype=torch.int32, device=DEV)
    ks = torch.zeros(256, dtype=torch.int32, device=DEV)
    keep = buf.counters.clone()
    crossed = 0
    for c in range(4):
        buf.counters[S.CTR_GRAD] = 100 + c
        buf.sample(sac.cfg.seed, rows, idx, gamma=sac.cfg.gamma, k_out=ks)
        got, i, k = rows.cpu().numpy(), idx.cpu().numpy().astype(np.int64), ks.cpu().numpy()
        last = (i + (k - 1) * 16) % cap
        # walks of two rows that a pure time-limit end cut short (not the newest step, not a crash): row_0 flew on, row_1 was truncated
        cut = (k == 2) & (ends[last] == S.END_TRUNCATED) & (last - last % 16 != newest)
        crossed += int(cut.sum())
        assert (ends[i[cut]] == 0).all()
        assert (k[cut] < n).all()
        # the terminal observation of the truncated step (its row's next_obs), which is not the reset observation the env went on from
        assert np.array_equal(got[cut, 28:49], ring[last[cut], 28:49])
        follows = (last[cut] + 16) % cap
        assert not (ring[last[cut], 28:49] == ring[follows, :21]).all(1).any()
        assert np.array_equal(ring[i[cut], 28:49], ring[last[cut], :21])         # (inside the episode next_obs is the next row's obs)
        # done = 0 there: the last column is 1 - gamma^(k-1), so the update bootstraps with (1 - last) gamma = gamma^k
        assert (ring[last[cut], 49] == 0).all()
        assert np.abs(got[cut, 49].astype(np.float64) - (1.0 - g ** (k[cut] - 1))).max(initial=0.0) <= (n + 1) * NC.U
        assert (got[cut, 49] < 1.0).all()
        want = ring[i[cut], 27].astype(np.float64) + g * ring[last[cut], 27].astype(np.float64)
        mag = np.abs(ring[i[cut], 27]).astype(np.float64) + g * np.abs(ring[last[cut], 27]).astype(np.float64)
        assert (np.abs(got[cut, 27] - want) <= (2 * n + 1) * NC.U * mag).all()
    buf.counters.copy_(keep)
    assert crossed > 0                                            # the crossing must happen: every 4th vec-step ends by the time limit


# ------------------------------------------------------------------------------------------------ 5. errors
def test_bad_arguments():
    L = _lib.lib()
    buf = S.ReplayBufferDevice(24, 4, 21, 6, DEV, n_steps=2)
    for n in (0, 17, -3):
        rc, rows, idx, _ = _nstep_raw(buf, buf.ends, n, 32)
        assert rc == K.FW_EUNSUPPORTED and b"n_steps" in L.fw_last_error(None)
    assert _nstep_raw(buf, None, 3, 32)[0] == K.FW_EINVAL
    out, ctr = torch.zeros((32, 50), device=DEV), buf.counters
    call = lambda ring=buf.ring, cap=24, row=50, d=21, N=4, batch=32, o=out: L.fw_replay_sample_nstep(
        _p(ring), cap, _p(ctr), 1, row, batch, _p(o), None, _p(buf.ends), d, N, 3, 0.99, None, None)
    assert call() == K.FW_OK
    assert call(ring=None) == K.FW_EINVAL and call(o=None) == K.FW_EINVAL and call(batch=0) == K.FW_EINVAL and call(cap=0) == K.FW_EINVAL
    assert call(N=0) == K.FW_EINVAL and call(N=5) == K.FW_EINVAL and call(d=0) == K.FW_EINVAL and call(d=24) == K.FW_EINVAL      # 24 rows: no multiple of 5; 2 d + 3 > 50
    term = torch.zeros(4, dtype=torch.uint8, device=DEV)
    mark = lambda e=buf.ends, cap=24, N=4, te=term: L.fw_replay_mark_ends(_p(e), cap, _p(ctr), _p(te), _p(term), N, None)
    assert mark() == K.FW_OK
    assert mark(e=None) == K.FW_EINVAL and mark(te=None) == K.FW_EINVAL and mark(N=0) == K.FW_EINVAL and mark(cap=22) == K.FW_EINVAL
    torch.cuda.synchronize()
    assert ctr.tolist() == [0, 0, 0, 0] and int(buf.ends.sum()) == 0          # neither entry point writes a counter
    with pytest.raises(ValueError):
        S.SAC(_env(), S.SACConfig(batch_size=32, net_arch=(64, 64), n_steps=17))
