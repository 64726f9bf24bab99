"""Hindsight goal relabelling from the device replay ring (fw_replay_sample_her, fw_her_reward, SACConfig.her_goals) on the GPU: the
kernel against fw_replay_sample with relabelling off, against sac.her_rows_reference and the per-env trajectory lists of
tests/her_cases.py, the reward's restatement against the env's own stored rewards, reproducibility under graph replay, the learner
with her_goals = 4, and the error codes."""
import ctypes as C

import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import sac as S

import her_cases as HC

pytestmark = pytest.mark.gpu
DEV = "cuda"
_p = S._p
SEED, B = 9, 64
TASKS = {0: S.HerTask(0, 0.0, 0.0), 1: S.HerTask(1, HC.DOME, HC.MIN_SPEED)}


def _t(x):
    return torch.as_tensor(x, device=DEV)


def _bits(x):
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else x).view(np.uint32)


def _buffer(stores, task=TASKS[0], goals=4, horizon=64):
    buf = S.ReplayBufferDevice(HC.RING_STEPS * HC.N_ENVS + 3, HC.N_ENVS, HC.D, HC.A, DEV, her_goals=goals, her_horizon=horizon, her_task=task)
    for s in stores:
        buf.store(*(_t(x) for x in s))
    return buf


def _her_raw(buf, prob, horizon, task, batch=B, seed=SEED, ends="own", d=HC.D, row=HC.ROW, j=True):
    """fw_replay_sample_her itself on buf's ring and counters: (rc, rows, idx, j)."""
    out, idx = torch.zeros((batch, buf.row), device=DEV), torch.full((batch,), -7, dtype=torch.int32, device=DEV)
    js = torch.full((batch,), -7, dtype=torch.int32, device=DEV) if j else None
    rc = _lib.lib().fw_replay_sample_her(_p(buf.ring), buf.capacity, _p(buf.counters), seed, row, batch, _p(out), _p(idx),
                                         _p(buf.ends if ends == "own" else ends), d, buf.num_envs, horizon, prob,
                                         None if task is None else C.byref(task), _p(js), None)
    return rc, out, idx, js


@pytest.fixture(scope="module")
def rings():
    """The scripted rings on the device, half full and wrapped, with their numpy twins and trajectory lists (made once, read only)."""
    out = {}
    for name, stored in (("half_full", HC.HALF), ("wrapped", HC.STEPS)):
        stores = HC.script()[:stored]
        buf = _buffer(stores)
        ring_np, cursor, size = HC.numpy_ring(stores)
        assert np.array_equal(_bits(buf.ring), _bits(ring_np)) and np.array_equal(buf.ends.cpu().numpy(), HC.numpy_ends(stores))
        assert buf.counters.tolist() == [cursor, size, stored, 0]
        out[name] = dict(buf=buf, ring=ring_np, ends=HC.numpy_ends(stores), cursor=cursor, size=size, traj=HC.trajectories(stores))
    return out


# ------------------------------------------------------------------------------------------------ 1. no relabelling
@pytest.mark.parametrize("name", ["half_full", "wrapped"])
def test_without_relabelling_it_is_fw_replay_sample(rings, name):
    buf = rings[name]["buf"]
    for c in (0, 5):
        buf.counters[S.CTR_GRAD] = c
        want, widx = torch.zeros((B, buf.row), device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
        _lib.check(_lib.lib().fw_replay_sample(_p(buf.ring), buf.capacity, _p(buf.counters), SEED, buf.row, B, _p(want), _p(widx), None))
        rc, rows, idx, js = _her_raw(buf, 0.0, 64, TASKS[1])
        assert rc == K.FW_OK
        assert np.array_equal(_bits(rows), _bits(want)) and torch.equal(idx, widx) and (js == -1).all()
    buf.counters[S.CTR_GRAD] = 0


# ------------------------------------------------------------------------------------------------ 2. the kernel against the reference
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", ["half_full", "wrapped"])
@pytest.mark.parametrize("horizon", HC.HORIZONS)
@pytest.mark.parametrize("prob", [0.5, 1.0])
def test_kernel_against_the_reference(rings, prob, horizon, name, variant):
    """j_out, idx_out and every copied column bit for bit; the three goal columns and the reward within one fp32 ulp of the float64
    reference (kernel and reference both compute in double: only the final rounding can differ)."""
    r, task = rings[name], TASKS[variant]
    buf, size = r["buf"], r["size"]
    seen_j = set()
    for c in range(3):
        buf.counters[S.CTR_GRAD] = c
        rc, rows, idx, js = _her_raw(buf, prob, horizon, task)
        assert rc == K.FW_OK
        got, i, j = rows.cpu().numpy(), idx.cpu().numpy().astype(np.int64), js.cpu().numpy()
        # the draws, restated in numpy: the start rows are fw_replay_sample's, the relabel decision and j* come from the second block
        want_idx, o0, o1 = HC.draws(SEED, c, B, size)
        assert np.array_equal(i, want_idx)
        relabel = o0 < np.uint64(int(float(np.float32(prob)) * 2.0 ** 32))
        assert np.array_equal(j >= 0, relabel)
        if prob == 0.5:
            assert 0.1 * B <= relabel.sum() <= 0.9 * B            # the draw is not stuck
        else:
            assert relabel.all()
        ref, ref_j = S.her_rows_reference(r["ring"], r["ends"], r["cursor"], size, HC.N_ENVS, i, relabel, o1, horizon, task)
        assert np.array_equal(j, ref_j)
        copied = np.ones(HC.ROW, dtype=bool)
        copied[[18, 19, 20, HC.RCOL, HC.NOBS + 18, HC.NOBS + 19, HC.NOBS + 20]] = False
        assert np.array_equal(got[:, copied].view(np.uint32), ref[:, copied].view(np.uint32))
        assert np.array_equal(got[:, copied].view(np.uint32), r["ring"][i][:, copied].view(np.uint32))
        assert np.array_equal(got[~relabel].view(np.uint32), r["ring"][i[~relabel]].view(np.uint32))      # not relabelled: the ring row
        # goal columns and reward: within one ulp of the float64 values
        nobs0 = r["ring"][i, HC.NOBS:HC.NOBS + 21]
        fut = r["ring"][(i + np.maximum(j, 0) * HC.N_ENVS) % len(r["ring"]), HC.NOBS:HC.NOBS + 21]
        goal64 = np.stack([fut[:, 5].astype(np.float64), fut[:, 11].astype(np.float64),
                           np.sqrt((fut[:, 6:9].astype(np.float64) ** 2) @ np.ones(3))], axis=1)
        rew64 = S.her_reward_reference(nobs0, got[:, 18:21], r["ring"][i, -1], task)
        for b in np.flatnonzero(relabel):
            for col in range(3):
                ulp = np.spacing(np.float32(abs(goal64[b, col])))
                assert abs(float(got[b, 18 + col]) - goal64[b, col]) <= ulp and got[b, HC.NOBS + 18 + col] == got[b, 18 + col], (b, col)
            assert abs(float(got[b, HC.RCOL]) - rew64[b]) <= np.spacing(np.float32(abs(rew64[b]))), b
            assert abs(float(got[b, HC.RCOL]) - float(ref[b, HC.RCOL])) <= np.spacing(np.float32(abs(rew64[b]))), b
        HC.check_rows(got, j, o1, r["traj"], horizon, f"{name} counter {c}")                # and against the lists, without ring arithmetic
        seen_j |= set(j[relabel].tolist())
    buf.counters[S.CTR_GRAD] = 0
    assert min(seen_j) == 0 and max(seen_j) <= horizon - 1 and (horizon == 1 or max(seen_j) >= 1)


# ------------------------------------------------------------------------------------------------ 3. the restatement against the env
ROLL_STEPS = 64


def _half_ulp(x):
    return 0.5 * np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("variant", [0, 1], ids=["tracking", "demo"])
def test_the_restated_reward_reproduces_the_envs(variant):
    """16 fp64 envs, 64 vec-steps of uniform actions through the learner's own act -> step -> store path; fw_her_reward on the ring
    rows with each row's own goal must give the stored reward.  The ring holds fp32 roundings of the fp64 values the env computed its
    reward from, so the two differ by what a half-ulp perturbation of every input does: the bound is twice its first-order size
    (sum of |d reward / d input| half_ulp(input), from the row's magnitudes; the factor of two covers the second order, the kinks taken at
    their steeper side and the rounding of the airspeed to fp32, which is no larger than the velocity components' share) plus a half ulp
    of the stored and of the recomputed reward.  Only variant-1 rows whose airspeed lies within that perturbation of min_speed (the -2
    step) are excluded, at most 1 % of the rows."""
    make = P.FixedwingLowLevelDemoVecEnv if variant else P.FixedwingLowLevelVecEnv
    env = make(16, seed=5)
    sac = S.SAC(env, S.SACConfig(batch_size=64, net_arch=(64, 64), learning_starts=10 ** 9, buffer_size=16 * ROLL_STEPS, seed=2, use_graphs=False))
    for _ in range(ROLL_STEPS):
        sac.collect_step()
    torch.cuda.synchronize()
    n = 16 * ROLL_STEPS
    assert sac.buffer.counters.tolist() == [0, n, ROLL_STEPS, 0]
    task = S.her_task_of(env.cfg)
    assert task.variant == variant
    rows = sac.buffer.ring
    goals = rows[:, HC.NOBS + 18:HC.NOBS + 21].contiguous()
    out = torch.full((n,), float("nan"), device=DEV)
    _lib.check(_lib.lib().fw_her_reward(_p(rows), HC.ROW, n, HC.D, _p(goals), C.byref(task), _p(out), None))
    got, ring = out.cpu().numpy().astype(np.float64), rows.cpu().numpy()
    stored, no = ring[:, HC.RCOL].astype(np.float64), ring[:, HC.NOBS:HC.NOBS + 21].astype(np.float64)
    hu = _half_ulp(no)
    speed = np.sqrt((no[:, 6:9] ** 2).sum(1))
    d_speed = (np.abs(no[:, 6:9]) * hu[:, 6:9]).sum(1) / speed
    w = (1.5, 1.2, 0.8) if variant else (1.0, 1.0, 0.5)
    bound = w[0] * (hu[:, 18] + hu[:, 5]) + w[1] * (hu[:, 19] + hu[:, 11]) + w[2] * (hu[:, 20] + d_speed)
    keep = np.ones(n, dtype=bool)
    if variant:
        a_norm, rho = np.sqrt((no[:, 12:18] ** 2).sum(1)), np.sqrt((no[:, 9:11] ** 2).sum(1))
        bound = bound + 0.3 * (hu[:, 3] + hu[:, 4])
        bound = bound + 0.05 * (np.abs(no[:, 12:18]) * hu[:, 12:18]).sum(1) / np.maximum(a_norm, 1e-300)
        bound = bound + (np.abs(no[:, 9:11]) * hu[:, 9:11]).sum(1) / np.maximum(rho, 1e-300)
        keep = np.abs(speed - float(task.min_speed)) > 2.0 * d_speed + _half_ulp(speed)
        assert (~keep).sum() <= 0.01 * n, f"{(~keep).sum()} of {n} rows fly within a rounding of min_speed"
    tol = 2.0 * bound + _half_ulp(stored) + _half_ulp(got)
    err = np.abs(got - stored)
    worst = int(np.argmax(np.where(keep, err / tol, 0.0)))
    print(f"variant {variant}: {int(keep.sum())} rows, worst |recomputed - stored| {err[worst]:.3e} against {tol[worst]:.3e}, "
          f"reward range [{stored.min():.4g}, {stored.max():.4g}], terminated rows {int((ring[:, -1] != 0).sum())}")
    assert np.isfinite(got).all() and (err[keep] <= tol[keep]).all()
    # it is the numpy statement's value too, to the rounding
    ref = S.her_reward_reference(ring[:, HC.NOBS:HC.NOBS + 21], ring[:, HC.NOBS + 18:HC.NOBS + 21], ring[:, -1], task)
    assert (np.abs(got - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all()
    env.close()


# ------------------------------------------------------------------------------------------------ 4. replay
def test_a_replayed_mark_store_sample_equals_eager_calls():
    stores = HC.script()[:8]
    _buffer(stores[:1])                                          # loads the kernels
    res = []
    for graph in (False, True):
        buf = _buffer([], task=TASKS[1], goals=4, horizon=5)
        stage = [_t(x).clone() for x in stores[0]]
        rows, idx = torch.zeros((B, buf.row), device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
        js = torch.zeros(B, dtype=torch.int32, device=DEV)

        def step():
            buf.store(*stage)                                    # mark, store, advance
            buf.sample(SEED, rows, idx, j_out=js)
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
            hist.append((rows.clone(), idx.clone(), js.clone()))
        torch.cuda.synchronize()
        res.append((buf.ring.clone(), buf.ends.clone(), buf.counters.clone(), hist))
    for x, y in zip(res[0][:3], res[1][:3]):
        assert torch.equal(x, y)
    assert res[0][2].tolist() == [32, 32, 8, 8]
    for (r0, i0, j0), (r1, i1, j1) in zip(res[0][3], res[1][3]):
        assert np.array_equal(_bits(r0), _bits(r1)) and torch.equal(i0, i1) and torch.equal(j0, j1)
    last = res[0][3][-1][2]
    assert int(last.max()) >= 1 and int(last.min()) == -1        # later steps do relabel from rows ahead, and leave some rows alone


# ------------------------------------------------------------------------------------------------ 5. the learner
VEC_STEPS = 8


def _env(seed=3):
    return P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=4), 16, seed=seed)      # a short time limit: ends inside the run


def _sac(fused=True, graphs=False, **kw):
    kw.setdefault("her_goals", 4)
    cfg = S.SACConfig(batch_size=64, net_arch=(64, 64), learning_starts=32, gradient_steps=2, seed=7, use_graphs=graphs,
                      fused_update=fused, buffer_size=16 * 6, **kw)                      # 6 vec-steps: the 8 of a run wrap the ring
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
    assert sac.buffer.her_goals == 4 and sac.buffer.her_prob == 0.8 and sac.buffer.counters.tolist() == [32, 96, 8, 12] and sac.n_updates == 12
    assert all(torch.isfinite(q).all() for q in sac.policy.parameters())
    ends = sac.buffer.ends.cpu().numpy()
    assert (ends & S.END_TRUNCATED).any()
    # the last gradient step's batch is the reference's at the counter it was drawn with
    idx, (want_idx, o0, o1) = sac.batch_idx.cpu().numpy(), HC.draws(sac.cfg.seed, 11, 64, 96)
    assert np.array_equal(idx, want_idx)
    relabel = o0 < np.uint64(int(float(np.float32(0.8)) * 2.0 ** 32))
    ref, ref_j = S.her_rows_reference(sac.buffer.ring.cpu().numpy(), ends, 32, 96, 16, idx, relabel, o1, 64, sac.buffer.her_task)
    got = sac.batch.cpu().numpy()
    keep = np.ones(50, dtype=bool); keep[27] = False
    assert np.array_equal(got[:, keep], ref[:, keep]) and 0.5 * 64 < relabel.sum() < 64 and ref_j.max() >= 1
    assert (np.abs(got[:, 27].astype(np.float64) - ref[:, 27]) <= np.spacing(np.abs(ref[:, 27]))).all()
    assert not np.array_equal(got[:, 18:21], sac.buffer.ring.cpu().numpy()[idx, 18:21])        # goals did change


def test_graph_replay_equals_eager_bit_for_bit(eager_run):
    b = _run(_sac(graphs=True))
    assert len(b._graphs) == 2 and all(isinstance(g, torch.cuda.CUDAGraph) for g in b._graphs.values())      # warm-up and training
    _same(eager_run, b)
    assert torch.equal(eager_run.fused.out, b.fused.out) and torch.equal(eager_run.batch, b.batch)


def test_fused_and_torch_learners_sample_the_same_batches():
    """As tests/test_sac_nstep_gpu.py: the two gradient steps differ in rounding, so the comparison is over the vec-step that follows
    a common checkpoint -- the rows stored, their ends, the counters and the batch drawn."""
    a = _run(_sac(), 5)
    b = _sac(fused=False)
    b.env.reset_tensor(); b._started = True
    b.env.set_state(a.env.get_state()); b.env.obs.copy_(a.env.obs)
    b.load_state_dict(a.state_dict(include_buffer=True))
    assert torch.equal(a.buffer.ends, b.buffer.ends) and torch.equal(a.buffer.ring, b.buffer.ring)
    a.collect_step(); b.collect_step()
    torch.cuda.synchronize()
    assert torch.equal(a.buffer.ring, b.buffer.ring) and torch.equal(a.buffer.ends, b.buffer.ends)
    assert a.buffer.counters.tolist() == b.buffer.counters.tolist() == [0, 96, 6, 8]
    assert torch.equal(a.batch_idx, b.batch_idx) and np.array_equal(_bits(a.batch), _bits(b.batch))


def test_state_dict_round_trip_continues_bit_identically():
    a = _run(_sac(), 7)                                           # the ring has wrapped
    sd = a.state_dict(include_buffer=True)
    assert sd["config"]["her_goals"] == 4 and sd["config"]["her_horizon"] == 64 and torch.equal(sd["buffer"]["ends"], a.buffer.ends.cpu())
    b = _sac()
    b.env.reset_tensor(); b._started = True
    b.env.set_state(a.env.get_state()); b.env.obs.copy_(a.env.obs)
    b.load_state_dict(sd)
    _run(a, 2); _run(b, 2)
    _same(a, b)
    assert a.buffer.counters.tolist() == [48, 96, 9, 14] and a.num_timesteps == b.num_timesteps == 144
    for (name, p), q in zip(a.policy.named_parameters(), b.policy.parameters()):
        assert torch.equal(p, q), name
    with pytest.raises(ValueError):                               # rows without ends cannot serve a relabelling learner
        b.load_state_dict(_sac(her_goals=0).state_dict(include_buffer=True))


def test_her_off_is_the_default_learner_bit_for_bit():
    a = _run(_sac(her_goals=0), 6)
    cfg = S.SACConfig(batch_size=64, net_arch=(64, 64), learning_starts=32, gradient_steps=2, seed=7, use_graphs=False, buffer_size=16 * 6)
    b = _run(S.SAC(_env(), cfg), 6)
    assert a.buffer.ends is None and b.buffer.ends is None and b.cfg.her_goals == 0
    _same(a, b)
    assert torch.equal(a.fused.out, b.fused.out) and torch.equal(a.batch, b.batch)


def test_the_learner_needs_the_lowlevel_task():
    env = P.FixedwingVecEnv(K.train_waypoints_v3_config(), 16, seed=0)
    with pytest.raises(ValueError, match="low-level task"):
        S.SAC(env, S.SACConfig(batch_size=32, net_arch=(64, 64), her_goals=4))
    env.close()
    demo = S.SAC(P.FixedwingLowLevelDemoVecEnv(16, seed=0), S.SACConfig(batch_size=32, net_arch=(64, 64), her_goals=2, her_horizon=8))
    t = demo.buffer.her_task
    assert (t.variant, t.dome, t.min_speed, demo.buffer.her_horizon) == (1, 800.0, 8.0, 8) and abs(demo.buffer.her_prob - 2 / 3) < 1e-15


# ------------------------------------------------------------------------------------------------ 6. error codes
def test_bad_arguments(rings):
    L, buf = _lib.lib(), rings["wrapped"]["buf"]
    keep = (buf.ring.clone(), buf.ends.clone(), buf.counters.clone())
    assert _her_raw(buf, 0.5, 8, TASKS[0], j=False)[0] == K.FW_OK              # j_out is optional
    rc = _her_raw(buf, 0.5, 8, TASKS[0], d=20)[0]                              # a wrong obs_dim
    assert rc == K.FW_EUNSUPPORTED and b"obs_dim 21" in L.fw_last_error(None)
    assert _her_raw(buf, 0.5, 8, TASKS[0], row=51)[0] == K.FW_EUNSUPPORTED
    for h in (0, 65):
        assert _her_raw(buf, 0.5, h, TASKS[0])[0] == K.FW_EUNSUPPORTED and b"horizon" in L.fw_last_error(None)
    for p in (1.5, -0.1, float("nan")):
        assert _her_raw(buf, p, 8, TASKS[0])[0] == K.FW_EINVAL and b"relabel_prob" in L.fw_last_error(None)
    assert _her_raw(buf, 0.5, 8, S.HerTask(2, 0.0, 0.0))[0] == K.FW_EINVAL and b"variant" in L.fw_last_error(None)
    assert _her_raw(buf, 0.5, 8, TASKS[0], ends=None)[0] == K.FW_EINVAL        # a NULL ends
    assert _her_raw(buf, 0.5, 8, None)[0] == K.FW_EINVAL and _her_raw(buf, 0.5, 8, TASKS[0], batch=0)[0] == K.FW_EINVAL
    rows, goals, out = buf.ring, torch.zeros((40, 3), device=DEV), torch.zeros(40, device=DEV)
    rew = lambda r=rows, row=50, n=40, d=21, g=goals, t=TASKS[1], o=out: L.fw_her_reward(_p(r), row, n, d, _p(g), C.byref(t), _p(o), None)
    assert rew() == K.FW_OK
    assert rew(r=None) == K.FW_EINVAL and rew(g=None) == K.FW_EINVAL and rew(o=None) == K.FW_EINVAL and rew(n=0) == K.FW_EINVAL
    assert rew(t=S.HerTask(-1, 0.0, 0.0)) == K.FW_EINVAL and rew(d=13) == K.FW_EUNSUPPORTED and rew(row=52) == K.FW_EUNSUPPORTED
    torch.cuda.synchronize()
    for x, y in zip(keep, (buf.ring, buf.ends, buf.counters)):               # the gather writes neither ring, nor ends, nor a counter
        assert torch.equal(x, y)
    with pytest.raises(ValueError):
        S.SAC(_env(), S.SACConfig(batch_size=32, net_arch=(64, 64), her_goals=4, her_horizon=65))
