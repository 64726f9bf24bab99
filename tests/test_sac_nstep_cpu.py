"""n-step returns from the replay ring, without a GPU: sac.nstep_rows_reference (the numpy statement of fw_replay_sample_nstep's
contract, which tests/test_sac_nstep_gpu.py holds the kernel to) against a computation from per-env trajectory lists, the done-column
encoding, and the config / checkpoint rules."""
import numpy as np
import pytest
import torch

from pyflyt_drone_amd import sac as S

import sac_cases as SC
import sac_nstep_cases as NC

D, A, GAMMA = 5, 2, 0.99


def _filled(stores):
    ring = SC.NumpyRing(NC.RING_STEPS * NC.N_ENVS + 3, NC.N_ENVS, D, A)      # capacity rounds down to 6 vec-steps
    for s in stores:
        ring.store(*s)
    return ring, NC.numpy_ends(stores)


@pytest.mark.parametrize("stored", [NC.HALF, NC.STEPS])
@pytest.mark.parametrize("n_steps", NC.N_STEPS)
def test_reference_against_the_trajectory_lists(stored, n_steps):
    stores = NC.script(D, A)[:stored]
    ring, ends = _filled(stores)
    assert ring.capacity == NC.RING_STEPS * NC.N_ENVS and (ring.size < ring.capacity) == (stored == NC.HALF)
    assert (ring.cursor != 0 and ring.steps > NC.RING_STEPS) == (stored == NC.STEPS)          # wrapped, and not back at row 0
    idx = np.arange(ring.size)
    rows, ks = S.nstep_rows_reference(ring.ring, ends, ring.cursor, ring.size, NC.N_ENVS, idx, n_steps, GAMMA, D)
    assert rows.dtype == np.float32 and rows.shape == (ring.size, ring.ring.shape[1]) and ks.dtype == np.int32
    traj = NC.trajectories(stores)
    NC.check_rows(rows, ks, traj, D, A, n_steps, GAMMA, f"{stored} stores")
    # the script does what it says: walks are cut by ends and by the newest step, and whole ones exist where they fit
    assert ks.min() == 1 and ks.max() == min(n_steps, min(stored, NC.RING_STEPS))      # (env 3 / env 0 fly through the whole window)
    kinds = {int(e) for e in ends[:ring.size]}
    assert kinds == {0, 1, 2, 3}


def test_the_script_places_the_ends_the_cases_need():
    stores = NC.script(D, A)
    flags = {k: v for k, v in NC.ENDS.items()}
    assert flags[(4, 3)] != (0, 0) and flags[(5, 3)] != (0, 0)                               # consecutive steps of one env
    assert any(t == NC.HALF - 1 for t, _ in flags) and any(t == NC.STEPS - 1 for t, _ in flags)      # one in each newest step
    for t, s in enumerate(stores):
        for e in range(NC.N_ENVS):
            assert (int(s[5][e]), int(s[6][e])) == flags.get((t, e), (0, 0))


@pytest.mark.parametrize("stored", [NC.HALF, NC.STEPS])
def test_one_step_returns_the_ring_rows(stored):
    ring, ends = _filled(NC.script(D, A)[:stored])
    idx = np.arange(ring.size)[::-1]
    rows, ks = S.nstep_rows_reference(ring.ring, ends, ring.cursor, ring.size, NC.N_ENVS, idx, 1, GAMMA, D)
    assert np.array_equal(rows.view(np.uint32), ring.ring[idx].view(np.uint32)) and (ks == 1).all()


@pytest.mark.parametrize("gamma", [0.99, 0.5, 0.999])
def test_the_done_column_hands_the_update_gamma_to_the_k(gamma):
    stores = NC.script(D, A)
    ring, ends = _filled(stores)
    g = float(np.float32(gamma))
    for n in NC.N_STEPS:
        idx = np.arange(ring.size)
        rows, ks = S.nstep_rows_reference(ring.ring, ends, ring.cursor, ring.size, NC.N_ENVS, idx, n, gamma, D)
        last_row = (idx + (ks - 1) * NC.N_ENVS) % ring.capacity
        done = ring.ring[last_row, -1].astype(np.float64)
        got = (1.0 - rows[:, -1].astype(np.float64)) * g            # what the gradient step forms
        assert np.abs(got - (1.0 - done) * g ** ks).max() <= (n + 1) * NC.U
        assert set(np.unique(done)) == {0.0, 1.0}


def test_edge_discounts():
    ring, ends = _filled(NC.script(D, A))
    idx = np.arange(ring.size)
    rcol = D + A
    for n in (3, 16):
        rows0, k0 = S.nstep_rows_reference(ring.ring, ends, ring.cursor, ring.size, NC.N_ENVS, idx, n, 0.0, D)
        rows1, k1 = S.nstep_rows_reference(ring.ring, ends, ring.cursor, ring.size, NC.N_ENVS, idx, n, 1.0, D)
        assert np.array_equal(k0, k1)                                # the walk does not depend on the discount
        # gamma 0: the reward is r_0, and a transition of more than one row never bootstraps (its last column is 1)
        assert np.array_equal(rows0[:, rcol], ring.ring[idx, rcol])
        assert np.array_equal(rows0[k0 > 1, -1], np.ones(int((k0 > 1).sum()), dtype=np.float32))
        # gamma 1: the plain sum, and the last column is done_(k-1) itself
        last_row = (idx + (k1 - 1) * NC.N_ENVS) % ring.capacity
        assert np.array_equal(rows1[:, -1], ring.ring[last_row, -1])
        for b in range(len(idx)):
            want = np.float32(0)
            for j in range(k1[b]):
                r = ring.ring[(idx[b] + j * NC.N_ENVS) % ring.capacity, rcol]
                want = r if j == 0 else np.float32(want + r)
            assert rows1[b, rcol] == want


def test_reference_rejects_what_the_entry_point_rejects():
    ring, ends = _filled(NC.script(D, A))
    args = (ring.ring, ends, ring.cursor, ring.size, NC.N_ENVS, np.arange(4))
    for n in (0, 17):
        with pytest.raises(ValueError):
            S.nstep_rows_reference(*args, n, GAMMA, D)
    with pytest.raises(ValueError):
        S.nstep_rows_reference(ring.ring, ends[:-1], ring.cursor, ring.size, NC.N_ENVS, np.arange(4), 3, GAMMA, D)
    with pytest.raises(ValueError):
        S.nstep_rows_reference(ring.ring, ends, ring.cursor, ring.size, NC.N_ENVS, np.array([ring.size]), 3, GAMMA, D)


def test_config_validation():
    assert S.SACConfig().n_steps == 1 and S.SACConfig(n_steps=16).n_steps == 16 and S.MAX_N_STEPS == 16
    for bad in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError):
            S.SACConfig(n_steps=bad)
    with pytest.raises(ValueError):
        S.ReplayBufferDevice(24, 4, D, A, "cpu", n_steps=17)


def test_checkpoint_rules():
    one, three = S.ReplayBufferDevice(24, 4, D, A, "cpu"), S.ReplayBufferDevice(24, 4, D, A, "cpu", n_steps=3)
    assert one.ends is None and one.n_steps == 1                     # off: no side ring at all
    assert three.ends.dtype == torch.uint8 and three.ends.shape == (24,)
    three.ends.copy_(torch.arange(24) % 4); three.ring.normal_(); three.counters.copy_(torch.tensor([8, 24, 8, 5]))
    # the rows travel with their ends
    sd = three.state_dict(include_buffer=True)
    assert torch.equal(sd["ends"], three.ends) and sd["ends"] is not three.ends
    assert "ends" not in three.state_dict() and "ends" not in one.state_dict(include_buffer=True)
    other = S.ReplayBufferDevice(24, 4, D, A, "cpu", n_steps=5)
    other.load_state_dict(sd)
    assert torch.equal(other.ends, three.ends) and torch.equal(other.ring, three.ring) and other.counters.tolist() == [8, 24, 8, 5]
    # without rows the ring starts empty, and so do its ends
    other.load_state_dict(three.state_dict())
    assert int(other.ends.sum()) == 0 and float(other.ring.abs().sum()) == 0.0 and other.counters.tolist() == [0, 0, 8, 5]
    # rows without ends cannot serve an n-step learner; a 1-step learner takes either checkpoint
    one.ring.normal_()
    with pytest.raises(ValueError):
        three.load_state_dict(one.state_dict(include_buffer=True))
    assert torch.equal(three.ends, torch.arange(24, dtype=torch.uint8) % 4)          # (the refused load changed nothing)
    one.load_state_dict(sd)
    assert torch.equal(one.ring, three.ring) and one.ends is None


# (i, limit, cursor, rows whose ends byte is set) -> k on a 24-row ring of 4 envs (vec-step t is rows 4 t .. 4 t + 3), worked out by hand
WALKS = [
    (1, 3, 20, (), 3),           # stops at the limit: rows 1, 5, 9; no end, and the newest vec-step (rows 16 .. 19) is further on
    (2, 5, 20, (6,), 2),         # stops at an ends byte: rows 2, 6
    (9, 5, 20, (), 3),           # stops at the newest vec-step: rows 9, 13, 17, and 17 lies in rows 16 .. 19
    (19, 5, 8, (), 4),           # wraps past the end of the ring: rows 19, 23, 3, 7, and 7 lies in the newest vec-step, rows 4 .. 7
    (14, 5, 0, (), 3),           # cursor == 0: the newest vec-step is the ring's last one, rows 20 .. 23; rows 14, 18, 22
]


@pytest.mark.parametrize("i,limit,cursor,marked,k", WALKS)
def test_the_walk_by_hand(i, limit, cursor, marked, k):
    cap, n = 24, 4
    ends = np.zeros(cap, dtype=np.uint8)
    ends[list(marked)] = S.END_TRUNCATED
    assert S._walk(i, limit, ends, n, cap, (cursor - n) % cap) == k
    rng = np.random.default_rng(i)
    ring = rng.standard_normal((cap, S.row_floats(D, A))).astype(np.float32)
    assert S.nstep_rows_reference(ring, ends, cursor, cap, n, [i], limit, GAMMA, D)[1].tolist() == [k]
    her_ring = rng.standard_normal((cap, S.HER_ROW_FLOATS)).astype(np.float32)
    js = S.her_rows_reference(her_ring, ends, cursor, cap, n, [i], [1], [2 ** 32 - 1], limit, S.HerTask(0, 100.0, 5.0))[1]
    assert js.tolist() == [k - 1]
