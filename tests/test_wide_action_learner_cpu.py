"""Six-action learner: the size / layout entry points of the C ABI and the eligibility rules of the fused update (no device)."""
import ctypes as C

import numpy as np
import pytest
import torch

from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R


def _L():
    return _lib.lib()


def _net(dp, ko):
    return dp * 64 + 64 + 64 * 64 + 64 + 64 * ko + ko


@pytest.mark.parametrize("d", [5, 21, 28, 64])
def test_param_count_a_follows_the_flat_layout(d):
    L, dp = _L(), (d + 1) & ~1
    assert L.fw_ppo_param_count_a(d, 4) == L.fw_ppo_param_count(d) == _net(dp, 4) + _net(dp, 1) + 4
    assert L.fw_ppo_param_count_a(d, 6) == _net(dp, 6) + _net(dp, 1) + 6


@pytest.mark.parametrize("a", [0, 1, 3, 5, 7, 8, -6])
def test_entry_points_refuse_other_action_widths(a):
    L = _L()
    assert L.fw_ppo_param_count_a(21, a) == K.FW_EINVAL
    assert "act_dim" in L.fw_last_error(None).decode()
    assert L.fw_ppo_moment_count_a(a) == K.FW_EINVAL
    smap = np.empty(2 * L.fw_ppo_moment_count_a(6), dtype=np.int32)
    assert L.fw_ppo_moment_map_a(21, a, smap.ctypes.data_as(C.c_void_p)) == K.FW_EINVAL
    assert L.fw_ppo_update_workspace_bytes_a(4, 64, 21, a) == K.FW_EINVAL
    # the launching entry points check the width before they look at anything else (no buffer is touched)
    assert L.fw_ppo_update_a(*([None] * 9), 4, 64, 21, a, None, None, None, 0, None) == K.FW_EINVAL
    assert L.fw_policy_act_a(None, None, 64, 21, a, 3, 0, None, 0, None, None, None, 0, None, None, None) == K.FW_EINVAL
    assert L.fw_collect_act_a(None, None, 0, 64, 21, a, None, None, 10.0, 1e-8, 3, 0, None, 0, None, None, None, 0, None, None,
                              None, None, None, None, None, 1, 10.0, 1e-8, 0.99, None, None, None) == K.FW_EINVAL
    assert "act_dim must be 4 or 6" in L.fw_last_error(None).decode()


def test_workspace_and_moment_counts():
    L = _L()
    assert L.fw_ppo_moment_count_a(4) == L.fw_ppo_moment_count()
    assert L.fw_ppo_moment_count_a(6) == L.fw_ppo_moment_count() + 2 * 256          # one more slot row of 256 threads
    for n_mb, bs, d in ((1, 16, 5), (40, 64, 21), (200, 128, 28)):
        w4 = L.fw_ppo_update_workspace_bytes(n_mb, bs, d)
        assert L.fw_ppo_update_workspace_bytes_a(n_mb, bs, d, 4) == w4
        # six actions: one more per-thread element in each of the 32 exchange regions, and a packed row 4 floats wider
        assert L.fw_ppo_update_workspace_bytes_a(n_mb, bs, d, 6) == w4 + 4 * 32 * 256 + 4 * 4 * n_mb * bs


def _map(d, a):
    L = _L()
    smap = np.empty(L.fw_ppo_moment_count_a(a), dtype=np.int32)
    assert L.fw_ppo_moment_map_a(d, a, smap.ctypes.data_as(C.c_void_p)) == K.FW_OK
    return smap


@pytest.mark.parametrize("d", [5, 21, 28, 63, 64])
def test_moment_map_a_covers_every_parameter_once(d):
    L = _L()
    old = np.empty(L.fw_ppo_moment_count(), dtype=np.int32)
    assert L.fw_ppo_moment_map(d, old.ctypes.data_as(C.c_void_p)) == K.FW_OK
    np.testing.assert_array_equal(_map(d, 4), old)                         # four actions: the map of before
    dp = (d + 1) & ~1
    for a in (4, 6):
        m = _map(d, a)
        owned = m[m >= 0]
        n = L.fw_ppo_param_count_a(d, a)
        assert len(owned) == len(set(owned.tolist()))                      # no parameter has two slots
        pad = set()                                                        # W1's zero row of an odd observation width has none
        if dp != d:
            for off in (0, _net(dp, a)):
                pad |= set(range(off + d * 64, off + dp * 64))
        assert set(owned.tolist()) == set(range(n)) - pad
        assert (m[len(m) // 2:] == -1).all()                               # the second half of the buffers stays unused


def test_moment_map_a6_places_the_second_head_word_in_row_9():
    d, dp = 21, 22
    m = _map(d, 6)
    tile_slots = 2 * 3 * 4 * 64 * 16
    o_wo = dp * 64 + 64 + 64 * 64 + 64                                     # Wo of the policy net
    for t in range(256):
        i, c = t >> 2, t & 3
        assert m[tile_slots + 7 * 256 + t] == o_wo + i * 6 + c             # Wo[i][c], c < 4
        assert m[tile_slots + 9 * 256 + t] == (o_wo + i * 6 + 4 + c if c < 2 else -1)      # Wo[i][4 + c], c < 2
    o_ls = _net(dp, 6) + _net(dp, 1)
    assert [m[tile_slots + 6 * 256 + k] for k in range(7)] == [o_ls + k for k in range(6)] + [-1]      # log_std[6]
    assert [m[tile_slots + 2 * 256 + k] for k in range(7)] == [o_wo + 64 * 6 + k for k in range(6)] + [-1]   # bo[6]


def test_six_actions_are_fused_only_when_asked():
    cuda = torch.device("cuda")                      # (a device object: nothing runs on it here)
    for d in (21, 28):
        pol = R.MlpPolicy(d, 6)
        assert not R.FusedPpoUpdate.fits(pol, d, cuda)                                        # the default: four actions only
        assert not R.FusedPpoUpdate.applies(pol, R.PPOConfig(), d, 64, cuda)
        assert R.FusedPpoUpdate.applies(pol, R.PPOConfig(fused_six_actions=True), d, 64, cuda)
        assert not R.FusedPpoUpdate.applies(pol, R.PPOConfig(fused_six_actions=True), d, 64, torch.device("cpu"))
        assert not R.FusedPpoUpdate.applies(pol, R.PPOConfig(fused_six_actions=True, fused_update=False), d, 64, cuda)
        assert R.FusedPpoUpdate.applies(R.MlpPolicy(d, 4), R.PPOConfig(fused_six_actions=True), d, 64, cuda)
        for a in (5, 8):
            for cfg in (R.PPOConfig(), R.PPOConfig(fused_six_actions=True)):
                assert not R.FusedPpoUpdate.applies(R.MlpPolicy(d, a), cfg, d, 64, cuda)
    assert R.PPOConfig().fused_six_actions is False
