"""Three-action learner (the high-level command task): the size / layout entry points of the C ABI (``*_a3``), the argument block
of ``fw_collect_act_hl`` and the eligibility rules of the fused paths (no device)."""
import ctypes as C
import re
from pathlib import Path

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


def _map3(d):
    L = _L()
    smap = np.empty(L.fw_ppo_moment_count_a3(), dtype=np.int32)
    assert L.fw_ppo_moment_map_a3(d, smap.ctypes.data_as(C.c_void_p)) == K.FW_OK
    return smap


@pytest.mark.parametrize("d", [5, 21, 30, 64])
def test_param_count_a3_follows_the_flat_layout(d):
    dp = (d + 1) & ~1
    assert _L().fw_ppo_param_count_a3(d) == _net(dp, 3) + _net(dp, 1) + 3


@pytest.mark.parametrize("d", [5, 21, 30, 63, 64])
def test_moment_map_a3_covers_every_parameter_once(d):
    L, dp = _L(), (d + 1) & ~1
    m = _map3(d)
    owned = m[m >= 0]
    assert len(owned) == len(set(owned.tolist()))                          # no parameter has two slots
    pad = set()                                                            # W1's zero row of an odd observation width has none
    if dp != d:
        for off in (0, _net(dp, 3)):
            pad |= set(range(off + d * 64, off + dp * 64))
    assert set(owned.tolist()) == set(range(L.fw_ppo_param_count_a3(d))) - pad
    assert (m[len(m) // 2:] == -1).all()                                   # the second half of the buffers stays unused


def test_moment_map_a3_leaves_the_fourth_places_as_padding():
    d, dp = 30, 30
    m = _map3(d)
    tile_slots = 2 * 3 * 4 * 64 * 16
    o_wo = dp * 64 + 64 + 64 * 64 + 64                                     # Wo of the policy net: rows of three
    for t in range(256):
        i, c = t >> 2, t & 3
        assert m[tile_slots + 7 * 256 + t] == (o_wo + i * 3 + c if c < 3 else -1)
    o_ls = _net(dp, 3) + _net(dp, 1)
    assert [m[tile_slots + 6 * 256 + k] for k in range(4)] == [o_ls, o_ls + 1, o_ls + 2, -1]            # log_std[3]
    assert [m[tile_slots + 2 * 256 + k] for k in range(4)] == [o_wo + 192, o_wo + 193, o_wo + 194, -1]  # bo[3]


def test_counts_and_workspace_are_the_four_action_ones():
    """Three actions keep every width of the four-action form: the moment slots, the exchange regions, the packed rows."""
    L = _L()
    assert L.fw_ppo_moment_count_a3() == L.fw_ppo_moment_count()
    for n_mb, bs, d in ((1, 16, 5), (40, 64, 21), (640, 256, 30)):
        assert L.fw_ppo_update_workspace_bytes_a3(n_mb, bs, d) == L.fw_ppo_update_workspace_bytes(n_mb, bs, d)


def test_the_a_family_still_refuses_three_actions():
    L = _L()
    assert L.fw_ppo_param_count_a(30, 3) == K.FW_EINVAL
    assert L.fw_ppo_moment_count_a(3) == K.FW_EINVAL
    smap = np.empty(L.fw_ppo_moment_count_a3(), dtype=np.int32)
    assert L.fw_ppo_moment_map_a(30, 3, smap.ctypes.data_as(C.c_void_p)) == K.FW_EINVAL
    assert L.fw_ppo_update_workspace_bytes_a(4, 64, 30, 3) == K.FW_EINVAL
    assert L.fw_ppo_update_a(*([None] * 9), 4, 64, 30, 3, None, None, None, 0, None) == K.FW_EINVAL
    assert "act_dim must be 4 or 6" in L.fw_last_error(None).decode()


@pytest.mark.parametrize("d", [0, -3, 65])
def test_bad_obs_dim_gives_einval(d):
    L = _L()
    smap = np.empty(L.fw_ppo_moment_count_a3(), dtype=np.int32)
    assert L.fw_ppo_moment_map_a3(d, smap.ctypes.data_as(C.c_void_p)) == K.FW_EINVAL
    assert "fw_ppo_moment_map_a3" in L.fw_last_error(None).decode()
    assert L.fw_ppo_update_workspace_bytes_a3(4, 64, d) == K.FW_EINVAL
    if d <= 0:
        assert L.fw_ppo_param_count_a3(d) == K.FW_EINVAL
    assert L.fw_ppo_moment_map_a3(30, None) == K.FW_EINVAL
    assert L.fw_ppo_update_workspace_bytes_a3(0, 64, 30) == K.FW_EINVAL and L.fw_ppo_update_workspace_bytes_a3(4, 0, 30) == K.FW_EINVAL
    # the launching entry point checks its arguments before it touches a buffer
    assert L.fw_ppo_update_a3(*([None] * 9), 4, 64, 30, None, None, None, 0, None) == K.FW_EINVAL
    assert "fw_ppo_update_a3" in L.fw_last_error(None).decode()


def test_three_actions_are_fused_only_when_asked():
    cuda = torch.device("cuda")                      # (a device object: nothing runs on it here)
    assert R.PPOConfig().fused_three_actions is False
    assert R.FusedPpoUpdate.act_dims(R.PPOConfig()) == (4,)
    assert R.FusedPpoUpdate.act_dims(R.PPOConfig(fused_six_actions=True)) == (4, 6)
    assert 3 in R.FusedPpoUpdate.act_dims(R.PPOConfig(fused_three_actions=True))
    assert 6 not in R.FusedPpoUpdate.act_dims(R.PPOConfig(fused_three_actions=True))
    assert set(R.FusedPpoUpdate.act_dims(R.PPOConfig(fused_three_actions=True, fused_six_actions=True))) == {3, 4, 6}
    pol = R.MlpPolicy(30, 3)
    assert not R.FusedPpoUpdate.fits(pol, 30, cuda)
    assert not R.FusedPpoUpdate.applies(pol, R.PPOConfig(), 30, 256, cuda)
    assert not R.FusedPpoUpdate.applies(pol, R.PPOConfig(fused_six_actions=True), 30, 256, cuda)
    assert R.FusedPpoUpdate.applies(pol, R.PPOConfig(fused_three_actions=True), 30, 256, cuda)
    assert not R.FusedPpoUpdate.applies(pol, R.PPOConfig(fused_three_actions=True), 30, 256, torch.device("cpu"))
    assert not R.FusedPpoUpdate.applies(pol, R.PPOConfig(fused_three_actions=True, fused_update=False), 30, 256, cuda)
    assert not R.FusedPpoUpdate.applies(pol, R.PPOConfig(fused_three_actions=True), 30, 250, cuda)      # not a multiple of 16
    assert R.FusedPpoUpdate.applies(R.MlpPolicy(30, 4), R.PPOConfig(fused_three_actions=True), 30, 256, cuda)
    assert not R.FusedPpoUpdate.applies(R.MlpPolicy(30, 6), R.PPOConfig(fused_three_actions=True), 30, 256, cuda)


def test_collect_hl_args_match_the_header():
    """config.FwCollectHlArgs is fw_collect_hl_args of include/fwsim.h: the size the library was compiled with, and the field names
    in the header's order."""
    assert _L().fw_sizeof_collect_hl_args() == C.sizeof(K.FwCollectHlArgs)
    text = (Path(__file__).resolve().parents[1] / "include" / "fwsim.h").read_text()
    body = re.search(r"typedef struct fw_collect_hl_args \{(.*?)\} fw_collect_hl_args;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [w.strip().lstrip("*") for w in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [n for n, _ in K.FwCollectHlArgs._fields_]


def test_collect_act_hl_refuses_a_null_handle():
    a = K.FwCollectHlArgs()
    assert _L().fw_collect_act_hl(None, C.byref(a), None) == K.FW_EINVAL
    assert "fw_collect_act_hl" in _L().fw_last_error(None).decode()


def test_a_sharded_job_refuses_the_flag(monkeypatch):
    """Sharded high-level training on the fused paths is not built: PPO says so instead of choosing another path."""
    class _Env:
        device, num_envs, obs_dim, act_dim = torch.device("cpu"), 4, 30, 3
    monkeypatch.setattr(R, "_dist", lambda: object())          # "a process group is up"
    with pytest.raises(ValueError, match="fused_three_actions"):
        R.PPO(_Env(), R.PPOConfig(fused_three_actions=True, use_graphs=False))
