"""PPOConfig.target_kl without a device: the option's validation, the new entry point in the binding and the header, the condition
tests/ppo_kl_cases.py puts on its own inputs, the torch path against the float64 restatement of SB3's loop, and the twins that must
not move (the option left at None, or a limit that never triggers)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_kl_cases as KC  # noqa: E402

from pyflyt_drone_amd import _lib  # noqa: E402
from pyflyt_drone_amd import config as K  # noqa: E402
from pyflyt_drone_amd import rollout as R  # noqa: E402

SHAPE_IDS = [f"{d}-{a}-{bs}" for d, a, bs in KC.SHAPES]


@pytest.fixture(scope="module")
def no_stop():
    """Per shape, computed once and left alone: the no-stop KL series of the float64 restatement and of the float32 torch step."""
    torch.set_num_threads(min(torch.get_num_threads(), 4))
    out = {}
    for d, a, bs in KC.SHAPES:
        ppo = KC.make_ppo(d, a, bs, diagnostics=True, fused_update=False)
        r64 = KC.Restated(ppo).train(KC.permutation(ppo), bs)
        ppo.train()
        out[(d, a, bs)] = (r64["kl"], ppo.diagnostic_series["approx_kl"].copy())
    return out


@pytest.mark.parametrize("bad", [0, 0.0, -0.01, float("nan"), float("inf"), "0.01", True, [0.01]])
def test_config_refuses_what_is_no_positive_number(bad):
    with pytest.raises(ValueError, match="target_kl"):
        R.PPOConfig(target_kl=bad)


def test_config_accepts_none_and_positive_numbers_and_refuses_the_all_reduce_path():
    assert R.PPOConfig().target_kl is None and R.PPOConfig().kl_stop is None
    assert R.PPOConfig(target_kl=0.01).kl_stop == float(np.float32(1.5 * 0.01))
    assert R.PPOConfig(target_kl=1).kl_stop == 1.5 and R.PPOConfig(target_kl=np.float32(0.5)).kl_stop == 0.75
    with pytest.raises(ValueError, match="not built"):
        R.PPOConfig(target_kl=0.01, dist_update="allreduce")
    R.PPOConfig(dist_update="allreduce")                       # (without the option: as before)


def test_the_entry_point_is_exported_declared_and_refuses_bad_arguments_and_the_abi_stays_7():
    assert "fw_ppo_update_kl" in _lib.EXPORTS
    L = _lib.lib()                              # (loads without a device; a missing or stale library is a failure, not a skip)
    assert hasattr(L, "fw_ppo_update_kl") and L.fw_abi_version() == K.FW_ABI_VERSION == 7
    header = open(os.path.join(_lib.INCLUDE, "fwsim.h")).read()
    decl = re.search(r"int32_t fw_ppo_update_kl\((.*?)\);", header, re.S)
    assert decl and "float target_kl" in decl.group(1) and "int32_t* minibatches_stepped" in decl.group(1)
    assert re.search(r"#define\s+FW_ABI_VERSION\s+7\b", header)
    assert C.sizeof(R._PpoHyper) == 48                         # fw_ppo_hyper keeps its size: the limit travels beside it
    one = C.c_void_p(16)                                       # (never dereferenced: the argument checks come first)
    tail = (one, one, one, 1 << 40, None)

    def call(act_dim=4, target_kl=0.01, stepped=one, diag=None, diag_floats=0, n_mb=8):
        return L.fw_ppo_update_kl(*([one] * 9), n_mb, 64, 21, act_dim, *tail, diag, diag_floats, target_kl, stepped)
    for t in (0.0, -1.0, float("nan"), float("inf")):
        assert call(target_kl=t) == K.FW_EINVAL and "target_kl must be positive and finite" in L.fw_last_error(None).decode()
    assert call(stepped=None) == K.FW_EINVAL and "minibatches_stepped is NULL" in L.fw_last_error(None).decode()
    for a in (0, 1, 2, 5, 7, -4):
        assert call(act_dim=a) == K.FW_EINVAL and "act_dim must be 3, 4 or 6" in L.fw_last_error(None).decode()
    assert call(diag=one, diag_floats=8 * 256 - 1) == K.FW_EINVAL and "diag smaller" in L.fw_last_error(None).decode()
    assert call(n_mb=0) == K.FW_EINVAL


@pytest.mark.parametrize("case", list(KC.CASES))
@pytest.mark.parametrize("shape", KC.SHAPES, ids=SHAPE_IDS)
def test_the_condition_on_the_inputs(shape, case, no_stop):
    """Every KL up to and including the stop sits at least 5 % of the limit away from it, in float64 and in float32, and both series put
    the stop where the case wants it.  (A guard on the inputs of the other tests, not a test of the feature: it uses no ``target_kl``
    and so holds on a tree without the option as well.)"""
    j = KC.CASES[case]
    k64, k32 = no_stop[shape]
    assert k64.shape == k32.shape == (KC.N_MB,)
    t = KC.pick_target_kl(k64, j)
    for name, series in (("float64 restatement", k64), ("float32 torch step", k32)):
        m, where = KC.margins(series, j, t)
        print(f"\n[kl cases] {shape} {case} {name}: target_kl {t:.6g}, smallest margin {m.min():.3f}")
        assert where, (name, series, t)
        assert m.min() >= KC.MARGIN, (name, m)


@pytest.mark.parametrize("diagnostics", [False, True], ids=["plain", "diagnostics"])
@pytest.mark.parametrize("case", list(KC.CASES))
@pytest.mark.parametrize("shape", KC.SHAPES, ids=SHAPE_IDS)
def test_torch_path_against_the_restatement(shape, case, diagnostics, no_stop):
    d, a, bs = shape
    j = KC.CASES[case]
    t = KC.pick_target_kl(no_stop[shape][0], j)
    ppo = KC.make_ppo(d, a, bs, target_kl=t, diagnostics=diagnostics, fused_update=False)
    ref = KC.Restated(ppo)
    want = ref.train(KC.permutation(ppo), bs, target_kl=t)
    assert want["stepped"] == (KC.N_MB if j is None else j) and want["stopped"] == (j is not None)
    ppo.train()
    computed = len(want["kl"])
    assert ppo.logs["minibatches_stepped"] == want["stepped"] and ppo.logs["epochs_run"] == want["epochs_run"]
    assert ppo.logs["kl_stopped"] is want["stopped"] and ppo._n_updates == want["epochs_run"]
    KC.compare_with_restated(ppo, ref)                          # parameters, moments and the optimiser's step count
    # the logged losses: means over the minibatches whose loss was computed, the stopping one included
    for i, k in enumerate(("policy_loss", "value_loss", "entropy_loss")):
        assert ppo.logs[k] == pytest.approx(want["losses"][:, i].mean(), rel=2e-3, abs=1e-5), k
    if j is None:
        assert ppo.stop_kl is None and ppo.early_stop_message() is None
    else:
        assert ppo.stop_kl == pytest.approx(want["kl"][-1], rel=2e-3) and ppo.stop_kl > ppo.cfg.kl_stop
        assert ppo.early_stop_message() == f"Early stopping at step {want['epochs_run'] - 1} due to reaching max kl: {ppo.stop_kl:.2f}"
    if diagnostics:                                             # the series hold the minibatches that ran, the device-side row counter kept up
        s = ppo.diagnostic_series
        assert all(v.shape == (computed,) for v in s.values()) and int(ppo._diag_i.item()) == computed
        np.testing.assert_allclose(s["approx_kl"], want["kl"], rtol=2e-3, atol=1e-6)
        assert ppo.diagnostics["train/approx_kl"] == pytest.approx(want["kl"].mean(), rel=2e-3)
        assert ppo.diagnostics["train/n_updates"] == want["epochs_run"]
    else:
        assert ppo.diagnostics == {}
    ppo.train()                                                 # a second update goes on from the counts of the first
    assert ppo._n_updates == want["epochs_run"] + ppo.logs["epochs_run"]
    step = {float(st["step"]) for st in ppo.optimizer.state.values()}
    assert step == {float(want["stepped"] + ppo.logs["minibatches_stepped"])}      # (every case steps at least three times)


def _state(ppo):
    par = [p.detach().clone() for p in ppo.policy.parameters()]
    mom = [(float(st["step"]), st["exp_avg"].clone(), st["exp_avg_sq"].clone()) for st in (ppo.optimizer.state[p] for p in ppo.policy.parameters())]
    return par, mom, ppo.perm_gen.get_state().clone()


@pytest.mark.parametrize("diagnostics", [False, True], ids=["plain", "diagnostics"])
@pytest.mark.parametrize("shape", KC.SHAPES, ids=SHAPE_IDS)
def test_none_and_a_limit_that_never_triggers_move_nothing(shape, diagnostics, no_stop):
    """Three learners on the same inputs -- a config without the field, one with ``target_kl=None``, one with a limit above every KL --
    end two updates bit-identical: parameters, moments, step counts, the five old keys of ``logs``, the series, the generator."""
    d, a, bs = shape
    t = KC.pick_target_kl(no_stop[shape][0], None)
    kw = dict(diagnostics=diagnostics, fused_update=False)
    plain, none, never = KC.make_ppo(d, a, bs, **kw), KC.make_ppo(d, a, bs, target_kl=None, **kw), KC.make_ppo(d, a, bs, target_kl=t, **kw)
    for call in range(2):
        for p in (plain, none, never):
            p.train()
        sp = _state(plain)
        for other in (none, never):
            so = _state(other)
            assert all(torch.equal(x, y) for x, y in zip(sp[0], so[0]))
            assert all(s0 == s1 and torch.equal(m0, m1) and torch.equal(v0, v1) for (s0, m0, v0), (s1, m1, v1) in zip(sp[1], so[1]))
            assert torch.equal(sp[2], so[2])
            assert {k: other.logs[k] for k in plain.logs} == plain.logs and other._n_updates == plain._n_updates == (call + 1) * KC.N_EPOCHS
            assert other.diagnostics == plain.diagnostics
            assert all(np.array_equal(other.diagnostic_series[k], v) for k, v in plain.diagnostic_series.items())
        assert list(plain.logs) == list(none.logs) == ["policy_loss", "value_loss", "entropy_loss", "adv_mean", "adv_std"]
        assert (never.logs["minibatches_stepped"], never.logs["epochs_run"], never.logs["kl_stopped"]) == (KC.N_MB, KC.N_EPOCHS, False)


def test_the_generator_ends_a_stopped_update_where_a_full_one_ends(no_stop):
    """The permutations of the epochs a stop leaves out are still drawn (the fused path draws all of them up front): the next update
    of both paths walks the same minibatches."""
    d, a, bs = KC.SHAPES[1]
    stop = KC.make_ppo(d, a, bs, target_kl=KC.pick_target_kl(no_stop[(d, a, bs)][0], 3), fused_update=False)
    full = KC.make_ppo(d, a, bs, fused_update=False)
    stop.train(); full.train()
    assert stop.logs["kl_stopped"] and torch.equal(stop.perm_gen.get_state(), full.perm_gen.get_state())
