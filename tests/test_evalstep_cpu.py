"""evalstep.select on fake envs (no device): which kind of vec-step a policy, an env and the caller's ``use_fused`` get.  The
expectations are written out from the rules ("One step object, one replay driver"), not computed."""
from types import SimpleNamespace

import pytest
import torch

from pyflyt_drone_amd import _lib, evalstep
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R

EVAL = dict(accept=("collect_step", "act_a", "act_hl"), default="collect_step")      # evaluate.ReplayedEvaluation
FLIGHT, COMMAND, HIGHLEVEL = dict(accept=("collect_step",)), dict(accept=("act_a",)), dict(accept=("act_hl",))      # the three fly functions
REFUSED = "refused"


def _fake_env(task, lanes=8, training=False, norm_obs=True, obs_dim=None, device="cuda", handle=True):
    """built like tests/test_flight_cpu.py's _fake_env; the "handle" of a device env is its lane count (the fake library returns it)"""
    cfg = {"waypoints": K.train_waypoints_v3_config, "lowlevel": K.lowlevel_config, "highlevel": K.highlevel_config}[task]()
    D = K.obs_dim(cfg) if obs_dim is None else obs_dim
    venv = SimpleNamespace(cfg=cfg, terminal_obs=None, obs=torch.zeros((2, D)))
    if task == "highlevel":                 # HighLevelCmdVecEnv: the handle is its base env's
        venv.command = venv.rejected = None
        venv.step_low = venv.collect_act_hl = venv.step_tensor = lambda *a: None
    elif handle:
        venv._h, venv.step_tensor = lanes, lambda *a: None
    return SimpleNamespace(venv=venv, training=training, num_envs=2, device=device, norm_obs=norm_obs, obs_dim=D)


# (env, policy width, use_fused, caller) -> the kind, or REFUSED (ValueError)
TABLE = [
    # the four-action policy on the waypoints task: fw_collect_step on the 8-lane mapping (16: the same mapping, two waves per SIMD)
    (dict(task="waypoints", lanes=8), 4, None, EVAL, "collect_step"),
    (dict(task="waypoints", lanes=16), 4, None, EVAL, "collect_step"),
    (dict(task="waypoints", lanes=8), 4, True, EVAL, "collect_step"),
    (dict(task="waypoints", lanes=8), 4, False, EVAL, "torch"),
    (dict(task="waypoints", lanes=1), 4, None, EVAL, "torch"),
    (dict(task="waypoints", lanes=1), 4, True, EVAL, REFUSED),
    (dict(task="waypoints", lanes=8, training=True), 4, None, EVAL, "torch"),
    (dict(task="waypoints", lanes=8, training=True), 4, True, EVAL, REFUSED),
    (dict(task="waypoints", lanes=8, norm_obs=False), 4, None, EVAL, "torch"),
    (dict(task="waypoints", lanes=8, norm_obs=False), 4, True, EVAL, REFUSED),
    (dict(task="waypoints", lanes=8, obs_dim=62), 4, None, EVAL, "collect_step"),
    (dict(task="waypoints", lanes=8, obs_dim=63), 4, None, EVAL, "torch"),          # the act waves take up to 62 features
    (dict(task="waypoints", lanes=8, obs_dim=63), 4, True, EVAL, REFUSED),
    (dict(task="waypoints", lanes=8, device="cpu"), 4, None, EVAL, "torch"),
    (dict(task="waypoints", lanes=8, device="cpu"), 4, True, EVAL, REFUSED),
    (dict(task="waypoints", lanes=8, handle=False), 4, None, EVAL, "torch"),
    (dict(task="waypoints", lanes=8, handle=False), 4, True, EVAL, REFUSED),
    (dict(task="waypoints", lanes=8), 6, True, EVAL, REFUSED),                      # six actions: the low-level task only
    # ... and in flight.fly: torch unless asked
    (dict(task="waypoints", lanes=8), 4, None, FLIGHT, "torch"),
    (dict(task="waypoints", lanes=8), 4, False, FLIGHT, "torch"),
    (dict(task="waypoints", lanes=8), 4, True, FLIGHT, "collect_step"),
    (dict(task="waypoints", lanes=1), 4, True, FLIGHT, REFUSED),
    (dict(task="waypoints", lanes=8, obs_dim=63), 4, True, FLIGHT, REFUSED),
    (dict(task="waypoints", lanes=8, training=True), 4, True, FLIGHT, REFUSED),
    (dict(task="waypoints", lanes=8, handle=False), 4, True, FLIGHT, REFUSED),
    (dict(task="waypoints", lanes=8), 4, True, COMMAND, REFUSED),
    (dict(task="waypoints", lanes=8), 4, True, HIGHLEVEL, REFUSED),
    # the six-action policy on the low-level task: fw_collect_act_a on either lane mapping, only on request
    (dict(task="lowlevel", lanes=8), 6, None, EVAL, "torch"),
    (dict(task="lowlevel", lanes=1), 6, None, EVAL, "torch"),
    (dict(task="lowlevel", lanes=8), 6, True, EVAL, "act_a"),
    (dict(task="lowlevel", lanes=1), 6, True, EVAL, "act_a"),
    (dict(task="lowlevel", lanes=8), 6, False, EVAL, "torch"),
    (dict(task="lowlevel", lanes=8, training=True), 6, True, EVAL, REFUSED),
    (dict(task="lowlevel", lanes=8, norm_obs=False), 6, True, EVAL, REFUSED),
    (dict(task="lowlevel", lanes=8, device="cpu"), 6, True, EVAL, REFUSED),
    (dict(task="lowlevel", lanes=8), 4, True, EVAL, "collect_step"),                # (the rules look at the policy's width, not the task's)
    (dict(task="lowlevel", lanes=1), 4, True, EVAL, REFUSED),
    (dict(task="lowlevel", lanes=1), 6, None, COMMAND, "torch"),
    (dict(task="lowlevel", lanes=1), 6, True, COMMAND, "act_a"),
    (dict(task="lowlevel", lanes=8), 6, True, COMMAND, "act_a"),
    (dict(task="lowlevel", lanes=8), 4, True, COMMAND, REFUSED),
    (dict(task="lowlevel", lanes=8, training=True), 6, True, COMMAND, REFUSED),
    (dict(task="lowlevel", lanes=8), 6, True, FLIGHT, REFUSED),
    # the three-action policy on the high-level command task's 30-value observation: fw_collect_act_hl, only on request
    (dict(task="highlevel"), 3, None, EVAL, "torch"),
    (dict(task="highlevel"), 3, True, EVAL, "act_hl"),
    (dict(task="highlevel"), 3, False, EVAL, "torch"),
    (dict(task="highlevel", training=True), 3, True, EVAL, REFUSED),
    (dict(task="highlevel", norm_obs=False), 3, True, EVAL, REFUSED),
    (dict(task="highlevel", device="cpu"), 3, True, EVAL, REFUSED),
    (dict(task="highlevel", obs_dim=36), 3, True, EVAL, REFUSED),
    (dict(task="highlevel"), 6, True, EVAL, REFUSED),
    (dict(task="highlevel"), 3, None, HIGHLEVEL, "torch"),
    (dict(task="highlevel"), 3, True, HIGHLEVEL, "act_hl"),
    (dict(task="highlevel", obs_dim=36), 3, True, HIGHLEVEL, REFUSED),
    (dict(task="highlevel"), 3, True, COMMAND, REFUSED),
    (dict(task="highlevel"), 3, True, FLIGHT, REFUSED),
]


@pytest.fixture
def fake_library(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: SimpleNamespace(fw_lanes_per_env=lambda h: h))


def test_select_follows_the_rules_of_each_kind(fake_library):
    assert evalstep.KINDS == ("collect_step", "act_a", "act_hl", "torch")
    policies = {}
    for env_kw, width, use_fused, caller, want in TABLE:
        env = _fake_env(**env_kw)
        pol = policies.setdefault((env.obs_dim, width), R.MlpPolicy(env.obs_dim, width))
        case = f"{env_kw} width {width} use_fused {use_fused} accept {caller['accept']}"
        if want == REFUSED:
            with pytest.raises(ValueError, match="use_fused=True"):
                evalstep.select(pol, env, use_fused, refusal="use_fused=True needs what this env or policy is not", **caller)
        else:
            assert evalstep.select(pol, env, use_fused, refusal="use_fused=True", **caller) == want, case


def test_select_takes_only_the_mlp_policy(fake_library):
    """a module without the two 64-64 nets, and a policy with a CNN front end, keep the torch forward"""
    env = _fake_env("waypoints")
    other = torch.nn.Linear(env.obs_dim, 4)
    cnn = R.MlpPolicy(env.obs_dim, 4)
    cnn.uses_image = True
    for pol in (other, cnn):
        assert evalstep.select(pol, env, None, refusal="use_fused=True", **EVAL) == "torch"
        with pytest.raises(ValueError, match="use_fused=True"):
            evalstep.select(pol, env, True, refusal="use_fused=True", **EVAL)
