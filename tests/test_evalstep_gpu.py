"""evalstep.replay_flight through the three recorders (flight.fly, command.fly, highlevel.fly), on the torch forward and on each
fused act: every split of T steps into graph replays and eager steps records the same flight, bit for bit."""
import numpy as np
import pytest
import torch

import pyflyt_drone_amd as P
from pyflyt_drone_amd import command, flight, highlevel
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import rollout as R

pytestmark = pytest.mark.gpu

N, T = 8, 11
# all eager; two replays and three eager steps; exactly one replay; a graph longer than the flight (all eager again)
GRAPH_STEPS = (0, 4, 11, 16)


def _frozen(venv):
    env = R.VecNormalizeDevice(venv, training=False, norm_reward=False)
    with torch.no_grad():                                      # statistics as after some training: not the identity
        env.obs_rms.mean.copy_(torch.linspace(-0.2, 0.3, env.obs_dim, dtype=torch.float64, device="cuda"))
        env.obs_rms.var.copy_(torch.linspace(0.5, 2.0, env.obs_dim, dtype=torch.float64, device="cuda"))
    return env


def _policy(obs_dim, act_dim, bias=None):
    torch.manual_seed(0)
    pol = R.MlpPolicy(obs_dim, act_dim).cuda()
    with torch.no_grad():
        pol.action_net.weight.mul_(30.0)
        if bias is not None:
            pol.action_net.bias.copy_(torch.tensor(bias))
    return pol


def _fly_waypoints(fused, gs):
    env = _frozen(P.FixedwingVecEnv(K.train_waypoints_v3_config(), N, seed=9))
    return env, flight.fly(_policy(env.obs_dim, 4), env, T, use_fused=fused, graph_steps=gs)


def _fly_lowlevel(fused, gs):
    env = _frozen(P.FixedwingVecEnv(K.lowlevel_config(max_episode_steps=300, motor_noise=True), N, seed=6))
    sched = command.step_schedule([(5, (0.0, 10.0, 15.0)), (6, (1.2, 14.0, 17.0))], N)
    return env, command.fly(_policy(env.obs_dim, 6), env, sched, use_fused=fused, graph_steps=gs)


def _fly_highlevel(fused, gs):
    torch.manual_seed(21)
    ctl = R.MlpPolicy(21, 6)
    with torch.no_grad():
        ctl.action_net.weight.mul_(1.5)
    g = np.random.default_rng(21)
    env = _frozen(highlevel.HighLevelCmdVecEnv(N, ctl, (g.normal(0.0, 1.0, 21), g.uniform(0.5, 4.0, 21)), max_duration_seconds=4.0, seed=9))
    return env, highlevel.fly(_policy(30, 3, bias=(0.0, 100.0, 15.0)), env, T, use_fused=fused, graph_steps=gs)


@pytest.mark.parametrize("fused", [None, True], ids=["torch", "fused"])
@pytest.mark.parametrize("fly", [_fly_waypoints, _fly_lowlevel, _fly_highlevel], ids=["flight", "command", "highlevel"])
def test_every_split_into_replays_and_eager_steps_records_the_same_flight(fly, fused, monkeypatch):
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", "8")             # (fw_collect_step's mapping; the other two acts take either)
    out = []
    for gs in GRAPH_STEPS:
        env, tr = fly(fused, gs)
        env.venv.close()
        out.append(tr)
    a = out[0]
    assert a.trace.shape[:2] == (T, N) and a.start.shape[0] == N and a.ended_at.shape == (N,)
    assert np.isfinite(a.trace).all() and not np.array_equal(a.trace[0], a.trace[T - 1]), "a flight that moves"
    for gs, b in zip(GRAPH_STEPS[1:], out[1:]):
        np.testing.assert_array_equal(b.trace, a.trace, err_msg=f"graph_steps={gs}")
        np.testing.assert_array_equal(b.start, a.start, err_msg=f"graph_steps={gs}")
        np.testing.assert_array_equal(b.ended_at, a.ended_at, err_msg=f"graph_steps={gs}")


@pytest.mark.parametrize("fused", [False, True], ids=["torch", "fused"])
def test_a_finished_evaluation_is_freed_by_reference_counting(fused, monkeypatch):
    """no reference cycle through the job or its step: the graph and the buffers go when the last reference goes, not whenever the
    cycle collector runs (which may be inside another capture)"""
    import gc
    import weakref
    from pyflyt_drone_amd import evaluate
    monkeypatch.setenv("FWSIM_LANES_PER_ENV", "8")
    env = _frozen(P.FixedwingVecEnv(K.train_waypoints_v3_config(flight_dome_size=30.0, max_duration_seconds=1.0), N, seed=9))
    job = evaluate.ReplayedEvaluation(_policy(env.obs_dim, 4), env, np.ones(N, dtype=np.int64), use_fused=fused)
    assert job.step.kind == ("collect_step" if fused else "torch")
    job.run(16)
    refs = [weakref.ref(job), weakref.ref(job.step), weakref.ref(job.graph)]
    gc.disable()
    try:
        del job
        assert [r() for r in refs] == [None, None, None]
    finally:
        gc.enable()
    env.venv.close()
