"""Command a trained low-level controller: fly a schedule of heading / altitude / airspeed steps and report how it follows them.

Loads a checkpoint of examples/train_lowlevel_cmd.py (best_model.pt / final_model.pt, with vecnorm.pt found next to it or given by
--vecnorm_path) exactly as examples/eval_lowlevel.py does, flies the default schedule -- heading steps of +-90 degrees, altitude
10 -> 18 m, airspeed 14 -> 18 m/s, 2000 steps -- on --num_envs envs through command.fly (fw_command_ll -> act -> fw_step ->
fw_trace_ll, replayed as hipGraphs) and prints the step-response summary of command.response_figures (DESIGN.md section 2d,
"Commanding the controller").  --fused runs the policy through the fused six-action kernel (fw_collect_act_a) instead of torch;
--save_trace writes the trace and the schedule to an .npz for plotting.

    python examples/command_lowlevel.py --model runs/lowlevel_ppo/models/final_model.pt [--fused] [--json] [--save_trace out.npz]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import checkpoint, command, rollout as R  # noqa: E402

# (steps, (psi [rad], h [m], V [m/s])): 2000 steps = 16.7 s at the task's 120 Hz
DEFAULT_SCHEDULE = [
    (200, (0.0, 10.0, 14.0)),
    (300, (math.pi / 2, 10.0, 14.0)),
    (300, (0.0, 10.0, 14.0)),
    (300, (-math.pi / 2, 10.0, 14.0)),
    (300, (0.0, 18.0, 14.0)),
    (300, (0.0, 18.0, 18.0)),
    (300, (0.0, 10.0, 14.0)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", type=str, required=True, help="best_model.pt or final_model.pt of examples/train_lowlevel_cmd.py")
    ap.add_argument("--vecnorm_path", type=str, default=None)
    ap.add_argument("--num_envs", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fused", action="store_true", help="the policy forward in the fused six-action kernel (fw_collect_act_a)")
    ap.add_argument("--json", action="store_true", help="also print the summary as one JSON line")
    ap.add_argument("--save_trace", type=str, default=None, help="write trace, start rows, schedule, dt and ended_at to this .npz")
    a = ap.parse_args()

    sd = torch.load(a.model, map_location="cpu", weights_only=True)
    env = R.VecNormalizeDevice(P.FixedwingLowLevelVecEnv(num_envs=a.num_envs, seed=a.seed), training=False, norm_reward=False, clip_obs=10.0)
    if sd["obs_dim"] != env.obs_dim:
        raise SystemExit(f"{a.model}: obs_dim {sd['obs_dim']} is not the low-level task's {env.obs_dim}")
    vecnorm = checkpoint.infer_vecnorm_path(a.model, a.vecnorm_path)
    if vecnorm:
        checkpoint.load_vecnormalize(vecnorm, env, training=False, norm_reward=False)
    else:                                  # no vecnorm.pt: the statistics saved with the model
        env.load_state_dict(sd["vecnormalize"])
        env.training, env.norm_reward = False, False
    policy = R.MlpPolicy(env.obs_dim, env.act_dim).to(env.device)
    policy.load_state_dict(sd["policy"])
    policy.eval()

    schedule = command.step_schedule(DEFAULT_SCHEDULE, a.num_envs, env.device)
    ct = command.fly(policy, env, schedule, use_fused=True if a.fused else None)
    fig = command.response_figures(ct)
    sc = fig["summary"]
    T = ct.trace.shape[0]
    print(f"{a.num_envs} envs x {T} steps ({T * ct.dt:.2f} s), {'fused' if a.fused else 'torch'} policy forward")
    units = {"heading": "rad", "altitude": "m", "airspeed": "m/s"}
    for ax in command.AXES:
        u = units[ax]
        print(f"  {ax:8s} {sc[f'{ax}_steps']:3d} steps, {sc[f'{ax}_reached']:.2f} reached 90 %; median t90 {sc[f'{ax}_t90']:.3f} s, "
              f"overshoot {sc[f'{ax}_overshoot']:.3f}, settling {sc[f'{ax}_settling']:.3f} s, steady-state error {sc[f'{ax}_ss_error']:.4f} {u}; "
              f"MAE {sc[f'{ax}_mae']:.4f} {u}, RMSE {sc[f'{ax}_rmse']:.4f} {u}")
    print(f"  survival rate {sc['survival_rate']:.3f}; envs that ended early: {int((ct.ended_at >= 0).sum())}")
    if a.save_trace:
        np.savez(a.save_trace, trace=ct.trace, start=ct.start, schedule=ct.schedule, dt=ct.dt, ended_at=ct.ended_at,
                 columns=np.array(command.TRACE_COLS))
        print(f"trace written to {a.save_trace}")
    if a.json:
        print(json.dumps({"model": a.model, "fused": a.fused, "envs": a.num_envs, "steps": T, **sc}))
    env.venv.close()


if __name__ == "__main__":
    main()
