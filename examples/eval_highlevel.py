"""Evaluate a trained high-level commander (examples/train_highlevel_cmd.py) above its frozen low-level controller.

The reference has no evaluation script for this task; the figures are this build's (DESIGN.md section 2e "Evaluation").  Loads the
commander's checkpoint (best_model.pt / final_model.pt, its normaliser statistics from the vecnorm.pt next to it or from the
checkpoint itself) and the controller's checkpoint, evaluates --episodes episodes deterministically on a HighLevelCmdVecEnv with
frozen statistics and prints the waypoint figures (reward, length, reach rates) and the command figures: how far the flight was from
the commanded heading / altitude / airspeed (MAE, RMSE, pooled over every evaluated step), the mean angular-rate norm, the mean
command change per step, the share of steps with the altitude or airspeed command on a bound of the action Box and the number of
actions rejected as non-finite.  --fused runs commander and controller through the fused kernel (fw_collect_act_hl) instead of
the torch forward.  --trace_steps N also flies N vec-steps from a reset and writes the flight record (highlevel.fly, fw_trace_hl).

    python examples/eval_highlevel.py --checkpoint runs/highlevel_ppo/models/final_model.pt \\
        --low_checkpoint runs/lowlevel_ppo/models/final_model.pt [--episodes 16] [--fused] [--trace_steps 600] [--out runs/highlevel_eval]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", type=str, required=True, help="the commander: best_model.pt or final_model.pt of examples/train_highlevel_cmd.py")
    ap.add_argument("--low_checkpoint", type=str, required=True, help="the low-level controller: a checkpoint of examples/train_lowlevel_cmd.py")
    ap.add_argument("--vecnorm_path", type=str, default=None)
    ap.add_argument("--episodes", type=int, default=16)
    ap.add_argument("--num_envs", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fused", action="store_true", help="commander and controller in the fused kernel (fw_collect_act_hl)")
    ap.add_argument("--controller_hz", type=int, default=None,
                    help="the rate the frozen controller runs at: 30 (default, once per agent step) or 120 (once per Aviary step, inside the step kernel)")
    ap.add_argument("--trace_steps", type=int, default=0, help="also record a flight of this many vec-steps (trace.npz)")
    ap.add_argument("--out", type=str, default=None, help="directory for evaluation.json and trace.npz")
    a = ap.parse_args()

    import numpy as np
    import torch
    import pyflyt_drone_amd as P
    from pyflyt_drone_amd import checkpoint, evaluate, highlevel, rollout as R

    sd = torch.load(a.checkpoint, map_location="cpu", weights_only=True)

    def make():
        venv = P.HighLevelCmdVecEnv(a.num_envs, low_checkpoint=a.low_checkpoint, flight_dome_size=200.0, max_duration_seconds=120.0,
                                    agent_hz=30, context_length=2, seed=a.seed, controller_hz=a.controller_hz)
        env = R.VecNormalizeDevice(venv, training=False, norm_reward=False, clip_obs=10.0)
        vecnorm = checkpoint.infer_vecnorm_path(a.checkpoint, a.vecnorm_path)
        if vecnorm:
            checkpoint.load_vecnormalize(vecnorm, env, training=False, norm_reward=False)
        else:                                  # no vecnorm.pt: the statistics saved with the model
            env.load_state_dict(sd["vecnormalize"])
            env.training, env.norm_reward = False, False
        return env

    env = make()
    if sd["obs_dim"] != env.obs_dim:
        raise SystemExit(f"{a.checkpoint}: obs_dim {sd['obs_dim']} is not the high-level command task's {env.obs_dim}")
    policy = R.MlpPolicy(env.obs_dim, env.act_dim).to(env.device)
    policy.load_state_dict(sd["policy"])
    policy.eval()

    r = evaluate.evaluate_policy(policy, env, n_eval_episodes=a.episodes, deterministic=True, use_fused=True if a.fused else None)
    sc = r.scalars(int(env.venv.cfg.num_targets))
    cs = r.command_scalars()
    print(f"{len(r.episode_lengths)} episodes, {sum(r.episode_lengths)} steps: mean reward {r.mean_reward:.2f} +/- {r.std_reward:.2f}, "
          f"mean length {r.mean_ep_length:.1f}")
    for k, v in sc.items():
        if "reach_rate" in k or "success" in k:
            print(f"  {k.split('/', 1)[1]:24s} {v:.3f}")
    print("how the controller followed the commands, and the commands themselves:")
    print(f"  heading  MAE {cs['eval/cmd_heading_mae']:.4f} rad   RMSE {cs['eval/cmd_heading_rmse']:.4f} rad   change per step {cs['eval/cmd_heading_delta']:.4f} rad")
    print(f"  altitude MAE {cs['eval/cmd_altitude_mae']:.4f} m     RMSE {cs['eval/cmd_altitude_rmse']:.4f} m     change per step {cs['eval/cmd_altitude_delta']:.4f} m")
    print(f"  airspeed MAE {cs['eval/cmd_airspeed_mae']:.4f} m/s   RMSE {cs['eval/cmd_airspeed_rmse']:.4f} m/s   change per step {cs['eval/cmd_airspeed_delta']:.4f} m/s")
    print(f"  mean angular-rate norm {cs['eval/ang_vel_mean']:.4f} rad/s   steps on a Box bound {cs['eval/cmd_saturation_rate']:.3f}   "
          f"rejected actions {int(cs['eval/rejected_actions'])}")
    env.venv.close()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "evaluation.json"), "w") as f:
            json.dump({"checkpoint": a.checkpoint, "low_checkpoint": a.low_checkpoint, "episodes": len(r.episode_lengths), "fused": bool(a.fused), "controller_hz": a.controller_hz or 30,
                       "episode_rewards": r.episode_rewards, "episode_lengths": r.episode_lengths,
                       **{k.split("/", 1)[1]: v for k, v in {**sc, **cs}.items()}}, f, indent=1)
    if a.trace_steps > 0:
        env = make()                           # a fresh env from the same seed
        tr = highlevel.fly(policy, env, a.trace_steps, use_fused=True if a.fused else None)
        env.venv.close()
        ended = int((tr.ended_at >= 0).sum())
        print(f"flight record: {a.trace_steps} vec-steps x {a.num_envs} envs, {ended} envs ended their first episode inside it")
        if a.out:
            np.savez(os.path.join(a.out, "trace.npz"), trace=tr.trace, start=tr.start, dt=tr.dt, ended_at=tr.ended_at,
                     columns=np.array(highlevel.HL_TRACE_COLS))


if __name__ == "__main__":
    main()
