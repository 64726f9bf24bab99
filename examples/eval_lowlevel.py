"""Device-resident counterpart of the reference's eval/eval_lowlevel.py: how well a trained low-level controller tracks its target.

Loads a checkpoint of examples/train_lowlevel_cmd.py (best_model.pt / final_model.pt, with vecnorm.pt found next to it or given by
--vecnorm_path), evaluates --num_episodes episodes deterministically on a FixedwingLowLevelVecEnv with frozen normaliser statistics
and prints, per episode, its steps and its heading / altitude / airspeed MAE, then the summary: MAE and RMSE of each error pooled
over every evaluated step, the mean angular-rate norm and the survival rate (definitions in DESIGN.md section 2d).  --fused runs
the policy through the fused six-action kernel (fw_collect_act_a) instead of torch.

    python examples/eval_lowlevel.py --model runs/lowlevel_ppo/models/final_model.pt [--num_episodes 20] [--fused] [--json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import checkpoint, evaluate, rollout as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", type=str, required=True, help="best_model.pt or final_model.pt of examples/train_lowlevel_cmd.py")
    ap.add_argument("--vecnorm_path", type=str, default=None)
    ap.add_argument("--num_episodes", type=int, default=20)
    ap.add_argument("--num_envs", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fused", action="store_true", help="the policy forward in the fused six-action kernel (fw_collect_act_a)")
    ap.add_argument("--json", action="store_true", help="also print the summary as one JSON line")
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

    r = evaluate.evaluate_policy(policy, env, n_eval_episodes=a.num_episodes, deterministic=True, use_fused=True if a.fused else None)
    for k, L in enumerate(r.episode_lengths):
        print(f"episode {k + 1:3d}: {L:5d} steps, heading MAE {r.heading_abs[k] / L:.4f} rad, altitude MAE {r.altitude_abs[k] / L:.4f} m, "
              f"airspeed MAE {r.airspeed_abs[k] / L:.4f} m/s{'' if r.survived[k] else ', terminated'}")
    sc = r.tracking_scalars()
    print(f"\nsummary over {len(r.episode_lengths)} episodes, {sum(r.episode_lengths)} steps:")
    print(f"  heading  MAE {sc['eval/heading_mae']:.4f} rad   RMSE {sc['eval/heading_rmse']:.4f} rad")
    print(f"  altitude MAE {sc['eval/altitude_mae']:.4f} m     RMSE {sc['eval/altitude_rmse']:.4f} m")
    print(f"  airspeed MAE {sc['eval/airspeed_mae']:.4f} m/s   RMSE {sc['eval/airspeed_rmse']:.4f} m/s")
    print(f"  mean angular-rate norm {sc['eval/ang_vel_mean']:.4f} rad/s")
    print(f"  survival rate {sc['eval/survival_rate']:.3f}   mean reward {r.mean_reward:.2f}   mean length {r.mean_ep_length:.1f}")
    if a.json:
        print(json.dumps({"model": a.model, "episodes": len(r.episode_lengths), "fused": a.fused,
                          **{k.split("/", 1)[1]: v for k, v in sc.items()}, "mean_reward": r.mean_reward,
                          "mean_ep_length": r.mean_ep_length}))
    env.venv.close()


if __name__ == "__main__":
    main()
