"""The low-level controller trained with TD3: the second off-policy learner beside examples/train_lowlevel_sac.py, on the same envs,
the same replay ring and the same evaluation.

SB3's ``TD3("MlpPolicy")`` defaults (lr 1e-3, buffer 1 000 000, batch 256, gamma 0.99, tau 0.005, policy_delay 2, target policy noise
0.2 clipped to 0.5, learning_starts 100) with the two departures ``TD3Config`` documents: net_arch (256, 256) instead of (400, 300), and
Gaussian exploration noise of sigma 0.1 on the action instead of none.  As in the SAC example there is one gradient step per env step
and 100 000 steps.  A vec-step -- act, env step, store, ``gradient_steps`` x (sample, update) -- is one captured graph per residue of
the gradient-step count modulo ``policy_delay`` (pyflyt_drone_amd/td3.py); ``--no-fused_update`` runs the gradient steps in torch on the
same act / store / sample / noise kernels.

``--env tracking`` (the default) trains on the low-level env of train/train_lowlevel_cmd.py (``FixedwingLowLevelVecEnv``);
``--env demo`` trains and evaluates on the env the reference's examples/lowlevel.py defines (``FixedwingLowLevelDemoVecEnv``).  In
``demo`` mode every evaluation line also carries the heading MAE and RMSE in degrees.

    python examples/train_lowlevel_td3.py --out runs/lowlevel_td3
    python examples/train_lowlevel_td3.py --env demo --out runs/lowlevel_td3_demo

``--n_steps k`` (1 ... 16) trains on k-step returns gathered from the ring; ``--her_goals n`` relabels goals in hindsight
(``--her_horizon``, 1 ... 64); not both.  Prioritized replay and running normalisation are not built for TD3.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import evaluate, rollout as R, td3 as T  # noqa: E402

TRAIN_CONFIG = dict(total_timesteps=100_000, learning_rate=1e-3, buffer_size=1_000_000, batch_size=256, gamma=0.99, tau=0.005,
                    policy_delay=2, target_policy_noise=0.2, target_noise_clip=0.5, action_noise_sigma=0.1, learning_starts=100,
                    net_arch=(256, 256), seed=0, n_eval_episodes=16, eval_freq=10_000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", choices=("tracking", "demo"), default="tracking",
                    help="tracking: the env of train/train_lowlevel_cmd.py; demo: the env examples/lowlevel.py defines")
    ap.add_argument("--total_timesteps", type=int, default=TRAIN_CONFIG["total_timesteps"])
    ap.add_argument("--num_envs", type=int, default=16)
    ap.add_argument("--gradient_steps", type=int, default=-1, help="per vec-step; -1: one per env (update-to-data 1)")
    ap.add_argument("--batch_size", type=int, default=TRAIN_CONFIG["batch_size"], help="rows per gradient step: a multiple of 16 up to 512")
    ap.add_argument("--policy_delay", type=int, default=TRAIN_CONFIG["policy_delay"], help="the actor and the targets step on every n-th gradient step (1 ... 8)")
    ap.add_argument("--action_noise_sigma", type=float, default=TRAIN_CONFIG["action_noise_sigma"], help="exploration noise on the tanh action")
    ap.add_argument("--n_steps", type=int, default=1, help="n-step returns (1 ... 16), cut at episode ends; 1: the 1-step target")
    ap.add_argument("--her_goals", type=int, default=0,
                    help="hindsight goal relabelling, SB3's n_sampled_goal: a sampled row is relabelled with probability n / (n + 1); 0: off")
    ap.add_argument("--her_horizon", type=int, default=64,
                    help="the relabelled goal is one the episode achieved at most this many steps ahead, minus one (1 ... 64)")
    ap.add_argument("--fused_update", action=argparse.BooleanOptionalAction, default=True, help="fw_td3_update (default) or the torch gradient step")
    ap.add_argument("--use_graphs", action=argparse.BooleanOptionalAction, default=True)
    ap.add_argument("--eval_freq", type=int, default=TRAIN_CONFIG["eval_freq"], help="env steps between evaluations")
    ap.add_argument("--eval_max_steps", type=int, default=1800, help="time limit of an evaluation episode (agent steps; --env tracking only)")
    ap.add_argument("--episode_stats", action="store_true", help="SB3's rollout/* figures in every evaluation line")
    ap.add_argument("--episode_fold", choices=("one", "wide", "auto"), default="one")
    ap.add_argument("--out", type=str, default="runs/lowlevel_td3")
    a = ap.parse_args()
    c = TRAIN_CONFIG
    os.makedirs(a.out, exist_ok=True)
    from pyflyt_drone_amd import config as K
    demo = a.env == "demo"
    if demo:
        env = P.FixedwingLowLevelDemoVecEnv(num_envs=a.num_envs, seed=c["seed"])
        eval_cfg = K.lowlevel_demo_config()
    else:
        env = P.FixedwingLowLevelVecEnv(num_envs=a.num_envs, seed=c["seed"])
        eval_cfg = K.lowlevel_config(max_episode_steps=a.eval_max_steps)
    model = T.TD3(env, T.TD3Config(learning_rate=c["learning_rate"], buffer_size=c["buffer_size"], batch_size=a.batch_size, gamma=c["gamma"],
                                   tau=c["tau"], policy_delay=a.policy_delay, target_policy_noise=c["target_policy_noise"],
                                   target_noise_clip=c["target_noise_clip"], action_noise_sigma=a.action_noise_sigma,
                                   learning_starts=c["learning_starts"], gradient_steps=a.gradient_steps, net_arch=c["net_arch"], seed=c["seed"],
                                   use_graphs=a.use_graphs, fused_update=a.fused_update, episode_stats=a.episode_stats,
                                   episode_fold=a.episode_fold, n_steps=a.n_steps, her_goals=a.her_goals, her_horizon=a.her_horizon))
    eval_env = R.VecNormalizeDevice(P.FixedwingVecEnv(eval_cfg, 16, seed=c["seed"], global_env_offset=a.num_envs), training=False,
                                    norm_obs=False, norm_reward=False)          # (a pass-through wrapper: TD3 does not normalise)
    t0 = time.perf_counter()
    state = {"next_eval": a.eval_freq, "train_s": 0.0, "mark": t0}

    def evaluate_now(td3):
        torch.cuda.synchronize()
        state["train_s"] += time.perf_counter() - state["mark"]
        r = evaluate.evaluate_policy(td3.policy, eval_env, c["n_eval_episodes"], deterministic=True)
        logs = td3.read_logs()
        trk = r.tracking_scalars()
        deg = {f"eval/heading_{k}_deg": round(math.degrees(trk[f"eval/heading_{k}"]), 4) for k in ("mae", "rmse")} if demo else {}
        line = {"timesteps": td3.num_timesteps, "n_updates": td3.n_updates, "n_actor_updates": td3.n_actor_updates,
                "env_steps_per_s": round(td3.num_timesteps / max(state["train_s"], 1e-9), 1),
                "eval_ep_rew_mean": round(float(sum(r.episode_rewards) / len(r.episode_rewards)), 3),
                "eval_ep_len_mean": round(float(sum(r.episode_lengths) / len(r.episode_lengths)), 1),
                **{k: round(float(v), 5) for k, v in trk.items()}, **deg,
                **{k: round(float(logs[k]), 5) for k in T.SCALARS},
                **{k: (round(v, 5) if math.isfinite(v) else None) for k, v in td3.rollout_stats.items()}}
        print(json.dumps(line), flush=True)
        state["mark"] = time.perf_counter()

    def on_step(td3):
        if td3.num_timesteps >= state["next_eval"]:
            evaluate_now(td3)
            state["next_eval"] += a.eval_freq
        return True

    print(json.dumps({"config": {**{k: v for k, v in c.items()}, "algo": "td3", "batch_size": a.batch_size, "policy_delay": a.policy_delay,
                                 "action_noise_sigma": a.action_noise_sigma, "total_timesteps": a.total_timesteps, "eval_freq": a.eval_freq,
                                 "env": a.env, "num_envs": a.num_envs, "gradient_steps": model.G,
                                 **({"n_steps": a.n_steps} if a.n_steps != 1 else {}),
                                 **({"her_goals": a.her_goals, "her_horizon": a.her_horizon} if a.her_goals else {}),
                                 "fused_update": a.fused_update, "use_graphs": a.use_graphs}}), flush=True)
    evaluate_now(model)                      # the untrained actor: the line later evaluations are read against
    try:
        model.learn(a.total_timesteps, callbacks=[on_step])
    finally:
        torch.save(model.state_dict(include_buffer=False), os.path.join(a.out, "final_model.pt"))
        env.close(); eval_env.venv.close()
    print(json.dumps({"done": model.num_timesteps, "wall_s": round(time.perf_counter() - t0, 1), "checkpoint": os.path.join(a.out, "final_model.pt")}), flush=True)


if __name__ == "__main__":
    main()
