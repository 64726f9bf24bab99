"""Device-resident counterpart of the reference's examples/lowlevel.py: the low-level controller trained with SAC instead of PPO.

Same hyper-parameters (SB3 ``SAC("MlpPolicy")``: net_arch [256, 256], buffer 200 000, batch 256, gamma 0.99, tau 0.02, lr 3e-4, one
gradient step per env step, automatic entropy coefficient, no VecNormalize, 100 000 steps).  A vec-step -- act, env step, store,
``gradient_steps`` x (sample, update) -- is one captured graph (pyflyt_drone_amd/sac.py); ``--no-fused_update`` runs the gradient
steps in torch on the same act / store / sample / noise kernels.

``--env tracking`` (the default) trains on the low-level env of train/train_lowlevel_cmd.py (``FixedwingLowLevelVecEnv``);
``--env demo`` trains and evaluates on the env the reference script itself defines (``FixedwingLowLevelDemoVecEnv``, DESIGN.md
section 2d: 120 m / 25 m/s start, its reward and episode ends, its constructor defaults) -- the like-for-like run of the script.
In ``demo`` mode every evaluation line also carries the heading MAE and RMSE in degrees, the unit the script reports.

    python examples/train_lowlevel_sac.py --out runs/lowlevel_sac
    python examples/train_lowlevel_sac.py --env demo --out runs/lowlevel_sac_demo

At thousands of envs the reference's update-to-data ratio of 1 is thousands of small gradient steps per vec-step; the large-env recipe
is one gradient step per vec-step on a batch as large as the env count (the wide form of ``fw_sac_update``, batches up to 8192):

    python examples/train_lowlevel_sac.py --num_envs 4096 --batch_size 4096 --gradient_steps 1 --total_timesteps 2000000

``--n_steps k`` (1 ... 16, default 1) trains on k-step returns gathered from the ring (``SACConfig.n_steps``): with so
few gradient steps per sample each one carries reward information k steps back instead of one.

``--her_goals n`` (default 0: off) relabels goals in hindsight as SB3's ``HerReplayBuffer(n_sampled_goal=n)`` with the "future"
strategy does: a sampled transition keeps its episode's target with probability 1 / (n + 1); otherwise its target becomes the heading,
altitude and airspeed the same episode reached at most ``--her_horizon`` - 1 steps later (1 ... 64, default 64) and its reward is
recomputed for that target (``SACConfig.her_goals``).  Both env variants; not together with ``--n_steps`` above 1.

``--prioritized`` draws every batch in proportion to the rows' priorities ``(|td| + 1e-6)^per_alpha`` (Schaul et al. 2016, the
proportional variant; ``SACConfig.prioritized``) and weights the critic loss by ``(N P(row))^-per_beta`` over its
maximum; ``--per_beta_steps n`` anneals that exponent from ``--per_beta`` to 1 over n gradient steps.  New rows enter with the largest
priority seen so far.  Both env variants; not together with ``--n_steps`` above 1 or ``--her_goals``.

``--normalize_obs`` / ``--normalize_reward`` put SB3's ``VecNormalize`` in front of the learner as it works with an off-policy buffer
(``SACConfig.normalize_obs`` / ``normalize_reward``): running statistics of the observations and of the
discounted return, moved after every env step; the ring keeps raw rows, the actor and every sampled batch read normalised ones
(clipped to ``--clip_obs`` / ``--clip_reward``, default 10).  The evaluation env is built by ``SAC.eval_env`` and reads the learner's
own statistics.  Both env variants, together with any of the options above.
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
from pyflyt_drone_amd import evaluate, sac as S  # noqa: E402

TRAIN_CONFIG = dict(total_timesteps=100_000, learning_rate=3e-4, buffer_size=200_000, batch_size=256, gamma=0.99, tau=0.02,
                    target_update_interval=1, learning_starts=100, net_arch=(256, 256), seed=0, n_eval_episodes=16, eval_freq=10_000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", choices=("tracking", "demo"), default="tracking",
                    help="tracking: the env of train/train_lowlevel_cmd.py; demo: the env examples/lowlevel.py defines for this run")
    ap.add_argument("--total_timesteps", type=int, default=TRAIN_CONFIG["total_timesteps"])
    ap.add_argument("--num_envs", type=int, default=16)
    ap.add_argument("--gradient_steps", type=int, default=-1, help="per vec-step; -1: one per env (update-to-data 1, as the reference)")
    ap.add_argument("--batch_size", type=int, default=TRAIN_CONFIG["batch_size"],
                    help="rows per gradient step: a multiple of 16 up to 512, or a multiple of 64 up to 8192; the large-env recipe is "
                         "--num_envs 4096 --batch_size 4096 --gradient_steps 1")
    ap.add_argument("--n_steps", type=int, default=1,
                    help="n-step returns (1 ... 16): the target is r_0 + gamma r_1 + ... + gamma^k bootstrap, cut at episode ends; 1: the 1-step target")
    ap.add_argument("--her_goals", type=int, default=0,
                    help="hindsight goal relabelling, SB3's n_sampled_goal: a sampled row is relabelled with probability n / (n + 1); 0: off")
    ap.add_argument("--her_horizon", type=int, default=64,
                    help="the relabelled goal is one the episode achieved at most this many steps ahead, minus one (1 ... 64)")
    ap.add_argument("--prioritized", action="store_true", help="prioritized replay (proportional): batches drawn by |TD error|, the critic loss importance-weighted")
    ap.add_argument("--per_alpha", type=float, default=0.6, help="priority exponent in [0, 1]; 0 draws uniformly over the filled rows")
    ap.add_argument("--per_beta", type=float, default=0.4, help="importance-weight exponent in [0, 1]")
    ap.add_argument("--per_beta_steps", type=int, default=0, help="> 0: anneal the importance-weight exponent from --per_beta to 1 over this many gradient steps")
    ap.add_argument("--normalize_obs", action="store_true", help="running observation normalisation (VecNormalize's norm_obs) in front of actor and critics")
    ap.add_argument("--normalize_reward", action="store_true", help="sampled rewards divided by the running std of the discounted return (VecNormalize's norm_reward)")
    ap.add_argument("--clip_obs", type=float, default=10.0, help="a normalised observation is clipped to +-clip_obs")
    ap.add_argument("--clip_reward", type=float, default=10.0, help="a normalised reward is clipped to +-clip_reward")
    ap.add_argument("--fused_update", action=argparse.BooleanOptionalAction, default=True,
                    help="fw_sac_update (default) or the torch gradient step")
    ap.add_argument("--use_graphs", action=argparse.BooleanOptionalAction, default=True)
    ap.add_argument("--eval_freq", type=int, default=TRAIN_CONFIG["eval_freq"], help="env steps between evaluations")
    ap.add_argument("--eval_max_steps", type=int, default=1800, help="time limit of an evaluation episode (agent steps; --env tracking only: demo evaluates on the script's own 60 s clock)")
    ap.add_argument("--episode_stats", action="store_true",
                    help="SB3's rollout/* figures (ep_rew_mean, ep_len_mean, success_rate over the last 100 training episodes, and the "
                         "rollout/interval/* means over all episodes since the last line) in every evaluation line")
    ap.add_argument("--episode_fold", choices=("one", "wide", "auto"), default="one",
                    help="the device form of the episode fold behind --episode_stats: one workgroup, one workgroup per span of envs "
                         "(large env counts), or chosen by the env count")
    ap.add_argument("--out", type=str, default="runs/lowlevel_sac")
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
    model = S.SAC(env, S.SACConfig(learning_rate=c["learning_rate"], buffer_size=c["buffer_size"], batch_size=a.batch_size,
                                   gamma=c["gamma"], tau=c["tau"], gradient_steps=a.gradient_steps,
                                   target_update_interval=c["target_update_interval"], learning_starts=c["learning_starts"],
                                   net_arch=c["net_arch"], seed=c["seed"], use_graphs=a.use_graphs, fused_update=a.fused_update,
                                   episode_stats=a.episode_stats, episode_fold=a.episode_fold, n_steps=a.n_steps,
                                   her_goals=a.her_goals, her_horizon=a.her_horizon, prioritized=a.prioritized, per_alpha=a.per_alpha,
                                   per_beta=a.per_beta, per_beta_steps=a.per_beta_steps, normalize_obs=a.normalize_obs,
                                   normalize_reward=a.normalize_reward, clip_obs=a.clip_obs, clip_reward=a.clip_reward))
    # (with both flags off: a pass-through wrapper; with --normalize_obs it reads the learner's own, live statistics)
    eval_env = model.eval_env(P.FixedwingVecEnv(eval_cfg, 16, seed=c["seed"], global_env_offset=a.num_envs))
    t0 = time.perf_counter()
    state = {"next_eval": a.eval_freq, "train_s": 0.0, "mark": t0}

    def evaluate_now(sac):
        torch.cuda.synchronize()
        state["train_s"] += time.perf_counter() - state["mark"]
        r = evaluate.evaluate_policy(sac.policy, eval_env, c["n_eval_episodes"], deterministic=True)
        logs = sac.read_logs()
        trk = r.tracking_scalars()
        deg = {f"eval/heading_{k}_deg": round(math.degrees(trk[f"eval/heading_{k}"]), 4) for k in ("mae", "rmse")} if demo else {}
        line = {"timesteps": sac.num_timesteps, "n_updates": sac.n_updates,
                "env_steps_per_s": round(sac.num_timesteps / max(state["train_s"], 1e-9), 1),
                "eval_ep_rew_mean": round(float(sum(r.episode_rewards) / len(r.episode_rewards)), 3),
                "eval_ep_len_mean": round(float(sum(r.episode_lengths) / len(r.episode_lengths)), 1),
                **{k: round(float(v), 5) for k, v in trk.items()}, **deg,
                **{k: round(float(logs[k]), 5) for k in S.SCALARS},
                **{k: (round(v, 5) if math.isfinite(v) else None) for k, v in sac.rollout_stats.items()}}
        print(json.dumps(line), flush=True)
        state["mark"] = time.perf_counter()

    def on_step(sac):
        if sac.num_timesteps >= state["next_eval"]:
            evaluate_now(sac)
            state["next_eval"] += a.eval_freq
        return True

    print(json.dumps({"config": {**{k: v for k, v in c.items()}, "batch_size": a.batch_size, "total_timesteps": a.total_timesteps, "eval_freq": a.eval_freq, **({"env": a.env} if demo else {}), "num_envs": a.num_envs, "gradient_steps": model.G,
                                 **({"n_steps": a.n_steps} if a.n_steps != 1 else {}),
                                 **({"her_goals": a.her_goals, "her_horizon": a.her_horizon} if a.her_goals else {}),
                                 **({"prioritized": True, "per_alpha": a.per_alpha, "per_beta": a.per_beta, "per_beta_steps": a.per_beta_steps} if a.prioritized else {}),
                                 **({"normalize_obs": a.normalize_obs, "normalize_reward": a.normalize_reward, "clip_obs": a.clip_obs, "clip_reward": a.clip_reward}
                                    if a.normalize_obs or a.normalize_reward else {}),
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
