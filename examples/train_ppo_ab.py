"""Device-resident counterpart of the reference's train/train_ppo_ab.py: PPO on the A -> B waypoint flight.

The reference reads configs/env.yaml and configs/ppo.yaml; their values are this file's ENV_KW and PPO_CONFIG: one target, reach
distance 2 m, dome 100 m, 120 s, quaternion attitude, 30 Hz, context 1, dense reward, the wind block switched off; 8 envs, 1024 steps,
batch 256, lr 3e-4, gamma 0.99, lambda 0.95, clip 0.2, ent 0, vf 0.5, seed 42 (epochs and gradient clip: SB3's defaults, 10 and 0.5);
observations and rewards normalised, clipped at 10.  The evaluation is the reference's -- every max(10000 // num_envs, 1000)
vec-steps, 10 episodes, deterministic, best model kept -- and records what its comment asks for ("success rate and arrival time"):
the reach rate, and the flight's path figures (evaluate.EvalResult.path_scalars, DESIGN.md section 2f: time to the target, path
length and efficiency, airspeed, altitude, control activity, the closest approach of the flights that missed).

The policy update runs on the torch path by default; --fused_learner puts collection and update on the fused four-action kernels
(fw_collect_step, fw_ppo_update).  With more envs than the reference's 8, n_steps shrinks so that one update still sees 8 x 1024 samples.

    python examples/train_ppo_ab.py --total_timesteps 2000000 [--num_envs 8] [--fused_learner] --out runs/ab_ppo
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import checkpoint, evaluate, rollout as R  # noqa: E402

PPO_CONFIG = dict(seed=42, total_timesteps=1_000_000_000, n_eval_episodes=10, num_envs=8, n_steps=1024, batch_size=256, n_epochs=10,
                  learning_rate=3e-4, gamma=0.99, gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                  normalize_obs=True, normalize_reward=True, clip_obs=10.0)
ENV_KW = dict(sparse_reward=False, num_targets=1, goal_reach_distance=2.0, flight_dome_size=100.0, max_duration_seconds=120.0,
              angle_representation="quaternion", agent_hz=30, context_length=1,
              wind_config={"enabled": False, "mode": "constant", "wind_enu_mps": [0.0, 0.0, 0.0]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pretrained_model", type=str, default=None)
    ap.add_argument("--vecnorm_path", type=str, default=None)
    ap.add_argument("--total_timesteps", type=int, default=None)
    ap.add_argument("--num_envs", type=int, default=PPO_CONFIG["num_envs"])
    ap.add_argument("--out", type=str, default="runs/ab_ppo")
    ap.add_argument("--fused_learner", action="store_true", help="the fused collector / update kernels instead of the torch path")
    ap.add_argument("--episode_stats", action="store_true",
                    help="SB3's rollout/* figures (ep_rew_mean, ep_len_mean, success_rate over the last 100 episodes, and the "
                         "rollout/interval/* means over all episodes since the last line) in every printed update line")
    ap.add_argument("--episode_fold", choices=("one", "wide", "auto"), default="one",
                    help="the device form of the episode fold behind --episode_stats: one workgroup, one workgroup per span of envs "
                         "(large env counts), or chosen by the env count")
    ap.add_argument("--diagnostics", action="store_true",
                    help="SB3's train/* figures (approx_kl, clip_fraction, explained_variance, ...) in every printed update line")
    ap.add_argument("--target_kl", type=float, default=None,
                    help="SB3's target_kl: end an update at the first minibatch whose approx_kl is above 1.5 x this (default: off)")
    a = ap.parse_args()
    cfg = PPO_CONFIG
    model_dir, log_dir = os.path.join(a.out, "models"), os.path.join(a.out, "logs")
    os.makedirs(model_dir, exist_ok=True); os.makedirs(log_dir, exist_ok=True)

    env = R.VecNormalizeDevice(P.FixedwingWaypointsVecEnv(num_envs=a.num_envs, seed=cfg["seed"], **ENV_KW), norm_obs=cfg["normalize_obs"],
                               norm_reward=cfg["normalize_reward"], clip_obs=cfg["clip_obs"], gamma=cfg["gamma"])
    eval_env = R.VecNormalizeDevice(P.FixedwingWaypointsVecEnv(num_envs=min(a.num_envs, 16), seed=cfg["seed"], global_env_offset=a.num_envs, **ENV_KW),
                                    training=False, norm_obs=True, norm_reward=False, clip_obs=cfg["clip_obs"])
    vecnorm = checkpoint.infer_vecnorm_path(a.pretrained_model, a.vecnorm_path, model_dir)
    if vecnorm:
        checkpoint.load_vecnormalize(vecnorm, env, training=True, norm_reward=True)
    n_steps = R.n_steps_for(cfg["num_envs"] * cfg["n_steps"], a.num_envs)      # holds the samples per update: n_steps ~ 1 / envs
    f = bool(a.fused_learner)
    model = R.PPO(env, R.PPOConfig(diagnostics=a.diagnostics, target_kl=a.target_kl, episode_stats=a.episode_stats, episode_fold=a.episode_fold, n_steps=n_steps, batch_size=cfg["batch_size"],
                                   n_epochs=cfg["n_epochs"], learning_rate=cfg["learning_rate"], gamma=cfg["gamma"],
                                   gae_lambda=cfg["gae_lambda"], clip_range=cfg["clip_range"], ent_coef=cfg["ent_coef"],
                                   vf_coef=cfg["vf_coef"], max_grad_norm=cfg["max_grad_norm"], seed=cfg["seed"],
                                   fused_update=f, fused_collect=f, one_launch_collect=f))
    if a.pretrained_model:
        checkpoint.set_parameters(a.pretrained_model, model)
    ev = evaluate.EvalCallback(eval_env, n_eval_episodes=cfg["n_eval_episodes"], eval_freq=max(10000 // a.num_envs, 1000), log_path=log_dir,
                               best_model_save_path=model_dir, num_targets_total=ENV_KW["num_targets"], verbose=1, path_figures=True)

    class Progress:
        t0, last = time.perf_counter(), 0
        def on_rollout_end(self, ppo):
            msg = ppo.early_stop_message()     # (--target_kl; learn() calls this hook right after train(): the update that just ended)
            if msg:
                print(msg, flush=True)
            if ppo.num_timesteps - self.last >= 4 * n_steps * a.num_envs:
                dt = time.perf_counter() - self.t0
                print(json.dumps({"timesteps": ppo.num_timesteps, "fps": round(ppo.num_timesteps / dt), **{k: round(v, 5) for k, v in ppo.logs.items()},
                                  **{k: round(v, 6) for k, v in ppo.diagnostics.items()}, **{k: round(v, 5) for k, v in ppo.rollout_stats.items()},
                                  **{k: round(float(v), 4) for k, v in ev.last_scalars.items()}}), flush=True)
                self.last = ppo.num_timesteps
            return True

    total = a.total_timesteps if a.total_timesteps is not None else cfg["total_timesteps"]
    try:
        model.learn(total, callbacks=[ev, Progress()], reset_num_timesteps=True)
    finally:
        checkpoint.save(os.path.join(model_dir, "final_model.pt"), model)
        checkpoint.save_vecnormalize(os.path.join(model_dir, "vecnorm.pt"), env)
        env.venv.close(); eval_env.venv.close()


if __name__ == "__main__":
    main()
