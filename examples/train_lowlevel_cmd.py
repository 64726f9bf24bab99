"""Device-resident counterpart of the reference's train/train_lowlevel_cmd.py (:27-48 config, :54-61 env, :63-100 train()).

The low-level controller of the hierarchical design: six actuator commands track a heading / height / speed target drawn per
episode (envs/fixedwing_envs/fixedwing_lowlevel_env.py).  Same PPO hyper-parameters (lr 3e-4, batch 64, 10 epochs, gamma 0.99,
lambda 0.95, clip 0.2, no entropy bonus, vf 0.5, max-grad-norm 0.5) and VecNormalize(norm_obs, norm_reward, clip_obs=10); the env
count goes from 32 to thousands and n_steps shrinks so that one update still sees 32 x 2048 = 65 536 samples.  Six actions: the
policy update runs on the torch path by default; --fused_learner puts it on the fused six-action learner (fw_ppo_update_a and the
three-launch collector fw_collect_act_a -> fw_step -> fw_collect_stats, PPOConfig.fused_six_actions).

    python examples/train_lowlevel_cmd.py --total_timesteps 2000000 --num_envs 4096 --out runs/lowlevel
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import checkpoint, evaluate, rollout as R  # noqa: E402

TRAIN_CONFIG = dict(total_timesteps=2_000_000, n_eval_episodes=10, learning_rate=3e-4, samples_per_update=32 * 2048, batch_size=64,
                    n_epochs=10, gamma=0.99, gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, seed=42,
                    wind={"enabled": False, "mode": "constant", "wind_enu_mps": [0.0, 0.0, 0.0]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pretrained_model", type=str, default=None)
    ap.add_argument("--vecnorm_path", type=str, default=None)
    ap.add_argument("--total_timesteps", type=int, default=None)
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--out", type=str, default="runs/lowlevel_ppo")
    ap.add_argument("--fused_learner", action="store_true", help="the fused six-action update / collector kernels instead of the torch path")
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
    cfg = TRAIN_CONFIG
    model_dir, log_dir = os.path.join(a.out, "models"), os.path.join(a.out, "logs")
    os.makedirs(model_dir, exist_ok=True); os.makedirs(log_dir, exist_ok=True)

    world, rank, local = R.init_distributed_from_env()          # torchrun: one process per GPU (RCCL); (1, 0, 0) otherwise
    dev = local if world > 1 else None
    # rank r simulates global envs [r * num_envs, (r + 1) * num_envs): target / wind / noise streams are keyed on the global id
    env = R.VecNormalizeDevice(P.FixedwingLowLevelVecEnv(num_envs=a.num_envs, seed=cfg["seed"], device=dev, global_env_offset=rank * a.num_envs,
                                                         wind_config=cfg["wind"]), norm_obs=True, norm_reward=True, clip_obs=10.0)
    eval_env = R.VecNormalizeDevice(P.FixedwingLowLevelVecEnv(num_envs=16, seed=cfg["seed"], device=dev, global_env_offset=world * a.num_envs,
                                                              wind_config=cfg["wind"]), training=False, norm_reward=False, clip_obs=10.0)
    vecnorm = checkpoint.infer_vecnorm_path(a.pretrained_model, a.vecnorm_path, model_dir)
    if vecnorm:
        checkpoint.load_vecnormalize(vecnorm, env, training=True, norm_reward=True)
    n_steps = R.n_steps_for(cfg["samples_per_update"], a.num_envs, world)      # holds the samples per update: n_steps ~ 1 / (envs x world)
    model = R.PPO(env, R.PPOConfig(diagnostics=a.diagnostics, target_kl=a.target_kl, episode_stats=a.episode_stats, episode_fold=a.episode_fold, n_steps=n_steps, batch_size=cfg["batch_size"], n_epochs=cfg["n_epochs"], learning_rate=cfg["learning_rate"],
                                   gamma=cfg["gamma"], gae_lambda=cfg["gae_lambda"], clip_range=cfg["clip_range"], ent_coef=cfg["ent_coef"],
                                   vf_coef=cfg["vf_coef"], max_grad_norm=cfg["max_grad_norm"], seed=cfg["seed"],
                                   fused_six_actions=a.fused_learner))
    if a.pretrained_model:
        checkpoint.set_parameters(a.pretrained_model, model)
    ev = evaluate.EvalCallback(eval_env, n_eval_episodes=max(cfg["n_eval_episodes"], 16), eval_freq=max(10000 // a.num_envs, 1) * 50,
                               log_path=log_dir, best_model_save_path=model_dir, verbose=1)
    ck = checkpoint.CheckpointCallback(save_freq=max(50000 // a.num_envs, 1) * 50, save_path=model_dir, name_prefix="lowlevel_ppo")

    class Progress:
        t0, last = time.perf_counter(), 0
        def on_rollout_end(self, ppo):
            msg = ppo.early_stop_message()     # (--target_kl; learn() calls this hook right after train(): the update that just ended)
            if msg:
                print(msg, flush=True)
            if ppo.num_timesteps - self.last >= 5 * n_steps * a.num_envs * world:
                dt = time.perf_counter() - self.t0
                print(json.dumps({"timesteps": ppo.num_timesteps, "fps": round(ppo.num_timesteps / dt), **{k: round(v, 5) for k, v in ppo.logs.items()}, **{k: round(v, 6) for k, v in ppo.diagnostics.items()}, **{k: round(v, 5) for k, v in ppo.rollout_stats.items()},
                                  **{k: round(float(v), 4) for k, v in ev.last_scalars.items()}}), flush=True)
                self.last = ppo.num_timesteps
            return True

    total = a.total_timesteps if a.total_timesteps is not None else cfg["total_timesteps"]
    try:
        model.learn(total, callbacks=[ev, ck, Progress()], reset_num_timesteps=True)
    finally:
        if model.rank == 0:                 # one writer per file in a multi-process job
            checkpoint.save(os.path.join(model_dir, "final_model.pt"), model)
            checkpoint.save_vecnormalize(os.path.join(model_dir, "vecnorm.pt"), env)
        env.venv.close(); eval_env.venv.close()


if __name__ == "__main__":
    main()
