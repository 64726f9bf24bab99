"""Device-resident counterpart of the reference's train/train_highlevel_cmd.py (:35-181 env, :185-206 config, :230-266 train()).

The high-level policy of the hierarchical design: it outputs (heading, altitude, airspeed) commands, a frozen low-level controller
(what examples/train_lowlevel_cmd.py trains and saves) turns each command into six actuator commands, and the waypoint task runs
underneath (dome 200 m, 120 s, 30 Hz, euler, context 2).  Same PPO hyper-parameters as the reference's TRAIN_CFG (16 envs, n_steps
1024, batch 256, 10 epochs, gamma 0.995, lambda 0.95, clip 0.2, no entropy bonus, seed 123).  The three-action policy trains on the
torch path by default (the env's vec-step is then three launches, fw_command_hl -> fw_collect_act_a -> fw_step); --fused_learner puts it
on the fused three-action learner (fw_ppo_update_a3) and collector (fw_collect_act_hl -> fw_step -> fw_collect_stats;
PPOConfig.fused_three_actions); --fused_eval puts the evaluations on the fused three-action path as well (fw_collect_act_hl -> fw_step ->
fw_eval_track_hl; off by default).  The evaluations record the command figures of evaluate.EvalResult.command_scalars.  The actions are the reference's: a raw Gaussian clipped to the Box in physical units.

    python examples/train_lowlevel_cmd.py --total_timesteps 2000000 --out runs/lowlevel_ppo
    python examples/train_highlevel_cmd.py --low_checkpoint runs/lowlevel_ppo/models/final_model.pt --total_timesteps 2000000
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyflyt_drone_amd as P  # noqa: E402
from pyflyt_drone_amd import checkpoint, evaluate, rollout as R  # noqa: E402

TRAIN_CFG = dict(total_timesteps=20_000_000, num_envs=16, learning_rate=3e-4, n_steps=1024, batch_size=256, n_epochs=10, gamma=0.995,
                 gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, seed=123,
                 wind={"enabled": False, "mode": "constant", "wind_enu_mps": [0.0, 0.0, 0.0]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--low_checkpoint", type=str, default=os.path.join("runs", "lowlevel_ppo", "models", "final_model.pt"),
                    help="the low-level controller: a checkpoint examples/train_lowlevel_cmd.py saved")
    ap.add_argument("--num_envs", type=int, default=None)
    ap.add_argument("--total_timesteps", type=int, default=None)
    ap.add_argument("--n_steps", type=int, default=None, help="default: the reference's 16 x 1024 samples per update, split over --num_envs")
    ap.add_argument("--out", type=str, default="runs/highlevel_ppo")
    ap.add_argument("--fused_learner", action="store_true", help="the fused three-action update / collector kernels instead of the torch path")
    ap.add_argument("--controller_hz", type=int, default=None,
                    help="the rate the frozen controller runs at: 30 (default, once per agent step, the reference's behaviour) or 120 "
                         "(once per Aviary step inside the step kernel: the rate it was trained at)")
    ap.add_argument("--fused_eval", action="store_true", help="the evaluations through the fused three-action kernels (use_fused=True) instead of the torch forward")
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
    cfg = TRAIN_CFG
    num_envs = a.num_envs if a.num_envs is not None else cfg["num_envs"]
    model_dir, log_dir = os.path.join(a.out, "models"), os.path.join(a.out, "logs")

    def make(n, seed):                      # a missing checkpoint raises FileNotFoundError here, as the reference does (:110-121)
        return P.HighLevelCmdVecEnv(n, low_checkpoint=a.low_checkpoint, flight_dome_size=200.0, max_duration_seconds=120.0, agent_hz=30,
                                    context_length=2, wind_config=cfg["wind"], seed=seed, controller_hz=a.controller_hz)

    venv = make(num_envs, cfg["seed"])
    os.makedirs(model_dir, exist_ok=True); os.makedirs(log_dir, exist_ok=True)
    env = R.VecNormalizeDevice(venv, norm_obs=True, norm_reward=True, clip_obs=10.0, gamma=cfg["gamma"])
    eval_env = R.VecNormalizeDevice(make(16, cfg["seed"] + 1000), training=False, norm_reward=False, clip_obs=10.0, gamma=cfg["gamma"])
    n_steps = a.n_steps if a.n_steps is not None else R.n_steps_for(cfg["num_envs"] * cfg["n_steps"], num_envs)
    model = R.PPO(env, R.PPOConfig(diagnostics=a.diagnostics, target_kl=a.target_kl, episode_stats=a.episode_stats, episode_fold=a.episode_fold, n_steps=n_steps, batch_size=cfg["batch_size"], n_epochs=cfg["n_epochs"], learning_rate=cfg["learning_rate"],
                                   gamma=cfg["gamma"], gae_lambda=cfg["gae_lambda"], clip_range=cfg["clip_range"], ent_coef=cfg["ent_coef"],
                                   vf_coef=cfg["vf_coef"], max_grad_norm=cfg["max_grad_norm"], seed=cfg["seed"],
                                   fused_three_actions=a.fused_learner))
    per_update = n_steps * num_envs
    ev = evaluate.EvalCallback(eval_env, n_eval_episodes=16, eval_freq=max(10 * per_update // num_envs, 1), log_path=log_dir,
                               best_model_save_path=model_dir, num_targets_total=int(venv.cfg.num_targets), verbose=1,
                               use_fused=True if a.fused_eval else None)

    class Progress:
        t0, last = time.perf_counter(), 0
        def on_rollout_end(self, ppo):
            msg = ppo.early_stop_message()     # (--target_kl; learn() calls this hook right after train(): the update that just ended)
            if msg:
                print(msg, flush=True)
            if ppo.num_timesteps - self.last >= 5 * per_update:
                dt = time.perf_counter() - self.t0
                print(json.dumps({"timesteps": ppo.num_timesteps, "fps": round(ppo.num_timesteps / dt), **{k: round(v, 5) for k, v in ppo.logs.items()}, **{k: round(v, 6) for k, v in ppo.diagnostics.items()}, **{k: round(v, 5) for k, v in ppo.rollout_stats.items()},
                                  **{k: round(float(v), 4) for k, v in ev.last_scalars.items()}}), flush=True)
                self.last = ppo.num_timesteps
            return True

    total = a.total_timesteps if a.total_timesteps is not None else cfg["total_timesteps"]
    t0 = time.perf_counter()
    try:
        model.learn(total, callbacks=[ev, Progress()], reset_num_timesteps=True)
    finally:
        import torch
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"final": True, "num_envs": num_envs, "n_steps": n_steps, "timesteps": model.num_timesteps, "wall_s": round(dt, 2),
                          "env_steps_per_s": round(model.num_timesteps / dt), "fused_learner": bool(a.fused_learner), "fused_eval": bool(a.fused_eval), "n_evals": ev.n_evals,
                          "rejected_actions": int(venv.rejected.item())}), flush=True)
        checkpoint.save(os.path.join(model_dir, "final_model.pt"), model)
        checkpoint.save_vecnormalize(os.path.join(model_dir, "vecnorm.pt"), env)
        venv.close(); eval_env.venv.close()


if __name__ == "__main__":
    main()
