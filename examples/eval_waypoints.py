"""Evaluate a trained waypoint / ObjLock / combined / A -> B policy and look at its flight.

Prints what the reference's eval/eval_waypoints.py prints -- mean reward +/- std, mean episode length -- plus the reach rates and the
flight's path figures (evaluate.EvalResult.path_scalars): airspeed, altitude, control activity, time to the
targets, path length and efficiency, and the closest approach of the flights that missed.  The evaluation is deterministic, with
frozen normaliser statistics (the vecnorm.pt next to the checkpoint, or the statistics saved in it); the path sums are carried on the
device inside the replayed evaluation (fw_eval_track_wp).  --fused runs act and step as one fw_collect_step launch.

--trace_steps N also flies N vec-steps from a reset and writes the flight record (flight.fly, fw_trace_rows) to trace.npz (trace,
start, dt, ended_at and the column map); --plot draws the XY and the 3-D path of env 0's first episode with its start, the points
where targets were reached and the start -> reach chords (needs matplotlib; without it the plot is skipped with a note).

    python examples/eval_waypoints.py --task ab --checkpoint runs/ab_ppo/models/best_model.pt [--episodes 20] [--fused] \\
        [--trace_steps 1800] [--plot] [--out runs/ab_eval]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def task_config(task: str):
    """the training config of the example that trains ``task``"""
    from pyflyt_drone_amd import config as K
    if task == "waypoints":
        return K.train_waypoints_v3_config()                     # examples/train_fixedwing_waypoints.py
    if task == "ab":                                             # examples/train_ppo_ab.py
        return K.waypoints_config(sparse_reward=False, num_targets=1, goal_reach_distance=2.0, flight_dome_size=100.0,
                                  max_duration_seconds=120.0, angle_representation="quaternion", agent_hz=30, context_length=1)
    if task == "objlock":
        return K.train_objlock_config()                          # examples/train_objlock.py
    if task == "combined":
        return K.train_waypoint_objlock_config()                 # examples/train_fixedwing_waypoints_objlock.py
    raise ValueError(task)


def plot_flight(tr, path: str, env_index: int = 0) -> bool:
    """XY and 3-D path of one env's first episode: the start, the points where a target was reached, the start -> reach chords"""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception as e:                                       # the example runs without matplotlib
        print(f"--plot: matplotlib is not importable ({e}); no figure written")
        return False
    import numpy as np
    rows = tr.episode(env_index)
    p = np.concatenate([tr.position(tr.start[env_index:env_index + 1]), tr.position(rows)], axis=0)
    reached = np.concatenate([[0], tr.targets_reached(rows)])
    hit = np.nonzero(np.diff(reached) > 0)[0] + 1                # indices into p
    legs = np.concatenate([p[0:1], p[hit]], axis=0)
    fig = plt.figure(figsize=(11, 5))
    ax = fig.add_subplot(1, 2, 1)
    ax.plot(p[:, 0], p[:, 1], "-", color="tab:blue", label="flight path")
    ax.plot(legs[:, 0], legs[:, 1], "--", color="tab:gray", label="start -> reach chords")
    ax.plot(p[0, 0], p[0, 1], "o", color="tab:green", label="start")
    if len(hit):
        ax.plot(p[hit, 0], p[hit, 1], "*", color="tab:red", markersize=12, label="target reached")
    ax.plot(p[-1, 0], p[-1, 1], "x", color="black", label="end")
    ax.set_xlabel("x [m]"); ax.set_ylabel("y [m]"); ax.set_aspect("equal", adjustable="datalim"); ax.grid(True, alpha=0.3); ax.legend()
    ax.set_title(f"env {env_index}: {len(rows)} steps, {int(reached[-1])} target(s) reached")
    ax3 = fig.add_subplot(1, 2, 2, projection="3d")
    ax3.plot(p[:, 0], p[:, 1], p[:, 2], "-", color="tab:blue")
    ax3.plot(legs[:, 0], legs[:, 1], legs[:, 2], "--", color="tab:gray")
    ax3.scatter(*p[0], color="tab:green")
    if len(hit):
        ax3.scatter(p[hit, 0], p[hit, 1], p[hit, 2], color="tab:red", marker="*", s=80)
    ax3.set_xlabel("x [m]"); ax3.set_ylabel("y [m]"); ax3.set_zlabel("z [m]")
    fig.tight_layout()
    fig.savefig(path, dpi=120)
    plt.close(fig)
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", type=str, default="waypoints", choices=["waypoints", "ab", "objlock", "combined"])
    ap.add_argument("--checkpoint", type=str, default=None, help="best_model.pt / final_model.pt of the task's training example; "
                    "without one a freshly initialised policy flies (a smoke run)")
    ap.add_argument("--vecnorm_path", type=str, default=None)
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--num_envs", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fused", action="store_true", help="act and step as one fw_collect_step launch")
    ap.add_argument("--trace_steps", type=int, default=0, help="also record a flight of this many vec-steps (trace.npz)")
    ap.add_argument("--plot", action="store_true", help="draw env 0's first episode of the recorded flight (flight.png)")
    ap.add_argument("--out", type=str, default=None, help="directory for evaluation.json, trace.npz and flight.png")
    a = ap.parse_args()

    import numpy as np
    import torch
    import pyflyt_drone_amd as P
    from pyflyt_drone_amd import checkpoint, evaluate, flight, rollout as R

    cfg = task_config(a.task)
    sd = torch.load(a.checkpoint, map_location="cpu", weights_only=True) if a.checkpoint else None

    def make():
        env = R.VecNormalizeDevice(P.FixedwingVecEnv(cfg, a.num_envs, seed=a.seed), training=False, norm_reward=False, clip_obs=10.0)
        if sd is not None:
            vecnorm = checkpoint.infer_vecnorm_path(a.checkpoint, a.vecnorm_path)
            if vecnorm:
                checkpoint.load_vecnormalize(vecnorm, env, training=False, norm_reward=False)
            else:                              # no vecnorm.pt: the statistics saved with the model
                env.load_state_dict(sd["vecnormalize"])
                env.training, env.norm_reward = False, False
        return env

    env = make()
    if sd is not None and sd["obs_dim"] != env.obs_dim:
        raise SystemExit(f"{a.checkpoint}: obs_dim {sd['obs_dim']} is not the {a.task} task's {env.obs_dim}")
    policy = R.MlpPolicy(env.obs_dim, env.act_dim).to(env.device)
    if sd is not None:
        policy.load_state_dict(sd["policy"])
    policy.eval()
    hz = float(cfg.agent_hz)

    r = evaluate.evaluate_policy(policy, env, n_eval_episodes=a.episodes, deterministic=True, use_fused=True if a.fused else None,
                                 path_figures=True)
    sc = r.scalars(int(cfg.num_targets), has_duck=a.task in ("objlock", "combined"))
    ps = r.path_scalars(hz)
    print(f"Mean reward: {r.mean_reward:.2f} +/- {r.std_reward:.2f}")
    print(f"Mean episode length: {r.mean_ep_length:.1f} steps ({r.mean_ep_length / hz:.1f} s), {len(r.episode_lengths)} episodes")
    for k, v in sc.items():
        if "reach_rate" in k or "success" in k or "strike" in k:
            print(f"  {k.split('/', 1)[1]:24s} {v:.3f}")
    print("the flight:")
    units = {"airspeed_mean": "m/s", "altitude_mean": "m", "altitude_min": "m", "ang_vel_mean": "rad/s", "throttle_mean": "",
             "action_delta_mean": "per step", "path_length_mean": "m", "time_to_first_target_s": "s", "time_per_target_s": "s",
             "path_efficiency": "(chord / flown)", "miss_distance_mean": "m"}
    for name in evaluate.PATH_SCALARS:
        if "eval/" + name in ps:
            print(f"  {name:24s} {ps['eval/' + name]:10.3f} {units[name]}")
        else:
            print(f"  {name:24s} {'-':>10s}")
    env.venv.close()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "evaluation.json"), "w") as f:
            json.dump({"task": a.task, "checkpoint": a.checkpoint, "episodes": len(r.episode_lengths), "fused": bool(a.fused),
                       "episode_rewards": r.episode_rewards, "episode_lengths": r.episode_lengths,
                       **{k.split("/", 1)[1]: v for k, v in {**sc, **ps}.items()}}, f, indent=1)
    if a.trace_steps > 0:
        env = make()                           # a fresh env from the same seed
        tr = flight.fly(policy, env, a.trace_steps, use_fused=True if a.fused else None)
        env.venv.close()
        ended = int((tr.ended_at >= 0).sum())
        print(f"flight record: {a.trace_steps} vec-steps x {a.num_envs} envs, {ended} envs ended their first episode inside it")
        if a.out:
            cols = tr.layout.columns()
            np.savez(os.path.join(a.out, "trace.npz"), trace=tr.trace, start=tr.start, dt=tr.dt, ended_at=tr.ended_at,
                     column_names=np.array(list(cols)), column_ranges=np.array(list(cols.values()), dtype=np.int64))
        if a.plot:
            out = os.path.join(a.out or ".", "flight.png")
            if plot_flight(tr, out):
                print(f"wrote {out}")
    elif a.plot:
        print("--plot needs --trace_steps N: there is no flight record to draw")


if __name__ == "__main__":
    main()
