"""Wall time per vec-step of the high-level command task on one GPU.

    python tools/bench_highlevel.py [--legs step highlevel host act collect update e2e hz] [--envs 16 4096] [--steps 2000] [--warmup 100] [--repeats 5]
                                    [--controller_hz 30 120] [--out profiles/r10_highlevel_bench.jsonl]

Legs (one JSON line per leg, size and launch mode):
  step       the direct-command step kernel (FW_TASK_WAYPOINTS_DIRECT) beside the four-action waypoint kernel of the same build: the headline
             config (train_waypoints_v3_config: f64, no wind) at --step-envs envs, uniform actions in [-1, 1] from a pool of 64 tensors, auto-resets
             on.  Both run the same 8 physics ticks per step; the four-action kernel has the axis-aligned tick and the scenario hand-off.
  highlevel  a whole vec-step of HighLevelCmdVecEnv (fw_command_hl -> fw_collect_act_a -> fw_step) on raw actions drawn wide of the Box;
             the controller is a seeded MlpPolicy(21, 6) with random weights.
  host       the same vec-step composed on the host as tests/test_highlevel_gpu.py composes it: numpy conditioning and normalisation,
             the torch forward of the controller, fw_step of the base env (observation download and action upload every step).
  act        the act side of a collected vec-step at --envs envs, graph-replayed: fw_collect_act_hl (one launch) beside the three launches
             it replaces, each alone and as a chain -- fw_collect_act_a (a four-action commander at the same 30 observations stands in
             for the three-action one, which has no launch of its own), fw_command_hl, fw_collect_act_a (the six-action controller).
  collect    a collected vec-step of rollout.PPO on the high-level env (PPOConfig.fused_three_actions on: fw_collect_act_hl -> fw_step ->
             fw_collect_stats; off: the torch path), n_steps 1024, rollouts replayed as hipGraphs: wall time per vec-step.
  update     one minibatch of the learner at 30 observations, batch 256 (the reference's) and 64: fw_ppo_update_a3 beside
             fw_ppo_update_a's six- and four-action forms (device time from events, tools/bench_wide_learner.py) and the torch path.
  e2e        env-steps/s of examples/train_highlevel_cmd.py's configuration (16 envs, n_steps 1024, batch 256, 10 epochs) over
             --updates updates after a warm-up update, fused beside torch.
  hz         the controller rate (HighLevelCmdVecEnv(controller_hz=...)), every rate of --controller_hz in the same session, f64,
             graph-replayed: the vec-step (30: fw_command_hl -> fw_collect_act_a -> fw_step; 120: fw_command_hl -> fw_step_hl), the
             step launch alone (fw_step with low_action as it stands / fw_step_hl: fw_step_kernel_wd with SRC = WD_HELD / WD_CTL) and the fused collected vec-step of rollout.PPO
             (fw_collect_act_hl -> step_low -> fw_collect_stats).  Each line carries its ratio to the 30 Hz line of the same session.
Modes: "graph" replays a captured hipGraph of 64 vec-steps, "eager" launches them one by one.  A timed region is --steps vec-steps
between two device synchronisations; --repeats regions, the median is reported with the spread.  Under `rocprofv3 --kernel-trace
--stats` the per-kernel averages of the three launches come out by name (fw_command_hl_kernel, fw_policy_act_kernel, fw_step_kernel_wd).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["step", "highlevel", "host"],
                    choices=["step", "highlevel", "host", "act", "collect", "update", "e2e", "hz"])
    ap.add_argument("--controller_hz", type=int, nargs="+", default=[30, 120])
    ap.add_argument("--updates", type=int, default=2)
    ap.add_argument("--n-steps", type=int, default=1024)
    ap.add_argument("--envs", type=int, nargs="+", default=[16, 4096])
    ap.add_argument("--step-envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--host-steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--modes", nargs="+", default=["graph", "eager"], choices=["graph", "eager"])
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import pyflyt_drone_amd as P
    from pyflyt_drone_amd import config as K, rollout as R
    from pyflyt_drone_amd.highlevel import HighLevelCmdVecEnv, condition_command
    assert torch.cuda.is_available(), "bench_highlevel.py needs a HIP device"
    dev_name = torch.cuda.get_device_name(0)
    lines = []

    def emit(line):
        line["device"] = dev_name
        print(json.dumps(line), flush=True)
        lines.append(line)

    def timed(stepper, steps):
        stepper.run(a.warmup)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            stepper.run(steps)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / steps * 1e6)
        return {"us_per_vec_step": round(float(np.median(us)), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                "vec_steps": steps, "repeats": a.repeats, "warmup": a.warmup}

    def pool_of(n, width, scale=None, shift=None, dtype=torch.float64):
        g = torch.Generator(device="cpu").manual_seed(0)
        if scale is None:
            return [(torch.rand((n, width), generator=g, dtype=torch.float64) * 2 - 1).to(dtype).cuda() for _ in range(bench.POOL)]
        return [(torch.randn((n, width), generator=g, dtype=torch.float64) * scale + shift).to(dtype).cuda() for _ in range(bench.POOL)]

    def controller(seed=21):
        torch.manual_seed(seed)
        p = R.MlpPolicy(21, 6)
        with torch.no_grad():
            for q in p.parameters():
                q.add_(0.1 * torch.randn_like(q))
        g = np.random.default_rng(seed)
        return p, g.normal(0.0, 1.0, 21), g.uniform(0.5, 4.0, 21)

    hl_scale = torch.tensor([2.0 * math.pi, 300.0, 40.0], dtype=torch.float64)
    hl_shift = torch.tensor([0.0, 60.0, 15.0], dtype=torch.float64)

    if "step" in a.legs:
        n = a.step_envs
        for name, cfg, width in (("waypoints_step", K.train_waypoints_v3_config(), 4),
                                 ("direct_step", K.waypoints_direct_config(sparse_reward=True, num_targets=8, goal_reach_distance=4.0,
                                                                           angle_representation="euler"), 6)):
            for mode in a.modes:
                env = P.FixedwingVecEnv(cfg, n, seed=42)
                env.reset_tensor()
                st = bench.Stepper(env, pool_of(n, width), use_graph=(mode == "graph"))
                r = timed(st, a.steps)
                c = env.get_counters()
                emit({"leg": name, "envs": n, "mode": mode, "lanes_per_env": env.lanes_per_env, **r,
                      "env_steps_per_s": round(n / r["us_per_vec_step"] * 1e6), "resets": c["resets"], "fallbacks": c["fallbacks"],
                      "scenario_hits": c["scenario_hits"]})
                env.close()

    if "highlevel" in a.legs:
        for n in a.envs:
            for mode in a.modes:
                pol, mean, var = controller()
                env = HighLevelCmdVecEnv(n, pol, (mean, var), seed=42)
                env.reset_tensor()
                st = bench.Stepper(env, pool_of(n, 3, hl_scale, hl_shift), use_graph=(mode == "graph"))
                r = timed(st, a.steps)
                emit({"leg": "highlevel_vec_step", "envs": n, "mode": mode, "lanes_per_env": env.lanes_per_env, **r,
                      "env_steps_per_s": round(n / r["us_per_vec_step"] * 1e6), "resets": env.get_counters()["resets"],
                      "rejected": int(env.rejected.item())})
                env.close()

    if "host" in a.legs:
        for n in a.envs:
            pol, mean, var = controller()
            pol = pol.cuda()
            B = P.FixedwingWaypointsDirectVecEnv(n, flight_dome_size=200.0, angle_representation="euler", seed=42)
            B.reset_tensor()
            pool = [p.cpu().numpy() for p in pool_of(n, 3, hl_scale, hl_shift)]

            class Host:
                i = 0
                def run(self, k):
                    for _ in range(k):
                        raw = pool[self.i % len(pool)]; self.i += 1
                        low = np.concatenate([B.obs.cpu().numpy()[:, 0:18], condition_command(raw, 200.0)], axis=1)
                        norm = np.clip((low - mean) / np.sqrt(var + 1e-8), -10.0, 10.0).astype(np.float32)
                        with torch.no_grad():
                            act = pol.action_net(pol.pi_net(torch.from_numpy(norm).cuda())).clamp(-1.0, 1.0)
                        B.step_tensor(act.to(torch.float64))
            r = timed(Host(), a.host_steps)
            emit({"leg": "host_composition", "envs": n, "mode": "eager", **r, "env_steps_per_s": round(n / r["us_per_vec_step"] * 1e6)})
            B.close()

    def graph_us(fn, per=64):
        """us per call of fn() replayed from a hipGraph of `per` calls (median of --repeats regions of --steps calls)"""
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side); torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(per):
                fn()

        class Rep:
            def run(self, k):
                for _ in range(max(k // per, 1)):
                    g.replay()
        return timed(Rep(), max(a.steps // per, 1) * per)      # (whole replays: the calls timed are the calls counted)

    def hl_ppo(n, fused, n_steps, controller_hz=None):
        pol, mean, var = controller()
        venv = HighLevelCmdVecEnv(n, pol, (mean, var), seed=42, controller_hz=controller_hz)
        env = R.VecNormalizeDevice(venv, norm_obs=True, norm_reward=True, clip_obs=10.0, gamma=0.995)
        return R.PPO(env, R.PPOConfig(n_steps=n_steps, batch_size=256, n_epochs=10, learning_rate=3e-4, gamma=0.995, gae_lambda=0.95,
                                      clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, seed=123, fused_three_actions=fused))

    if "act" in a.legs:
        import ctypes as C
        from pyflyt_drone_amd import _lib
        L = _lib.lib()
        for n in a.envs:
            pol, mean, var = controller()
            env = HighLevelCmdVecEnv(n, pol, (mean, var), seed=42)
            env.reset_tensor()
            b = env.base
            f64 = int(env.torch_dtype == torch.float64)
            torch.manual_seed(3)
            flats = {}
            for A in (3, 4):
                f = R.FusedPpoUpdate(R.MlpPolicy(30, A).cuda(), None, 30); f.load_params_from_torch(); flats[A] = f.flat
            om, ov = torch.zeros(30, dtype=torch.float64, device="cuda"), torch.ones(30, dtype=torch.float64, device="cuda")
            rng = torch.tensor([5, 0], dtype=torch.int64, device="cuda")
            f32 = dict(dtype=torch.float32, device="cuda")
            oc, lp, val = torch.zeros((n, 30), **f32), torch.zeros(n, **f32), torch.zeros(n, **f32)
            ar = {A: torch.zeros((n, A), **f32) for A in (3, 4, 6)}
            ae4 = torch.zeros((n, 4), dtype=env.torch_dtype, device="cuda")
            st = lambda: b._stream()

            def fused():
                h = K.FwCollectHlArgs()
                h.params, h.rng, h.nets = flats[3].data_ptr(), rng.data_ptr(), 3
                h.obs_mean, h.obs_var, h.clip_obs, h.eps_obs = om.data_ptr(), ov.data_ptr(), 10.0, 1e-8
                h.obs_copy, h.act_raw, h.logp, h.value = oc.data_ptr(), ar[3].data_ptr(), lp.data_ptr(), val.data_ptr()
                env.collect_act_hl(h)

            def commander():
                _lib.check(L.fw_collect_act_a(R._p(flats[4]), R._p(b.obs), f64, n, 30, 4, R._p(om), R._p(ov), 10.0, 1e-8, 3, 0, R._p(rng), 0,
                                              R._p(oc), R._p(ar[4]), R._p(ae4), f64, R._p(lp), R._p(val), None, None, None, None, None, 0,
                                              0.0, 0.0, 0.0, None, None, st()))

            def command():
                _lib.check(L.fw_command_hl(b._h, R._p(ar[3]), 0, None, R._p(b.obs), R._p(env.low_obs), R._p(env.command), R._p(env.rejected),
                                           st()), b._h)

            def ctrl():
                _lib.check(L.fw_collect_act_a(R._p(env._flat), R._p(env.low_obs), f64, n, 21, 6, R._p(env.low_mean), R._p(env.low_var),
                                              env.clip_obs, env.epsilon, 1, 1, None, 0, None, R._p(ar[6]), R._p(env.low_action), f64, R._p(lp),
                                              None, None, None, None, None, None, 0, 0.0, 0.0, 0.0, None, None, st()))

            def chain():
                commander(); command(); ctrl()
            for name, fn in (("fw_collect_act_hl", fused), ("three_launch_chain", chain), ("fw_collect_act_a_commander4", commander),
                             ("fw_command_hl", command), ("fw_collect_act_a_controller6", ctrl)):
                r = graph_us(fn)
                r["us_per_call"] = r.pop("us_per_vec_step")
                emit({"leg": "act", "what": name, "envs": n, "mode": "graph", **r})
            env.close()

    if "collect" in a.legs:
        for n in a.envs:
            for fused in (True, False):
                ppo = hl_ppo(n, fused, a.n_steps)
                for _ in range(2):                       # eager, then the capture
                    ppo.collect_rollouts()
                torch.cuda.synchronize()
                us = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter(); ppo.collect_rollouts(); torch.cuda.synchronize()
                    us.append((time.perf_counter() - t0) / a.n_steps * 1e6)
                emit({"leg": "collect", "path": "fused_three_actions" if fused else "torch", "collect_fused": ppo._collect_fused, "envs": n,
                      "n_steps": a.n_steps, "graph": ppo._g_rollout is not None, "us_per_vec_step": round(float(np.median(us)), 2),
                      "us_min": round(min(us), 2), "us_max": round(max(us), 2), "repeats": a.repeats})
                ppo.env.venv.close()

    if "update" in a.legs:
        import ctypes as C
        from pyflyt_drone_amd import _lib
        import bench_wide_learner as W
        L = _lib.lib()

        def a3_us(B, n_mb, reps):
            g = torch.Generator(device="cuda"); g.manual_seed(1)
            S, D = n_mb * B, 30
            flat0 = torch.randn(L.fw_ppo_param_count_a3(D), device="cuda", generator=g) * 0.1
            ns = L.fw_ppo_moment_count_a3()
            obs, act = torch.randn((S, D), device="cuda", generator=g), torch.randn((S, 3), device="cuda", generator=g)
            lp, adv, ret = (torch.randn(S, device="cuda", generator=g) for _ in range(3))
            perm = torch.randperm(S, device="cuda", generator=g).to(torch.int32)
            ws = torch.zeros(int(L.fw_ppo_update_workspace_bytes_a3(n_mb, B, D)), dtype=torch.uint8, device="cuda")
            loss = torch.zeros(16, device="cuda")
            H = R._PpoHyper(lr=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, beta1=0.9, beta2=0.999, eps=1e-5,
                            adv_mean=0.0, adv_std=1.0, norm_adv=1, step0=0)
            times = []
            for r in range(reps + 1):
                flat, m, v = flat0.clone(), torch.zeros(ns, device="cuda"), torch.zeros(ns, device="cuda")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(L.fw_ppo_update_a3(*[R._p(x) for x in (flat, m, v, obs, act, lp, adv, ret, perm)], n_mb, B, D, C.byref(H), R._p(loss),
                                              R._p(ws), ws.numel(), None))
                e1.record(); torch.cuda.synchronize()
                stw = C.c_uint32(0)
                _lib.check(L.fw_ppo_update_status(R._p(ws), ws.numel(), C.byref(stw), None, None))
                assert stw.value == 0, stw.value
                if r:
                    times.append(e0.elapsed_time(e1) * 1e3 / n_mb)
            times.sort()
            return times[len(times) // 2], times
        for B in (256, 64):
            n_mb = 640
            for _ in range(2):                           # alternating: the two forms in the same session, twice
                med, all_ = a3_us(B, n_mb, a.repeats)
                emit({"leg": "update", "path": "fw_ppo_update_a3", "act_dim": 3, "obs_dim": 30, "batch": B, "n_mb": n_mb,
                      "us_per_minibatch": round(med, 3), "all_us": [round(x, 3) for x in all_]})
                for A in (6, 4):
                    med, all_ = W.fused_update_us(30, A, B, n_mb, a.repeats)
                    emit({"leg": "update", "path": "fw_ppo_update_a", "act_dim": A, "obs_dim": 30, "batch": B, "n_mb": n_mb,
                          "us_per_minibatch": round(med, 3), "all_us": [round(x, 3) for x in all_]})
            emit({"leg": "update", "path": "torch (autograd + Adam, hipGraph per minibatch)", "act_dim": 3, "obs_dim": 30, "batch": B, "n_mb": 64,
                  "us_per_minibatch": round(W.torch_update_us(30, 3, B, 64), 3)})

    if "e2e" in a.legs:
        for fused in (True, False):
            ppo = hl_ppo(16, fused, a.n_steps)
            ppo.collect_rollouts(); ppo.train()          # warm-up update (allocations, graph captures)
            ppo.collect_rollouts(); ppo.train()
            torch.cuda.synchronize()
            t_roll = t_upd = 0.0
            for _ in range(a.updates):
                t0 = time.perf_counter(); ppo.collect_rollouts(); torch.cuda.synchronize()
                t1 = time.perf_counter(); ppo.train(); torch.cuda.synchronize()
                t_roll += t1 - t0; t_upd += time.perf_counter() - t1
            steps = a.updates * a.n_steps * 16
            assert all(torch.isfinite(q).all() for q in ppo.policy.parameters())
            emit({"leg": "e2e", "path": "fused_three_actions" if fused else "torch", "envs": 16, "n_steps": a.n_steps, "updates": a.updates,
                  "env_steps_per_s": round(steps / (t_roll + t_upd)), "rollout_s_per_update": round(t_roll / a.updates, 4),
                  "update_s_per_update": round(t_upd / a.updates, 4), "minibatches_per_update": 10 * a.n_steps * 16 // 256})
            ppo.env.venv.close()

    if "hz" in a.legs:
        for n in a.envs:
            base = {}

            def emit_hz(what, hz, r, **more):
                key = "us_per_call" if "us_per_call" in r else "us_per_vec_step"
                if hz == 30:
                    base.setdefault(what, r[key])
                ratio = round(r[key] / base[what], 3) if what in base else None
                emit({"leg": "hz", "what": what, "controller_hz": hz, "envs": n, "dtype": "float64", "mode": "graph", **r,
                      "ratio_to_30hz": ratio, **more})
            for hz in a.controller_hz:
                pol, mean, var = controller()
                env = HighLevelCmdVecEnv(n, pol, (mean, var), seed=42, controller_hz=hz)
                env.reset_tensor()
                r = timed(bench.Stepper(env, pool_of(n, 3, hl_scale, hl_shift), use_graph=True), a.steps)
                emit_hz("vec_step", hz, r, lanes_per_env=env.lanes_per_env, launches=2 if env.controller_in_step else 3,
                        resets=env.get_counters()["resets"], rejected=int(env.rejected.item()))
                r = graph_us(env.step_low)
                r["us_per_call"] = r.pop("us_per_vec_step")
                emit_hz("step_launch_alone", hz, r, kernel="fw_step_kernel_wd<WD_CTL>" if env.controller_in_step else "fw_step_kernel_wd<WD_HELD>")
                env.close()
            for hz in a.controller_hz:
                ppo = hl_ppo(n, True, a.n_steps, controller_hz=hz)
                for _ in range(2):                       # eager, then the capture
                    ppo.collect_rollouts()
                torch.cuda.synchronize()
                us = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter(); ppo.collect_rollouts(); torch.cuda.synchronize()
                    us.append((time.perf_counter() - t0) / a.n_steps * 1e6)
                emit_hz("collected_vec_step_fused", hz, {"us_per_vec_step": round(float(np.median(us)), 2), "us_min": round(min(us), 2),
                                                         "us_max": round(max(us), 2), "repeats": a.repeats, "n_steps": a.n_steps},
                        collect_fused=ppo._collect_fused, graph=ppo._g_rollout is not None)
                ppo.env.venv.close()

    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
