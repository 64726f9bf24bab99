"""Dev tool: what the learner's diagnostics mode costs, and that the plain entry points did not move.

  diag     device time per minibatch of fw_ppo_update_diag against the plain entry point of the width (fw_ppo_update_a / _a3) from the
           SAME library, at the three reference shapes (obs 28 / batch 128 / 4 actions, 21 / 64 / 6, 30 / 256 / 3): the two arms
           alternate in one process, --reps regions each (one region = one launch of --n_mb minibatches, timed with events), medians
  kl       device time per minibatch of fw_ppo_update_kl (PPOConfig.target_kl) with a limit that never triggers -- without its
           diagnostics buffer and with it, as the learner calls it -- against the plain and the diagnostics form from the same
           library, same shapes: four arms alternating in one process, medians
  parent   the plain entry points of this build against the parent commit's library (--parent_lib, or FWSIM_LIB), same shapes, arms
           alternating in one process; a second copy of the parent's library is a third arm, so the A/A spread of the parent against
           itself comes from the same call
  e2e      env-steps/s of examples/train_fixedwing_waypoints.py with and without --diagnostics over --total_timesteps steps each
           (child processes, one at a time, the two arms in turn --e2e_repeats times; evaluations and checkpoints included, as a user
           runs it), and a closing line with the medians

    python tools/bench_learner_diag.py --what diag --out profiles/r13_learner_diag_bench.jsonl
    python tools/bench_learner_diag.py --what kl --out profiles/r33_ppo_target_kl.jsonl
    python tools/bench_learner_diag.py --what parent --parent_lib /path/to/parent/libfwsim_hip.so --out profiles/r13_learner_diag_bench.jsonl
    python tools/bench_learner_diag.py --what e2e --out profiles/r13_learner_diag_bench.jsonl
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((28, 128, 4), (21, 64, 6), (30, 256, 3))      # (obs_dim, batch, act_dim): waypoints, low-level control, high-level command


class _Hyper(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("lr", "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "beta1", "beta2", "eps",
                                         "adv_mean", "adv_std")] + [("norm_adv", C.c_int32), ("step0", C.c_int32)]


def load(path):
    """A library by path, with the argument types of the learner entry points this tool calls (several builds side by side)."""
    L = C.CDLL(os.path.abspath(path))
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    for name, res, args in (("fw_ppo_param_count_a", i32, [i32, i32]), ("fw_ppo_param_count_a3", i32, [i32]),
                            ("fw_ppo_moment_count_a", i32, [i32]), ("fw_ppo_moment_count_a3", i32, []),
                            ("fw_ppo_update_workspace_bytes_a", i64, [i32, i32, i32, i32]), ("fw_ppo_update_workspace_bytes_a3", i64, [i32, i32, i32]),
                            ("fw_ppo_update_a", i32, [vp] * 9 + [i32, i32, i32, i32, vp, vp, vp, i64, vp]),
                            ("fw_ppo_update_a3", i32, [vp] * 9 + [i32, i32, i32, vp, vp, vp, i64, vp]),
                            ("fw_ppo_update_status", i32, [vp, i64, vp, vp, vp]),
                            ("fw_ppo_diag_floats", i64, [i32]),
                            ("fw_ppo_update_diag", i32, [vp] * 9 + [i32, i32, i32, i32, vp, vp, vp, i64, vp, vp, i64]),
                            ("fw_ppo_update_kl", i32, [vp] * 9 + [i32, i32, i32, i32, vp, vp, vp, i64, vp, vp, i64, C.c_float, vp])):
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    L.fw_last_error.restype = C.c_char_p; L.fw_last_error.argtypes = [vp]
    return L


class Problem:
    """The buffers of one shape: n_mb minibatches of fresh samples, a parameter image and zeroed moments per launch."""

    def __init__(self, L, D, B, A, n_mb):
        import torch
        self.torch, self.D, self.B, self.A, self.n_mb = torch, D, B, A, n_mb
        g = torch.Generator(device="cuda"); g.manual_seed(1)
        S = n_mb * B
        n_par = L.fw_ppo_param_count_a3(D) if A == 3 else L.fw_ppo_param_count_a(D, A)
        self.ns = L.fw_ppo_moment_count_a3() if A == 3 else L.fw_ppo_moment_count_a(A)
        self.flat0 = torch.randn(n_par, device="cuda", generator=g) * 0.1
        self.obs, self.act = torch.randn((S, D), device="cuda", generator=g), torch.randn((S, A), device="cuda", generator=g)
        self.lp, self.adv, self.ret = (torch.randn(S, device="cuda", generator=g) for _ in range(3))
        self.perm = torch.randperm(S, device="cuda", generator=g).to(torch.int32)
        wsb = L.fw_ppo_update_workspace_bytes_a3(n_mb, B, D) if A == 3 else L.fw_ppo_update_workspace_bytes_a(n_mb, B, D, A)
        self.ws = torch.zeros(int(wsb), dtype=torch.uint8, device="cuda")
        self.loss = torch.zeros(16, device="cuda")
        self.H = _Hyper(lr=3e-4, clip_range=0.2, ent_coef=0.001, vf_coef=0.5, max_grad_norm=0.5, beta1=0.9, beta2=0.999, eps=1e-5,
                        adv_mean=0.0, adv_std=1.0, norm_adv=1, step0=0)
        self.diag = None

    def region(self, L, diag):
        """One timed launch; returns (us per minibatch, parameter image after it).  diag: False (plain), True (fw_ppo_update_diag),
        "kl" (fw_ppo_update_kl with a limit no KL reaches, its diagnostics buffer left out), "kl_diag" (the same with the buffer passed:
        what FusedPpoUpdate.run does under PPOConfig.target_kl)."""
        torch = self.torch
        p = lambda t: C.c_void_p(t.data_ptr())
        flat, m, v = self.flat0.clone(), torch.zeros(self.ns, device="cuda"), torch.zeros(self.ns, device="cuda")
        head = [p(x) for x in (flat, m, v, self.obs, self.act, self.lp, self.adv, self.ret, self.perm)]
        tail = [C.byref(self.H), p(self.loss), p(self.ws), self.ws.numel(), None]
        if diag in (True, "kl_diag") and self.diag is None:
            self.diag = torch.zeros(int(L.fw_ppo_diag_floats(self.n_mb)), device="cuda")
        stepped = torch.zeros(1, dtype=torch.int32, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        if diag == "kl":
            rc = L.fw_ppo_update_kl(*head, self.n_mb, self.B, self.D, self.A, *tail, None, 0, 1e30, p(stepped))
        elif diag == "kl_diag":
            rc = L.fw_ppo_update_kl(*head, self.n_mb, self.B, self.D, self.A, *tail, p(self.diag), self.diag.numel(), 1e30, p(stepped))
        elif diag:
            rc = L.fw_ppo_update_diag(*head, self.n_mb, self.B, self.D, self.A, *tail, p(self.diag), self.diag.numel())
        elif self.A == 3:
            rc = L.fw_ppo_update_a3(*head, self.n_mb, self.B, self.D, *tail)
        else:
            rc = L.fw_ppo_update_a(*head, self.n_mb, self.B, self.D, self.A, *tail)
        e1.record(); torch.cuda.synchronize()
        if rc != 0:
            raise RuntimeError(L.fw_last_error(None).decode())
        st = C.c_uint32(0)
        L.fw_ppo_update_status(p(self.ws), self.ws.numel(), C.byref(st), None, None)
        if st.value:
            raise RuntimeError(f"status word {st.value}")
        if diag in ("kl", "kl_diag") and int(stepped.item()) != self.n_mb:
            raise RuntimeError(f"the limit triggered: {int(stepped.item())} of {self.n_mb} minibatches stepped")
        return e0.elapsed_time(e1) * 1e3 / self.n_mb, flat


def alternate(prob, arms, reps):
    """arms: [(name, library, diag)].  One warm-up region per arm, then reps rounds over the arms in turn; medians and all figures."""
    times = {name: [] for name, _, _ in arms}
    images = {}
    for r in range(reps + 1):
        for name, L, diag in arms:
            us, flat = prob.region(L, diag)
            images[name] = flat
            if r:
                times[name].append(us)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return med, times, images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("diag", "kl", "parent", "e2e"), default="diag")
    ap.add_argument("--n_mb", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent_lib", type=str, default=os.environ.get("FWSIM_LIB"))
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--total_timesteps", type=int, default=120 * 65536)
    ap.add_argument("--e2e_repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert a.reps >= 5, "medians of at least 5 regions"
    rows = []
    here = os.path.join(ROOT, "pyflyt-drone_amd", "csrc", "libfwsim_hip.so")
    if a.what == "e2e":
        # (child processes, started before this process has touched the device -- it never does in this mode)
        for diag in [False, True] * a.e2e_repeats:      # (the two arms in turn: the spread between repeats of one arm is in the file)
            out = tempfile.mkdtemp(prefix="fw_diag_e2e_")
            cmd = [sys.executable, os.path.join(ROOT, "examples", "train_fixedwing_waypoints.py"), "--num_envs", str(a.num_envs),
                   "--total_timesteps", str(a.total_timesteps), "--out", out] + (["--diagnostics"] if diag else [])
            t0 = time.perf_counter()
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            wall = time.perf_counter() - t0
            shutil.rmtree(out, ignore_errors=True)
            if p.returncode != 0:
                raise RuntimeError(p.stderr[-2000:])
            lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{") and "timesteps" in l]
            last = lines[-1]
            rows.append({"what": "e2e", "example": "train_fixedwing_waypoints.py", "diagnostics": diag, "num_envs": a.num_envs,
                         "total_timesteps": a.total_timesteps, "env_steps_per_s_last_line": last["fps"], "timesteps_last_line": last["timesteps"],
                         "wall_s_process": round(wall, 2), "update_lines": len(lines),
                         "every_line_has_train_scalars": all(all(k in l for k in ("train/approx_kl", "train/clip_fraction", "train/explained_variance")) for l in lines),
                         "last_line": last})
        med = lambda d: sorted(r["env_steps_per_s_last_line"] for r in rows if r["diagnostics"] == d)[a.e2e_repeats // 2]
        rows.append({"what": "e2e_summary", "repeats_per_arm": a.e2e_repeats, "median_env_steps_per_s_plain": med(False),
                     "median_env_steps_per_s_diagnostics": med(True), "diagnostics_over_plain": round(med(True) / med(False), 4),
                     "all_plain": [r["env_steps_per_s_last_line"] for r in rows if r["diagnostics"] is False],
                     "all_diagnostics": [r["env_steps_per_s_last_line"] for r in rows if r["diagnostics"] is True]})
    else:
        import torch
        dev = torch.cuda.get_device_name(0)
        this = load(here)
        if a.what == "diag":
            for D, B, A in SHAPES:
                prob = Problem(this, D, B, A, a.n_mb)
                med, times, images = alternate(prob, [("plain", this, False), ("diag", this, True)], a.reps)
                rows.append({"what": "diag", "obs_dim": D, "batch": B, "act_dim": A, "n_mb": a.n_mb, "regions": a.reps,
                             "plain_us_per_minibatch": round(med["plain"], 3), "diag_us_per_minibatch": round(med["diag"], 3),
                             "diag_over_plain": round(med["diag"] / med["plain"], 4),
                             "plain_all_us": [round(x, 3) for x in times["plain"]], "diag_all_us": [round(x, 3) for x in times["diag"]],
                             "same_parameters": bool(torch.equal(images["plain"], images["diag"])), "device": dev})
        elif a.what == "kl":
            for D, B, A in SHAPES:
                prob = Problem(this, D, B, A, a.n_mb)
                med, times, images = alternate(prob, [("plain", this, False), ("diag", this, True), ("kl", this, "kl"), ("kl_diag", this, "kl_diag")], a.reps)
                rows.append({"what": "kl", "obs_dim": D, "batch": B, "act_dim": A, "n_mb": a.n_mb, "regions": a.reps,
                             "plain_us_per_minibatch": round(med["plain"], 3), "diag_us_per_minibatch": round(med["diag"], 3),
                             "kl_us_per_minibatch": round(med["kl"], 3), "kl_over_plain": round(med["kl"] / med["plain"], 4),
                             "kl_with_diag_buffer_us_per_minibatch": round(med["kl_diag"], 3),      # (what the learner runs)
                             "kl_with_diag_buffer_over_plain": round(med["kl_diag"] / med["plain"], 4),
                             "kl_with_diag_buffer_over_diag": round(med["kl_diag"] / med["diag"], 4),
                             "all_us": {k: [round(x, 3) for x in v] for k, v in times.items()},
                             "same_parameters": bool(torch.equal(images["plain"], images["kl"]) and torch.equal(images["diag"], images["kl"]) and torch.equal(images["kl_diag"], images["kl"])),
                             "device": dev})
        else:
            if not a.parent_lib:
                raise SystemExit("--parent_lib (or FWSIM_LIB): the parent commit's libfwsim_hip.so")
            tmp = tempfile.mkdtemp(prefix="fw_parent_copy_")
            twin = os.path.join(tmp, "libfwsim_parent_twin.so")
            shutil.copy(a.parent_lib, twin)          # (another path: loaded as a module of its own)
            parent, parent2 = load(a.parent_lib), load(twin)
            for D, B, A in SHAPES:
                prob = Problem(this, D, B, A, a.n_mb)
                med, times, images = alternate(prob, [("parent", parent, False), ("this", this, False), ("parent_twin", parent2, False)], a.reps)
                aa = abs(med["parent_twin"] - med["parent"]) / med["parent"]
                ab = (med["this"] - med["parent"]) / med["parent"]
                rows.append({"what": "plain_vs_parent", "obs_dim": D, "batch": B, "act_dim": A, "n_mb": a.n_mb, "regions": a.reps,
                             "parent_us_per_minibatch": round(med["parent"], 3), "this_us_per_minibatch": round(med["this"], 3),
                             "parent_twin_us_per_minibatch": round(med["parent_twin"], 3),
                             "this_over_parent_minus_1": round(ab, 5), "aa_spread_parent_vs_itself": round(aa, 5),
                             "inside_aa_spread": bool(abs(ab) <= aa),
                             "region_spread_parent": round((max(times["parent"]) - min(times["parent"])) / med["parent"], 5),
                             "all_us": {k: [round(x, 3) for x in v] for k, v in times.items()},
                             "same_parameters": bool(torch.equal(images["parent"], images["this"])), "device": dev})
            shutil.rmtree(tmp, ignore_errors=True)
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
