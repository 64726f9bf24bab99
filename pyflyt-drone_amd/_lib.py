"""ctypes binding of ``csrc/libfwsim_hip.so`` (the C ABI of ``include/fwsim.h``).

There is no CPU fallback: if the shared library is missing, or no HIP device
is present, env construction raises.  Building is done by
``__graft_entry__.build()`` / :func:`build` with ``hipcc --offload-arch=gfx950``.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import torch

from . import config as K

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("FWSIM_LIB") or os.path.join(CSRC, "libfwsim_hip.so")      # FWSIM_LIB: A/B builds of the same ABI (dev tools)
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

EXPORTS = (
    "fw_sizeof_config", "fw_abi_version", "fw_state_dim", "fw_obs_dim", "fw_act_dim", "fw_validate_config", "fw_create", "fw_reset",
    "fw_step", "fw_seed", "fw_get_state", "fw_set_state", "fw_get_counters", "fw_observe", "fw_render", "fw_num_envs", "fw_lanes_per_env", "fw_capture_wave", "fw_axis_aligned", "fw_aux_wave", "fw_step_shape", "fw_obs_wave", "fw_last_error",
    "fw_destroy", "fw_gae", "fw_eval_track", "fw_eval_track_ll", "fw_command_ll", "fw_command_hl", "fw_trace_ll", "fw_normalize_obs", "fw_normalize_obs_workspace_bytes", "fw_ppo_update_workspace_bytes", "fw_ppo_param_count", "fw_ppo_moment_count", "fw_ppo_moment_map", "fw_ppo_update", "fw_policy_act", "fw_policy_terminal_value", "fw_rollout_post", "fw_collect_act", "fw_collect_stats", "fw_collect_stats_workspace_bytes", "fw_collect_step", "fw_collect_finish", "fw_collect_step_workspace_bytes", "fw_collect_workspace_init", "fw_collect_close", "fw_collect_status", "fw_ppo_update_status",
    "fw_ppo_param_count_a", "fw_ppo_moment_count_a", "fw_ppo_moment_map_a", "fw_ppo_update_workspace_bytes_a", "fw_ppo_update_a",
    "fw_policy_act_a", "fw_collect_act_a",
    "fw_ppo_param_count_a3", "fw_ppo_moment_count_a3", "fw_ppo_moment_map_a3", "fw_ppo_update_workspace_bytes_a3", "fw_ppo_update_a3",
    "fw_collect_act_hl", "fw_sizeof_collect_hl_args", "fw_eval_track_hl", "fw_trace_hl",
    "fw_ppo_diag_floats", "fw_ppo_update_diag", "fw_ppo_update_kl",
    "fw_episode_state_bytes", "fw_episode_fold",
    "fw_episode_fold_span", "fw_episode_fold_workspace_bytes", "fw_episode_fold_wide",
    "fw_trace_rows", "fw_eval_track_wp",
    "fw_step_hl", "fw_sizeof_step_hl_args", "fw_controller_forward",
    "fw_probe",
    "fw_sizeof_sac_hyper", "fw_sac_param_count", "fw_sac_update_workspace_bytes", "fw_sac_act", "fw_replay_store", "fw_replay_sample",
    "fw_sac_noise", "fw_sac_update",
    "fw_replay_mark_ends", "fw_replay_sample_nstep",
    "fw_sizeof_her_task", "fw_replay_sample_her", "fw_her_reward",
    "fw_replay_per_mark_new", "fw_replay_per_rebuild", "fw_replay_sample_per", "fw_replay_per_update", "fw_sac_update_weighted",
    "fw_sac_act_norm", "fw_replay_normalize",
    "fw_sizeof_td3_hyper", "fw_td3_param_count", "fw_td3_update_workspace_bytes", "fw_td3_act", "fw_td3_update",
)


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp"))]
    deps = srcs + [os.path.join(INCLUDE, "fwsim.h")]
    stale = (not os.path.exists(LIB_PATH)) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(p) for p in deps)
    if force or stale:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        # -save-temps (into a scratch directory): the device assembly of exactly this build is checked for a register-allocator
        # hazard that silently corrupts lanes (tools/check_isa.py) -- a build that has it must not ship
        import shutil
        import tempfile
        tmp = tempfile.mkdtemp(prefix="fwsim_build_")
        try:
            cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-save-temps",
                   "-o", LIB_PATH, os.path.join(CSRC, "fwsim.hip")]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd, cwd=tmp)
            asm = [f for f in os.listdir(tmp) if f.endswith(".s") and "gfx950" in f]
            if not asm:
                raise RuntimeError("hipcc left no gfx950 assembly to check")
            hits = check_isa(open(os.path.join(tmp, asm[0])).read())
            if hits:
                os.remove(LIB_PATH)
                raise RuntimeError("ISA check failed (tools/check_isa.py: spill stores before the exec restore of a join block, "
                                   "or a last-block-done ticket that can overtake its partial sums): "
                                   + "; ".join(f"{n[:60]} {lab}" for n, lab, _ in hits[:6]))
            if verbose:
                print("ISA check: no spill store precedes the exec restore of its block; ticket atomics sit behind a vmcnt(0) wait")
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return LIB_PATH


def check_isa(text: str):
    """tools/check_isa.py, importable from the package's own build step."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fw_check_isa", os.path.join(os.path.dirname(CSRC.rstrip(os.sep)), "..", "tools", "check_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.scan(text) + mod.scan_ticket(text)


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
                "pyflyt_drone_amd has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        vp, i32, u64, i64 = C.c_void_p, C.c_int32, C.c_uint64, C.c_int64
        L.fw_sizeof_config.restype = i32; L.fw_sizeof_config.argtypes = []
        L.fw_abi_version.restype = i32; L.fw_abi_version.argtypes = []
        L.fw_state_dim.restype = i32; L.fw_state_dim.argtypes = []
        L.fw_obs_dim.restype = i32; L.fw_obs_dim.argtypes = [vp]
        L.fw_act_dim.restype = i32; L.fw_act_dim.argtypes = [vp]
        L.fw_validate_config.restype = i32; L.fw_validate_config.argtypes = [vp, C.c_char_p, i32]
        L.fw_create.restype = i32; L.fw_create.argtypes = [vp, i32, i32, u64, i64, C.POINTER(vp)]
        L.fw_reset.restype = i32; L.fw_reset.argtypes = [vp, vp, vp, vp, vp]
        L.fw_step.restype = i32; L.fw_step.argtypes = [vp] * 9
        L.fw_observe.restype = i32; L.fw_observe.argtypes = [vp, vp, vp]
        L.fw_seed.restype = i32; L.fw_seed.argtypes = [vp, u64]
        L.fw_get_state.restype = i32; L.fw_get_state.argtypes = [vp, vp]
        L.fw_set_state.restype = i32; L.fw_set_state.argtypes = [vp, vp]
        L.fw_get_counters.restype = i32; L.fw_get_counters.argtypes = [vp, vp]
        L.fw_num_envs.restype = i32; L.fw_num_envs.argtypes = [vp]
        L.fw_lanes_per_env.restype = i32; L.fw_lanes_per_env.argtypes = [vp]
        L.fw_capture_wave.restype = i32; L.fw_capture_wave.argtypes = [vp]
        L.fw_axis_aligned.restype = i32; L.fw_axis_aligned.argtypes = [vp]
        if hasattr(L, "fw_aux_wave"):          # (an A/B library of an older commit predates it; build() insists on it)
            L.fw_aux_wave.restype = i32; L.fw_aux_wave.argtypes = [vp]
        if hasattr(L, "fw_step_shape"):        # (an A/B library of an older commit predates it; build() insists on it)
            L.fw_step_shape.restype = i32; L.fw_step_shape.argtypes = [vp]
        if hasattr(L, "fw_obs_wave"):          # (an A/B library of an older commit predates it; build() insists on it)
            L.fw_obs_wave.restype = i32; L.fw_obs_wave.argtypes = [vp]
        L.fw_render.restype = i32; L.fw_render.argtypes = [vp, i32, vp, vp]
        L.fw_last_error.restype = C.c_char_p; L.fw_last_error.argtypes = [vp]
        L.fw_destroy.restype = i32; L.fw_destroy.argtypes = [vp]
        L.fw_gae.restype = i32
        L.fw_eval_track.restype = i32
        L.fw_eval_track.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]
        if hasattr(L, "fw_episode_fold"):      # (an A/B library of an older commit -- FWSIM_LIB, tools/bench_lib.py -- predates the pair; build() insists on it)
            L.fw_episode_state_bytes.restype = i64; L.fw_episode_state_bytes.argtypes = [i32, i32]
            L.fw_episode_fold.restype = i32
            L.fw_episode_fold.argtypes = [vp, i32, vp, vp, vp, i32, vp, i32, i32, vp]
        if hasattr(L, "fw_episode_fold_wide"):  # the multi-workgroup form (an A/B library of an older commit predates it; build() insists on it)
            L.fw_episode_fold_span.restype = i32; L.fw_episode_fold_span.argtypes = []
            L.fw_episode_fold_workspace_bytes.restype = i64; L.fw_episode_fold_workspace_bytes.argtypes = [i32]
            L.fw_episode_fold_wide.restype = i32
            L.fw_episode_fold_wide.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, vp]
        L.fw_eval_track_ll.restype = i32
        L.fw_eval_track_ll.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]
        L.fw_eval_track_hl.restype = i32
        L.fw_eval_track_hl.argtypes = ([vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, i32, C.c_double, C.c_double] + [vp] * 12 + [i32, i32, vp])
        L.fw_trace_hl.restype = i32
        L.fw_trace_hl.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, vp]
        if hasattr(L, "fw_trace_rows"):        # (an A/B library of an older commit predates the pair; build() insists on it)
            L.fw_trace_rows.restype = i32
            L.fw_trace_rows.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp]
            L.fw_eval_track_wp.restype = i32
            L.fw_eval_track_wp.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32] + [vp] * 12 + [i32, i32, vp]
        L.fw_command_ll.restype = i32
        L.fw_command_ll.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
        L.fw_command_hl.restype = i32
        L.fw_command_hl.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
        L.fw_trace_ll.restype = i32
        L.fw_trace_ll.argtypes = [vp, vp, vp, vp, i32, i32, vp, i32, vp, vp]
        L.fw_gae.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, vp]
        L.fw_normalize_obs.restype = i32
        L.fw_normalize_obs.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, C.c_float, C.c_float, vp, vp, vp, vp]
        L.fw_normalize_obs_workspace_bytes.restype = i64; L.fw_normalize_obs_workspace_bytes.argtypes = [i32]
        L.fw_ppo_update_workspace_bytes.restype = i64; L.fw_ppo_update_workspace_bytes.argtypes = [i32, i32, i32]
        L.fw_ppo_param_count.restype = i32; L.fw_ppo_param_count.argtypes = [i32]
        L.fw_ppo_moment_count.restype = i32; L.fw_ppo_moment_count.argtypes = []
        L.fw_ppo_moment_map.restype = i32; L.fw_ppo_moment_map.argtypes = [i32, vp]
        L.fw_ppo_update.restype = i32
        L.fw_ppo_update.argtypes = [vp] * 9 + [i32, i32, i32, vp, vp, vp, i64, vp]
        L.fw_policy_act.restype = i32
        L.fw_policy_act.argtypes = [vp, vp, i32, i32, i32, i32, vp, i64, vp, vp, vp, i32, vp, vp, vp]
        L.fw_policy_terminal_value.restype = i32
        L.fw_policy_terminal_value.argtypes = [vp, vp, i32, i32, i32, vp, vp, C.c_float, C.c_float, vp, vp, vp, vp]
        f32, f64 = C.c_float, C.c_double
        L.fw_collect_act.restype = i32
        L.fw_collect_act.argtypes = [vp, vp, i32, i32, i32, vp, vp, f32, f32, i32, i32, vp, i64, vp, vp, vp, i32, vp, vp,
                                     vp, vp, vp, vp, vp, i32, f32, f32, f32, vp, vp, vp]
        L.fw_collect_stats_workspace_bytes.restype = i64; L.fw_collect_stats_workspace_bytes.argtypes = [i32]
        L.fw_collect_stats.restype = i32
        L.fw_collect_stats.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, f64, vp, vp, vp, vp, vp]
        L.fw_collect_step_workspace_bytes.restype = i64; L.fw_collect_step_workspace_bytes.argtypes = [vp]
        L.fw_collect_step.restype = i32; L.fw_collect_step.argtypes = [vp, vp, vp]
        L.fw_collect_finish.restype = i32; L.fw_collect_finish.argtypes = [vp, vp, vp]
        L.fw_collect_workspace_init.restype = i32; L.fw_collect_workspace_init.argtypes = [vp, vp, i64, vp]
        L.fw_collect_close.restype = i32; L.fw_collect_close.argtypes = [vp, vp, vp, vp]
        L.fw_collect_status.restype = i32; L.fw_collect_status.argtypes = [vp, vp, i64, vp, vp]
        L.fw_ppo_update_status.restype = i32; L.fw_ppo_update_status.argtypes = [vp, i64, vp, vp, vp]
        # the *_a forms: the same with the action width (4 or 6) after obs_dim
        L.fw_ppo_param_count_a.restype = i32; L.fw_ppo_param_count_a.argtypes = [i32, i32]
        L.fw_ppo_moment_count_a.restype = i32; L.fw_ppo_moment_count_a.argtypes = [i32]
        L.fw_ppo_moment_map_a.restype = i32; L.fw_ppo_moment_map_a.argtypes = [i32, i32, vp]
        L.fw_ppo_update_workspace_bytes_a.restype = i64; L.fw_ppo_update_workspace_bytes_a.argtypes = [i32, i32, i32, i32]
        L.fw_ppo_update_a.restype = i32
        L.fw_ppo_update_a.argtypes = [vp] * 9 + [i32, i32, i32, i32, vp, vp, vp, i64, vp]
        # the three-action learner (the high-level command task): the argument lists of the four-action entry points
        L.fw_ppo_param_count_a3.restype = i32; L.fw_ppo_param_count_a3.argtypes = [i32]
        L.fw_ppo_moment_count_a3.restype = i32; L.fw_ppo_moment_count_a3.argtypes = []
        L.fw_ppo_moment_map_a3.restype = i32; L.fw_ppo_moment_map_a3.argtypes = [i32, vp]
        L.fw_ppo_update_workspace_bytes_a3.restype = i64; L.fw_ppo_update_workspace_bytes_a3.argtypes = [i32, i32, i32]
        L.fw_ppo_update_a3.restype = i32
        L.fw_ppo_update_a3.argtypes = [vp] * 9 + [i32, i32, i32, vp, vp, vp, i64, vp]
        # the diagnostics form: the *_a argument list (act_dim 3, 4 or 6), then the diagnostics buffer and its size in floats
        L.fw_ppo_diag_floats.restype = i64; L.fw_ppo_diag_floats.argtypes = [i32]
        L.fw_ppo_update_diag.restype = i32
        L.fw_ppo_update_diag.argtypes = [vp] * 9 + [i32, i32, i32, i32, vp, vp, vp, i64, vp, vp, i64]
        if hasattr(L, "fw_ppo_update_kl"):     # target_kl early stopping (an A/B library of an older commit predates it; build() insists on it)
            # fw_ppo_update_diag's list (diag may be None), then target_kl and the device int32 the stepped count goes to
            L.fw_ppo_update_kl.restype = i32
            L.fw_ppo_update_kl.argtypes = [vp] * 9 + [i32, i32, i32, i32, vp, vp, vp, i64, vp, vp, i64, C.c_float, vp]
        L.fw_collect_act_hl.restype = i32; L.fw_collect_act_hl.argtypes = [vp, vp, vp]
        L.fw_sizeof_collect_hl_args.restype = i32; L.fw_sizeof_collect_hl_args.argtypes = []
        if hasattr(L, "fw_step_hl"):           # (an A/B library of an older commit predates the pair; build() insists on it)
            L.fw_step_hl.restype = i32; L.fw_step_hl.argtypes = [vp, vp, vp]
            L.fw_sizeof_step_hl_args.restype = i32; L.fw_sizeof_step_hl_args.argtypes = []
            L.fw_controller_forward.restype = i32
            L.fw_controller_forward.argtypes = [vp, vp, i32, i32, vp, vp, f32, f32, vp, i32, vp]
            if L.fw_sizeof_step_hl_args() != C.sizeof(K.FwStepHlArgs):
                raise RuntimeError("fw_step_hl_args layout mismatch between include/fwsim.h and config.FwStepHlArgs")
        if hasattr(L, "fw_probe"):             # the test hook (an A/B library of an older commit predates it; build() insists on it)
            L.fw_probe.restype = i32; L.fw_probe.argtypes = [vp, i32, i32, vp, i32, vp, i32, i32, vp]
        if hasattr(L, "fw_sac_update"):        # the off-policy learner (an A/B library of an older commit predates it; build() insists on it)
            L.fw_sizeof_sac_hyper.restype = i32; L.fw_sizeof_sac_hyper.argtypes = []
            L.fw_sac_param_count.restype = i32; L.fw_sac_param_count.argtypes = [i32, i32, i32]
            L.fw_sac_update_workspace_bytes.restype = i64; L.fw_sac_update_workspace_bytes.argtypes = [i32, i32, i32, i32]
            L.fw_sac_act.restype = i32
            L.fw_sac_act.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, u64, i64, vp, vp, vp, vp, vp, vp, vp]
            L.fw_replay_store.restype = i32
            L.fw_replay_store.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
            L.fw_replay_sample.restype = i32; L.fw_replay_sample.argtypes = [vp, i64, vp, u64, i32, i32, vp, vp, vp]
            L.fw_sac_noise.restype = i32; L.fw_sac_noise.argtypes = [u64, vp, i32, i32, vp, vp]
            L.fw_sac_update.restype = i32; L.fw_sac_update.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp]
        if hasattr(L, "fw_replay_sample_nstep"):   # n-step returns (an A/B library of an older commit predates the pair; build() insists on it)
            L.fw_replay_mark_ends.restype = i32; L.fw_replay_mark_ends.argtypes = [vp, i64, vp, vp, vp, i32, vp]
            L.fw_replay_sample_nstep.restype = i32
            L.fw_replay_sample_nstep.argtypes = [vp, i64, vp, u64, i32, i32, vp, vp, vp, i32, i32, i32, C.c_float, vp, vp]
        if hasattr(L, "fw_replay_sample_her"):     # hindsight relabelling (an A/B library of an older commit predates the three; build() insists on them)
            L.fw_sizeof_her_task.restype = i32; L.fw_sizeof_her_task.argtypes = []
            L.fw_replay_sample_her.restype = i32
            L.fw_replay_sample_her.argtypes = [vp, i64, vp, u64, i32, i32, vp, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp]
            L.fw_her_reward.restype = i32; L.fw_her_reward.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
        if hasattr(L, "fw_replay_sample_per"):     # prioritized replay (an A/B library of an older commit predates the five; build() insists on them)
            f32 = C.c_float
            L.fw_replay_per_mark_new.restype = i32; L.fw_replay_per_mark_new.argtypes = [vp, i64, vp, vp, i32, vp]
            L.fw_replay_per_rebuild.restype = i32; L.fw_replay_per_rebuild.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp]
            L.fw_replay_sample_per.restype = i32
            L.fw_replay_sample_per.argtypes = [vp, i64, vp, u64, i32, i32, vp, vp, vp, vp, vp, vp, vp, f32, i64, vp]
            L.fw_replay_per_update.restype = i32; L.fw_replay_per_update.argtypes = [vp, i64, vp, vp, i32, f32, f32, vp, vp]
            L.fw_sac_update_weighted.restype = i32
            L.fw_sac_update_weighted.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp]
        if hasattr(L, "fw_replay_normalize"):      # running normalisation for SAC (an A/B library of an older commit predates the pair; build() insists on it)
            f32 = C.c_float
            L.fw_sac_act_norm.restype = i32
            L.fw_sac_act_norm.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, u64, i64, vp, vp, vp, vp, vp, vp, vp, vp, f32, f32, vp]
            L.fw_replay_normalize.restype = i32
            L.fw_replay_normalize.argtypes = [vp, i32, i32, i32, vp, vp, f32, f32, vp, f32, f32, vp]
        if hasattr(L, "fw_td3_update"):            # TD3 (an A/B library of an older commit predates the five; build() insists on them)
            f32 = C.c_float
            L.fw_sizeof_td3_hyper.restype = i32; L.fw_sizeof_td3_hyper.argtypes = []
            L.fw_td3_param_count.restype = i32; L.fw_td3_param_count.argtypes = [i32, i32, i32]
            L.fw_td3_update_workspace_bytes.restype = i64; L.fw_td3_update_workspace_bytes.argtypes = [i32, i32, i32, i32]
            L.fw_td3_act.restype = i32
            L.fw_td3_act.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, u64, i64, vp, vp, vp, vp, f32, vp, vp]
            L.fw_td3_update.restype = i32; L.fw_td3_update.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, i64, vp]
        L.fw_policy_act_a.restype = i32
        L.fw_policy_act_a.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, i64, vp, vp, vp, i32, vp, vp, vp]
        L.fw_collect_act_a.restype = i32
        L.fw_collect_act_a.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, f32, f32, i32, i32, vp, i64, vp, vp, vp, i32, vp, vp,
                                       vp, vp, vp, vp, vp, i32, f32, f32, f32, vp, vp, vp]
        L.fw_rollout_post.restype = i32
        L.fw_rollout_post.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, C.c_double, C.c_float, C.c_float, vp, vp, vp, vp, vp]
        if L.fw_abi_version() != K.FW_ABI_VERSION:
            raise RuntimeError("libfwsim_hip.so ABI version does not match the Python binding; rebuild")
        if L.fw_state_dim() != K.FW_STATE_DIM:
            raise RuntimeError("FW_STATE_DIM mismatch between include/fwsim.h and config.py")
        if L.fw_sizeof_config() != C.sizeof(K.FwConfig):
            raise RuntimeError("fw_config layout mismatch between include/fwsim.h and config.FwConfig")
        if L.fw_sizeof_collect_hl_args() != C.sizeof(K.FwCollectHlArgs):
            raise RuntimeError("fw_collect_hl_args layout mismatch between include/fwsim.h and config.FwCollectHlArgs")
        _lib = L
    return _lib


def check(rc: int, handle=None) -> None:
    """Map ABI error codes onto the reference's exception types
    (``ValueError`` for bad configuration, ``RuntimeError`` otherwise)."""
    if rc == K.FW_OK:
        return
    msg = lib().fw_last_error(handle)
    msg = msg.decode() if msg else f"fwsim error {rc}"
    if rc in (K.FW_EINVAL, K.FW_EVERSION):
        raise ValueError(msg)
    if rc == K.FW_ENOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def devptr(t):
    """the device address of tensor ``t`` as a ``void*`` argument; None (an argument left out) stays None"""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(device):
    """torch's current stream on ``device`` as a ``void* hip_stream`` argument"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# fw_collect_act_a's previous-step block when there is nothing to finalise: prev_reward, prev_terminated, prev_truncated,
# prev_terminal_obs, ret_var, norm_reward, clip_reward, eps_reward, gamma, rew_out, start_out
NOTHING_TO_FINALISE = (None, None, None, None, None, 0, 0.0, 0.0, 0.0, None, None)


def collect_act_a(params, obs, n: int, obs_dim: int, act_dim: int, obs_mean, obs_var, clip_obs: float, eps_obs: float, *, nets: int,
                  deterministic: int, stream, rng=None, env_offset: int = 0, obs_copy=None, act_raw=None, act_env=None, logp=None,
                  value=None, prev=NOTHING_TO_FINALISE) -> None:
    """``fw_collect_act_a`` by keyword.  Tensors in (None: an output left out); ``obs`` / ``act_env`` say their own dtype.  ``prev``:
    the eleven arguments of the previous-step block as the C call takes them (pointers, not tensors).  The defaults are the
    policy-only call of a frozen policy: no rollout rows, no value, nothing of a previous step to finalise."""
    check(lib().fw_collect_act_a(devptr(params), devptr(obs), int(obs.dtype == torch.float64), n, obs_dim, act_dim, devptr(obs_mean),
                                 devptr(obs_var), float(clip_obs), float(eps_obs), nets, deterministic, devptr(rng), int(env_offset),
                                 devptr(obs_copy), devptr(act_raw), devptr(act_env),
                                 int(act_env is not None and act_env.dtype == torch.float64), devptr(logp), devptr(value), *prev, stream))


def validate(cfg: K.FwConfig) -> None:
    buf = C.create_string_buffer(256)
    rc = lib().fw_validate_config(C.byref(cfg), buf, 256)
    if rc != K.FW_OK:
        raise ValueError(buf.value.decode())
