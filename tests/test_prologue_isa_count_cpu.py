"""tools/tick_isa_count.py --prologue on a hand-made device assembly of a two-wave step kernel: the path from the kernel's entry to
the s_barrier of each wave, counted by opcode class along the shortest path (the rare branch skipped), the longest path's total,
and the scalar / vector waits in front of the first vector load."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("tick_isa_count", os.path.join(ROOT, "tools", "tick_isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _two_wave(extra_scalar_trip=True):
    """entry (kernel arguments, one wait) -> second wave: one load, LDS, barrier, end
                                         -> step wave: (a second scalar round trip), state loads, a rare branch, barrier, the loop"""
    trip = ["\ts_load_dword s9, s[4:5], 0x0", "\ts_waitcnt lgkmcnt(0)"] if extra_scalar_trip else []
    return "\n".join([
        "_Z4stepPd:", "; %bb.0:", "\ts_load_dwordx4 s[4:7], s[0:1], 0x0", "\tv_cmp_lt_u32_e32 vcc, 63, v0", "\ts_waitcnt lgkmcnt(0)",
        "\ts_cbranch_vccnz .LBB0_6",
        "; %bb.1:", *trip, "\tv_mov_b32_e32 v1, s4", "\tglobal_load_dwordx2 v[2:3], v[0:1], off", "\tglobal_load_dwordx4 v[4:7], v[0:1], off offset:16",
        "\ts_waitcnt vmcnt(1)", "\tv_mul_f64 v[8:9], v[2:3], v[2:3]", "\ts_cbranch_execz .LBB0_3",
        "; %bb.2:", "\tv_rcp_f64_e32 v[10:11], v[8:9]", "\tv_fma_f64 v[2:3], v[2:3], v[10:11], v[2:3]", "\tv_mul_f64 v[2:3], v[2:3], v[10:11]",
        ".LBB0_3:", "\ts_waitcnt vmcnt(0)", "\tv_fma_f64 v[4:5], v[4:5], v[6:7], v[8:9]", "\ts_barrier", "\tds_read_b64 v[12:13], v14",
        ".LBB0_4:                                ; =>This Loop Header: Depth=1",
        "\tv_mov_b32_dpp v20, v4 row_shr:1 row_mask:0xf bank_mask:0xf", "\tv_add_f64 v[4:5], v[4:5], v[12:13]",
        "\tglobal_store_dwordx2 v[0:1], v[4:5], off", "\ts_cbranch_scc1 .LBB0_4",
        "; %bb.5:", "\ts_endpgm",
        ".LBB0_6:", "\tglobal_load_dword v2, v[0:1], off", "\ts_waitcnt vmcnt(0)", "\tv_mul_lo_u32 v2, v2, v2", "\tds_write_b32 v3, v2",
        "\ts_waitcnt lgkmcnt(0)", "\ts_barrier", "\ts_endpgm", ".Lfunc_end0:", ""])


def test_both_waves_are_found_and_told_apart_by_their_vector_loads():
    T = _tool()
    r = T.prologue_report(T.blocks(_two_wave()))
    assert list(r) == ["step_wave", "second_wave"]
    s, a = r["step_wave"], r["second_wave"]
    assert (s["barrier_block"], a["barrier_block"]) == ("BB0_3", "BB0_6")
    assert s["vector_loads"] == 2 and a["vector_loads"] == 1


def test_step_wave_counts_stop_at_the_barrier_and_skip_the_rare_branch():
    T = _tool()
    s = T.prologue_report(T.blocks(_two_wave()))["step_wave"]
    # entry 4 + block 1: 2 + 6 + the barrier's block up to and including s_barrier: 3; the rare branch adds 3 on the longest path
    assert s["total"] == 15 and s["max_path"] == 18 and s["path_blocks"] == 3
    c = s["classes"]
    assert c["memory"] == 4 and c["s_waitcnt"] == 4 and c["branch"] == 2 and c["mul_f64"] == 1 and c["fma_f64"] == 1 and c["other_f64"] == 0
    assert c["dpp"] == 0 and sum(c.values()) == s["total"]            # nothing of the loop behind the barrier, nor the ds_read behind it


def test_waits_in_front_of_the_first_vector_load():
    T = _tool()
    s = T.prologue_report(T.blocks(_two_wave(True)))["step_wave"]
    assert (s["before_first_vector_load"], s["waits_lgkmcnt_before_first_vector_load"], s["waits_vmcnt_before_first_vector_load"]) == (7, 2, 0)
    s = T.prologue_report(T.blocks(_two_wave(False)))["step_wave"]     # the second scalar round trip gone: one wait, two instructions fewer
    assert (s["before_first_vector_load"], s["waits_lgkmcnt_before_first_vector_load"], s["total"]) == (5, 1, 13)
    a = T.prologue_report(T.blocks(_two_wave()))["second_wave"]
    assert (a["total"], a["before_first_vector_load"], a["waits_lgkmcnt_before_first_vector_load"]) == (10, 4, 1)
    assert a["classes"]["memory"] == 3 and a["classes"]["s_waitcnt"] == 3


def test_vector_loads_are_a_class_not_an_opcode():
    T = _tool()
    for op in ("global_load_dword", "global_load_dwordx4", "buffer_load_dwordx2", "flat_load_dword", "scratch_load_dword"):
        assert T.is_vector_load(op), op
    for op in ("s_load_dwordx2", "ds_read_b64", "global_store_dword", "v_mov_b32_e32"):
        assert not T.is_vector_load(op), op


def test_report_goes_through_the_command_line(tmp_path, capsys):
    T = _tool()
    p = tmp_path / "k.s"
    p.write_text(_two_wave())
    assert T.main(["--prologue", str(p), "step"]) == 0
    out = capsys.readouterr().out
    assert "step wave: entry -> s_barrier in BB0_3" in out and "second wave: entry -> s_barrier in BB0_6" in out
    assert "2 s_waitcnt on lgkmcnt" in out
