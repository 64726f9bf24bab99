"""tools/tick_isa_count.py --substep on a hand-made device assembly: the split of register moves by kind (agpr / copy / literal,
scalar moves included) along the common path and over all blocks, and the per-block table of the sub-step loop."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("tick_isa_count", os.path.join(ROOT, "tools", "tick_isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TICK = ["v_fma_f64 v[0:1], v[2:3], v[4:5], v[0:1]", "v_mov_b32_dpp v6, v0 row_shr:1 row_mask:0xf bank_mask:0xf", "v_add_f64 v[0:1], v[0:1], v[6:7]"]


def _listing():
    """A sub-step loop with the tick unrolled into it: a head that copies (2 vector, 1 scalar, 1 AGPR), a tick, a rare block that
    rebuilds two coefficients and copies one pair, a second tick with the outputs' store, a latch with one AGPR read and one literal."""
    return "\n".join([
        "_Z4stepPd:", "; %bb.0:", "\ts_mov_b32 s0, 0",
        ".LBB0_1:                                ; =>This Loop Header: Depth=1",
        "\tv_mov_b64_e32 v[10:11], v[0:1]", "\tv_mov_b32_e32 v12, v13", "\ts_mov_b64 s[4:5], s[6:7]", "\tv_accvgpr_write_b32 a0, v0",
        *("\t" + i for i in TICK), "\ts_cbranch_execz .LBB0_3",
        "; %bb.2:                                ;   in Loop: Header=BB0_1 Depth=1",
        "\tv_mov_b32_e32 v8, 0x3fe00000", "\ts_mov_b32 s8, 0x9999999a", "\tv_mov_b64_e32 v[14:15], v[10:11]", "\tv_cndmask_b32_e32 v0, v0, v8, vcc",
        ".LBB0_3:                                ;   in Loop: Header=BB0_1 Depth=1", *("\t" + i for i in TICK),
        "\tglobal_store_dwordx2 v[12:13], v[0:1], off", "\ts_cbranch_vccnz .LBB0_5",
        "; %bb.4:                                ;   in Loop: Header=BB0_1 Depth=1", "\tv_accvgpr_read_b32 v0, a0", "\tv_mov_b32_e32 v20, 0", "\ts_branch .LBB0_1",
        ".LBB0_5:", "\ts_endpgm", ".Lfunc_end0:", ""])


def test_move_kinds():
    T = _tool()
    kind = T.move_kind
    assert kind("v_accvgpr_write_b32", "v_accvgpr_write_b32 a0, v0") == "agpr" and kind("v_accvgpr_read_b32", "v_accvgpr_read_b32 v0, a0") == "agpr"
    assert kind("v_accvgpr_mov_b32", "v_accvgpr_mov_b32 a1, a0") == "agpr"
    assert kind("v_mov_b64_e32", "v_mov_b64_e32 v[10:11], v[0:1]") == "copy" and kind("v_mov_b32_e32", "v_mov_b32_e32 v1, s3") == "copy"
    assert kind("s_mov_b64", "s_mov_b64 s[4:5], s[6:7]") == "copy" and kind("s_mov_b64", "s_mov_b64 s[4:5], exec") == "copy"
    assert kind("s_mov_b32", "s_mov_b32 s4, vcc_lo") == "copy"
    assert kind("v_mov_b32_e32", "v_mov_b32_e32 v8, 0x3fe00000") == "literal" and kind("v_mov_b32_e32", "v_mov_b32_e32 v8, 0") == "literal"
    assert kind("s_mov_b32", "s_mov_b32 s8, 0x9999999a") == "literal" and kind("s_mov_b64", "s_mov_b64 s[0:1], -1") == "literal"
    assert kind("v_mov_b32_e32", "v_mov_b32_e32 v8, -1.0") == "literal"
    for op, txt in (("v_mov_b32_dpp", "v_mov_b32_dpp v6, v0 row_shr:1"), ("v_cndmask_b32_e32", "v_cndmask_b32_e32 v0, v0, v8, vcc"),
                    ("v_fma_f64", TICK[0]), ("s_add_i32", "s_add_i32 s0, s0, 1"), ("s_movk_i32", "s_movk_i32 s0, 0x100")):
        assert kind(op, txt) is None, op
    assert T.MOVE_KINDS == ("agpr", "copy", "literal")


def test_substep_report_splits_the_moves_and_lists_the_blocks():
    T = _tool()
    r = T.substep_report(T.blocks(_listing()), 2)
    assert r["tick_loop"] is None and r["header"] == "BB0_1"
    k = r["move_kinds"]
    # common path: head, BB0_3, the latch (the rare block is skipped); all blocks: the rare block's two literals and one copy on top
    assert (k["agpr"]["executed"], k["copy"]["executed"], k["literal"]["executed"]) == (2, 3, 1)
    assert (k["agpr"]["all"], k["copy"]["all"], k["literal"]["all"]) == (2, 4, 3)
    assert all(q["tick"] == 0 and q["outer"] == q["executed"] for q in k.values())
    # the vector half of the kinds is the `moves` class; the scalar moves stay in `salu` there
    assert r["executed"]["moves"] == 5 and r["all"]["moves"] == 7
    rows = r["per_block"]
    assert [q["block"] for q in rows] == ["BB0_1", "%bb.2", "BB0_3", "%bb.4"]
    assert [q["on_path"] for q in rows] == [True, False, True, True]
    head, rare, second, latch = rows
    assert (head["total"], head["f64"], head["dpp"], head["agpr"], head["copy"], head["literal"], head["other"]) == (8, 2, 1, 1, 3, 0, 1)
    assert (rare["total"], rare["cndmask"], rare["copy"], rare["literal"], rare["other"]) == (4, 1, 1, 2, 0)
    assert (second["total"], second["f64"], second["dpp"], second["other"]) == (5, 2, 1, 2)
    assert (latch["total"], latch["agpr"], latch["literal"], latch["other"]) == (3, 1, 1, 1)
    for q in rows:
        assert q["total"] == q["f64"] + q["dpp"] + q["cndmask"] + q["agpr"] + q["copy"] + q["literal"] + q["other"]
    assert sum(q["total"] for q in rows) == sum(r["all"].values())


def test_the_printed_report_has_both_tables(tmp_path, capsys):
    T = _tool()
    path = tmp_path / "listing.s"
    path.write_text(_listing())
    assert T.main(["--substep", str(path), "step"]) == 0
    out = capsys.readouterr().out
    assert "moves by kind" in out and "per block" in out
    lines = [l.split() for l in out.splitlines()]
    assert ["agpr", "2", "0", "2", "2"] in lines and ["copy", "3", "0", "3", "4"] in lines and ["literal", "1", "0", "1", "3"] in lines
    assert ["BB0_1*", "8", "2", "1", "0", "1", "3", "0", "1"] in lines and ["%bb.2", "4", "0", "0", "1", "0", "1", "2", "0"] in lines
