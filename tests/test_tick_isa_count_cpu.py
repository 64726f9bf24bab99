"""tools/tick_isa_count.py on a hand-made device assembly: the `moves` class, the sub-step report (outer part, tick, executed per
sub-step along the common path) with the tick loop rolled and unrolled, and that a loop with memory instructions is never taken
for the tick loop."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("tick_isa_count", os.path.join(ROOT, "tools", "tick_isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TICK = ["v_fma_f64 v[0:1], v[2:3], v[4:5], v[0:1]", "v_mov_b32_dpp v6, v0 row_shr:1 row_mask:0xf bank_mask:0xf", "v_add_f64 v[0:1], v[0:1], v[6:7]"]
RARE = ["v_rcp_f64_e32 v[8:9], v[0:1]", "v_mul_f64 v[0:1], v[0:1], v[8:9]"]


def _rolled():
    return "\n".join([
        "_Z4stepPd:", "; %bb.0:", "\ts_mov_b32 s0, 0",
        ".LBB0_1:                                ; =>This Loop Header: Depth=1", "                                        ;     Child Loop BB0_2 Depth 2",
        "\tv_accvgpr_write_b32 a0, v0", "\tv_mov_b64_e32 v[10:11], v[0:1]", "\ts_cbranch_execz .LBB0_5",
        ".LBB0_2:                                ;   Parent Loop BB0_1 Depth=1", "                                        ; =>  This Inner Loop Header: Depth=2",
        *("\t" + i for i in TICK), "\ts_cbranch_execz .LBB0_4",
        "; %bb.3:                                ;   in Loop: Header=BB0_2 Depth=2", *("\t" + i for i in RARE),
        ".LBB0_4:                                ;   in Loop: Header=BB0_2 Depth=2", "\ts_add_i32 s0, s0, 1", "\ts_cbranch_scc1 .LBB0_2",
        ".LBB0_5:                                ;   in Loop: Header=BB0_1 Depth=1", "\tv_accvgpr_read_b32 v0, a0", "\tglobal_store_dwordx2 v[12:13], v[0:1], off",
        "\ts_cbranch_vccnz .LBB0_7",
        "; %bb.6:                                ;   in Loop: Header=BB0_1 Depth=1", "\tv_mov_b32_e32 v20, v21", "\ts_branch .LBB0_1",
        ".LBB0_7:", "\ts_endpgm", ".Lfunc_end0:", ""])


def _unrolled():
    return "\n".join([
        "_Z4stepPd:", "; %bb.0:", "\ts_mov_b32 s0, 0",
        ".LBB0_1:                                ; =>This Loop Header: Depth=1",
        "\tv_accvgpr_write_b32 a0, v0", *("\t" + i for i in TICK), "\ts_cbranch_execz .LBB0_3",
        "; %bb.2:                                ;   in Loop: Header=BB0_1 Depth=1", *("\t" + i for i in RARE),
        ".LBB0_3:                                ;   in Loop: Header=BB0_1 Depth=1", *("\t" + i for i in TICK),
        "\tglobal_store_dwordx2 v[12:13], v[0:1], off", "\ts_cbranch_vccnz .LBB0_5",
        "; %bb.4:                                ;   in Loop: Header=BB0_1 Depth=1", "\tv_mov_b32_e32 v20, v21", "\ts_branch .LBB0_1",
        ".LBB0_5:", "\ts_endpgm", ".Lfunc_end0:", ""])


def test_moves_are_register_copies_without_dpp():
    T = _tool()
    for op in ("v_accvgpr_write_b32", "v_accvgpr_read_b32", "v_accvgpr_mov_b32", "v_mov_b32_e32", "v_mov_b64_e32", "v_mov_b32_e64"):
        assert T.classify(op) == "moves", op
    assert T.classify("v_mov_b32_dpp") == "dpp" and T.classify("v_cndmask_b32_e32") == "cndmask" and T.classify("s_mov_b32") == "salu"
    assert "moves" in T.CLASSES


def test_substep_report_of_a_rolled_tick_loop():
    T = _tool()
    bl = T.blocks(_rolled())
    assert T.tick_loop(bl)[0] == "BB0_2" and T.substep_loop(bl)[0] == "BB0_1"
    r = T.substep_report(bl, 2)
    # outer: header 3, BB0_5 3, the latch 2 (the loop exit is not the way of a sub-step that is followed by another); tick: 4 + 2
    assert (r["tick_loop"], r["trips"], r["outer_total"], r["tick_total"], r["executed_total"]) == ("BB0_2", 2, 8, 6, 20)
    assert r["outer"]["moves"] == 4 and r["tick"]["moves"] == 0 and r["executed"]["moves"] == 4
    assert r["executed"]["dpp"] == 2 and r["executed"]["fma_f64"] == 2 and r["executed"]["memory"] == 1
    assert r["all"]["other_f64"] == 1 and r["all"]["mul_f64"] == 1 and r["executed"]["mul_f64"] == 0      # the rare branch: all blocks only


def test_an_unrolled_tick_loop_is_not_mistaken_for_the_substep_loop():
    T = _tool()
    bl = T.blocks(_unrolled())
    assert T.tick_loop(bl) == (None, []) and T.substep_loop(bl)[0] == "BB0_1"
    r = T.substep_report(bl, 2)
    assert r["tick_loop"] is None and r["tick_total"] == 0 and r["executed_total"] == r["outer_total"] == 12
    assert r["executed"]["dpp"] == 2 and r["executed"]["moves"] == 2 and r["all"]["mul_f64"] == 1


def test_contraction_diff_names_the_sum_that_fused_the_other_product():
    """tools/fma_contraction_diff.py on two hand-made listings of `a*b + (c + c)*d`: fma(a, b, (c + c)*d) against
    fma(c + c, d, a*b).  (Leaves are anonymous: the two products must differ in structure to be told apart.)"""
    spec = importlib.util.spec_from_file_location("fma_contraction_diff", os.path.join(ROOT, "tools", "fma_contraction_diff.py"))
    D = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(D)

    def listing(first):
        body = ["v_add_f64 v[10:11], v[4:5], v[4:5]"]
        body += (["v_mul_f64 v[8:9], v[10:11], v[6:7]", "v_fma_f64 v[0:1], v[0:1], v[2:3], v[8:9]"] if first else
                 ["v_mul_f64 v[8:9], v[0:1], v[2:3]", "v_fmac_f64_e32 v[8:9], v[10:11], v[6:7]", "v_mov_b64_e32 v[0:1], v[8:9]"])
        return "\n".join(["_Z4stepPd:", "; %bb.0:", ".LBB0_1:                                ; =>This Loop Header: Depth=1",
                          "\tv_mov_b32_dpp v20, v0 row_shr:1 row_mask:0xf bank_mask:0xf", *("\t" + i for i in body),
                          "\tglobal_store_dwordx2 v[12:13], v[0:1], off", "\ts_cbranch_scc1 .LBB0_1", "; %bb.2:", "\ts_endpgm", ".Lfunc_end0:", ""])

    a, b, c = (D.Walk(listing(f), 2, False) for f in (True, False, True))
    (ta, _), (tb, _), (tc, _) = a.sums(), b.sums(), c.sums()
    assert ta == tc and set(ta) == set(tb) and len(ta) == 2           # c + c and the sum of products: the same unfused sums in all three ...
    differ = [k for k in ta if ta[k] != tb[k]]
    assert len(differ) == 1 and all(p.startswith("fma<") for p in list(ta[differ[0]]) + list(tb[differ[0]]))    # ... one with another product fused
