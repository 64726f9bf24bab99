"""tools/kernel_resources.py on a hand-made device assembly: the table of figures, the device-code verdict (the comparison of
tools/check_isa.py --same-device-code), and what makes it exit non-zero."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _asm(kernels):
    """kernels: [(name, body lines, vgprs, scratch, vgpr_spill)] in file order -- the shape of hipcc's -save-temps output"""
    text, meta = "\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n", "amdhsa.kernels:\n"
    for n, (name, body, vgprs, scratch, spill) in enumerate(kernels):
        text += (f"\t.text\n\t.protected\t{name} ; -- Begin function {name}\n\t.globl\t{name}\n{name}:\n; %bb.0:\n"
                 + "".join(f"\t{ln}\n" for ln in body)
                 + f".LBB{n}_1:                                ; %Flow{100 + n}\n\ts_endpgm\n"
                 + f"\t.section\t.rodata,\"a\",@progbits\n\t.amdhsa_kernel {name}\n\t\t.amdhsa_next_free_vgpr {vgprs}\n\t.end_amdhsa_kernel\n\t.text\n"
                 + f".Lfunc_end{n}:\n\t.size\t{name}, .Lfunc_end{n}-{name}\n                                        ; -- End function\n"
                 + f"\t.section\t.AMDGPU.csdata,\"\",@progbits\n; Kernel info:\n; codeLenInByte = 8\n; NumSgprs: 20\n; NumVgprs: {vgprs}\n"
                 + f"; NumAgprs: 4\n; ScratchSize: {scratch}\n; Occupancy: 2\n")
        meta += (f"  - .agpr_count:     4\n    .args:\n      - .offset:         0\n        .size:           8\n"
                 f"    .group_segment_fixed_size: 512\n    .name:           {name}\n    .private_segment_fixed_size: {scratch}\n"
                 f"    .sgpr_count:     20\n    .sgpr_spill_count: 3\n    .symbol:         {name}.kd\n    .vgpr_count:     {vgprs}\n"
                 f"    .vgpr_spill_count: {spill}\n    .wavefront_size: 64\n")
    return text + "\t.text\n\t.amdgpu_metadata\n---\n" + meta + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n"


A = ("_Z1aPf", ["v_add_f32 v0, v0, v1", "s_cbranch_scc1 .LBB0_1"], 12, 0, 0)
B = ("_Z1bPf", ["v_mul_f32 v0, v0, v1"], 30, 0, 0)
NEW = ("_Z1cPf", ["v_sub_f32 v0, v0, v1"], 64, 0, 0)


def test_a_new_kernel_beside_unchanged_ones_passes_and_the_table_carries_the_figures():
    T = _tool()
    # the new kernel goes first: the old ones' local labels and IR block names are renumbered, their code is not
    lines, rc = T.report(_asm([A, B]), _asm([NEW, (A[0], ["v_add_f32 v0, v0, v1", "s_cbranch_scc1 .LBB1_1"]) + A[2:], B]))
    assert rc == 0
    assert lines[-1] == "# 2 existing kernels identical, 0 different, 1 new (0 of them with scratch or spilled vector registers), 0 removed"
    at = lines.index("_Z1aPf")
    assert lines[at + 1] == "    20 | 12 | 4 | 0 | 2 | 3 | 0 | 512 | unchanged | identical"
    assert lines[lines.index("_Z1cPf") + 1] == "    NEW    20 | 64 | 4 | 0 | 2 | 3 | 0 | 512"


def test_a_changed_kernel_a_removed_one_and_a_new_one_with_scratch_each_fail():
    T = _tool()
    lines, rc = T.report(_asm([A, B]), _asm([A, (B[0], ["v_mul_f32 v0, v0, v2"]) + B[2:]]))
    assert rc == 1 and lines[lines.index("_Z1bPf") + 1].endswith("| unchanged | DIFFERENT") and "1 different" in lines[-1]
    lines, rc = T.report(_asm([A, B]), _asm([A, B[:2] + (31, 0, 0)]))                   # (the figure sits in the .amdhsa_kernel block too)
    assert rc == 1 and "WAS 20 | 30 | 4" in lines[lines.index("_Z1bPf") + 1]
    lines, rc = T.report(_asm([A, B]), _asm([A]))
    assert rc == 1 and lines[-2] == "_Z1bPf\n    REMOVED" and "1 removed" in lines[-1]
    for bad in (NEW[:3] + (16, 0), NEW[:3] + (0, 2)):
        lines, rc = T.report(_asm([A, B]), _asm([A, B, bad]))
        assert rc == 1 and lines[lines.index("_Z1cPf") + 1].endswith("SCRATCH / VGPR SPILL") and "1 new (1 of them" in lines[-1]


def test_a_name_map_compares_a_renamed_kernel_with_its_predecessor(tmp_path, capsys):
    """The optional third argument, lines of `new_mangled_name old_mangled_name`: a renamed kernel with the same body is identical, one
    with a changed instruction is DIFFERENT (exit status 1) -- neither is NEW plus REMOVED -- and a pair that names a kernel its build
    does not have is an error."""
    T = _tool()
    renamed = "_Z1bILi1EEvPf"                            # _Z1bPf with one more template parameter
    paths = {}
    for name, text in (("parent.s", _asm([A, B])),
                       ("same.s", _asm([(renamed,) + B[1:], (A[0], ["v_add_f32 v0, v0, v1", "s_cbranch_scc1 .LBB1_1"]) + A[2:]])),
                       ("changed.s", _asm([A, (renamed, ["v_mul_f32 v0, v0, v2"]) + B[2:]])),
                       ("names.txt", f"{renamed} {B[0]}\n"),
                       ("absent_new.txt", f"_Z1zPf {B[0]}\n"), ("absent_old.txt", f"{renamed} _Z1zPf\n")):
        (tmp_path / name).write_text(text)
        paths[name] = str(tmp_path / name)
    run = lambda this, *names: T.main(["kernel_resources.py", paths["parent.s"], paths[this]] + [paths[n] for n in names])

    assert run("same.s", "names.txt") == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[-1] == "# 2 existing kernels identical, 0 different, 0 new (0 of them with scratch or spilled vector registers), 0 removed"
    assert lines[lines.index(B[0]) + 1] == "    20 | 30 | 4 | 0 | 2 | 3 | 0 | 512 | unchanged | identical" and renamed not in lines

    assert run("changed.s", "names.txt") == 1
    lines = capsys.readouterr().out.splitlines()
    assert lines[lines.index(B[0]) + 1].endswith("| unchanged | DIFFERENT") and lines[-1].startswith("# 1 existing kernels identical, 1 different, 0 new") and lines[-1].endswith(", 0 removed")

    assert run("same.s") == 1                            # without the map: NEW plus REMOVED
    out = capsys.readouterr().out
    assert "1 new" in out and "1 removed" in out

    for names in ("absent_new.txt", "absent_old.txt"):
        assert run("same.s", names) == 2
        cap = capsys.readouterr()
        assert cap.out == "" and "name map" in cap.err and "_Z1zPf" in cap.err
