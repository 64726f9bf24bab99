"""Per-kernel resources of two builds of csrc/fwsim.hip, side by side: registers, scratch, occupancy, spills, LDS, and whether a
kernel's device code is the same in both.

    python tools/kernel_resources.py PARENT.s THIS.s [NAMES.txt] > profiles/rNN_<what>_resources.txt

PARENT.s / THIS.s: the gfx950 device assembly of the two builds (`hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared
-save-temps`, the file `*-hip-amdgcn-amd-amdhsa-gfx950.s`).  The comparison is the one of `tools/check_isa.py --same-device-code`
(its `functions()`); this tool only adds the table of figures, read from the code-object metadata and the "Kernel info" comment of
each kernel.  Exits non-zero when an existing kernel differs or is gone, or a new one uses scratch or spills vector registers.

NAMES.txt (optional): lines of `new_mangled_name old_mangled_name`, for a change that renames kernels (a template that gains a
parameter, two kernels that become one).  THIS.s is read with every new name replaced by its old one, so a renamed kernel is compared
with its predecessor instead of being listed as NEW plus REMOVED.  A pair whose new name is not a function of THIS.s, or whose old name
is not one of PARENT.s, is an error (exit status 2)."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_isa import functions  # noqa: E402

COLS = ("sgprs", "vgprs", "agprs", "scratch", "occupancy", "sgpr_spill", "vgpr_spill", "lds")


def resources(text):
    """{kernel: {column: figure}} of a device assembly text."""
    out = {}
    for blk in re.split(r"^  - \.agpr_count:", text[text.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        f = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)", "    .agpr_count:" + blk, re.M))
        out[f["name"]] = dict(sgprs=int(f["sgpr_count"]), scratch=int(f["private_segment_fixed_size"]), lds=int(f["group_segment_fixed_size"]),
                              sgpr_spill=int(f["sgpr_spill_count"]), vgpr_spill=int(f["vgpr_spill_count"]))
    for m in re.finditer(r"^\s*\.amdhsa_kernel (_Z\w+)\n.*?^; Kernel info:\n(.*?)^\s*\.(?:text|section)", text, re.S | re.M):
        info = dict(re.findall(r"^; (\w+)\s*:\s*(\d+)", m.group(2), re.M))
        if m.group(1) in out:
            out[m.group(1)].update(occupancy=int(info["Occupancy"]), vgprs=int(info["NumVgprs"]), agprs=int(info["NumAgprs"]))
    return out


def row(k):
    return " | ".join(str(k.get(c, "?")) for c in COLS)


def report(parent_text, this_text):
    """(lines of the table, exit code)"""
    old, new = resources(parent_text), resources(this_text)
    code_old, code_new = functions(parent_text), functions(this_text)
    lines = ["# kernel resources (hipcc -O3 --offload-arch=gfx950; code-object metadata and the Kernel info comments of the device assembly) of every kernel,",
             "# parent commit -> this build, and whether the kernel's device code is identical (tools/check_isa.py --same-device-code: the function's text,",
             "# its .amdhsa_kernel block included, up to the numbering of local labels and IR block names).",
             "# columns: SGPRs | VGPRs | AGPRs | ScratchSize [bytes/lane] | Occupancy [waves/SIMD] | SGPRs Spill | VGPRs Spill | LDS Size [bytes/block] | device code"]
    same = diff = fresh = bad_new = 0
    for name in sorted(new):
        k = new[name]
        lines.append(name)
        if name not in old:
            fresh += 1
            clean = k["scratch"] == 0 and k["vgpr_spill"] == 0
            bad_new += not clean
            lines.append(f"    NEW    {row(k)}" + ("" if clean else " | SCRATCH / VGPR SPILL"))
            continue
        res = "unchanged" if row(old[name]) == row(k) else f"WAS {row(old[name])}"
        ident = name in code_old and code_old.get(name) == code_new.get(name)
        ok = ident and res == "unchanged"
        same += ok
        diff += not ok
        lines.append(f"    {row(k)} | {res} | {'identical' if ident else 'DIFFERENT'}")
    gone = sorted(set(old) - set(new))
    lines += [f"{name}\n    REMOVED" for name in gone]
    lines.append(f"# {same} existing kernels identical, {diff} different, {fresh} new ({bad_new} of them with scratch or spilled vector registers), {len(gone)} removed")
    return lines, (1 if diff or bad_new or gone else 0)


def rename(parent_text, this_text, pairs):
    """this_text with the new mangled name of every (new, old) pair replaced by the old one; ValueError for a pair that names a
    kernel its build does not have, or an old name that this build still uses."""
    old_names, new_names = set(functions(parent_text)), set(functions(this_text))
    for new, old in pairs:
        if new not in new_names:
            raise ValueError(f"name map: {new} is not a function of THIS.s")
        if old not in old_names:
            raise ValueError(f"name map: {old} is not a function of PARENT.s")
        if old in new_names:
            raise ValueError(f"name map: {old} is still a function of THIS.s")
    to_old = dict(pairs)
    return re.sub(r"\b_Z\w+", lambda m: to_old.get(m.group(0), m.group(0)), this_text)


def main(argv):
    parent, this = open(argv[1]).read(), open(argv[2]).read()
    pairs = []
    if len(argv) > 3:
        pairs = [tuple(l.split()) for l in open(argv[3]).read().splitlines() if l.strip() and not l.startswith("#")]
        try:
            this = rename(parent, this, pairs)
        except ValueError as e:
            print(e, file=sys.stderr)
            return 2
    table, rc = report(parent, this)
    if pairs:
        table.insert(4, f"# {len(pairs)} kernels of this build are listed under their predecessors' names ({os.path.basename(argv[3])}: new name -> old name)")
    print("\n".join(table))
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv))
