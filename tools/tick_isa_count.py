"""Static instruction accounting of the physics tick loop of the fw_step kernels (runs on a CPU, no GPU needed).

At one wave per SIMD (the 8-lane step kernels run 512 single-wave workgroups at 4096 envs) nothing hides a stall, and the tick's
f64 stream is issue-bound: every instruction taken out of it saves about its issue slot, in every wave, 8 times per launch.
This tool is the yardstick for that stream.  It reads the device assembly that a `-save-temps` build leaves (the recipe of
_lib.build) and, per step kernel instantiation, finds the tick loop -- the loop that holds the group sums of the surface
wrench (v_mov_b32_dpp) -- and prints:

  * the instruction count of the loop body by opcode class, over all of its blocks (`all`) and along the shortest and the
    longest path from the loop header to its back edge (`min path` / `max path`: wave-uniform branches and branches whose exec
    mask can come out empty take either side; the shortest path is the common tick -- no stalled surface in the wave, no
    angular-motion clamp, no renormalisation of the quaternion);
  * the split at the first DPP move of the loop: `surface` is what precedes it (actuator lag, body-frame velocities,
    surface_wrench: lane-parallel), `rigid` the rest (wrench sums, rigid-body update, contact test: replicated in all 8 lanes).
    The scheduler moves a few instructions across that line; the split is a guide, the totals are exact.

usage:  python tools/tick_isa_count.py <fwsim ...gfx950.s> [kernel-name substring ...]
        (default substring: fw_step_kernel_g8; `--json` prints the tables as one JSON object)
"""
import json
import re
import subprocess
import sys
from collections import Counter, OrderedDict

CLASSES = ("fma_f64", "mul_f64", "add_f64", "other_f64", "cndmask", "dpp", "other_valu", "salu", "s_nop", "s_waitcnt",
           "branch", "memory")


def classify(op):
    op = re.sub(r"_e(32|64)$", "", op)
    if op in ("v_fma_f64", "v_fmac_f64"):
        return "fma_f64"
    if op == "v_mul_f64":
        return "mul_f64"
    if op == "v_add_f64":
        return "add_f64"
    if op.startswith("v_cndmask"):
        return "cndmask"
    if op.endswith("_dpp") or op.startswith("v_mov_b32_dpp"):
        return "dpp"
    if op.startswith("v_") and "f64" in op:
        return "other_f64"
    if op.startswith(("global_", "buffer_", "ds_", "scratch_", "flat_", "s_load", "s_buffer_load")):
        return "memory"
    if op.startswith("v_"):
        return "other_valu"
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith(("s_branch", "s_cbranch", "s_setpc")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    return "other_valu"


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: d for n, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def functions(text):
    for fn in re.split(r"\n(?=_Z[\w]+:)", text):
        name = fn.split(":", 1)[0]
        if name.startswith("_Z"):
            yield name, fn


def blocks(fn):
    """[(label, [opcodes], header-of-innermost-loop or None, depth, {'Parent Loop' headers})] in layout order."""
    out = []
    cur = None
    for line in fn.split("\n"):
        m = re.match(r"(\.LBB\d+_\d+):(.*)", line)
        if m or line.startswith("; %bb."):
            cur = [m.group(1) if m else line.split()[1], [], None, 0, set()]
            out.append(cur)
            rest = m.group(2) if m else line.split(":", 1)[1]
        else:
            rest = line
        if cur is None:
            continue
        s = rest.strip()
        h = re.search(r"Loop Header: Depth=(\d+)", s)
        if h:
            cur[2] = cur[0].replace(".L", ""); cur[3] = int(h.group(1))
        p = re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", s)
        if p:
            cur[4].add(p.group(1))
        i = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", s)
        if i:
            cur[2] = i.group(1); cur[3] = int(i.group(2))
        if m or not s or s.startswith((";", ".", "//")):
            continue
        op = s.split()[0]
        if re.match(r"^[a-z_][a-z0-9_]*$", op) and (op.startswith(("v_", "s_", "global_", "buffer_", "ds_", "scratch_", "flat_"))):
            cur[1].append((op, s))
    return out


def tick_loop(bl):
    """The loop (header label) that contains the most DPP moves; ties go to the deeper loop."""
    # a block of a nested loop belongs to every enclosing loop: walk the header chain
    parent = {}
    for b in bl:
        lab = b[0].replace(".L", "")
        if b[2] == lab:
            for p in b[4]:
                parent.setdefault(lab, set()).add(p)
    def ancestors(h):
        seen, todo = set(), [h]
        while todo:
            x = todo.pop()
            for p in parent.get(x, ()):
                if p not in seen:
                    seen.add(p); todo.append(p)
        return seen
    loops = {}
    for b in bl:
        if b[2] is None:
            continue
        for h in {b[2]} | ancestors(b[2]):
            loops.setdefault(h, []).append(b)
    best = None
    for h, bs in loops.items():
        ndpp = sum(1 for b in bs for op, _ in b[1] if classify(op) == "dpp")
        depth = next((b[3] for b in bs if b[0].replace(".L", "") == h), 0)
        key = (ndpp, depth)
        if ndpp and (best is None or key > best[0]):
            best = (key, h, bs)
    return (best[1], best[2]) if best else (None, [])


def paths(bs, header):
    """Shortest / longest instruction count from the header to a back edge, over the loop's acyclic body."""
    labs = [b[0].replace(".L", "") for b in bs]
    idx = {l: i for i, l in enumerate(labs)}
    n = [len(b[1]) for b in bs]
    succ = {}
    for i, b in enumerate(bs):
        ops = b[1]
        s = []
        last = ops[-1] if ops else ("", "")
        for op, txt in ops[-2:]:
            if op.startswith(("s_branch", "s_cbranch")):
                t = txt.split()[-1].replace(".L", "")
                s.append(t)
        if not last[0].startswith("s_branch") and i + 1 < len(bs):
            s.append(labs[i + 1])
        succ[labs[i]] = s
    memo = {}
    def walk(l, stack):
        if l in memo:
            return memo[l]
        res = None
        stack = stack | {l}
        for t in succ[l]:
            if t == header or t not in idx:            # back edge / loop exit
                r = (0, 0)
            elif t in stack:                            # an inner loop's back edge: not counted again
                continue
            else:
                r = walk(t, stack)
            res = r if res is None else (min(res[0], r[0]), max(res[1], r[1]))
        res = (0, 0) if res is None else res
        memo[l] = (res[0] + n[idx[l]], res[1] + n[idx[l]])
        return memo[l]
    return walk(header, frozenset())


def count(bs):
    ops = [op for b in bs for op, _ in b[1]]
    c = Counter(classify(op) for op in ops)
    first = next((k for k, op in enumerate(ops) if classify(op) == "dpp"), len(ops))
    return ops, c, first


def report(path, subs):
    text = open(path).read()
    fns = [(n, f) for n, f in functions(text) if any(s in n or s in demangle([n])[n] for s in subs)]
    dm = demangle([n for n, _ in fns])
    res = OrderedDict()
    for name, fn in fns:
        bl = blocks(fn)
        header, bs = tick_loop(bl)
        if not bs:
            continue
        ops, c, first = count(bs)
        lo, hi = paths(bs, header)
        surf = Counter(classify(op) for op in ops[:first])
        rig = Counter(classify(op) for op in ops[first:])
        res[dm[name]] = OrderedDict(
            header=header, blocks=len(bs), all=len(ops), min_path=lo, max_path=hi,
            surface=first, rigid=len(ops) - first,
            classes=OrderedDict((k, c.get(k, 0)) for k in CLASSES),
            surface_classes=OrderedDict((k, surf.get(k, 0)) for k in CLASSES),
            rigid_classes=OrderedDict((k, rig.get(k, 0)) for k in CLASSES))
    return res


def main(argv):
    as_json = "--json" in argv
    argv = [a for a in argv if a != "--json"]
    if not argv:
        print(__doc__)
        return 2
    res = report(argv[0], argv[1:] or ["fw_step_kernel_g8"])
    if as_json:
        print(json.dumps(res, indent=1))
        return 0
    w = max(len(k) for k in CLASSES)
    for name, r in res.items():
        print(f"{name}\n  tick loop {r['header']} ({r['blocks']} blocks): all {r['all']}, min path {r['min_path']}, "
              f"max path {r['max_path']}; surface {r['surface']} + rigid {r['rigid']}")
        print(f"  {'class':<{w}} {'all':>6} {'surface':>8} {'rigid':>6}")
        for k in CLASSES:
            print(f"  {k:<{w}} {r['classes'][k]:>6} {r['surface_classes'][k]:>8} {r['rigid_classes'][k]:>6}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
