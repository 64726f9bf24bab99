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
  * `--substep`: the loop that encloses the tick loop (one iteration = one sub-step of the agent step: the ticks of an Aviary
    step plus the task logic), counted along its common path -- every wave-uniform skip taken that does not skip the ticks, no
    rare branch of the tick: `outer` (the path outside the tick loop), `tick` (the tick's common path) and `executed` = outer +
    trips x tick, the instructions a wave issues per sub-step when nothing special happens (`--ticks N`: trips, default 2);
    `all blocks` counts every block of the loop once, rare branches included (a rolled tick loop's body once, not per trip).
    A kernel whose tick loop is unrolled has no inner loop: the path through the sub-step loop is then its own total and the
    outer / tick split is not made.

The `moves` class is register copying: v_accvgpr_read / write / mov, and v_mov_b32 / v_mov_b64 without DPP.  `--substep` splits
it by kind (move_kind): `agpr` = v_accvgpr_* (the allocator parking values in the accumulation registers), `copy` = a v_mov or
s_mov from a register (phi copies at joins and loop heads), `literal` = a v_mov or s_mov of a constant (coefficients rebuilt in
place).  The s_mov of either kind belong to the `salu` class of the table above and are listed here as well, since they are
the scalar half of the same copying.  The per-block table lists every block of the sub-step loop in layout order, the blocks
of the common path marked `*`, with its instructions by f64 arithmetic, DPP, v_cndmask, the three kinds of move and the rest.

A loop is taken for the tick loop only if it holds no memory instruction (the tick has none; the sub-step loop stores the step's
outputs): with the tick loop unrolled the tick-loop report is left out instead of counting the sub-step loop in its place.

  * `--prologue`: kernel entry to the s_barrier in front of the sub-step loop, for the step wave and for the second wave of a
    two-wave step kernel (the wave that issues more vector loads on its way is the step wave): instructions by opcode class along
    the shortest path (every skip of a rare branch taken), the longest path's total, and how many s_waitcnt on lgkmcnt / vmcnt
    stand in front of the path's first vector load -- the serial round trips a launch pays before its state is even requested.
    (A one-wave kernel meets its only barrier at the very end: the report then spans the kernel and says nothing about a prologue.)

usage:  python tools/tick_isa_count.py [--substep | --prologue] [--ticks N] [--json] <fwsim ...gfx950.s> [kernel-name substring ...]
        (default substring: fw_step_kernel_g8; `--json` prints the tables as one JSON object)
"""
import json
import re
import subprocess
import sys
from collections import Counter, OrderedDict

CLASSES = ("fma_f64", "mul_f64", "add_f64", "other_f64", "cndmask", "dpp", "moves", "other_valu", "salu", "s_nop", "s_waitcnt",
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
    if op.startswith("v_accvgpr_") or op in ("v_mov_b32", "v_mov_b64"):
        return "moves"
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


MOVE_KINDS = ("agpr", "copy", "literal")


def move_kind(op, txt):
    """agpr / copy / literal for an instruction that only moves a value (see the module text); None for everything else."""
    op = re.sub(r"_e(32|64)$", "", op)
    if op.startswith("v_accvgpr_"):
        return "agpr"
    if op not in ("v_mov_b32", "v_mov_b64", "s_mov_b32", "s_mov_b64"):
        return None
    parts = txt.split(None, 1)
    toks = [t.strip() for t in parts[1].split(",")] if len(parts) > 1 else []
    src = toks[1].split()[0] if len(toks) > 1 and toks[1] else ""
    return "copy" if re.fullmatch(r"[vsa]\d+|[vsa]\[\d+:\d+\]|vcc(_lo|_hi)?|exec(_lo|_hi)?|m0", src) else "literal"


def block_row(b):
    """One row of the per-block table: instructions of a block by what they are there for."""
    c = Counter(classify(op) for op, _ in b[1])
    k = Counter(move_kind(op, txt) for op, txt in b[1])
    f64 = c["fma_f64"] + c["mul_f64"] + c["add_f64"] + c["other_f64"]
    row = OrderedDict(block=b[0].replace(".L", ""), total=len(b[1]), f64=f64, dpp=c["dpp"], cndmask=c["cndmask"],
                      agpr=k["agpr"], copy=k["copy"], literal=k["literal"])
    row["other"] = row["total"] - f64 - c["dpp"] - c["cndmask"] - k["agpr"] - k["copy"] - k["literal"]
    return row


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


def loops_of(bl):
    """{header: [blocks]}: a block of a nested loop belongs to every enclosing loop (walk the header chain)."""
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
    return loops


def ndpp(bs):
    return sum(1 for b in bs for op, _ in b[1] if classify(op) == "dpp")


def has_memory(bs):
    return any(classify(op) == "memory" for b in bs for op, _ in b[1])


def dpp_loops(bl):
    """[(dpp moves, depth, header, blocks)] of the loops that hold DPP moves, the one with most of them (ties: the deeper) first."""
    out = []
    for h, bs in loops_of(bl).items():
        depth = next((b[3] for b in bs if b[0].replace(".L", "") == h), 0)
        if ndpp(bs):
            out.append((ndpp(bs), depth, h, bs))
    return sorted(out, key=lambda x: (-x[0], -x[1]))


def tick_loop(bl):
    """The loop (header label) that contains the most DPP moves; ties go to the deeper loop.  (None, []) where that loop holds
    memory instructions: it is the sub-step loop then, with the tick loop unrolled into it."""
    ls = dpp_loops(bl)
    if not ls or has_memory(ls[0][3]):
        return None, []
    return ls[0][2], ls[0][3]


def substep_loop(bl):
    """The loop one iteration of which is a sub-step: the outermost loop that holds all the DPP moves of the tick loop (rolled),
    or the loop with the most DPP moves itself where it holds memory instructions (tick loop unrolled)."""
    ls = dpp_loops(bl)
    if not ls:
        return None, []
    top = ls[0][0]
    best = min((x for x in ls if x[0] == top), key=lambda x: x[1])
    return best[2], best[3]


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


def common_path(bs, header, longest=False):
    """Block labels from the header to the back edge along the common path: the shortest path among those that run the most
    DPP moves (the group sums of the tick: a path that skips the ticks is not the common one).  longest: the longest such path
    instead, through the rare branches."""
    labs = [b[0].replace(".L", "") for b in bs]
    idx = {l: i for i, l in enumerate(labs)}
    big = 1 + sum(len(b[1]) for b in bs)
    cost = [(-len(b[1]) if longest else len(b[1])) - big * sum(1 for op, _ in b[1] if classify(op) == "dpp") for b in bs]
    succ = {}
    for i, b in enumerate(bs):
        ops, s = b[1], []
        last = ops[-1] if ops else ("", "")
        for op, txt in ops[-2:]:
            if op.startswith(("s_branch", "s_cbranch")):
                s.append(txt.split()[-1].replace(".L", ""))
        if not last[0].startswith("s_branch") and i + 1 < len(bs):
            s.append(labs[i + 1])
        succ[labs[i]] = s
    memo = {}
    def walk(l, stack):
        if l in memo:
            return memo[l]
        best = None
        stack = stack | {l}
        for t in succ[l]:
            if t not in idx:                            # a loop exit: not the way of a sub-step that is followed by another
                continue
            if t == header:
                r = (0, [])
            elif t in stack:
                continue
            else:
                r = walk(t, stack)
            if best is None or r[0] < best[0]:
                best = r
        best = best or (0, [])
        memo[l] = (best[0] + cost[idx[l]], [l] + best[1])
        return memo[l]
    return walk(header, frozenset())[1]


def substep_report(bl, trips):
    sh, sbs = substep_loop(bl)
    if not sbs:
        return None
    bmap = {b[0].replace(".L", ""): b for b in sbs}
    path = common_path(sbs, sh)
    th, tbs = tick_loop(bl)
    tl = {b[0].replace(".L", "") for b in tbs}
    outer = Counter(classify(op) for l in path if l not in tl for op, _ in bmap[l][1])
    tick = Counter(classify(op) for l in path if l in tl for op, _ in bmap[l][1])
    rolled = bool(tl) and th != sh
    if not rolled:
        tick = Counter()
    ex = Counter({k: outer.get(k, 0) + (trips if rolled else 0) * tick.get(k, 0) for k in CLASSES})
    every = Counter(classify(op) for b in sbs for op, _ in b[1])       # all blocks of the loop, each counted once
    on_path = set(path)
    kinds = OrderedDict()
    for k in MOVE_KINDS:
        k_outer = sum(1 for l in path if l not in tl for op, txt in bmap[l][1] if move_kind(op, txt) == k)
        k_tick = sum(1 for l in path if l in tl for op, txt in bmap[l][1] if move_kind(op, txt) == k) if rolled else 0
        kinds[k] = OrderedDict(outer=k_outer, tick=k_tick, executed=k_outer + (trips if rolled else 0) * k_tick,
                               all=sum(1 for b in sbs for op, txt in b[1] if move_kind(op, txt) == k))
    per_block = []
    for b in sbs:
        row = block_row(b)
        row["on_path"] = row["block"] in on_path
        row["block"] = row["block"].rstrip(":")
        per_block.append(row)
    return OrderedDict(move_kinds=kinds, per_block=per_block, header=sh, blocks=len(sbs), path_blocks=len(path), tick_loop=th if rolled else None, trips=trips if rolled else 0,
                       outer=OrderedDict((k, outer.get(k, 0)) for k in CLASSES), tick=OrderedDict((k, tick.get(k, 0)) for k in CLASSES),
                       executed=OrderedDict((k, ex.get(k, 0)) for k in CLASSES), all=OrderedDict((k, every.get(k, 0)) for k in CLASSES),
                       outer_total=sum(outer.values()), tick_total=sum(tick.values()), executed_total=sum(ex.values()))


def is_vector_load(op):
    """A load through the vector memory path (what brings the state and the launch constants in): a class, not one opcode."""
    return classify(op) == "memory" and op.startswith(("global_load", "buffer_load", "flat_load", "scratch_load"))


def successors(bl):
    """{label: [successor labels]} of a function's blocks in layout order (branch targets of the last two instructions, and the
    fall-through unless the block ends in an unconditional branch or the program's end)."""
    labs = [b[0].replace(".L", "") for b in bl]
    succ = {}
    for i, b in enumerate(bl):
        ops, s = b[1], []
        last = ops[-1] if ops else ("", "")
        for op, txt in ops[-2:]:
            if op.startswith(("s_branch", "s_cbranch")):
                s.append(txt.split()[-1].replace(".L", ""))
        if not last[0].startswith(("s_branch", "s_endpgm", "s_setpc")) and i + 1 < len(bl):
            s.append(labs[i + 1])
        succ[labs[i]] = s
    return labs, succ


def prologue_report(bl):
    """Kernel entry -> s_barrier, for every barrier of the function that can be reached without passing another one: a two-wave
    step kernel has two, the second wave's (it draws the noise, meets the barrier and ends) and the step wave's in front of the
    sub-step loop; the step wave is the one that issues more vector loads on its way (the state).  Counted along the shortest
    path (every wave-uniform skip of a rare branch taken: the common launch) by opcode class, with the longest path's total
    beside it, and the number of s_waitcnt on lgkmcnt / vmcnt in front of the first vector load of the path."""
    if not bl:
        return None
    labs, succ = successors(bl)
    idx = {l: i for i, l in enumerate(labs)}

    def upto_barrier(b):
        ops = b[1]
        k = next((j for j, (op, _) in enumerate(ops) if op == "s_barrier"), None)
        return (ops, False) if k is None else (ops[:k + 1], True)

    memo = {}

    def walk(l, stack):
        """{barrier block: (min count, min path, max count)} reachable from l without crossing another barrier"""
        if l in memo:
            return memo[l]
        ops, hit = upto_barrier(bl[idx[l]])
        if hit:
            memo[l] = {l: (len(ops), [l], len(ops))}
            return memo[l]
        out = {}
        stack = stack | {l}
        for t in succ[l]:
            if t not in idx or t in stack:
                continue
            for tgt, (lo, path, hi) in walk(t, stack).items():
                cand = (lo + len(ops), [l] + path, hi + len(ops))
                if tgt not in out:
                    out[tgt] = cand
                else:
                    cur = out[tgt]
                    best = cand if cand[0] < cur[0] else cur
                    out[tgt] = (best[0], best[1], max(cur[2], cand[2]))
        memo[l] = out
        return out

    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * len(bl) + 100))
    found = walk(labs[0], frozenset())
    waves = []
    for tgt, (lo, path, hi) in found.items():
        ops = [op for l in path for op, _ in upto_barrier(bl[idx[l]])[0]]
        txt = [t for l in path for _, t in upto_barrier(bl[idx[l]])[0]]
        c = Counter(classify(op) for op in ops)
        first = next((k for k, op in enumerate(ops) if is_vector_load(op)), len(ops))
        waits = [t for op, t in zip(ops[:first], txt[:first]) if op == "s_waitcnt"]
        waves.append(OrderedDict(
            barrier_block=tgt, path_blocks=len(path), total=lo, max_path=hi,
            vector_loads=sum(1 for op in ops if is_vector_load(op)),
            classes=OrderedDict((k, c.get(k, 0)) for k in CLASSES),
            before_first_vector_load=first,
            waits_lgkmcnt_before_first_vector_load=sum(1 for t in waits if "lgkmcnt" in t),
            waits_vmcnt_before_first_vector_load=sum(1 for t in waits if "vmcnt" in t)))
    if not waves:
        return None
    waves.sort(key=lambda w: -w["vector_loads"])
    out = OrderedDict(step_wave=waves[0])
    if len(waves) > 1:
        out["second_wave"] = waves[1]
    return out


def count(bs):
    ops = [op for b in bs for op, _ in b[1]]
    c = Counter(classify(op) for op in ops)
    first = next((k for k, op in enumerate(ops) if classify(op) == "dpp"), len(ops))
    return ops, c, first


def report(path, subs, substep=False, trips=2, prologue=False):
    text = open(path).read()
    fns = [(n, f) for n, f in functions(text) if any(s in n or s in demangle([n])[n] for s in subs)]
    dm = demangle([n for n, _ in fns])
    res = OrderedDict()
    for name, fn in fns:
        bl = blocks(fn)
        if prologue:
            r = prologue_report(bl)
            if r:
                res[dm[name]] = r
            continue
        if substep:
            r = substep_report(bl, trips)
            if r:
                res[dm[name]] = r
            continue
        header, bs = tick_loop(bl)
        if not bs:
            if dpp_loops(bl):
                res[dm[name]] = None          # the tick loop is unrolled into the sub-step loop: see --substep
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
    substep = "--substep" in argv
    prologue = "--prologue" in argv
    trips = 2
    if "--ticks" in argv:
        i = argv.index("--ticks"); trips = int(argv[i + 1]); argv = argv[:i] + argv[i + 2:]
    argv = [a for a in argv if a not in ("--json", "--substep", "--prologue")]
    if not argv:
        print(__doc__)
        return 2
    res = report(argv[0], argv[1:] or ["fw_step_kernel_g8"], substep, trips, prologue)
    if as_json:
        print(json.dumps(res, indent=1))
        return 0
    w = max(len(k) for k in CLASSES)
    for name, r in res.items():
        if prologue:
            print(name)
            for wave, q in r.items():
                print(f"  {wave.replace('_', ' ')}: entry -> s_barrier in {q['barrier_block']} ({q['path_blocks']} blocks on the shortest path): "
                      f"{q['total']} instructions (longest path {q['max_path']}), {q['vector_loads']} vector loads; in front of the first one: "
                      f"{q['before_first_vector_load']} instructions, {q['waits_lgkmcnt_before_first_vector_load']} s_waitcnt on lgkmcnt, "
                      f"{q['waits_vmcnt_before_first_vector_load']} on vmcnt")
            print(f"  {'class':<{w}} " + " ".join(f"{wave:>12}" for wave in r))
            for k in CLASSES:
                print(f"  {k:<{w}} " + " ".join(f"{q['classes'][k]:>12}" for q in r.values()))
        elif r is None:
            print(f"{name}\n  tick loop: unrolled into the sub-step loop (no loop of its own; --substep counts the sub-step)")
        elif substep:
            how = (f"tick loop {r['tick_loop']} x {r['trips']}" if r["tick_loop"] else "tick loop unrolled")
            print(f"{name}\n  sub-step loop {r['header']} ({r['blocks']} blocks, {r['path_blocks']} on the common path), {how}: "
                  f"outer {r['outer_total']}, tick {r['tick_total']}, executed per sub-step {r['executed_total']}")
            print(f"  {'class':<{w}} {'outer':>6} {'tick':>6} {'executed':>9} {'all blocks':>11}")
            for k in CLASSES:
                print(f"  {k:<{w}} {r['outer'][k]:>6} {r['tick'][k]:>6} {r['executed'][k]:>9} {r['all'][k]:>11}")
            print("  moves by kind (v_accvgpr_* | v_mov / s_mov from a register | v_mov / s_mov of a constant):")
            for k, q in r["move_kinds"].items():
                print(f"  {k:<{w}} {q['outer']:>6} {q['tick']:>6} {q['executed']:>9} {q['all']:>11}")
            print("  per block (layout order; * = on the common path):")
            print(f"  {'block':<12} {'total':>6} {'f64':>5} {'dpp':>5} {'cndmask':>8} {'agpr':>5} {'copy':>5} {'literal':>8} {'other':>6}")
            for q in r["per_block"]:
                print(f"  {q['block'] + ('*' if q['on_path'] else ''):<12} {q['total']:>6} {q['f64']:>5} {q['dpp']:>5} {q['cndmask']:>8} "
                      f"{q['agpr']:>5} {q['copy']:>5} {q['literal']:>8} {q['other']:>6}")
        else:
            print(f"{name}\n  tick loop {r['header']} ({r['blocks']} blocks): all {r['all']}, min path {r['min_path']}, "
                  f"max path {r['max_path']}; surface {r['surface']} + rigid {r['rigid']}")
            print(f"  {'class':<{w}} {'all':>6} {'surface':>8} {'rigid':>6}")
            for k in CLASSES:
                print(f"  {k:<{w}} {r['classes'][k]:>6} {r['surface_classes'][k]:>8} {r['rigid_classes'][k]:>6}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
