"""Which sums of the sub-step loop of a step kernel are contracted into FMAs differently in two builds?  (runs on a CPU)

hipcc contracts `a*b + c*d` into fma(a, b, c*d) or fma(c, d, a*b) by what else is in the basic block, so the same source rounds
differently once a loop around it is unrolled or a branch around it goes away.  Bit-identity between kernel variants then breaks
in a handful of sums out of hundreds.  This tool finds them from the two device assemblies (`-save-temps`, the recipe of
_lib.build):

  * each listing is walked symbolically along the common path of the sub-step loop (tools/tick_isa_count.py: common_path; a rolled
    tick loop is walked `--ticks` times, default 2): every v_fma_f64 / v_fmac_f64 / v_mul_f64 / v_add_f64 becomes a node over the
    nodes its operand registers hold; v_mov / v_accvgpr moves and DPP moves are followed; everything else is an opaque node over
    its register operands; registers read before they are written, constants, lane reads and shuffles are anonymous leaves;
  * every sum (add or fma) gets the hash of its UNFUSED expression -- fma(a, b, c) as a*b + c, operands of + and * sorted -- and a
    pattern: plain add, or fma with the hash of the product it has fused;
  * sums with the same unfused expression and another pattern in the other build are printed with their instructions.

Leaves are anonymous, so symmetric expressions (the x / y / z components of a vector) share a hash: counts are compared, not
instances.  A difference that is only an operand hoisted out of the loop (a leaf in one build, a product in the other) shows as
an unmatched expression on both sides with the same pattern.  Nothing here replaces the twin tests on the GPU; it tells where to
look.

usage:  python tools/fma_contraction_diff.py [--ticks N] [--longest] PARENT.s THIS.s [kernel-name substring]   (default: g8xs)
        --longest: the path through the rare branches (stall, clamp, renormalisation) instead of the common one
"""
import hashlib
import os
import re
import sys
from collections import Counter, defaultdict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tick_isa_count as T  # noqa: E402

F64 = {"v_fma_f64": "fma", "v_mul_f64": "mul", "v_add_f64": "add", "v_fmac_f64": "fma"}
MOVES = ("v_mov_b32", "v_mov_b64", "v_accvgpr_write_b32", "v_accvgpr_read_b32", "v_accvgpr_mov_b32", "s_mov_b32", "s_mov_b64")
NO_RESULT = ("s_cbranch", "s_branch", "s_waitcnt", "s_nop", "s_cmp", "s_barrier", "global_store", "ds_write", "buffer_store", "v_cmp",
             "s_and_saveexec", "s_or_b64", "s_andn2", "s_and_b64", "s_xor")
LEAF_OPS = ("in", "const", "ds_bpermute_b32", "s_brev_b32", "v_readlane_b32", "v_readfirstlane_b32")


def regs_of(tok):
    m = re.fullmatch(r"([vsa])\[(\d+):(\d+)\]", tok)
    if m:
        return [f"{m.group(1)}{i}" for i in range(int(m.group(2)), int(m.group(3)) + 1)]
    return [tok] if re.fullmatch(r"[vsa]\d+", tok) else None


class Walk:
    """The expression graph of one listing: nodes[id] = (op, operand ids); f64 = [(id, instruction text, block)]."""

    def __init__(self, fn_text, ticks, longest):
        self.nodes, self.reg, self.f64, self.memo = [], {}, [], {}
        bl = T.blocks(fn_text)
        header, bs = T.substep_loop(bl)
        tick = {b[0].replace(".L", "") for b in T.tick_loop(bl)[1]}
        path = T.common_path(bs, header, longest)
        inner = [l for l in path if l in tick]
        if inner and len(inner) < len(path):             # a rolled tick loop: its blocks `ticks` times
            i0 = path.index(inner[0])
            assert path[i0:i0 + len(inner)] == inner
            path = path[:i0] + inner * ticks + path[i0 + len(inner):]
        bmap = {b[0].replace(".L", ""): b for b in bs}
        for l in path:
            for op, txt in bmap[l][1]:
                self.step(re.sub(r"_e(32|64)$", "", op), txt, l)

    def mk(self, op, *args):
        self.nodes.append((op, args))
        return len(self.nodes) - 1

    def rd1(self, r):
        if r not in self.reg:
            self.reg[r] = self.mk("in", r)
        return self.reg[r]

    def rd(self, tok):
        neg, ab = tok.startswith("-"), False
        t = tok[1:] if neg else tok
        if t.startswith("|") and t.endswith("|"):
            ab, t = True, t[1:-1]
        rs = regs_of(t)
        if rs is None:
            v = self.mk("const", t)
        elif len(rs) == 1:
            v = self.rd1(rs[0])
        else:
            parts = [self.rd1(x) for x in rs]
            p0 = self.nodes[parts[0]]
            whole = len(rs) == 2 and p0[0] == "lo" and self.nodes[parts[1]] == ("hi", p0[1])
            v = p0[1][0] if whole else self.mk("pair", *parts)
        v = self.mk("abs", v) if ab else v
        return self.mk("neg", v) if neg else v

    def wr(self, tok, v):
        rs = regs_of(tok) or []
        if len(rs) == 1:
            self.reg[rs[0]] = v
        for i, r in enumerate(rs if len(rs) > 1 else []):
            self.reg[r] = self.mk(("lo", "hi")[i] if len(rs) == 2 else f"part{i}", v)

    def step(self, op, txt, block):
        parts = txt.split(None, 1)
        toks = [t.strip() for t in parts[1].split(",")] if len(parts) > 1 else []
        toks = [t if t.startswith("|") else t.split()[0] for t in toks if t]
        if op in F64:
            a = [self.rd(toks[1]), self.rd(toks[2]), self.rd(toks[0])] if op == "v_fmac_f64" else [self.rd(t) for t in toks[1:]]
            v = self.mk(F64[op], *a)
            self.wr(toks[0], v)
            self.f64.append((v, txt, block))
        elif op in MOVES and len(toks) == 2:
            dst, src = regs_of(toks[0]), regs_of(toks[1])
            for i, d in enumerate(dst or []):
                self.reg[d] = self.rd1(src[i]) if src and len(src) == len(dst) else self.mk("const", toks[1])
        elif op.startswith("v_mov_b32_dpp"):
            self.reg[regs_of(toks[0])[0]] = self.mk("dpp", self.rd1(regs_of(toks[1])[0]))
        elif not op.startswith(NO_RESULT) and toks and regs_of(toks[0]):
            self.wr(toks[0], self.mk(op, *[self.rd(t) for t in toks[1:] if regs_of(t.lstrip("-").strip("|"))]))

    def leaf(self, v):
        op, a = self.nodes[v]
        if op in ("lo", "hi"):
            return self.leaf(a[0])
        return op in LEAF_OPS or (op in ("pair", "v_cndmask_b32") and all(self.leaf(x) for x in a))

    def unfused(self, v):
        """hash of the expression of node v with every fma taken apart"""
        if v in self.memo:
            return self.memo[v]
        h = lambda s: hashlib.md5(s.encode()).hexdigest()[:10]       # noqa: E731
        op, a = self.nodes[v]
        u = self.unfused
        if op in ("lo", "hi"):
            r = u(a[0])
        elif self.leaf(v):
            r = "L"
        elif op == "pair":
            n = [self.nodes[x] for x in a]
            if len(a) == 2 and n[0][0] == n[1][0] == "dpp" and self.nodes[n[0][1][0]][0] == "lo" and self.nodes[n[1][1][0]] == ("hi", self.nodes[n[0][1][0]][1]):
                r = h("D" + u(self.nodes[n[0][1][0]][1][0]))          # both halves of one value through the same DPP move
            else:
                r = h("P" + ",".join(u(x) for x in a))
        elif op in ("neg", "abs"):
            r = h(op + u(a[0]))
        elif op in ("mul", "add"):
            r = h(op + ",".join(sorted(u(x) for x in a)))
        elif op == "fma":
            r = h("add" + ",".join(sorted([self.product(v), u(a[2])])))
        else:
            r = h(op + ",".join(u(x) for x in a))
        self.memo[v] = r
        return r

    def product(self, v):
        return hashlib.md5(("mul" + ",".join(sorted(self.unfused(x) for x in self.nodes[v][1][:2]))).encode()).hexdigest()[:10]

    def sums(self):
        """{unfused hash: Counter of patterns}, {unfused hash: [(pattern, instruction, block)]}"""
        table, where = defaultdict(Counter), defaultdict(list)
        for v, txt, block in self.f64:
            op = self.nodes[v][0]
            if op in ("add", "fma"):
                p = "add" if op == "add" else "fma<" + self.product(v) + ">"
                table[self.unfused(v)][p] += 1
                where[self.unfused(v)].append((p, txt, block))
        return table, where


def function(path, sub):
    for name, fn in T.functions(open(path).read()):
        if sub in name or sub in T.demangle([name])[name]:
            return fn
    raise SystemExit(f"no function matching {sub!r} in {path}")


def main(argv):
    ticks, longest = 2, "--longest" in argv
    if "--ticks" in argv:
        i = argv.index("--ticks"); ticks = int(argv[i + 1]); argv = argv[:i] + argv[i + 2:]
    argv = [a for a in argv if a != "--longest"]
    if len(argv) < 2:
        print(__doc__)
        return 2
    sub = argv[2] if len(argv) > 2 else "g8xs"
    a, b = Walk(function(argv[0], sub), ticks, longest), Walk(function(argv[1], sub), ticks, longest)
    (ta, wa), (tb, wb) = a.sums(), b.sums()
    for name, w in (("parent", a), ("this", b)):
        c = Counter(w.nodes[v][0] for v, _, _ in w.f64)
        print(f"{name}: {len(w.f64)} f64 arithmetic instructions on the path: fma {c['fma']}, mul {c['mul']}, add {c['add']}")
    keys = sorted(set(ta) | set(tb))
    bad = [k for k in keys if ta[k] != tb[k]]
    for k in bad:
        print(f"sum {k}: parent {dict(ta[k])}  this {dict(tb[k])}")
        for name, w in (("parent", wa), ("this  ", wb)):
            for p, txt, block in w[k]:
                print(f"    {name} {block:<10} {p:<16} {txt}")
    print(f"{len(bad)} of {len(keys)} distinct sums differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
