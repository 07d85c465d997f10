#!/usr/bin/env python3
"""Static census of ONE gfx950 kernel of a built library (no GPU needed): the instruction mix per segment between s_barrier instructions,
loop bodies on lines of their own.  tools/isa_summary.py gives the whole-kernel counts of every kernel; this is the table a change that
removes per-wave instructions starts from.

  python tools/isa_segments.py [--lib gyeeta_amd/lib/libgysketch.so] [--kernel 'k_digest_bins<false, 8u>'] [out.txt]

Segments are in ADDRESS order (the compiler's block layout: a cold block, e.g. a hand-over, may sit behind the code that follows it in the
source).  Loops are the natural loops of the control-flow graph (a backward branch alone is not one: a block laid out of line, the rare side
of an `if`, returns with a backward branch).  A loop's body is taken out of the segment's straight-line count and listed under the segment
that holds its instructions, by the address of its header; a loop inside a loop is listed on its own and not counted in the outer one.  A
loop that holds a barrier (the merge loop itself) is not listed.  Counts are STATIC instructions, s_nop left out."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_summary import klass  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
COLS = ["valu", "salu", "lds", "vmem", "smem", "branch", "waitcnt"]


def device_asm(lib):
    with tempfile.TemporaryDirectory() as t:
        fat, elf = os.path.join(t, "fatbin"), os.path.join(t, "gfx950.elf")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               "--input=" + fat, "--output=" + elf])
        return subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "-C", elf], text=True)


def kernel_instrs(asm, want):
    """[(addr, mnemonic, operands, encoding words)] of the first function whose demangled name contains `want`"""
    want = want.replace(" ", "")
    out, on, name = [], False, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            if on:
                break
            on = want in m.group(1).replace(" ", "")
            name = m.group(1) if on else name
            continue
        if not on:
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-F]+):\s*((?:[0-9A-F]{8}\s*)+)", line)
        if m and m.group(1) != "s_nop" and not m.group(1).startswith("s_code_end"):
            out.append((int(m.group(3), 16), m.group(1), m.group(2), m.group(4).split()))
    return name, out


def branch_target(addr, mn, words):
    if not (mn.startswith("s_cbranch") or mn == "s_branch"):
        return None
    simm = int(words[0], 16) & 0xFFFF
    simm -= 0x10000 if simm & 0x8000 else 0
    return addr + 4 + 4 * simm


def natural_loops(instrs):
    """[(set of instruction indices, header address)] of the natural loops: basic blocks, dominators, back edges (an edge whose head dominates its
    tail).  A backward branch alone is no loop: a block the compiler laid out of line (the rare side of an `if`) returns with one."""
    n = len(instrs)
    index = {a: i for i, (a, _, _, _) in enumerate(instrs)}
    tgt = [branch_target(a, mn, w) for a, mn, _, w in instrs]
    leaders = {0}
    for i in range(n):
        if tgt[i] is not None:
            if tgt[i] in index:
                leaders.add(index[tgt[i]])
            if i + 1 < n:
                leaders.add(i + 1)
    starts = sorted(leaders)
    block_of = {}
    for bi, st in enumerate(starts):
        for j in range(st, starts[bi + 1] if bi + 1 < len(starts) else n):
            block_of[j] = bi
    nb = len(starts)
    succ = [[] for _ in range(nb)]
    for bi, st in enumerate(starts):
        last = (starts[bi + 1] if bi + 1 < nb else n) - 1
        mn = instrs[last][1]
        if tgt[last] is not None and tgt[last] in index:
            succ[bi].append(block_of[index[tgt[last]]])
        if mn != "s_branch" and not mn.startswith(("s_endpgm", "s_setpc")) and last + 1 < n:
            succ[bi].append(block_of[last + 1])
    pred = [[] for _ in range(nb)]
    for u in range(nb):
        for v in succ[u]:
            pred[v].append(u)
    full = (1 << nb) - 1
    dom = [full] * nb  # bit sets
    dom[0] = 1
    changed = True
    while changed:
        changed = False
        for v in range(1, nb):
            d = full
            for u in pred[v]:
                d &= dom[u]
            d |= 1 << v
            if d != dom[v]:
                dom[v], changed = d, True
    loops = {}
    for u in range(nb):
        for v in succ[u]:
            if dom[u] >> v & 1:  # back edge u -> v
                body, work = loops.setdefault(v, {v}), [u]
                while work:
                    x = work.pop()
                    if x not in body:
                        body.add(x)
                        work += pred[x]
    out = []
    for v, body in loops.items():
        idx = set()
        for b in body:
            idx.update(range(starts[b], starts[b + 1] if b + 1 < nb else n))
        out.append((idx, instrs[starts[v]][0]))
    return out


def census(instrs):
    barriers = [i for i, x in enumerate(instrs) if x[1].startswith("s_barrier")]
    loops = [(idx, head) for idx, head in natural_loops(instrs) if not any(b in idx for b in barriers)]
    owner = [None] * len(instrs)  # innermost loop of an instruction
    for li, (idx, _) in sorted(enumerate(loops), key=lambda x: -len(x[1][0])):
        for j in idx:
            owner[j] = li
    bounds = [-1] + barriers + [len(instrs)]
    rows = []
    for s in range(len(bounds) - 1):
        lo, hi = bounds[s] + 1, bounds[s + 1]
        straight, per_loop = {}, {}
        for j in range(lo, hi):
            d = straight if owner[j] is None else per_loop.setdefault(owner[j], {})
            c = klass(instrs[j][1])
            d[c] = d.get(c, 0) + 1
        rows.append(("segment %d" % s, instrs[lo][0] if lo < hi else 0, hi - lo, straight))
        for li in sorted(per_loop, key=lambda x: loops[x][1]):
            rows.append(("  loop @%x" % loops[li][1], loops[li][1], sum(per_loop[li].values()), per_loop[li]))
    return rows, len(barriers)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "gyeeta_amd", "lib", "libgysketch.so"))
    ap.add_argument("--kernel", default="k_digest_bins<false, 8u>")
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    name, instrs = kernel_instrs(device_asm(a.lib), a.kernel)
    if not instrs:
        sys.exit("no kernel matching %r in %s" % (a.kernel, a.lib))
    rows, nb = census(instrs)
    lines = ["# static census per barrier segment, gfx950 (tools/isa_segments.py): %s" % re.sub(r"\(.*", "", name),
             "# %d instructions, %d bytes, %d barriers; a segment's own line counts its straight-line code, its loop bodies follow it" % (
                 len(instrs), instrs[-1][0] - instrs[0][0] + 4 * len(instrs[-1][3]), nb),
             "%-24s %8s %7s " % ("where", "address", "instrs") + " ".join("%7s" % c for c in COLS)]
    tot = {}
    for label, addr, n, mix in rows:
        lines.append("%-24s %8x %7d " % (label, addr, n if label.startswith(" ") else sum(mix.values())) + " ".join("%7d" % mix.get(c, 0) for c in COLS))
        for c, v in mix.items():
            tot[c] = tot.get(c, 0) + v
    lines.append("%-24s %8s %7d " % ("total", "", sum(tot.values())) + " ".join("%7d" % tot.get(c, 0) for c in COLS))
    text = "\n".join(lines) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
