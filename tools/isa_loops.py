#!/usr/bin/env python3
"""Order of global loads, vmcnt waits, MFMAs and LDS writes in the barrier loops of a gfx950 assembly listing.

Input: the `-S` output of a .hip file, e.g.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-honor-nans --cuda-device-only -S cenet_amd/csrc/attn_diff.hip -o attn_diff.s
    python3 tools/isa_loops.py attn_diff.s [--match dattn_] [--md] [--all-loops]

Per kernel it prints the resource lines (VGPR + AGPR, scratch bytes, waves per SIMD) and, per loop that holds an `s_barrier`
(the cycle of basic blocks around it), the events in program order in compact form:
    L<n>  n global / buffer loads in a row          W     s_waitcnt with a vmcnt field (the count in brackets when not 0)
    M<n>  n MFMAs in a row                          S<n>  n LDS writes in a row          B  s_barrier
    |     a basic-block boundary (label) between two events (`/` with --md)
A loop is FLAGGED (`DRAIN`) when a vmcnt wait follows a load and precedes an MFMA inside one trip: the wait then stands between
the prefetch and the tile body, so the loads it waits for cannot overlap the body.  A register prefetch is right when the
loop reads  L<n> M<m> W S<k> B : all loads first, one wait in front of the LDS writes.
--all-loops lists the loops without an `s_barrier` too (the sra_* tile loops order their LDS traffic with wave barriers alone; a
staging loop that was not unrolled), in the same notation, a trip starting at the loop's first block in the listing.
"""
import argparse
import re
import subprocess
import sys

LOAD = re.compile(r"^(global_load|buffer_load|flat_load|scratch_load)")
LDSW = re.compile(r"^(ds_write|ds_store)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^s_cbranch_\w+\s+(\.LBB\d+_\d+)|^s_branch\s+(\.LBB\d+_\d+)")
VMCNT = re.compile(r"vmcnt\((\d+)\)")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(text):
    """yield (symbol, body lines, resources) per kernel"""
    lines = text.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"^(\w+):\s*(;.*)?$", lines[i])
        if m and i > 0 and any(m.group(1) in lines[k] and "@function" in lines[k] for k in range(max(0, i - 4), i)):
            sym = m.group(1)
            j = i + 1
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                j += 1
            res = {}
            k = j
            while k < len(lines) and k < j + 120:
                mm = re.match(r"^;\s*(NumVgprs|NumAgprs|ScratchSize|Occupancy|TotalNumVgprs):\s*(\d+)", lines[k])
                if mm:
                    res[mm.group(1)] = int(mm.group(2))
                if re.match(r"^\s*\.text|^\s*\.section", lines[k]) and k > j + 3 and "Occupancy" in res:
                    break
                k += 1
            yield sym, lines[i + 1:j], res
            i = j
        i += 1


def barrier_loops(body, all_loops=False):
    """Loops that hold an s_barrier: the strongly connected components of the block graph (branch targets + fall-through) with a
    barrier inside.  (Not the compiler's `in Loop: Header=` comments: a loop entered at two blocks is irreducible and gets none.)
    Returns [(label of the first block, instructions of one trip, from behind the barrier to the barrier)].
    all_loops: the components without a barrier as well (a loop that synchronises with wave barriers alone, a staging loop),
    in listing order; one trip of such a loop runs from its first block in the listing, the loop's header, around to it."""
    blocks = [["entry", []]]
    for raw in body:
        s = raw.strip()
        m = LABEL.match(s)
        if m:
            blocks.append([m.group(1), [m.group(1) + ":"]])
        else:
            blocks[-1][1].append(s.split(";")[0].strip())
    idx = {b[0]: n for n, b in enumerate(blocks)}
    succ = []
    for n, (_, ins) in enumerate(blocks):
        out = set()
        for i in ins:
            m = BRANCH.match(i)
            if m and (m.group(1) or m.group(2)) in idx:
                out.add(idx[m.group(1) or m.group(2)])
        real = [i for i in ins if i and not i.endswith(":")]
        if n + 1 < len(blocks) and not (real and re.match(r"s_branch|s_endpgm|s_setpc", real[-1])):
            out.add(n + 1)
        succ.append(sorted(out))

    def reach(src, allowed):
        seen, todo = set(), [src]
        while todo:
            for t in succ[todo.pop()]:
                if t in allowed and t not in seen:
                    seen.add(t)
                    todo.append(t)
        return seen

    every = set(range(len(blocks)))
    pred = [[p for p in every if n in succ[p]] for n in every]
    out, done = [], set()
    starts = [n for n, (_, ins) in enumerate(blocks) if any(i.startswith("s_barrier") for i in ins)]
    if all_loops:  # barrier blocks first, so that a loop with a barrier keeps its barrier-to-barrier trip
        starts += list(range(len(blocks)))
    for n in starts:
        if n in done:
            continue
        fwd = reach(n, every)
        if n not in fwd:
            continue  # a barrier outside any loop
        back, todo = {n}, [n]
        while todo:
            for p in pred[todo.pop()]:
                if p not in back:
                    back.add(p)
                    todo.append(p)
        scc = sorted(fwd & back)
        done.update(scc)
        # one trip in execution order: reverse post-order of the cycle's blocks from the barrier block's successors
        inside, seen, post = set(scc), {n}, []

        def walk(b):
            seen.add(b)
            for t in succ[b]:
                if t in inside and t not in seen:
                    walk(t)
            post.append(b)

        for t in reversed(succ[n]):
            if t in inside and t not in seen:
                walk(t)
        if any(i.startswith("s_barrier") for i in blocks[n][1]):
            order = post[::-1] + [n]
        else:  # (scc[0] == n: the blocks are visited in listing order and n is the first of its component not done)
            order = [n] + post[::-1]
        out.append((order[0], blocks[order[0]][0], [i for b in order for i in blocks[b][1]]))
    return [(label, ins) for _, label, ins in sorted(out)]


def shape(ins):
    ev = []  # (kind, count or vmcnt)
    valu = 0
    for s in ins:
        if not s:
            continue
        if LABEL.match(s):
            kind = "|"
        elif LOAD.match(s):
            kind = "L"
        elif s.startswith("v_mfma") or s.startswith("v_smfmac"):
            kind = "M"
        elif LDSW.match(s):
            kind = "S"
        elif s.startswith("s_barrier"):
            kind = "B"
        elif s.startswith("s_waitcnt") and VMCNT.search(s):
            kind = "W" + ("" if VMCNT.search(s).group(1) == "0" else "[%s]" % VMCNT.search(s).group(1))
        else:
            if s.startswith("v_"):
                valu += 1
            continue
        if kind == "|":
            if ev and ev[-1][0] != "|":
                ev.append(["|", 1])
        elif ev and ev[-1][0] == kind and kind in "LMS":
            ev[-1][1] += 1
        else:
            ev.append([kind, 1])
    while ev and ev[-1][0] == "|":
        ev.pop()
    # a wait after a load and in front of an MFMA of the same trip
    seen_load = waited = drain = False
    for k, _ in ev:
        if k == "L":
            seen_load, waited = True, False
        elif k.startswith("W") and seen_load:
            waited = True
        elif k == "M" and waited:
            drain = True
        elif k == "B":
            seen_load = waited = False
    txt = " ".join(k + (str(n) if k in "LMS" else "") for k, n in ev)
    return txt, valu, drain


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("--match", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--md", action="store_true", help="markdown table rows")
    ap.add_argument("--all-loops", action="store_true",
                    help="also the loops without an s_barrier (a trip then starts at the loop's first block in the listing)")
    a = ap.parse_args()
    text = open(a.asm).read()
    ks = list(kernels(text))
    names = demangle([k[0] for k in ks])
    flagged = 0
    if a.md:
        print("| instance | VGPR+AGPR | scratch B | waves/SIMD | loop | VALU in loop | shape | |")
        print("|---|---|---|---|---|---|---|---|")
    for sym, body, res in ks:
        name = names[sym].replace("void ", "").replace("(DiffArgs)", "")
        if a.match not in name:
            continue
        loops = barrier_loops(body, a.all_loops)
        regs = "%d+%d" % (res.get("NumVgprs", -1), res.get("NumAgprs", 0))
        head = (name, regs, res.get("ScratchSize", -1), res.get("Occupancy", -1))
        if not loops:
            continue
        for label, ins in loops:
            txt, valu, drain = shape(ins)
            flagged += drain
            if a.md:  # (block boundaries as `/`: a `|` would end the table cell)
                print("| `%s` | %s | %d | %d | `%s` | %d | `%s` | %s |" % (head + (label, valu, txt.replace("|", "/"), "DRAIN" if drain else "")))
            else:
                print("%s  regs %s scratch %d waves %d" % head)
                print("    %s  VALU %d  %s%s" % (label, valu, txt, "   <-- DRAIN" if drain else ""))
    print(("%d loop(s) flagged" % flagged) if not a.md else "\n%d loop(s) flagged" % flagged)
    return 0


if __name__ == "__main__":
    sys.exit(main())
