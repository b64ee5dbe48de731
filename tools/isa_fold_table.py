#!/usr/bin/env python3
"""Two builds of csrc/windtunnel.hip compared kernel by kernel: which functions are identical, the resources of every k_march3 instantiation,
and what one trip round each of its marching loops executes on a plain column (profiles/march_unit_fold_isa.txt).

    python tools/isa_fold_table.py PARENT.s BRANCH.s          # the gfx950 .s files of tools/check_store_hazard.py build() at either commit

Loops: every backward branch closes a span (tools/isa_loops.py loops); spans that overlap are one loop (the peeled iterations of a chain unit
enter its loop at several labels).  Two counts per loop, by the same rule on both builds:
  static  every instruction between the loop's first label and its last backward branch, whatever path reaches it: rare paths (clamp, guarded
          division, far-field rows, body columns) included, no branch followed - so every loop of every kernel has a row.  What the compiler
          lays out inside the span differs from build to build (a peeled first trip, a cold block moved out), so these counts are coarse.
  trip    tools/isa_loops.py follow(): one trip from a label on the branches a plain interior column takes in the chain loops it was written
          for (a fixed direction per branch opcode); where that walk does not come back, once more with every conditional branch to the label
          taken.  hipcc turns conditions round from build to build, so in some solo loops the walk leaves the loop or goes twice round it: a
          trip is printed only where both builds give one with the same number of memory instructions.  (Choosing the directions per loop -
          the fewest instructions, or the chain loop's number of floating-point operations - was tried: there are paths round these loops that
          skip a whole stage, and no rule tried tells them from the plain column's.)"""
import re
import sys
from collections import Counter

import isa_loops as L

FP = re.compile(r"^v_(pk_)?(add|sub|mul|fma|fmac|mad|mac|max|min|rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|ldexp|frexp_mant|frexp_exp_i32|trunc|floor|rndne|fract|cvt_\w+)_(f16|f32|f64)")
FIXED = {"s_cbranch_execz": True, "s_cbranch_scc0": True, "s_cbranch_vccnz": True}


def funcs(path):
    """{function: its instruction lines, local labels renumbered, comments and directives dropped}"""
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        s = ln.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def meta(path):
    t = open(path).read()
    r = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", t, re.S):
        b = m.group(0)
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", b).group(1))      # noqa: E731
        r[re.search(r"\.name:\s+(\S+)", b).group(1)] = dict(vgpr=g("vgpr_count"), sgpr=g("sgpr_count"), scratch=g("private_segment_fixed_size"),
                                                            lds=g("group_segment_fixed_size"))
    return r


def count(c, s):
    op = s.split()[0]
    k = L.classify(s)
    c[k] += 1
    c["ex"] += 1
    if k.startswith("v_"):
        c["vec"] += 1
    m = FP.match(op)
    if m:
        c["fp"] += 1
        c["op " + op] += 1
        c["fpops"] += 2 if m.group(1) else 1              # operations on values: a packed instruction works on two
        if m.group(1):
            c["pkfp"] += 1
    return op


def op_diff(a, b):
    """the floating-point opcodes whose counts differ: 'opcode parent -> branch'"""
    ops = sorted(k for k in set(a) | set(b) if k.startswith("op ") and a[k] != b[k])
    return "; ".join(f"{k[3:]} {a[k]} -> {b[k]}" for k in ops)


def is_instr(s):
    return bool(s) and not s.startswith((";", ".", "//")) and not s.endswith(":")


def walk(lines, pos, hdr, back_edge, limit=6000):
    c, i, n = Counter(), pos[hdr] + 1, 0
    while n < limit:
        if i >= len(lines):
            return None
        raw = lines[i]
        s = raw.strip()
        i += 1
        if raw.startswith(hdr + ":"):
            return c
        if not is_instr(s):
            continue
        n += 1
        op = count(c, s)
        if op == "s_branch" or (op.startswith("s_cbranch") and (FIXED.get(op, False) or (back_edge and s.split()[1] == hdr))):
            tgt = s.split()[1]
            if tgt not in pos:
                return None
            if tgt == hdr:
                return c
            i = pos[tgt]
    return None


def kernel_loops(path, sym):
    """[(static counts, trip counts or None)] of the kernel's marching loops, in code order"""
    name, lines = L.kernel_lines(path, sym)
    assert name == sym, (name, sym)
    pos = {}
    for i, l in enumerate(lines):
        m = L.LABEL.match(l)
        if m:
            pos[m.group(1)] = i
    spans, seen = [], set()
    nins = sum(is_instr(l.strip()) for l in lines)
    for tgt, a, b, c, _ in L.loops(lines):
        if tgt in seen or not (300 < sum(c.values()) < min(8000, nins // 2)) or c.get("vmem", 0) < 18:      # (a span of half the kernel is no marching loop)
            continue
        seen.add(tgt)
        spans.append((a, b, tgt))
    spans.sort()
    clusters = []
    for a, b, tgt in spans:
        if clusters and a <= clusters[-1][1]:
            clusters[-1][1] = max(clusters[-1][1], b)
            clusters[-1][2].append(tgt)
        else:
            clusters.append([a, b, [tgt]])
    out = []
    for a, b, labels in clusters:
        st = Counter()
        for l in lines[a:b + 1]:
            if is_instr(l.strip()):
                count(st, l.strip())
        trip = None
        for tgt in labels:
            c = walk(lines, pos, tgt, False) or walk(lines, pos, tgt, True)
            if c is not None and c["ex"] >= 300 and c["vmem"] >= 18 and (trip is None or c["ex"] < trip["ex"]):
                trip = c                                 # (entered at a label behind the first: the shortest trip is the loop's own)
        out.append((st, trip))
    return out


def decode(sym):
    t, _, d, e, fd = re.match(r"_ZN2wt8k_march3I([fd])Li(\d)ELi(\d)ELb([01])ELi(\d+)E", sym).groups()
    return f"{'fp32' if t == 'f' else 'fp64'} depth {d} {'emit ' if e == '1' else 'plain'} FD {int(fd):2d}", (t, int(d), int(e), int(fd))


def main():
    pa, pb = sys.argv[1], sys.argv[2]
    fa, fb = funcs(pa), funcs(pb)
    ma, mb = meta(pa), meta(pb)
    print(f"functions: parent {len(fa)}, branch {len(fb)}; same set of symbols: {set(fa) == set(fb)}")
    other = [k for k in fa if "k_march3" not in k]
    ident = [k for k in other if fa[k] == fb.get(k)]
    print(f"not k_march3: {len(other)} functions, {len(ident)} identical instruction for instruction" +
          ("" if len(ident) == len(other) else "  DIFFER: " + " ".join(k for k in other if k not in ident)))
    k3 = sorted((k for k in fa if "k_march3" in k), key=lambda k: decode(k)[1])
    print(f"k_march3: {len(k3)} instantiations, {sum(fa[k] == fb[k] for k in k3)} identical")
    print()
    print("resources (parent -> branch)")
    print(f"{'instantiation':28s} {'instructions':>16s} {'VGPRs':>10s} {'SGPRs':>10s} {'scratch':>8s} {'LDS':>14s}  waves/SIMD")
    missed = []
    for k in k3:
        a, b = ma[k], mb[k]
        wa, wb = min(2, 512 // ((a["vgpr"] + 7) // 8 * 8)), min(2, 512 // ((b["vgpr"] + 7) // 8 * 8))
        print(f"{decode(k)[0]:28s} {len(fa[k]):7d} -> {len(fb[k]):5d} {a['vgpr']:4d} -> {b['vgpr']:3d} {a['sgpr']:4d} -> {b['sgpr']:3d} {a['scratch']:3d} -> {b['scratch']:1d} "
              f"{a['lds']:6d} -> {b['lds']:5d}  {wa} -> {wb}")
        if b["scratch"] or wb < wa or b["lds"] != a["lds"]:
            missed.append((decode(k)[0], "resources"))
    print()
    print("loops in code order; parent -> branch")
    for k in k3:
        la, lb = kernel_loops(pa, k), kernel_loops(pb, k)
        tag, (_, depth, emit, fd) = decode(k)
        print(tag)
        kinds = ("chain -x", "chain +x", "solo body", "solo lean") if depth >= 3 else ("solo body", "solo lean")
        if len(la) != len(lb):
            print(f"    loops found: parent {len(la)}, branch {len(lb)}")
            missed.append((tag, "loops"))
        if len(la) != len(kinds):
            kinds = tuple(f"loop {i}" for i in range(max(len(la), len(lb))))
        for i, ((sa, ta), (sb, tb)) in enumerate(zip(la, lb)):
            flag = ""
            if sa["vmem"] != sb["vmem"] or sa["lds"] != sb["lds"]:
                flag += " MEM"
            if sa["fp"] != sb["fp"] or sa["pkfp"] != sb["pkfp"]:
                flag += " ARITH" + (" (other operations)" if sa["fpops"] != sb["fpops"] else " (same operations, packed differently)")
            if flag:
                missed.append((tag, kinds[i] + " static" + flag))
                if "ARITH" in flag:
                    flag += "\n" + " " * 22 + op_diff(sa, sb)
            print(f"    {kinds[i]:9s} static  instructions {sa['ex']:4d} -> {sb['ex']:4d}  vmem {sa['vmem']:3d} -> {sb['vmem']:3d}  lds {sa['lds']:3d} -> {sb['lds']:3d}  fp arith {sa['fp']:4d} -> {sb['fp']:4d}  "
                  f"packed fp {sa['pkfp']:4d} -> {sb['pkfp']:4d}  fp operations {sa['fpops']:4d} -> {sb['fpops']:4d}  v_mov {sa['v_mov']:3d} -> {sb['v_mov']:3d} ({sb['v_mov'] - sa['v_mov']:+3d}){flag if flag else '  ok'}")
            if ta is None or tb is None or ta["vmem"] != tb["vmem"] or ta["lds"] != tb["lds"]:
                print(f"    {'':9s} trip    the walk {'does not come back' if ta is None or tb is None else 'goes different ways'}: parent "
                      f"{'-' if ta is None else '%d executed, %d vmem' % (ta['ex'], ta['vmem'])}, branch {'-' if tb is None else '%d executed, %d vmem' % (tb['ex'], tb['vmem'])}")
                missed.append((tag, kinds[i] + " trip not paired"))
                continue
            flag = ""
            if ta["fp"] != tb["fp"] or ta["pkfp"] != tb["pkfp"]:
                flag = " ARITH" + (" (other operations)" if ta["fpops"] != tb["fpops"] else " (same operations, packed differently)")
                missed.append((tag, kinds[i] + " trip" + flag))
                flag += "\n" + " " * 22 + op_diff(ta, tb)
            print(f"    {'':9s} trip    executed {ta['ex']:4d} -> {tb['ex']:4d} ({tb['ex'] - ta['ex']:+3d})  vector {ta['vec']:4d} -> {tb['vec']:4d}  fp arith {ta['fp']:4d} -> {tb['fp']:4d}  packed fp {ta['pkfp']:3d} -> {tb['pkfp']:3d}  "
                  f"fp operations {ta['fpops']:4d} -> {tb['fpops']:4d}  v_pk_* {ta['v_pk']:3d} -> {tb['v_pk']:3d}  v_mov {ta['v_mov']:3d} -> {tb['v_mov']:3d} ({tb['v_mov'] - ta['v_mov']:+3d})  vmem {ta['vmem']:2d} -> {tb['vmem']:2d}  "
                  f"lds {ta['lds']:2d} -> {tb['lds']:2d}  scalar {ta['salu']:3d} -> {tb['salu']:3d} ({tb['salu'] - ta['salu']:+3d})  s_nop {ta['s_nop']:3d} -> {tb['s_nop']:3d}{flag if flag else '  ok'}")
    print()
    print("rows that miss a condition:")
    for m in missed:
        print("   ", *m)
    if not missed:
        print("    none")


if __name__ == "__main__":
    main()
