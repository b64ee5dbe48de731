#!/usr/bin/env python3
"""Two builds of csrc/polar.hip compared function by function across the fold of the batched step kernels into k_step_batch<T, EMIT,
LOADMODE, COLL, WALL, FAR> and k_step_half_batch<EMIT, COLL, FAR> (profiles/polar_step_fold_isa.txt).

    python tools/polar_step_fold_table.py PARENT.s BRANCH.s      # the gfx950 .s files of tools/check_store_hazard.py build() at either commit

Each instantiation of the branch is paired with the parent's kernel of the same (storage, T, EMIT, COLL, WALL, FAR), whatever its name was.
A function is its instruction lines, comments and directives stripped, labels renumbered (tools/isa_fold_table.py funcs); "up to kernarg
offsets" also blanks the immediate offset of every scalar load from the kernel-argument segment, whose base is the SGPR pair the kernel
starts with."""
import os
import re
import sys
from collections import Counter

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import isa_fold_table as F          # noqa: E402
import _polar_isa as P              # noqa: E402

OLD = re.compile(r"^_Z\d+k_step_(|les_|ibb_|wind_|trt_|profile_|half_|trt_half_)batchI([fd]?)((?:L[bi]\d+E)+)E")
COUNTED = re.compile(r"^(global_|buffer_|flat_|scratch_|ds_)|" + F.FP.pattern[1:])
COLLS, WALLS, FARS = ("BGK", "LES", "TRT", "TRT+LES"), ("half-way", "interp", "moving"), ("axial", "inclined", "profile")


def old_variant(name):
    """the parent's kernel names read as (storage, T, EMIT, COLL, WALL, FAR)"""
    m = OLD.match(name)
    if not m:
        return None
    kind, t = m.group(1), m.group(2)
    a = [int(x) for x in re.findall(r"L[bi](\d+)E", m.group(3))]
    if kind == "half_":
        return ("half", "f", a[0], a[1], P.HALFWAY, a[2])
    if kind == "trt_half_":
        return ("half", "f", a[0], a[1], P.HALFWAY, P.INCLINED)
    coll = {"": P.BGK, "les_": P.LES}.get(kind, a[2] if len(a) > 2 else None)
    wall = a[3] if len(a) > 3 else (P.INTERP if kind == "ibb_" else P.HALFWAY)
    far = {"wind_": P.INCLINED, "trt_": P.INCLINED, "profile_": P.PROFILE}.get(kind, P.AXIAL)
    return ("native", t, a[0], coll, wall, far)


def kernarg_blind(lines):
    """the lines with the offsets of the loads from the kernel-argument segment blanked.  The segment's base is s[0:1] at entry unless the
    kernel's first instructions say otherwise; a load from it is an s_load_* whose base is a pair no instruction has written."""
    written, out = set(), []
    for s in lines:
        m = re.match(r"^(s_load_dword\w*)\s+(\S+),\s*s\[(\d+):(\d+)\],\s*(\S+)$", s)
        if m and (int(m.group(3)), int(m.group(4))) not in written and not m.group(5).startswith("s"):
            s = f"{m.group(1)} {m.group(2)}, s[{m.group(3)}:{m.group(4)}], OFF"
        d = re.match(r"^s_\w+\s+s\[(\d+):(\d+)\]", s)
        if d and not s.startswith(("s_cmp", "s_cbranch", "s_waitcnt", "s_bitcmp")):
            for lo in range(int(d.group(1)), int(d.group(2))):
                written.add((lo, lo + 1))
        out.append(s)
    return out


def vector_stream(lines):
    """the vector and memory instructions in order, SGPR names blanked: what the lanes execute, whatever the scalar unit's registers are called"""
    return [re.sub(r"\bs(\d+|\[\d+:\d+\])", "S", s) for s in lines if s.startswith(("v_", "global_", "buffer_", "flat_", "ds_", "scratch_"))]


def waves(vgpr):
    return min(8, 512 // ((vgpr + 7) // 8 * 8))


def label(v):
    st, t, e, c, w, f = v
    return f"{'half ' if st == 'half' else 'fp32 ' if t == 'f' else 'fp64 '}{'emit ' if e else 'plain'} {COLLS[c]:7s} {WALLS[w]:8s} {FARS[f]}"


def main():
    pa, pb = sys.argv[1], sys.argv[2]
    fa, fb = F.funcs(pa), F.funcs(pb)
    ma, mb = F.meta(pa), F.meta(pb)
    olds = {old_variant(k): k for k in fa if old_variant(k)}
    news = {P.step_variant(k): k for k in fb if P.step_variant(k)}
    print(f"step kernels: parent {len(olds)}, branch {len(news)}; the same variants: {set(olds) == set(news)}; "
          f"the branch holds exactly the 80 + 12 built ones: {set(news) == P.step_variants_built()}")
    rest_a = {k: v for k, v in fa.items() if not old_variant(k)}
    rest_b = {k: v for k, v in fb.items() if not P.step_variant(k)}
    same = [k for k in rest_a if rest_a[k] == rest_b.get(k)]
    print(f"every other function: parent {len(rest_a)}, branch {len(rest_b)}, the same symbols: {set(rest_a) == set(rest_b)}, "
          f"{len(same)} identical instruction for instruction" + ("" if len(same) == len(rest_a) else "  DIFFER: " + " ".join(sorted(set(rest_a) - set(same)))))
    exact = blind = 0
    differ, scalar, missed = [], [], []
    for v in sorted(olds):
        a, b = fa[olds[v]], fb[news[v]]
        ra, rb = ma[olds[v]], mb[news[v]]
        if a == b:
            exact += 1
        elif kernarg_blind(a) == kernarg_blind(b):
            blind += 1
        else:
            differ.append(v)
            if vector_stream(a) == vector_stream(b):
                scalar.append(v)
    print(f"step kernels identical instruction for instruction: {exact}; identical up to kernarg offsets: {blind}; otherwise: {len(differ)}, "
          f"of which {len(scalar)} execute the same vector and memory instructions in the same order (scalar loads grouped or scalar registers named differently)")
    print()
    print("waves: waves per SIMD that the VGPR count allows (512 VGPRs, granule 8, at most 8)")
    print(f"{'variant':44s} {'verdict':10s} {'instructions':>14s} {'VGPRs':>10s} {'waves':>7s} {'SGPRs':>10s} {'scratch':>8s}")
    for v in sorted(olds):
        a, b = fa[olds[v]], fb[news[v]]
        ra, rb = ma[olds[v]], mb[news[v]]
        verdict = "identical" if a == b else "offsets" if v not in differ else "scalar" if v in scalar else "differs"
        print(f"{label(v):44s} {verdict:10s} {len(a):6d} -> {len(b):4d} {ra['vgpr']:4d} -> {rb['vgpr']:3d} {waves(ra['vgpr']):2d} -> {waves(rb['vgpr']):1d} "
              f"{ra['sgpr']:4d} -> {rb['sgpr']:3d} {ra['scratch']:3d} -> {rb['scratch']:1d}")
        if rb["scratch"] or waves(rb["vgpr"]) < waves(ra["vgpr"]):
            missed.append((label(v), "loses a wave or gains scratch"))
    print("\nthe kernels that differ otherwise, by mnemonic (parent -> branch).  counted: global, buffer, flat, scratch and LDS accesses and "
          "floating-point and conversion instructions")
    for v in differ:
        if v in scalar:
            continue
        ca = Counter(s.split()[0] for s in fa[olds[v]] if COUNTED.match(s))
        cb = Counter(s.split()[0] for s in fb[news[v]] if COUNTED.match(s))
        d = "; ".join(f"{k} {ca[k]} -> {cb[k]}" for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k])
        va = Counter(s.split()[0] for s in vector_stream(fa[olds[v]]))
        vb = Counter(s.split()[0] for s in vector_stream(fb[news[v]]))
        e = "; ".join(f"{k} {va[k]} -> {vb[k]}" for k in sorted(set(va) | set(vb)) if va[k] != vb[k])
        print(f"{label(v):44s} counted: {'all equal' if not d else 'differ: ' + d}; every vector and memory instruction: "
              f"{'all equal, in another order' if not e else 'differ: ' + e}")
        if d:
            missed.append((label(v), "counts by mnemonic"))
    print()
    print("rows that miss a condition:" + ("  none" if not missed else ""))
    for m in missed:
        print("   ", *m)


if __name__ == "__main__":
    main()
