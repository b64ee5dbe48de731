#!/usr/bin/env python3
"""Two builds of csrc/polar.hip compared function by function across the fold of k_wallvel_batch into k_step_batch<..., WALL_MOVING, ...> and
of the four momentum-exchange kernels into k_mex_batch<E, Link> (profiles/polar_host_once_isa.txt).

    python tools/polar_host_once_table.py PARENT.s BRANCH.s      # the gfx950 .s files of tools/check_store_hazard.py build() at either commit

A function is its instruction lines, comments and directives stripped, labels renumbered (tools/isa_fold_table.py funcs).  The parent's
k_wallvel_batch<T, EMIT, LOADMODE, COLL, FAR> is paired with the branch's k_step_batch<T, EMIT, LOADMODE, COLL, 2, FAR>, the parent's
k_mex_batch<T>, k_mex_ibb_batch<T>, k_mex_wallvel_batch<T> and k_mex_half_batch with the branch's k_mex_batch<E, Link> of the same element
and rule; every other function with the one of the same symbol.  Required: every pair but the mex kernels identical instruction for
instruction with equal VGPRs, SGPRs, scratch and LDS; every mex pair with equal VGPRs, SGPRs and LDS, no scratch, and equal counts by
mnemonic of every vector and memory instruction."""
import os
import re
import sys
from collections import Counter

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import isa_fold_table as F                      # noqa: E402
import _polar_isa as P                          # noqa: E402
from polar_step_fold_table import vector_stream  # noqa: E402

WALLVEL = re.compile(r"^_Z\d+k_wallvel_batchI([fd])((?:L[bi]\d+E)+)E")
OLD_MEX = re.compile(r"^_Z\d+k_mex_(|ibb_|wallvel_|half_)batch(?:I([fd])Ev|P)")      # (k_mex_half_batch was no template)
RULES = {"": "Halfway", "ibb_": "Interp", "wallvel_": "Moving", "half_": "Halfway"}


def old_step(name):
    """the parent's step kernels read as (storage, T, EMIT, COLL, WALL, FAR)"""
    m = WALLVEL.match(name)
    if not m:
        return P.step_variant(name)
    a = [int(x) for x in re.findall(r"L[bi](\d+)E", m.group(2))]
    return ("native", m.group(1), a[0], a[2], P.MOVING, a[3])


def old_mex(name):
    """the parent's mex kernels read as (E, link rule)"""
    m = OLD_MEX.match(name)
    if not m:
        return None
    return ("half" if m.group(1) == "half_" else m.group(2), RULES[m.group(1)])


def main():
    pa, pb = sys.argv[1], sys.argv[2]
    fa, fb = F.funcs(pa), F.funcs(pb)
    ma, mb = F.meta(pa), F.meta(pb)
    pairs, mex = [], []
    new_step = {P.step_variant(k): k for k in fb if P.step_variant(k)}
    new_mex = {P.mex_variant(k): k for k in fb if P.mex_variant(k)}
    unpaired = []
    for k in fa:
        if old_step(k):
            pairs.append((k, new_step.pop(old_step(k), None)))
        elif old_mex(k):
            mex.append((k, new_mex.pop(old_mex(k), None)))
        else:
            pairs.append((k, k if k in fb else None))
    unpaired = [a for a, b in pairs + mex if b is None]
    extra = sorted(set(fb) - {b for _, b in pairs + mex})
    nstep = sum(1 for a, _ in pairs if old_step(a))
    moving = sum(1 for a, _ in pairs if WALLVEL.match(a))
    print(f"functions: parent {len(fa)}, branch {len(fb)}; parent functions without a partner: {len(unpaired)}; branch functions without one: {len(extra)}")
    print(f"step kernels: {nstep} pairs, {moving} of them k_wallvel_batch -> k_step_batch<..., WALL_MOVING, ...>; "
          f"the branch holds exactly the 120 + 12 built ones: {set(P.step_variant(k) for k in fb if P.step_variant(k)) == P.step_variants_built()}")
    same = [(a, b) for a, b in pairs if b and fa[a] == fb[b]]
    res = [(a, b) for a, b in pairs if b and (ma.get(a) != mb.get(b))]
    print(f"every function but the momentum-exchange kernels: {len(pairs)} pairs, {len(same)} identical instruction for instruction, "
          f"{len(pairs) - len(res)} with equal VGPRs, SGPRs, scratch and LDS")
    for a, b in pairs:
        if b and (fa[a] != fb[b] or ma.get(a) != mb.get(b)):
            print(f"    DIFFERS: {a} -> {b}  {ma.get(a)} -> {mb.get(b)}")
    print(f"    of the {moving} moving-wall step kernels: {sum(1 for a, b in same if WALLVEL.match(a))} identical; "
          f"with scratch: {sum(1 for a, b in pairs if WALLVEL.match(a) and mb[b]['scratch'])}")
    print()
    print("momentum-exchange kernels (parent -> branch)")
    print(f"{'E, rule':16s} {'verdict':34s} {'instructions':>14s} {'VGPRs':>10s} {'SGPRs':>10s} {'scratch':>8s} {'LDS':>14s}")
    missed = list(unpaired) + extra
    for a, b in sorted(mex, key=lambda p: str(old_mex(p[0]))):
        if b is None:
            continue
        la, lb, ra, rb = fa[a], fb[b], ma[a], mb[b]
        va, vb = vector_stream(la), vector_stream(lb)
        ca, cb = Counter(s.split()[0] for s in va), Counter(s.split()[0] for s in vb)
        allc = Counter(s.split()[0] for s in la), Counter(s.split()[0] for s in lb)
        if la == lb:
            verdict = "identical"
        elif va == vb:
            verdict = "same vector and memory stream"
        elif ca == cb:
            verdict = "same vector and memory mnemonics"
        else:
            verdict = "DIFFERS"
        e, rule = old_mex(a)
        print(f"{e + ', ' + rule:16s} {verdict:34s} {len(la):6d} -> {len(lb):4d} {ra['vgpr']:4d} -> {rb['vgpr']:3d} {ra['sgpr']:4d} -> {rb['sgpr']:3d} "
              f"{ra['scratch']:3d} -> {rb['scratch']:1d} {ra['lds']:6d} -> {rb['lds']:5d}")
        d = "; ".join(f"{k} {allc[0][k]} -> {allc[1][k]}" for k in sorted(set(allc[0]) | set(allc[1])) if allc[0][k] != allc[1][k])
        print(f"{'':16s} counts by mnemonic, every instruction: {'all equal' if not d else d}")
        if ca != cb or rb["scratch"] or any(ra[k] != rb[k] for k in ("vgpr", "sgpr", "lds")):
            missed.append(b)
    missed += [b or a for a, b in pairs if b is None or fa[a] != fb[b] or ma.get(a) != mb.get(b)]
    print()
    print("rows that miss a condition:" + ("  none" if not missed else ""))
    for m in missed:
        print("   ", m)


if __name__ == "__main__":
    main()
