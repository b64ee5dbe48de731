"""The plain-column loop of the four-step fp32 marching kernel divides the two momenta of a site by its density on ONE reciprocal
(div2_shared / collide2_shared in csrc/step_march.hpp): no v_div_scale / v_div_fmas / v_div_fixup on that path, and the instructions they cost gone.

Same ISA, same loop and same branch-following policy as test_marching_loop_instruction_budget (tests/test_build_hazards.py, tools/isa_loops.py): the
path of a column without body, clamp or far-field rows, whose every site lies inside the ranges of veldiv_guard."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_store_hazard as chk          # noqa: E402
import isa_loops as L                     # noqa: E402

SYM = "_ZN2wt8k_march3IfLi2ELi4ELb0ELi%dEEEvNS_11MarchParamsIT_EE"
# FD -> (memory instructions, packed at most, executed / vector at most: the counts of this change + 1 %, the parent's executed / vector counts)
#   17: two-operation division by tau, tiling windows    886 / 732
#    1: three-operation division by tau                  922 / 768
#   49: overlapping windows                              849 / 715
LOOPS = {17: (21, 496, 894, 739, 1030, 805), 1: (21, 532, 931, 775, 1066, 841), 49: (18, 496, 857, 722, 985, 785)}
DIVISION_PARTS = ("v_div_scale", "v_div_fmas", "v_div_fixup")


@pytest.fixture(scope="module")
def isa_file():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    return [p for p in chk.build() if "windtunnel" in os.path.basename(p)][0]


def _path_ops(lines, header, limit=20000):
    """The mnemonics L.follow(lines, header) counts, in order: one trip round the loop under its default policy."""
    taken = {"s_cbranch_execz": True, "s_cbranch_scc0": True, "s_cbranch_vccnz": True}
    pos = {m.group(1): i for i, l in enumerate(lines) for m in [L.LABEL.match(l)] if m}
    ops, i = [], pos[header] + 1
    while len(ops) < limit:
        s = lines[i].strip()
        i += 1
        if lines[i - 1].startswith(header + ":"):
            break
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        op = s.split()[0]
        ops.append(op)
        if op == "s_branch" or (op.startswith("s_cbranch") and taken.get(op, False)):
            i = pos[s.split()[1]]
    return ops


def _plain_column_loop(lines, vmem):
    """The chain units' loop as the budget test picks it: the shortest trip of 700 .. 1300 executed instructions with `vmem` memory instructions."""
    best = None
    for tgt, _, _, c, _ in L.loops(lines):
        if not (800 < sum(c.values()) < 4000):
            continue
        try:
            cc, _ = L.follow(lines, tgt)
        except (KeyError, IndexError):
            continue
        tot = sum(cc.values())
        if 700 < tot < 1300 and cc.get("vmem", 0) == vmem and (best is None or tot < sum(best[1].values())):
            best = (tgt, cc)
    return best


@pytest.mark.parametrize("fd", sorted(LOOPS))
def test_plain_column_loop_shares_the_reciprocal(isa_file, fd):
    vmem, pk_max, ex_max, valu_max, ex_parent, valu_parent = LOOPS[fd]
    assert ex_max <= ex_parent - 90 and valu_max <= valu_parent - 50          # what the change is for
    name, lines = L.kernel_lines(isa_file, SYM % fd)
    assert name == SYM % fd
    best = _plain_column_loop(lines, vmem)
    assert best is not None, f"no marching loop found in {name}"
    tgt, cc = best
    executed, valu = sum(cc.values()), sum(v for k, v in cc.items() if k.startswith("v_"))
    print(f"FD {fd}: {executed} executed, {valu} vector, {cc.get('v_pk', 0)} packed, {cc.get('vmem', 0)} memory instructions per trip")
    assert cc.get("vmem", 0) == vmem and cc.get("v_pk", 0) <= pk_max, cc
    assert executed <= ex_max and valu <= valu_max, (executed, valu, ex_max, valu_max)
    ops = _path_ops(lines, tgt)
    assert len(ops) == executed                                               # the same path
    left = [op for op in ops if op.startswith(DIVISION_PARTS)]
    assert left == [], left
