"""A start state in which no two sites are alike, the check that a reference computed from it can tell a misplaced read, and the cases that
tests/test_rough_start_host.py (CPU: every reference is sensitive, and on or off the stability net as meant) and tests/test_gpu_rough_start.py
(GPU: the stepping kernels against those references, bit for bit) both read.

From init_equilibrium a disturbance leaves the body and the borders at one cell per step; every site farther away holds the same nine numbers as
its neighbours, and a kernel that reads the right value from the wrong column, row or step computes the right bits there.  From rough_state every
such read changes bits — assert_sensitive is the condition that makes that true of a given reference."""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from lbm_numpy import E, clamp_events, weights

TAU, U0 = 0.58, 0.06
CALLS = (4, 3, 7, 1, 6)                         # whole passes, remainders 3 = 3 and 7 = 4 + 3 or 3 + 2 + 2, a single step
STEPS = sum(CALLS)
SEAM = 64                                       # rows of the smallest marching window (fp64); every seam of 128-row windows is one of these
NAMES = ("f", "rho", "ux", "uy")


def rough_state(nx, ny, u0, dtype, seed, amp_u=0.03, amp_rho=0.03, amp_neq=0.02):
    """f[9][NY][NX]: the equilibrium of a density 1 + amp_rho r and a velocity (u0 + amp_u r, amp_u r), every population scaled by 1 + amp_neq r;
    r uniform in [-1, 1), independent per site and per field.  Computed in float64 and rounded once to `dtype`."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(-1.0, 1.0, size=(12, ny, nx))
    rho = 1.0 + amp_rho * r[0]
    ux = float(u0) + amp_u * r[1]
    uy = amp_u * r[2]
    uu = ux * ux + uy * uy
    w = weights(np.float64)
    f = np.empty((9, ny, nx), np.float64)
    for k, (ex, ey) in enumerate(E):
        eu = ex * ux + ey * uy
        f[k] = float(w[k]) * rho * (1.0 + 3.0 * eu + 4.5 * eu * eu - 1.5 * uu) * (1.0 + amp_neq * r[3 + k])
    return f.astype(dtype)


def body_mask(nx, ny, seed):
    """The generator of test_gpu_tiling_windows._mask reduced to: a NACA 4412 at 12 degrees, runs of solids on rows s - 3 .. s + 2 about every
    64-row seam (what the seam flags cover), solids on columns 0 - 2 and NX - 3 .. NX - 1 (inlet and outlet inside the march), on row 0 and on
    row NY - 1."""
    from airfoil_cfd_tool_amd import geometry
    rng = np.random.default_rng(seed)
    m = np.array(geometry.build_geometry(nx, ny, 12.0, None, "naca4412").mask, dtype=np.uint8)
    for s in range(SEAM, ny, SEAM):
        for r in range(s - 3, min(s + 3, ny)):
            x0 = int(rng.integers(0, nx))
            m[r, x0:x0 + int(rng.integers(1, max(2, nx // 4)))] = 1
    for row in (0, ny - 1):
        x0 = int(rng.integers(0, nx - 2))
        m[row, x0:x0 + int(rng.integers(1, nx // 2 + 1))] = 1
    for cols in (slice(0, 3), slice(nx - 3, nx)):
        y0 = int(rng.integers(1, ny - 1))
        m[y0:y0 + int(rng.integers(1, ny // 4 + 2)), cols] = 1
    return m


def _bits(f):
    f = np.ascontiguousarray(f)
    return f.view(np.uint32 if f.dtype == np.float32 else np.uint64)


def _like_neighbour(f):
    """[8][NY - 2][NX - 2]: the nine populations of an interior site are bit-equal to those of its neighbour in direction E[1 + k]."""
    b = _bits(f)
    _, ny, nx = b.shape
    mid = b[:, 1:ny - 1, 1:nx - 1]
    return np.stack([(mid == b[:, 1 + ey:ny - 1 + ey, 1 + ex:nx - 1 + ex]).all(axis=0) for ex, ey in E[1:]])


def uniform_share(f):
    """The share of interior sites whose nine populations are bit-equal to those of ALL eight neighbours: what a test is blind on."""
    return float(_like_neighbour(f).all(axis=0).mean())


def insensitive_counts(ref_f, ref_prev_f, mask):
    """Among interior fluid sites: (sites bit-equal to any one fluid neighbour, sites bit-equal to their own state one step earlier)."""
    fluid = np.asarray(mask) == 0
    ny, nx = fluid.shape
    mid = fluid[1:ny - 1, 1:nx - 1]
    like = _like_neighbour(ref_f)
    for k, (ex, ey) in enumerate(E[1:]):
        like[k] &= fluid[1 + ey:ny - 1 + ey, 1 + ex:nx - 1 + ex]
    same = (_bits(ref_f) == _bits(ref_prev_f)).all(axis=0)[1:ny - 1, 1:nx - 1]
    return int((like.any(axis=0) & mid).sum()), int((same & mid).sum())


def assert_sensitive(ref_f, ref_prev_f, mask):
    """The condition under which a comparison with ref_f notices a read from the wrong site or the wrong step.  Both counts are zero by
    choice of the input: a case that does not meet them is a wrong case."""
    assert mask.shape[0] > 2 and mask.shape[1] > 2 and (mask[1:-1, 1:-1] == 0).any()
    assert np.isfinite(ref_f).all() and np.isfinite(ref_prev_f).all()
    like, same = insensitive_counts(ref_f, ref_prev_f, mask)
    assert like == 0, f"{like} interior fluid sites hold the bits of a fluid neighbour"
    assert same == 0, f"{same} interior fluid sites hold the bits they held one step earlier"


# --------------------------------------------------------------------------------------------------------------------------------------------
# the cases
# --------------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One reference: the oracle's run of `steps` steps over `mask` from rough_state(seed, amp_u).  `before`: (mask, steps) run first from
    that start (a mask change in mid-run).  `net`: the run is meant to reach the speed clamp."""
    nx: int
    ny: int
    mask: str                                   # "empty" or "body"
    dtype: str
    steps: int = STEPS
    tau: float = TAU
    seed: int = 1
    amp_u: float = 0.03
    before: Optional[Tuple[str, int]] = None
    net: bool = False

    @property
    def id(self):
        tag = f"{self.nx}x{self.ny}-{self.mask}-{self.dtype}-{self.steps}-tau{self.tau:.6g}-seed{self.seed}"
        return tag + ("-net" if self.net else "") + (f"-after-{self.before[0]}{self.before[1]}" if self.before else "")


def f32_from_bits(bits):
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


_MASKS = {}


def mask_of(kind, nx, ny):
    """The mask of a case (shared, read-only)."""
    key = (kind, nx, ny)
    if key not in _MASKS:
        m = np.zeros((ny, nx), np.uint8) if kind == "empty" else body_mask(nx, ny, 4100 + nx + ny)
        m.setflags(write=False)
        _MASKS[key] = m
    return _MASKS[key]


def start_of(case):
    return rough_state(case.nx, case.ny, U0, np.dtype(case.dtype), case.seed, amp_u=case.amp_u)


def reference(oracle, case, with_prev=False):
    """(start state, mask, the oracle's populations, its (rho, ux, uy)[, its populations one step earlier])."""
    f0 = start_of(case)
    f, mask = f0, mask_of(case.mask, case.nx, case.ny)
    if case.before:
        f, _ = oracle.run(mask_of(case.before[0], case.nx, case.ny), case.before[1], case.tau, U0, np.dtype(case.dtype), f=f)
    if not with_prev:
        ref_f, ref_m = oracle.run(mask, case.steps, case.tau, U0, np.dtype(case.dtype), f=f)
        return f0, mask, ref_f, ref_m
    prev, _ = oracle.run(mask, case.steps - 1, case.tau, U0, np.dtype(case.dtype), f=f)
    ref_f, ref_m = oracle.run(mask, 1, case.tau, U0, np.dtype(case.dtype), f=prev)
    return f0, mask, ref_f, ref_m, prev


def net_counts(oracle, case):
    """The oracle's clamp events after every call of CALLS, and its state at the end."""
    f, mask, counts = start_of(case), mask_of(case.mask, case.nx, case.ny), []
    for n in CALLS:
        f, macro = oracle.run(mask, n, case.tau, U0, np.dtype(case.dtype), f=f)
        counts.append(clamp_events(*macro, mask))
    return counts, f, macro


def clamp_counts(case, ref_m):
    """wt_clamp_events counted on the oracle's (rho, ux, uy)."""
    return clamp_events(*ref_m, mask_of(case.mask, case.nx, case.ny))


DTYPES = ("float32", "float64")
MASKS = ("empty", "body")
# a. every kernel form: (NX, NY, fuse_chunk).  64 x 262 in units of six columns: one chain block, [24, 48), and solo units; 128 + 128 + 6 rows on
# fp32 tiling windows, 120 + 120 + 22 on overlapping ones, four 64-row windows + 6 for fp64.  150 x 390 in units of nine.
SMALL = ((64, 262, 6), (150, 390, 9))
# b. the division by tau of the four-step fp32 kernel: (tau bits, fast_div, fast_div_two_op_active, pass_depth)
DIVISIONS = ((0x3f147ae1, 1, 1.0, 4), (0x3f5119d3, 1, 0.0, 4), (0x3f147ae1, 0, 0.0, 3))
# c. the stability net.  The velocity noise of a site is of the shortest wavelength and decays within a dozen steps at this tau, so no amplitude
# leaves a site on the net after the 21 steps: the oracle's counts over the steps run (0, 33), (0, 30), (0, 10), (0, 3), (0, 2), (0, 0), .. at 0.3
# and (111, 2002), (61, 1413), (21, 815), (5, 266), (0, 141), (0, 46), (0, 31), (0, 12), (0, 2), (0, 1), (0, 1), (0, 0), .. at 0.5.  The count is
# therefore taken after every call of CALLS (net_counts), and the amplitude is the first of 0.3, 0.4, 0.5 at which the first two of them (steps 4 and
# 7) hold speed clamps; at 0.5 the first holds density clamps too, and the start state holds negative populations.
NET_AMP_U = 0.5
# d. the plan cut by measured time
LARGE = (1000, 646)
# e. switches in mid-run: 320 x 240 and 320 x 480 hold as many 120-row as 128-row windows
SWITCH_NX, SWITCH_NY, SWITCH_FIRST, SWITCH_THEN = 320, (240, 480), 9, 10
# f. three slabs cut by the caller
SLAB_NX, SLAB_NY, SLAB_EDGES, SLAB_HALO, SLAB_CALLS = 150, 390, (0, 47, 101, 150), 13, (30, 17)
# g. the shortest units: (NX, NY, fuse_chunk).  A cost limit of one column (every column costs one or more) makes the cut by columns close a unit
# after every marched column, whatever the mask, except where that would leave a window's last unit — the one that also emits the outlet column —
# shorter than a four-step pass allows (two columns): one marched column per unit at two and three steps per pass, at four steps one per unit and
# two in the last.  tests/_march_plan_check.hip holds that of build_march_plan.  The lattice is SMALL[0]'s: the same references.
SHORTEST = (64, 262, 1)


def shortest_unit_count(nx, ny, depth, dtype, overlap):
    """fuse_units of a SHORTEST plan without chain blocks: the marched columns 0 .. NX - 2 of every window, one unit each (four steps: the last
    two columns in one); a plan of overlapping windows is dealt to the eight XCDs in whole workgroups of four units (padded with empty units)
    once it holds 16 workgroups or more."""
    rows = 64 if dtype == "float64" else (120 if overlap else 128)          # from window to window
    live = -(-ny // rows) * (nx - 1 - (1 if depth == 4 else 0))
    groups = -(-live // 4)
    return 32 * -(-groups // 8) if overlap and groups >= 16 else live


def case_small(nx, ny, mask, dtype):
    return Case(nx, ny, mask, dtype, seed=11)


def case_division(tau_bits):
    return Case(64, 262, "empty", "float32", tau=f32_from_bits(tau_bits), seed=12)


def case_net(mask, dtype):
    return Case(64, 262, mask, dtype, seed=13, amp_u=NET_AMP_U, net=True)


def case_large(mask, dtype):
    return Case(LARGE[0], LARGE[1], mask, dtype, seed=14)


def case_layout_switch(ny, dtype="float32"):
    return Case(SWITCH_NX, ny, "body", dtype, steps=SWITCH_FIRST + SWITCH_THEN, seed=15)


def case_rewrite(ny, dtype):
    """The second state of a run that is written over after SWITCH_FIRST steps (the first is case_layout_switch's start)."""
    return Case(SWITCH_NX, ny, "body", dtype, steps=SWITCH_THEN, seed=16)


def case_mask_change(ny, dtype):
    return Case(SWITCH_NX, ny, "body", dtype, steps=SWITCH_THEN, seed=15, before=("empty", SWITCH_FIRST))


def case_slabs(dtype):
    return Case(SLAB_NX, SLAB_NY, "body", dtype, steps=sum(SLAB_CALLS), seed=17)


def all_cases():
    cases = [case_small(nx, ny, m, d) for nx, ny, _ in SMALL for m in MASKS for d in DTYPES]
    cases += [case_division(bits) for bits in sorted({d[0] for d in DIVISIONS})]
    cases += [case_net(m, d) for m in MASKS for d in DTYPES]
    cases += [case_large(m, d) for m in MASKS for d in DTYPES]
    for ny in SWITCH_NY:
        cases += [case_layout_switch(ny)]
        cases += [c(ny, d) for c in (case_rewrite, case_mask_change) for d in DTYPES]
    cases += [case_slabs(d) for d in DTYPES]
    assert len(set(cases)) == len(cases)
    return cases


ALL_CASES = all_cases()
