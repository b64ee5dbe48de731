"""Every batch step kernel on the stability net from a rough start: the cases, their inputs and the reference runs that
tests/test_polar_net_rough_host.py pins and tests/test_gpu_polar_net_rough.py compares the kernels with.  Test infrastructure only.

_net_cases reaches the net by 170 steps from equilibrium and covers k_step_batch with the Smagorinsky collision and with interpolated walls; the rough-start cases of
_restart_cases and _trt_cases cover every step kernel and stay off the net on purpose.  Here the two meet: the variants, members and
steppers of _restart_cases and _trt_cases (all 24 model combinations), the lattices they share with _net_cases, and _net_cases' masks and
wall distances (net_mask keeps TILE_FAST tiles up- and downstream of the body).  Members 0 and 2 start from a rough state whose noise
already lies beyond the bounds (velocity 0.5 against U_MAX = 0.35, density 0.8 about 1 against [0.5, 2.0]), so thousands of cells sit on
all three bounds after the first step, in every tile class; member 1 starts with _restart_cases' amplitudes and stays healthy.

The calls are (1, 2, 1, 3, 5, 7), 19 steps: both walk directions, and a checkpoint at steps 1, 3, 4, 7, 12 and 19.  The noise is of the
shortest wavelength and decays, so the early checkpoints are the crowded ones.
"""
import functools

import numpy as np

import lbm_numpy
import _half_reference as half
import _net_cases as nc
import _restart_cases as rc
import _trt_cases as tc
from _rough_start import insensitive_counts, rough_state

LATTICES = {name: rc.LATTICES[name] for name in ("96x48-f32", "37x299-f32", "24x140-f64")}
assert all(nc.CASES[name] == shape for name, shape in LATTICES.items())
HALF_LATTICES = rc.HALF_LATTICES
B = rc.B
DRIVEN, HEALTHY = (0, 2), 1
SEEDS = tuple(700 + m for m in range(B))
NET_AMPS = dict(amp_u=0.5, amp_rho=0.8, amp_neq=0.02)
CALLS = (1, 2, 1, 3, 5, 7)
MARKS = tuple(int(v) for v in np.cumsum(CALLS))
STEPS = MARKS[-1]
KINDS = nc.KINDS

NATIVE_VARIANTS = rc.NATIVE_VARIANTS + tc.NATIVE_VARIANTS
HALF_VARIANTS = rc.HALF_VARIANTS + tc.HALF_VARIANTS
NATIVE_CASES = [(lat, v, False) for lat in LATTICES for v in NATIVE_VARIANTS]
HALF_CASES = [(lat, v, True) for lat in HALF_LATTICES for v in HALF_VARIANTS]
ALL_CASES = NATIVE_CASES + HALF_CASES
assert len(NATIVE_CASES) == 48 and len(HALF_CASES) == 16 and all(lat in LATTICES for lat in HALF_LATTICES)


def case_id(lattice, variant, stored):
    return f"{lattice}-{variant}-{'half' if stored else 'native'}"


IDS = [case_id(*c) for c in ALL_CASES]


def is_trt(variant):
    return "trt" in variant.split("+")


def stepper(variant, m, mask, q, dtype, stored=False):
    """state -> (state', (rho, ux, uy), ...) of member m: _trt_cases.stepper for a variant with the two-relaxation-time collision,
    _restart_cases.stepper for the others."""
    return (tc.stepper if is_trt(variant) else rc.stepper)(variant, m, mask, q, dtype, stored)


def configure(b, variant, masks, q):
    """The engine calls of a variant, up to and including init_equilibrium."""
    (tc.configure if is_trt(variant) else rc.configure)(b, variant, masks, q)


@functools.lru_cache(maxsize=None)
def starts(lattice):
    """The members' start populations [B][9][NY][NX] of the lattice's dtype, read-only."""
    nx, ny, dtype = LATTICES[lattice]
    f = np.stack([rough_state(nx, ny, rc.U0[m], np.dtype(dtype), SEEDS[m], **(rc.AMPS if m == HEALTHY else NET_AMPS)) for m in range(B)])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def classes_of(lattice, stored):
    """Per member, {class: [NY][NX] bool}: _net_cases.cell_classes for the native kernels; the half kernels have no tile classes, so
    for them the one class "all" of the interior fluid cells."""
    _, _, dtype = LATTICES[lattice]
    masks, _ = nc.inputs(lattice)
    return [{"all": nc.interior_fluid(masks[m])} if stored else nc.cell_classes(masks[m], dtype) for m in range(B)]


class MemberRun:
    """One member's reference run.  Per checkpoint k: states[k] = (state, (rho, ux, uy)), state being populations or, in a half case,
    float16 deviations; events[k] = lbm_numpy.clamp_events of those planes; insensitive[k] = _rough_start.insensitive_counts of the
    populations (Load of the halves) against those one step earlier.  per_step[s][kind][cls] = the cells of that class at that bound
    after step s + 1; finite = every population of every step was; max_abs = the largest |population|."""

    def __init__(self):
        self.states, self.events, self.insensitive, self.per_step = [], [], [], []
        self.finite, self.max_abs = True, 0.0

    def met(self, kind, cls):
        """(step, cell) pairs of the class at the bound over the whole run."""
        return sum(step[kind][cls] for step in self.per_step)


@functools.lru_cache(maxsize=None)
def reference(lattice, variant, stored=False):
    """(masks, q or None, start [B], [MemberRun]), every array read-only.  `stored`: the start is Store of the start populations and
    the states are float16 deviations.  Stepped one step at a time, continued from its own states."""
    nx, ny, dtype = LATTICES[lattice]
    masks, q = nc.inputs(lattice)
    if "ibb" not in variant:
        q = None
    start = starts(lattice)
    if stored:
        start = np.stack([half.store(f) for f in start])
        start.setflags(write=False)
    classes = classes_of(lattice, stored)
    runs = []
    for m in range(B):
        step = stepper(variant, m, masks[m], None if q is None else q[m], dtype, stored)
        run, s = MemberRun(), start[m]
        for n in range(1, STEPS + 1):
            prev = s
            s, macro = step(s)[:2]
            pops = half.load(s) if stored else s
            run.finite = run.finite and bool(np.isfinite(pops).all()) and all(bool(np.isfinite(p).all()) for p in macro)
            run.max_abs = max(run.max_abs, float(np.abs(pops).max()))
            ev = nc.event_cells(macro)
            run.per_step.append({kind: {cls: int((ev[kind] & cells).sum()) for cls, cells in classes[m].items()} for kind in KINDS})
            if n in MARKS:
                for a in (s, *macro):
                    a.setflags(write=False)
                run.states.append((s, macro))
                run.events.append(lbm_numpy.clamp_events(*macro, masks[m]))
                run.insensitive.append(insensitive_counts(pops, half.load(prev) if stored else prev, masks[m]))
        runs.append(run)
    return masks, q, start, runs


def table():
    """The reference's clamp events (density, speed) of every member of every case at the checkpoints, as text."""
    lines = [f"clamp events (density, speed) of the NumPy references at steps {MARKS}; members {DRIVEN} are driven, member {HEALTHY} is healthy",
             f"start: rough_state with {NET_AMPS} (driven), {rc.AMPS} (healthy), seeds {SEEDS}"]
    for case in ALL_CASES:
        runs = reference(*case)[3]
        for m, run in enumerate(runs):
            lines.append(f"{case_id(*case):<40} member {m}  " + "  ".join(f"({a}, {b})" for a, b in run.events))
    return "\n".join(lines) + "\n"
