"""The cases of the two-relaxation-time collision of batched sweeps: what tests/test_polar_trt_host.py (CPU: every reference is finite,
off the stability net, and tells the collision from its neighbours) and tests/test_gpu_polar_trt.py (GPU: the batch kernels against those
references, bit for bit) both read.

Two families.  From equilibrium: the lattices of test_gpu_polar_les.py's CASES (chosen by the step's tile classes), 60 steps, three members
with different tau, U0 and magic number; one tau lies within 1e-3 of 0.5 and the magic numbers are 3/16, 1/4 and 1/12.  From the rough start:
_restart_cases' lattices, members (tau, U0, Smagorinsky constant, cross-flow, seed) and calls (4, 3, 7, 1, 4), every member with a magic
number of its own, under every combination of the collision with the Smagorinsky model, interpolated walls, the inclined free stream and half
storage that a batch can run.
"""
import functools

import numpy as np

import lbm_numpy
import _half_reference as half
import _les_reference as les
import _restart_cases as rc
import _trt_reference as trt

MAGIC = (3.0 / 16.0, 1.0 / 4.0, 1.0 / 12.0)                 # member m's magic number, in both families
OTHER_MAGIC = (1.0 / 12.0, 3.0 / 16.0, 1.0 / 4.0)           # "another magic" of the sensitivity checks

# ---- from equilibrium --------------------------------------------------------------------------
EQ_STEPS = 60
# lattice -> (NX, NY, dtype, members (shape, angle, tau, u0, magic)); the shapes and angles are test_gpu_polar_les.CASES' own
EQ_CASES = {
    "96x48-f32": (96, 48, "float32", [("naca0012", 10.0, 0.5008, 0.04, MAGIC[0]), ("naca2412", 6.0, 0.9, 0.03, MAGIC[1]), ("naca4412", -4.0, 0.62, 0.06, MAGIC[2])]),
    "40x300-f32": (40, 300, "float32", [("block", 0.0, 0.5008, 0.04, MAGIC[0]), ("block", 0.0, 0.56, 0.05, MAGIC[1]), ("block", 0.0, 0.9, 0.03, MAGIC[2])]),
    "37x299-f32": (37, 299, "float32", [("block", 0.0, 0.5008, 0.04, MAGIC[2]), ("block", 0.0, 0.6, 0.06, MAGIC[0]), ("block", 0.0, 2.0, 0.03, MAGIC[1])]),
    "24x140-f64": (24, 140, "float64", [("block", 0.0, 0.5008, 0.04, MAGIC[1]), ("block", 0.0, 0.9, 0.03, MAGIC[2]), ("block", 0.0, 0.58, 0.06, MAGIC[0])]),
}


def eq_masks(name):
    from test_gpu_polar_les import CASES, _masks
    nx, ny, dtype, members = EQ_CASES[name]
    assert CASES[name][:3] == (nx, ny, dtype) and [m[:2] for m in CASES[name][3]] == [m[:2] for m in members]
    return _masks(nx, ny, members)


@functools.lru_cache(maxsize=None)
def eq_reference(name):
    """(masks, per member (f, (rho, ux, uy), the BGK oracle's f)) after EQ_STEPS steps from equilibrium, read-only."""
    nx, ny, dtype, members = EQ_CASES[name]
    masks = eq_masks(name)
    out = []
    for mask, (_, _, tau, u0, magic) in zip(masks, members):
        f, macro = trt.run(mask, EQ_STEPS, tau, u0, magic, dtype=np.dtype(dtype))
        bgk, _ = lbm_numpy.run(mask, EQ_STEPS, tau, u0, np.dtype(dtype))
        for a in (f, bgk, *macro):
            a.setflags(write=False)
        out.append((f, macro, bgk))
    return masks, out


# ---- from the rough start ----------------------------------------------------------------------
NATIVE_VARIANTS = ("trt", "trt+les", "trt+ibb", "trt+ibb+les", "trt+wind", "trt+wind+les", "trt+wind+ibb", "trt+wind+ibb+les")
HALF_VARIANTS = ("trt", "trt+les", "trt+wind", "trt+wind+les")
NATIVE_CASES = [(lat, v) for lat in rc.LATTICES for v in NATIVE_VARIANTS]
HALF_CASES = [(lat, v) for lat in rc.HALF_LATTICES for v in HALF_VARIANTS]
assert len(NATIVE_CASES) + len(HALF_CASES) == 32


def rc_variant(variant):
    """The _restart_cases variant with the same models and the single-relaxation-time collision."""
    rest = [p for p in variant.split("+") if p != "trt"]
    order = [p for p in ("wind", "ibb", "les") if p in rest]
    return "+".join(order) if order else "bgk"


def stepper(variant, m, mask, q, dtype, stored=False, magic=None, swap=False):
    """state -> (state', (rho, ux, uy)) of member m: one step of the variant's reference, on populations or, `stored`, on halves.
    magic: the member's (default MAGIC[m]); swap: tp and tm exchanged in the pairs (a deliberately wrong collision)."""
    tau, u0, cs, v0 = rc.TAU[m], rc.U0[m], rc.CS[m], rc.V0[m]
    lam = MAGIC[m] if magic is None else magic
    c = les.les_constant(cs, dtype) if "les" in variant else None
    base = functools.partial(trt.step, swap=True) if swap else trt.step
    extra = (lam, c, q if "ibb" in variant else None)
    if "wind" in variant:
        base, extra = half.windy(base), (v0, *extra)
    if stored:
        return lambda h: half.half_step(base, h, mask, tau, u0, *extra)
    return lambda f: base(f, mask, tau, u0, *extra)


def _march(step, s):
    prev = res = None
    for _ in range(rc.STEPS):
        prev = s
        res = step(s)
        s = res[0]
    return s, res[1], prev


@functools.lru_cache(maxsize=None)
def reference(lattice, variant, stored=False):
    """(masks, q, start [B], per member (state after STEPS steps, its (rho, ux, uy), the state one step earlier)), read-only.
    `stored`: the states are float16 deviations (the start is Store of the rough state), else populations."""
    nx, ny, dtype = rc.LATTICES[lattice]
    masks, q = rc.setup(lattice, "interpolated" if "ibb" in variant else "halfway")
    start = rc.starts(lattice)
    if stored:
        start = np.stack([half.store(f) for f in start])
        start.setflags(write=False)
    out = []
    for m in range(rc.B):
        s, macro, prev = _march(stepper(variant, m, masks[m], None if q is None else q[m], dtype, stored), start[m])
        for a in (s, prev, *macro):
            a.setflags(write=False)
        out.append((s, macro, prev))
    return masks, q, start, out


def alternatives(lattice, variant, stored=False):
    """Per member, the final states of three neighbours of the case's reference from the same masks and starts: the same models with the
    single-relaxation-time collision ("bgk"), tp and tm exchanged ("swap"), and another magic number ("magic")."""
    nx, ny, dtype = rc.LATTICES[lattice]
    masks, q, start, _ = reference(lattice, variant, stored)
    out = []
    for m in range(rc.B):
        qm = None if q is None else q[m]
        out.append({
            "bgk": _march(rc.stepper(rc_variant(variant), m, masks[m], qm, dtype, stored), start[m])[0],
            "swap": _march(stepper(variant, m, masks[m], qm, dtype, stored, swap=True), start[m])[0],
            "magic": _march(stepper(variant, m, masks[m], qm, dtype, stored, magic=OTHER_MAGIC[m]), start[m])[0],
        })
    return out


def configure(b, variant, masks, q):
    """The engine calls of a variant, up to and including init_equilibrium."""
    rc.configure(b, rc_variant(variant), masks, q)
    b.enable_trt(MAGIC)


def interior_fluid(mask):
    inner = np.zeros(mask.shape, bool)
    inner[1:-1, 1:-1] = True
    return inner & (np.asarray(mask) == 0)
