"""The rough-start cases of the batched step kernels: what tests/test_polar_restart_host.py (CPU: every reference is sensitive and off the
stability net, and every model under test acts) and tests/test_gpu_polar_restart.py (GPU: the batch kernels against those references, bit
for bit) both read.  The start states are _rough_start.rough_state's and the bodies _rough_start.body_mask's; a batch can take them since
wtp_write_f exists.

Every case has three members with different tau, U0, Smagorinsky constant, cross-flow and seed, so member m's state is never member
m +- 1's, and runs 19 steps as calls of (4, 3, 7, 1, 4): both walk directions, emitting and non-emitting steps.  The lattices are chosen by
the step's tile classes, as in test_gpu_polar_les.py: 96x48 fp32 has ragged tiles only; 37x299 fp32 a FAST tile of 256 rows and a ragged one
per column, odd NX and NY, and two 256-row runs of the half kernel; 24x140 fp64 a FAST tile of 128 rows and a ragged one.

Amplitudes (velocity, density, non-equilibrium): rough_state's defaults 0.03 / 0.03 / 0.02, for the native cases and for the half ones:
at binary16 they too leave no interior fluid site with the bits of a neighbour or of itself one step earlier (the host test asserts it).
"""
import functools

import numpy as np

import lbm_numpy
import _half_reference as half
import _ibb_reference as ibb
import _les_reference as les
import _wind_reference as wind
from _rough_start import body_mask, rough_state

LATTICES = {"96x48-f32": (96, 48, "float32"), "37x299-f32": (37, 299, "float32"), "24x140-f64": (24, 140, "float64")}
HALF_LATTICES = ("96x48-f32", "37x299-f32")
# (tau, u0, cs, v0 / u0, seed, (shape, angle) of the airfoil of the interpolated walls at 96x48)
MEMBERS = ((0.56, 0.08, 0.17, 0.6, 31, ("naca2412", 6.0)), (0.9, 0.03, 0.0, -0.25, 32, ("naca0012", 10.0)), (0.62, 0.06, 0.1, 0.3, 33, ("naca4412", -4.0)))
B = len(MEMBERS)
CALLS = (4, 3, 7, 1, 4)
STEPS = sum(CALLS)
AMPS = dict(amp_u=0.03, amp_rho=0.03, amp_neq=0.02)
NATIVE_VARIANTS = ("bgk", "les", "ibb", "ibb+les", "wind", "wind+les", "wind+ibb", "wind+ibb+les")
HALF_VARIANTS = ("bgk", "les", "wind", "wind+les")
NATIVE_CASES = [(lat, v) for lat in LATTICES for v in NATIVE_VARIANTS]
HALF_CASES = [(lat, v) for lat in HALF_LATTICES for v in HALF_VARIANTS]

TAU = [m[0] for m in MEMBERS]
U0 = [m[1] for m in MEMBERS]
CS = [m[2] for m in MEMBERS]
V0 = [m[1] * m[3] for m in MEMBERS]


def _random_q(nx, ny, dtype, rng):
    """Wall distances in (0, 1] in every entry, with exact 0.5, exact 1, values close to 0 and just below 0.5 among them
    (test_gpu_polar_ibb._random_q's recipe)."""
    q = 1.0 - rng.random((8, ny, nx))
    pick = rng.random(q.shape)
    q[pick < 0.10] = 0.5
    q[(pick >= 0.10) & (pick < 0.20)] = 1.0
    q[(pick >= 0.20) & (pick < 0.25)] = 2.0 ** -12
    q[(pick >= 0.25) & (pick < 0.30)] = np.nextafter(0.5, 0.0)
    q = q.astype(dtype)
    assert (q > 0).all() and (q <= 1).all()
    return q


@functools.lru_cache(maxsize=None)
def setup(lattice, walls):
    """(masks [B][NY][NX], q [B][8][NY][NX] of the lattice's dtype or None), read-only.  walls "halfway": body_mask, no distances.
    "interpolated": at 96x48 an airfoil per member with geometry.wall_distances' true distances, on the block lattices body_mask with a
    seeded random field in (0, 1]."""
    from airfoil_cfd_tool_amd import geometry
    nx, ny, dtype = LATTICES[lattice]
    masks = [body_mask(nx, ny, 500 + 7 * m + nx) for m in range(B)]
    q = None
    if walls == "interpolated":
        if lattice == "96x48-f32":
            geoms = [geometry.build_geometry(nx, ny, a, None, s) for *_, (s, a) in MEMBERS]
            masks = [np.array(g.mask, dtype=np.uint8) for g in geoms]
            q = [geometry.wall_distances(g.xp, g.yp, g.mask, nx, ny).astype(dtype) for g in geoms]
        else:
            rng = np.random.default_rng(900 + nx)
            q = [_random_q(nx, ny, dtype, rng) for _ in range(B)]
        q = np.stack(q)
        q.setflags(write=False)
    masks = np.stack(masks)
    masks.setflags(write=False)
    return masks, q


@functools.lru_cache(maxsize=None)
def starts(lattice):
    """The members' rough start states [B][9][NY][NX] of the lattice's dtype, read-only."""
    nx, ny, dtype = LATTICES[lattice]
    f = np.stack([rough_state(nx, ny, U0[m], np.dtype(dtype), MEMBERS[m][4], **AMPS) for m in range(B)])
    f.setflags(write=False)
    return f


def stepper(variant, m, mask, q, dtype, stored=False):
    """state -> (state', (rho, ux, uy)[, te]) of member m: one step of the variant's reference, on populations or, `stored`, on halves."""
    tau, u0, cs, v0 = TAU[m], U0[m], CS[m], V0[m]
    c = les.les_constant(cs, dtype)
    if "ibb" in variant:
        base, extra = ibb.step, (q, c if "les" in variant else None)
    elif "les" in variant:
        base, extra = les.step, (c,)
    else:
        base, extra = lbm_numpy.step, ()
    if "wind" in variant:
        base, extra = half.windy(base), (v0, *extra)
    if stored:
        return lambda h: half.half_step(base, h, mask, tau, u0, *extra)
    return lambda f: base(f, mask, tau, u0, *extra)


@functools.lru_cache(maxsize=None)
def reference(lattice, variant, stored=False):
    """(masks, q, start [B], per member (state after STEPS steps, its (rho, ux, uy), the state one step earlier, te of the last step or
    None)).  `stored`: the states are float16 deviations (the start is Store of the rough state), else populations."""
    nx, ny, dtype = LATTICES[lattice]
    masks, q = setup(lattice, "interpolated" if "ibb" in variant else "halfway")
    start = starts(lattice)
    if stored:
        start = np.stack([half.store(f) for f in start])
        start.setflags(write=False)
    out = []
    for m in range(B):
        step = stepper(variant, m, masks[m], None if q is None else q[m], dtype, stored)
        s, prev, res = start[m], None, None
        for _ in range(STEPS):
            prev = s
            res = step(s)
            s = res[0]
        te = res[2] if len(res) > 2 else None
        for a in (s, prev, *res[1]):
            a.setflags(write=False)
        out.append((s, res[1], prev, te))
    return masks, q, start, out


def configure(b, variant, masks, q):
    """The engine calls of a variant, up to and including init_equilibrium."""
    b.set_masks(masks)
    if "ibb" in variant:
        b.enable_interpolated_walls()
        b.set_wall_distances(q)
    if "les" in variant:
        b.enable_les(CS)
    if "wind" in variant:
        b.enable_wind(V0)
    b.init_equilibrium(U0)
