"""Batched sweeps at many members: the cases, the per-member inputs and the cached reference runs that tests/test_polar_many_host.py
pins and tests/test_gpu_polar_many.py compares the kernels with.  Test infrastructure only.

A case is a lattice (chosen by step_tile's tile classes, as in tests/test_gpu_polar_wind.py), a number of members B and a step
count.  Every member has its own mask, tau, U0, Smagorinsky constant, cross-flow, wall distances and reference point, all drawn from
one seeded generator per case, so that a member which runs with another member's value of anything computes another state: the host
test asserts that on the references alone.  B = 67 is prime and above 64, B = 35 is odd, B = 1024 is WTP_MAX_MEMBERS.

The read-backs of a plain batch fall after 5 steps and after every sample_every steps; those of a batch with the models on after every
sample_every steps.  The member walk of the step kernels is reversed on every other step (the step that brings the count to an even
number walks backwards), so states written by either walk are compared in every case.
"""
import functools
import hashlib

import numpy as np

import lbm_numpy
import _ibb_reference as ibb
import _les_reference as les
import _net_cases as nc
import _wind_reference as wind
from _mex_reference import count_links

# name -> (NX, NY, dtype, B, steps, sample_every)
CASES = {
    "67-96x48-f32": (96, 48, "float32", 67, 36, 12),             # ragged tiles only: site_general
    "67-24x300-f32": (24, 300, "float32", 67, 24, 8),            # a FAST / INLET tile of 256 rows and a ragged one that holds row NY-1
    "35-24x140-f64": (24, 140, "float64", 35, 24, 8),            # a tile of 128 rows and a ragged one
    "1024-16x12-f32": (16, 12, "float32", 1024, 21, 7),          # WTP_MAX_MEMBERS: site_general
}
BODY = ("67-96x48-f32", "67-24x300-f32", "35-24x140-f64")        # the cases whose members hold a net_mask body
MAX = "1024-16x12-f32"
FIRST_READ = 5                                                   # a read-back of the plain batch after an odd number of steps
VARIANTS = ("les", "ibb", "wind", "wind+les")                    # one model alone (and wind with the other collision)
VARIANT_STEPS = 24
# the sub-range test: set_masks(first=41) with 5 masks, set_wall_distances(first=43) with 2 members
SUB_CASE, SUB_MASKS, SUB_Q = "67-96x48-f32", (41, 5), (43, 2)


class Members:
    """The inputs of a case's members: masks [B][NY][NX], q [B][8][NY][NX] of the case's dtype, and tau, u0, cs, v0, xref, yref [B]
    doubles.  Every array read-only."""

    def __init__(self, **kw):
        for k, v in kw.items():
            v.setflags(write=False)
            setattr(self, k, v)

    def params(self, m):
        return float(self.tau[m]), float(self.u0[m]), float(self.cs[m]), float(self.v0[m])


def small_mask(nx, ny, m):
    """The body of member m of the 16x12 lattice: a block of 2x3 or 3x2 cells whose orientation and position follow m, with a free
    cell between it and the boundary cells."""
    h, w = (2, 3) if m & 1 == 0 else (3, 2)
    ni, nj = nx - 6, ny - 6
    i0, j0 = 2 + (m >> 1) % ni, 2 + (m // (2 * ni)) % nj
    mask = np.zeros((ny, nx), np.uint8)
    mask[j0:j0 + h, i0:i0 + w] = 255
    assert not mask[[0, 1, ny - 2, ny - 1], :].any() and not mask[:, [0, 1, nx - 2, nx - 1]].any()
    return mask


@functools.lru_cache(maxsize=None)
def members(name):
    nx, ny, dtype, B, _, _ = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 401)
    if name == MAX:
        masks = np.stack([small_mask(nx, ny, m) for m in range(B)])
    else:
        masks = np.stack([nc.net_mask(nx, ny, rng) for _ in range(B)])         # shifted and sprinkled anew for every member
    tau = rng.uniform(0.52, 0.9, B)
    u0 = rng.uniform(0.03, 0.08, B)
    cs = rng.uniform(0.05, 0.2, B)
    cs[rng.choice(B, round(B / 5), replace=False)] = 0.0                     # one member in five is a BGK member
    r = rng.uniform(-0.3, 0.6, B)
    r[rng.choice(B, round(B / 6), replace=False)] = 0.0                      # one in six an axial one
    v0 = u0 * r
    xref = 0.3641 * nx + rng.uniform(-3.0, 3.0, B)
    yref = 0.5 * ny + rng.uniform(-3.0, 3.0, B)
    q = np.stack([nc.random_q(nx, ny, dtype, rng) for _ in range(B)])
    return Members(masks=masks, q=q, tau=tau, u0=u0, cs=cs, v0=v0, xref=xref, yref=yref)


@functools.lru_cache(maxsize=None)
def sub_inputs():
    """What the sub-range test uploads in the middle of SUB_CASE's batch: (masks [5][NY][NX], q [2][8][NY][NX]), read-only."""
    nx, ny, dtype, *_ = CASES[SUB_CASE]
    rng = np.random.default_rng(977)
    masks = np.stack([nc.net_mask(nx, ny, rng) for _ in range(SUB_MASKS[1])])
    q = np.stack([nc.random_q(nx, ny, dtype, rng) for _ in range(SUB_Q[1])])
    masks.setflags(write=False)
    q.setflags(write=False)
    return masks, q


@functools.lru_cache(maxsize=None)
def listed_members():
    """The members of the 1024 batch whose state is compared with the models on: the ends, the neighbours of 64 and 512, and 28 more
    drawn once."""
    fixed = [0, 1, 2, 63, 64, 65, 511, 512, 513, 1021, 1022, 1023]
    rng = np.random.default_rng(1024)
    rest = [m for m in rng.permutation(1024).tolist() if m not in fixed][:28]
    out = sorted(fixed + rest)
    assert len(set(out)) == 40
    return tuple(out)


def plain_marks(name):
    """The step counts at which the plain batch is read back."""
    _, _, _, _, steps, every = CASES[name]
    return (FIRST_READ,) + tuple(range(every, steps + 1, every))


def model_marks(name):
    _, _, _, _, steps, every = CASES[name]
    return tuple(range(every, steps + 1, every))


def walk_is_reversed(step):
    """Whether the step that brings the count to `step` walks the members backwards (rev = steps done before it & 1)."""
    return (step - 1) & 1 == 1


def frozen(out):
    f, macro = out[0], tuple(out[1])
    for a in (f, *macro):
        a.setflags(write=False)
    return f, macro


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_member(variant, mask, steps, tau, u0, cs, v0, q, dtype, f=None):
    """(f, (rho, ux, uy)) of one member after `steps` steps of the variant's reference, from `f` (default: the variant's start state).
    "all" is wind + LES + interpolated walls: wind.run(..., base_step=ibb.step) with q and les_constant(cs)."""
    dtype = np.dtype(dtype)
    c = les.les_constant(cs, dtype)
    if variant == "all":
        return frozen(wind.run(mask, steps, tau, u0, v0, q, c, base_step=ibb.step, dtype=dtype, f=f))
    if variant == "wind":
        return frozen(wind.run(mask, steps, tau, u0, v0, dtype=dtype, f=f))
    if variant == "wind+les":
        return frozen(wind.run(mask, steps, tau, u0, v0, c, base_step=les.step, dtype=dtype, f=f))
    if variant == "les":
        return frozen(les.run(mask, steps, tau, u0, c, dtype, f=f))
    assert variant == "ibb"
    return frozen(ibb.run(mask, steps, tau, u0, q, None, dtype, f=f))


@functools.lru_cache(maxsize=None)
def plain_reference(name, oracle):
    """states[k][m] = (f, (rho, ux, uy)) of member m at plain_marks(name)[k], by `oracle`.run (the C oracle or lbm_numpy)."""
    nx, ny, dtype, B, _, _ = CASES[name]
    mem = members(name)
    out = [[] for _ in plain_marks(name)]
    for m in range(B):
        tau, u0, _, _ = mem.params(m)
        f, done = None, 0
        for k, mark in enumerate(plain_marks(name)):
            f, macro = frozen(oracle.run(mem.masks[m], mark - done, tau, u0, np.dtype(dtype), f=f))
            done = mark
            out[k].append((f, macro))
    return out


@functools.lru_cache(maxsize=None)
def model_reference(name):
    """states[k][m] = (f, (rho, ux, uy)) of member m at model_marks(name)[k] with wind, LES and interpolated walls on."""
    nx, ny, dtype, B, _, every = CASES[name]
    mem = members(name)
    out = [[] for _ in model_marks(name)]
    for m in range(B):
        f = None
        for k in range(len(out)):
            f, macro = run_member("all", mem.masks[m], every, *mem.params(m), mem.q[m], dtype, f=f)
            out[k].append((f, macro))
    return out


@functools.lru_cache(maxsize=None)
def variant_reference(variant):
    """[m] = (f, macro) of SUB_CASE's members after VARIANT_STEPS steps with one model alone."""
    nx, ny, dtype, B, _, _ = CASES[SUB_CASE]
    mem = members(SUB_CASE)
    return [run_member(variant, mem.masks[m], VARIANT_STEPS, *mem.params(m), mem.q[m], dtype) for m in range(B)]


@functools.lru_cache(maxsize=None)
def listed_reference():
    """{m: (f, macro)} of the listed members of the 1024 batch after its steps with wind + LES (half-way walls)."""
    nx, ny, dtype, B, steps, _ = CASES[MAX]
    mem = members(MAX)
    return {m: run_member("wind+les", mem.masks[m], steps, *mem.params(m), None, dtype) for m in listed_members()}


def counts(name):
    """Per member: (FAST interior fluid cells, links, faces) of the case's masks."""
    from _loads_reference import loads_reference
    nx, ny, dtype, B, _, _ = CASES[name]
    mem = members(name)
    ones = np.ones((ny, nx))
    fast = [int((nc.fast_cells(mem.masks[m], dtype) & nc.interior_fluid(mem.masks[m])).sum()) for m in range(B)]
    links = [count_links(mem.masks[m]) for m in range(B)]
    faces = [loads_reference(ones, mem.masks[m], 0.0, 0.0).n for m in range(B)]
    return fast, links, faces
