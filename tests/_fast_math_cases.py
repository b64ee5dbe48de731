"""The contracted (option "fast_math") marching kernels from a rough start: a NumPy model of csrc/d2q9.hpp collide_contracted, the cases and call
patterns, and the references that tests/test_fast_math_host.py (CPU: the references are usable — the model stays inside half the device's bound,
injected misreads and wrong collisions leave it) and tests/test_gpu_fast_math_rough.py (GPU: every contracted kernel form against them) both read.

v_rcp_f32 and v_rsq_f32 cannot be reproduced on the CPU, so the device is held to a bound, not to bits: max |device - fp64 oracle| <= BOUND * d32
per plane (f, rho, ux, uy) at every call boundary, where d32 = max |fp32 oracle - fp64 oracle| over that plane at that step count — the rounding
noise of the bit-exact arithmetic on the very case, computed here at every comparison and never written down.  The fp64 oracle starts from the
float64 copy of the fp32 rough state.  No code under test enters the yardstick."""
from collections import namedtuple

import numpy as np

import _rough_start as rs
from lbm_numpy import E, OPP, RHO_MAX, RHO_MIN, U_MAX, clamp_events
from lbm_numpy import step as ieee_step

BOUND = 4.0                                     # the device: at most BOUND * d32 from the fp64 oracle, per plane, at every boundary
MODEL_BOUND = 2.0                               # the model: half of it
RHO_TOL, U_TOL = 1e-5, 5e-6                     # BASELINE.md's tolerance (tests/test_gpu_fast_math.py); BOUND * d32 stays below it
EVEN = (4, 6, 2, 10)                            # every depth takes these in whole contracted passes
ODD = (3, 7, 5, 9)                              # depths 3 and 4 only: a two-step plan would take single steps, which collide in IEEE arithmetic
NAMES = rs.NAMES
NEAR = 1e-5                                     # no site of a net reference this close (relative) to a clamp threshold


# --------------------------------------------------------------------------------------------------------------------------------------------
# the model
# --------------------------------------------------------------------------------------------------------------------------------------------
def omega_of(tau, T=np.float32):
    """What FastDiv.rtau holds (make_fastdiv): tau rounded to binary32, then RN(1 / tau) in binary32."""
    return T(1.0) / T(tau)


def _fma(a, b, c, T):
    """fmaf through float64: the product of two binary32 numbers is exact there, the sum is rounded twice."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(T)


def _nudge(x, rng):
    """Every element moved by -1, 0 or +1 ulp (what the hardware's rcp / rsq may differ from the rounded quotient by)."""
    if rng is None or x.dtype != np.float32:
        return x
    return (np.ascontiguousarray(x).view(np.int32) + rng.integers(-1, 2, size=x.shape, dtype=np.int32)).view(np.float32)


def stream(f, sol):
    """The nine populations that arrive at the interior sites [1:NY-1, 1:NX-1] (pull stream, half-way bounce-back): lbm_numpy.step's."""
    _, ny, nx = f.shape
    fin = []
    for i, (ex, ey) in enumerate(E):
        src = f[i, 1 - ey:ny - 1 - ey, 1 - ex:nx - 1 - ex]
        src_solid = sol[1 - ey:ny - 1 - ey, 1 - ex:nx - 1 - ex]
        fin.append(np.where(src_solid, f[OPP[i], 1:ny - 1, 1:nx - 1], src))
    return fin


def collide_contracted(fin, omega, rng=None, clamp_first=False):
    """csrc/d2q9.hpp collide_contracted, operation for operation, on arrays of the dtype of fin (binary64: plain arithmetic).
    clamp_first: the WRONG collision that clamps the density before it takes the reciprocal (test_fast_math_host.py)."""
    T = fin[0].dtype.type
    with np.errstate(all="ignore"):
        r = fin[0]
        for k in range(1, 9):
            r = r + fin[k]
        lo, hi = T(RHO_MIN), T(RHO_MAX)
        if clamp_first:
            r = np.where(r < lo, lo, r)
            r = np.where(hi < r, hi, r)
        inv = _nudge(T(1.0) / r, rng)
        u = (fin[1] + fin[5] + fin[8] - fin[3] - fin[6] - fin[7]) * inv
        v = (fin[2] + fin[5] + fin[6] - fin[4] - fin[7] - fin[8]) * inv
        r = np.where(r < lo, lo, r)
        r = np.where(hi < r, hi, r)
        spd2 = _fma(u, u, v * v, T)
        over = spd2 > T(U_MAX) * T(U_MAX)
        if over.any():
            rsq = _nudge((1.0 / np.sqrt(np.where(over, spd2, T(1.0)).astype(np.float64))).astype(T), rng)
            k = T(U_MAX) * rsq
            u = np.where(over, u * k, u)
            v = np.where(over, v * k, v)
        w0r, wsr, wdr = (T(4.0) / T(9.0)) * r, (T(1.0) / T(9.0)) * r, (T(1.0) / T(36.0)) * r
        uu = _fma(u, u, v * v, T)
        c = _fma(T(-1.5), uu, T(1.0), T)
        eq = [None] * 9
        eq[0] = w0r * c

        def pair(e, w, plus, minus):
            t = _fma(T(4.5) * e, e, c, T)
            eq[plus] = w * _fma(T(3.0), e, t, T)
            eq[minus] = w * _fma(T(-3.0), e, t, T)
        pair(u, wsr, 1, 3)
        pair(v, wsr, 2, 4)
        pair(u + v, wdr, 5, 7)
        pair(u - v, wdr, 8, 6)
        fo = [_fma(omega, eq[k] - fin[k], fin[k], T) for k in range(9)]
    return fo, (r, u, v)


def contracted_step(f, solid, tau, u0, rng=None, *, omega=None, clamp_first=False, misread=None):
    """lbm_numpy.step with the collision of the interior fluid sites replaced by collide_contracted; far field, outlet, solids and bounce-back
    are the oracle's own.  rng: rcp and rsq moved by a random -1 / 0 / +1 ulp.  omega, clamp_first: a wrong collision; misread(fin, f): a wrong
    read, applied to the streamed populations (both for test_fast_math_host.py)."""
    T = f.dtype.type
    fo, (rho_o, ux_o, uy_o) = ieee_step(f, solid, tau, u0)
    sol = np.asarray(solid) != 0
    fin = stream(f, sol)
    if misread is not None:
        misread(fin, f)
    out, (r, u, v) = collide_contracted(fin, omega_of(tau, T) if omega is None else T(omega), rng, clamp_first)
    fluid = ~sol[1:-1, 1:-1]
    for k in range(9):
        fo[k, 1:-1, 1:-1][fluid] = out[k][fluid]
    for plane, new in ((rho_o, r), (ux_o, u), (uy_o, v)):
        plane[1:-1, 1:-1][fluid] = new[fluid]
    return fo, (rho_o, ux_o, uy_o)


def pre_clamp(f, solid):
    """(density, speed) of the interior sites before the stability net, of the step that starts from f (binary64 arithmetic)."""
    fin = stream(np.asarray(f, np.float64), np.asarray(solid) != 0)
    r = sum(fin[1:], fin[0])
    with np.errstate(all="ignore"):
        u = (fin[1] + fin[5] + fin[8] - fin[3] - fin[6] - fin[7]) / r
        v = (fin[2] + fin[5] + fin[6] - fin[4] - fin[7] - fin[8]) / r
    return r, np.hypot(u, v)


# --------------------------------------------------------------------------------------------------------------------------------------------
# the cases: (Case, calls[, fuse_chunk]) — all of them fp32 cases of _rough_start
# --------------------------------------------------------------------------------------------------------------------------------------------
SMALL = tuple((rs.case_small(nx, ny, m, "float32"), chunk) for nx, ny, chunk in rs.SMALL for m in rs.MASKS)        # a.
# b. case_net's lattice, amplitude and masks (fuse_chunk 6) from another seed.  A count of clamp events is the same in every arithmetic only if no
# site is about to join or leave it: seeds 13 (case_net's own) and 14 each hold one interior fluid site whose speed before the net lies within
# NEAR of 0.35 in the step of a first boundary (13: 0.35 (1 + 9.1e-7) at step 4); 15 is the first seed with none at any boundary of either pattern.
NET_SEED, NET_CHUNK = 15, 6
NET = tuple(rs.Case(64, 262, m, "float32", seed=NET_SEED, amp_u=rs.NET_AMP_U, net=True) for m in rs.MASKS)
MASK_CHANGE = tuple(rs.case_mask_change(ny, "float32") for ny in rs.SWITCH_NY)                                      # c.
MASK_CHANGE_CALLS = (rs.SWITCH_THEN,)
SLABS, SLAB_CALLS = rs.case_slabs("float32"), rs.SLAB_CALLS                                                         # d.
LARGE, LARGE_CALLS = rs.case_large("body", "float32"), EVEN                                                         # the measured plan (GPU)


def host_runs():
    """Every (case, calls) whose reference the host file examines with the model: a and b in both patterns, c, d."""
    runs = [(c, calls) for c in [s[0] for s in SMALL] + list(NET) for calls in (EVEN, ODD)]
    runs += [(c, MASK_CHANGE_CALLS) for c in MASK_CHANGE]
    runs += [(SLABS, SLAB_CALLS)]
    assert all(c.net or c in rs.ALL_CASES for c, _ in runs)
    return runs


def run_id(case, calls):
    return case.id + "-calls" + "+".join(str(n) for n in calls)


def schedule(case, calls):
    """[(mask kind, steps)] per call; a case with `before` runs that first, as a call of its own, on that mask."""
    return ([tuple(case.before)] if case.before else []) + [(case.mask, n) for n in calls]


# --------------------------------------------------------------------------------------------------------------------------------------------
# the references
# --------------------------------------------------------------------------------------------------------------------------------------------
# One per call boundary.  steps: done so far; mask: the kind the call ran on; planes: the fp64 oracle's (f, rho, ux, uy); d32: the yardstick per
# plane; net cases: events / events32 = clamp_events of the fp64 / fp32 oracle, near = interior fluid sites of the fp64 oracle within NEAR of a
# clamp threshold in the boundary's step.
Ref = namedtuple("Ref", "steps mask planes d32 events events32 near")
_REFS = {}


def _near_threshold(prev64, mask):
    r, s = pre_clamp(prev64, mask)
    fluid = np.asarray(mask)[1:-1, 1:-1] == 0
    close = np.zeros(r.shape, bool)
    for x, t in ((r, RHO_MIN), (r, RHO_MAX), (s, U_MAX)):
        close |= np.abs(x - t) <= NEAR * t
    return int((close & fluid).sum())


def references(oracle, case, calls):
    """[Ref] for the boundaries of schedule(case, calls); computed once per run, shared and read-only."""
    key = (case, tuple(calls))
    if key in _REFS:
        return _REFS[key]
    f32 = rs.start_of(case)
    assert f32.dtype == np.float32
    f64 = f32.astype(np.float64)
    refs, done = [], 0
    for kind, n in schedule(case, calls):
        mask = rs.mask_of(kind, case.nx, case.ny)
        f32, m32 = oracle.run(mask, n, case.tau, rs.U0, np.float32, f=f32)
        prev64, _ = oracle.run(mask, n - 1, case.tau, rs.U0, np.float64, f=f64)
        f64, m64 = oracle.run(mask, 1, case.tau, rs.U0, np.float64, f=prev64)
        done += n
        planes = (f64,) + tuple(m64)
        d32 = tuple(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip((f32,) + tuple(m32), planes))
        for a in planes:
            a.setflags(write=False)
        net = case.net
        refs.append(Ref(done, kind, planes, d32, clamp_events(*m64, mask) if net else None, clamp_events(*m32, mask) if net else None,
                        _near_threshold(prev64, mask) if net else None))
    _REFS[key] = refs
    return refs


def ratios(planes, ref):
    """max |plane - fp64 oracle| / d32 per plane (NaN where a plane holds one: no bound is met then)."""
    return tuple(float(np.abs(np.asarray(a, np.float64) - b).max()) / d for a, b, d in zip(planes, ref.planes, ref.d32))


def over(planes, ref, factor):
    """The planes that are NOT within factor * d32 of the reference: [(name, ratio)]."""
    return [(name, q) for name, q in zip(NAMES, ratios(planes, ref)) if not q <= factor]


def assert_yardstick(ref):
    """d32 is a rounding noise, and BOUND times it stays below BASELINE's tolerance."""
    assert all(np.isfinite(a).all() for a in ref.planes)
    assert all(0.0 < d for d in ref.d32), ref.d32
    assert BOUND * ref.d32[1] <= RHO_TOL and BOUND * max(ref.d32[2:]) <= U_TOL, ref.d32


def model_run(case, calls, rng=None, keep_last=False, **wrong):
    """The model through schedule(case, calls): [(f, rho, ux, uy)] per boundary; keep_last: also the state before the last step of every call."""
    f = rs.start_of(case)
    out, last = [], []
    for kind, n in schedule(case, calls):
        mask = rs.mask_of(kind, case.nx, case.ny)
        for i in range(n):
            if i == n - 1:
                last.append(f)
            f, macro = contracted_step(f, mask, case.tau, rs.U0, rng, **wrong)
        out.append((f,) + tuple(macro))
    return (out, last) if keep_last else out
