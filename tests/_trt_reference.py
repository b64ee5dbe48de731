"""The two-relaxation-time collision of batched sweeps (include/wt_polar.h, wtp_enable_trt) in NumPy: test infrastructure only.

The boundary and solid branches are oracle.lbm_numpy.step's own, taken by calling it; only the interior fluid cells are recomputed
here, in the header's order of operations, one rounding per operation in the lattice's dtype:

    n[k] = fin[k] - eq[k]                                   k = 0..8
    tp   = tau                                              (model without Smagorinsky)
    tp   = te of the Smagorinsky section, from these n[k]   (c given)
    tm   = 0.5 + lam / (tp - 0.5)
    fo[0] = fin[0] - n[0] / tp
    for (k, o) in (1,3), (2,4), (5,7), (6,8):
        s  = 0.5 * (n[k] + n[o]);   a  = 0.5 * (n[k] - n[o])
        ds = s / tp;                da = a / tm
        fo[k] = (fin[k] - ds) - da
        fo[o] = (fin[o] - ds) + da

The gather is the half-way one, or with wall distances `q` that of _ibb_reference.wall_incoming.  step returns (f_out, (rho, ux, uy)), so
that _half_reference.half_step and _half_reference.windy wrap it unchanged: the extra arguments are (lam, c, q).
"""
import numpy as np

import lbm_numpy
from lbm_numpy import E, OPP, RHO_MAX, RHO_MIN, U_MAX, feq
from _ibb_reference import wall_incoming

PAIRS = ((1, 3), (2, 4), (5, 7), (6, 8))
assert all(OPP[k] == o for k, o in PAIRS)


def collide(fin, rho, ux, uy, tau, lam, c=None, swap=False):
    """The collision above on lists of arrays: fin[9] and the clamped moments, all of one dtype T.  Returns (fo[9], tp, tm).
    `swap` exchanges the roles of tp and tm in the pairs (a deliberately wrong collision, for the sensitivity checks)."""
    T = fin[0].dtype.type
    tau, lam = T(tau), T(lam)
    with np.errstate(all="ignore"):
        n = [fin[i] - feq(i, rho, ux, uy, T) for i in range(9)]
        if c is None:
            tp = tau
        else:
            c = T(c)
            pxx = n[1] + n[3] + n[5] + n[6] + n[7] + n[8]
            pyy = n[2] + n[4] + n[5] + n[6] + n[7] + n[8]
            pxy = n[5] - n[6] + n[7] - n[8]
            qq = np.sqrt((pxx * pxx + T(2.0) * (pxy * pxy)) + pyy * pyy)
            tp = T(0.5) * (tau + np.sqrt(tau * tau + (c * qq) / rho))
        tm = T(0.5) + lam / (tp - T(0.5))
        fo = [None] * 9
        fo[0] = fin[0] - n[0] / tp
        ts, ta = (tm, tp) if swap else (tp, tm)
        for k, o in PAIRS:
            s = T(0.5) * (n[k] + n[o])
            a = T(0.5) * (n[k] - n[o])
            ds = s / ts
            da = a / ta
            fo[k] = (fin[k] - ds) - da
            fo[o] = (fin[o] - ds) + da
    assert all(np.asarray(v).dtype == fin[0].dtype for v in fo)
    return fo, tp, tm


def step(f, solid, tau, u0, lam, c=None, q=None, swap=False):
    """One step with the two-relaxation-time collision.  lam: the magic number; c: None, or the Smagorinsky constant
    c = (T)(18 sqrt(2) Cs^2) (_les_reference.les_constant); q: None for half-way walls, or the wall distances [8][NY][NX] of f's dtype.
    Returns (f_out, (rho, ux, uy))."""
    T = f.dtype.type
    _, ny, nx = f.shape
    sol = solid != 0
    fo, (rho_o, ux_o, uy_o) = lbm_numpy.step(f, solid, tau, u0)
    inner = (slice(1, ny - 1), slice(1, nx - 1))
    fluid = ~sol[inner]
    if q is not None:
        assert q.shape == (8, ny, nx) and q.dtype == f.dtype
    fin = []
    for i, (ex, ey) in enumerate(E):                                     # pull-stream (html:324-333)
        src = f[i, 1 - ey:ny - 1 - ey, 1 - ex:nx - 1 - ex]                # f_i(x - e_i)
        if i == 0:
            fin.append(src)
            continue
        src_solid = sol[1 - ey:ny - 1 - ey, 1 - ex:nx - 1 - ex]
        k = OPP[i]                                                        # the link's direction: x + e_k = x - e_i is solid
        if q is None:
            refl = f[k][inner]
        else:
            behind = (slice(1 + ey, ny - 1 + ey), slice(1 + ex, nx - 1 + ex))  # x - e_k = x + e_i
            refl = wall_incoming(q[k - 1][inner], f[k][inner], f[k][behind], sol[behind], f[i][inner])
        fin.append(np.where(src_solid, refl, src))
    rho = fin[0]
    for i in range(1, 9):
        rho = rho + fin[i]
    with np.errstate(all="ignore"):
        ux = (fin[1] + fin[5] + fin[8] - fin[3] - fin[6] - fin[7]) / rho
        uy = (fin[2] + fin[5] + fin[6] - fin[4] - fin[7] - fin[8]) / rho
        rho = np.minimum(np.maximum(rho, T(RHO_MIN)), T(RHO_MAX))
        spd2 = ux * ux + uy * uy
        over = spd2 > T(U_MAX) * T(U_MAX)
        kk = T(U_MAX) / np.sqrt(spd2)
        ux = np.where(over, ux * kk, ux)
        uy = np.where(over, uy * kk, uy)
    out, _, _ = collide(fin, rho, ux, uy, tau, lam, c, swap)
    for i in range(9):
        fo[i][inner] = np.where(fluid, out[i], fo[i][inner])
    for dst, v in ((rho_o, rho), (ux_o, ux), (uy_o, uy)):
        dst[inner] = np.where(fluid, v, dst[inner])
    assert fo.dtype == f.dtype and rho_o.dtype == f.dtype
    return fo, (rho_o, ux_o, uy_o)


def run(solid, steps, tau, u0, lam, c=None, q=None, dtype=np.float32, f=None, swap=False):
    """`steps` steps from `f` (default: the uniform equilibrium at u0).  Returns (f, (rho, ux, uy)) of the last step."""
    ny, nx = solid.shape
    macro = None
    if f is None:
        f, macro = lbm_numpy.equilibrium_init(nx, ny, u0, dtype)
    if q is not None:
        q = np.ascontiguousarray(q, dtype=f.dtype)
    for _ in range(steps):
        f, macro = step(f, solid, tau, u0, lam, c, q, swap)
    return f, macro


# ---- the channel of the wall-position check ------------------------------------------------------
CHANNEL = dict(nx=64, ny=14, tau=2.0, u0=0.04, steps=7264, column=48)


def channel_mask(nx=CHANNEL["nx"], ny=CHANNEL["ny"]):
    """Rows 0 and NY - 1 solid: half-way walls at y = 1 and y = NY - 1 (cell j covers [j, j + 1))."""
    m = np.zeros((ny, nx), np.uint8)
    m[0, :] = m[ny - 1, :] = 1
    return m


def wall_offsets(ux_column):
    """The zeros of the parabola fitted to ux over rows 1 .. NY - 2 of one column (cell centres y = j + 0.5), as distances outside
    the half-way walls y = 1 and y = NY - 1: (1 - lower zero, upper zero - (NY - 1)); positive = the flow's wall lies outside."""
    u = np.asarray(ux_column, np.float64)
    ny = u.size
    y = np.arange(1, ny - 1) + 0.5
    a, b, c = np.polyfit(y, u[1:ny - 1], 2)
    lo, hi = sorted(np.roots([a, b, c]).real)
    return 1.0 - lo, hi - (ny - 1.0)
