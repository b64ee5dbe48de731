"""The Smagorinsky collision of batched sweeps (include/wt_polar.h, wtp_enable_les) in NumPy: test infrastructure only.

The boundary, solid and macro branches are oracle.lbm_numpy.step's own, taken by calling it; only the collision of the
interior fluid cells is recomputed here, in the header's order of operations, one rounding per operation in the lattice's
dtype.  With c = 0 every population comes out as lbm_numpy.step's, bit for bit (tests/test_polar_les_host.py).
"""
import math

import numpy as np

import lbm_numpy
from lbm_numpy import E, OPP, feq


def les_constant(cs, dtype):
    """c = (T)(18.0 * sqrt(2.0) * cs * cs): the product left to right in double, rounded to T once."""
    return np.dtype(dtype).type(18.0 * math.sqrt(2.0) * float(cs) * float(cs))


def step(f, solid, tau, u0, c):
    """One step with the Smagorinsky collision.  Returns (f_out, (rho, ux, uy), te): te [NY][NX] is the effective relaxation
    time of the interior fluid cells and tau everywhere else (solid and boundary cells do not collide)."""
    T = f.dtype.type
    _, ny, nx = f.shape
    sol = solid != 0
    fo, (rho_o, ux_o, uy_o) = lbm_numpy.step(f, solid, tau, u0)
    tau, c = T(tau), T(c)
    inner = (slice(1, ny - 1), slice(1, nx - 1))
    fluid = ~sol[inner]
    # the clamped pre-collision moments of the interior cells, as the oracle stored them (html:335-350)
    rho, ux, uy = rho_o[inner], ux_o[inner], uy_o[inner]
    fin = []
    for i, (ex, ey) in enumerate(E):                                   # pull-stream with half-way bounce-back (html:324-333)
        src = f[i, 1 - ey:ny - 1 - ey, 1 - ex:nx - 1 - ex]
        src_solid = sol[1 - ey:ny - 1 - ey, 1 - ex:nx - 1 - ex]
        fin.append(np.where(src_solid, f[OPP[i]][inner], src))
    with np.errstate(all="ignore"):
        n = [fin[i] - feq(i, rho, ux, uy, T) for i in range(9)]
        pxx = n[1] + n[3] + n[5] + n[6] + n[7] + n[8]
        pyy = n[2] + n[4] + n[5] + n[6] + n[7] + n[8]
        pxy = n[5] - n[6] + n[7] - n[8]
        q = np.sqrt((pxx * pxx + T(2.0) * (pxy * pxy)) + pyy * pyy)
        te = T(0.5) * (tau + np.sqrt(tau * tau + (c * q) / rho))
        for i in range(9):
            fo[i][inner] = np.where(fluid, fin[i] - n[i] / te, fo[i][inner])
    te_o = np.full((ny, nx), tau, dtype=f.dtype)
    te_o[inner] = np.where(fluid, te, tau)
    assert te_o.dtype == f.dtype and fo.dtype == f.dtype
    return fo, (rho_o, ux_o, uy_o), te_o


def run(solid, steps, tau, u0, c, dtype=np.float32, f=None):
    """`steps` steps from `f` (default: the uniform equilibrium at u0).  Returns (f, (rho, ux, uy), te) of the last step."""
    ny, nx = solid.shape
    if f is None:
        f, macro = lbm_numpy.equilibrium_init(nx, ny, u0, dtype)
    else:
        macro = None
    te = np.full((ny, nx), np.dtype(dtype).type(tau), dtype=dtype)
    for _ in range(steps):
        f, macro, te = step(f, solid, tau, u0, c)
    return f, macro, te
