"""The inclined free stream of batched sweeps (include/wt_polar.h, wtp_enable_wind) in NumPy: test infrastructure only.

Every branch but the far field is the base step's own, taken by calling it: oracle.lbm_numpy.step, _les_reference.step, or
_ibb_reference.step with either collision.  The far field does not depend on the collision or the wall rule, so one wrapper
serves all four.  The header's definition:

  Far field.  Member m holds a cross-flow V0[m] of the batch's dtype T, rounded once from the caller's double.  In the step, a
  far-field cell is one that is not solid, not in the outlet column, and lies in column 0, row 0 or row NY-1.  Without the model
  such a cell writes feq_k(1, U0, 0) and stores (1, U0, 0).  With the model on it writes feq_k(1, U0, V0) and stores (1, U0, V0).
  feq is the step's own: oracle/lbm_numpy.feq's order, one rounding per operation in T, no contraction.
  Start.  While the model is on, wtp_init_equilibrium fills every cell of member m with feq_k(1, u0, v0), evaluated in double on
  the host: w*(1 + 3*eu + 4.5*eu*eu - 1.5*uu) with eu = ex*u0 + ey*v0 and uu = u0*u0 + v0*v0, rounded to T once.  The
  macroscopic planes become (1, (T)u0, (T)v0).
"""
import numpy as np

import lbm_numpy
from lbm_numpy import E, feq


def far_field(solid):
    """[NY][NX] bool: the cells that take the step's far-field branch."""
    sol = np.asarray(solid) != 0
    ny, nx = sol.shape
    far = np.zeros((ny, nx), bool)
    far[:, 0] = far[0, :] = far[ny - 1, :] = True
    far[:, nx - 1] = False
    return far & ~sol


def wind_step(base_step, f, solid, tau, u0, v0, *extra):
    """One step of `base_step(f, solid, tau, u0, *extra)` with the far field of (u0, v0).  Returns what the base step returns:
    (f_out, (rho, ux, uy)) and whatever follows them."""
    T = f.dtype.type
    out = base_step(f, solid, tau, u0, *extra)
    fo, (rho, ux, uy) = out[0], out[1]
    far = far_field(solid)
    one, u, v = T(1.0), T(u0), T(v0)
    for k in range(9):
        fo[k][far] = feq(k, one, u, v, T)
    rho[far], ux[far], uy[far] = one, u, v
    assert fo.dtype == f.dtype and uy.dtype == f.dtype
    return (fo, (rho, ux, uy), *out[2:])


def wind_init(nx, ny, u0, v0, dtype):
    """The start state: (f [9][NY][NX], (rho, ux, uy)), every cell alike."""
    T = np.dtype(dtype).type
    u0, v0 = float(u0), float(v0)
    w = (4 / 9,) + (1 / 9,) * 4 + (1 / 36,) * 4
    f = np.empty((9, ny, nx), dtype=dtype)
    for k, (ex, ey) in enumerate(E):
        eu = ex * u0 + ey * v0
        uu = u0 * u0 + v0 * v0
        f[k] = T(w[k] * (1 + 3 * eu + 4.5 * eu * eu - 1.5 * uu))
    return f, (np.full((ny, nx), T(1.0), dtype=dtype), np.full((ny, nx), T(u0), dtype=dtype), np.full((ny, nx), T(v0), dtype=dtype))


def run(solid, steps, tau, u0, v0, *extra, base_step=lbm_numpy.step, dtype=np.float32, f=None):
    """`steps` wrapped steps from `f` (default: wind_init).  Returns what the last step returned."""
    ny, nx = solid.shape
    out = None
    if f is None:
        f, macro = wind_init(nx, ny, u0, v0, dtype)
        out = (f, macro)
    for _ in range(steps):
        out = wind_step(base_step, f, solid, tau, u0, v0, *extra)
        f = out[0]
    return out
