"""The prescribed far-field profile of batched sweeps (include/wt_polar.h, wtp_enable_far_profile / wtp_set_far_profile) in NumPy: test
infrastructure only.

Every branch but the far field is the base step's own, taken by calling it: oracle.lbm_numpy.step, _les_reference.step,
_ibb_reference.step or _trt_reference.step.  The far field does not depend on the collision or the wall rule, so one wrapper serves all
of them, in the manner of _wind_reference.wind_step.  The header's definition:

  A far-field cell is one that is not solid, not in the outlet column, and lies in column 0, row 0 or row NY-1.  Member m holds three
  tables of the batch's dtype T, each with three planes (rho, ux, uy): left[3][NY] for the cells (0, j), bottom[3][NX] for the cells
  (i, 0), top[3][NX] for the cells (i, NY-1).  A far-field cell (i, j) takes left[.][j] if i == 0, else bottom[.][i] if j == 0, else
  top[.][i].  The cell writes feq_k(rho, ux, uy) and stores (rho, ux, uy).  feq is the step's own: oracle/lbm_numpy.feq's order, one
  rounding per operation in T, no contraction.

MISREADS are wrong readings of that paragraph, each a function (left, bottom, top) -> planes; the host tests show that the reference
tells every one of them from the definition on every case the GPU tests use.
"""
import numpy as np

import lbm_numpy
from lbm_numpy import feq
from _wind_reference import far_field, wind_init


def planes(left, bottom, top):
    """[3][NY][NX] of the tables' dtype: (rho, ux, uy) of every border cell as the definition assigns them; 0 elsewhere."""
    left, bottom, top = np.asarray(left), np.asarray(bottom), np.asarray(top)
    ny, nx = left.shape[1], bottom.shape[1]
    assert left.shape == (3, ny) and bottom.shape == (3, nx) and top.shape == (3, nx) and left.dtype == bottom.dtype == top.dtype
    p = np.zeros((3, ny, nx), left.dtype)
    p[:, 0, :] = bottom
    p[:, ny - 1, :] = top
    p[:, :, 0] = left                                                      # the corners of column 0 belong to `left`
    return p


def _top_for_bottom(left, bottom, top):
    return planes(left, top, bottom)


def _corner_from_rows(left, bottom, top):
    p = planes(left, bottom, top)
    p[:, 0, 0], p[:, -1, 0] = bottom[:, 0], top[:, 0]
    return p


def _shifted(left, bottom, top):
    return planes(np.roll(left, 1, axis=1), np.roll(bottom, 1, axis=1), np.roll(top, 1, axis=1))


def _swapped_velocity(left, bottom, top):
    return planes(left, bottom, top)[[0, 2, 1]]


def _unit_density(left, bottom, top):
    p = planes(left, bottom, top)
    p[0] = 1
    return p


MISREADS = {"top for bottom": _top_for_bottom, "corner from bottom and top": _corner_from_rows, "entry shifted by one": _shifted,
            "ux and uy swapped": _swapped_velocity, "rho forced to 1": _unit_density}


def profile_step(base_step, f, solid, tau, u0, tables, *extra, read=planes):
    """One step of `base_step(f, solid, tau, u0, *extra)` with the far field of `tables` = (left, bottom, top).  Returns what the base
    step returns: (f_out, (rho, ux, uy)) and whatever follows them.  `read`: planes, or one of MISREADS."""
    T = f.dtype.type
    out = base_step(f, solid, tau, u0, *extra)
    fo, (rho, ux, uy) = out[0], out[1]
    far = far_field(solid)
    p = read(*tables)
    assert p.dtype == f.dtype and p.shape == (3,) + far.shape
    r, u, v = p[0][far], p[1][far], p[2][far]
    for k in range(9):
        fo[k][far] = feq(k, r, u, v, T)
    rho[far], ux[far], uy[far] = r, u, v
    assert fo.dtype == f.dtype and uy.dtype == f.dtype
    return (fo, (rho, ux, uy), *out[2:])


def run(solid, schedule, tau, u0, *extra, base_step=lbm_numpy.step, dtype=np.float32, f=None, v0=0.0, read=planes):
    """Wrapped steps from `f` (default: wind_init at (u0, v0), the start wtp_init_equilibrium gives).  `schedule` is a list of
    (steps, tables): `steps` steps with `tables`, then the next entry.  Returns what the last step returned."""
    ny, nx = solid.shape
    out = None
    if f is None:
        f, macro = wind_init(nx, ny, u0, v0, dtype)
        out = (f, macro)
    for steps, tables in schedule:
        for _ in range(steps):
            out = profile_step(base_step, f, solid, tau, u0, tables, *extra, read=read)
            f = out[0]
    return out


def uniform_tables(nx, ny, u0, v0, dtype):
    """(1, (T)u0, (T)v0) in every entry."""
    T = np.dtype(dtype).type
    row = np.array([T(1.0), T(u0), T(v0)], dtype=dtype)
    return (np.repeat(row[:, None], ny, axis=1), np.repeat(row[:, None], nx, axis=1), np.repeat(row[:, None], nx, axis=1))


def random_tables(nx, ny, dtype, seed):
    """In-bounds tables in which no two entries are alike: rho in [0.9, 1.1), speed below 0.15."""
    rng = np.random.default_rng(seed)
    n = 3 * (ny + 2 * nx)
    for _ in range(8):
        v = np.concatenate([0.9 + 0.2 * rng.random(n // 3), -0.1 + 0.2 * rng.random(n - n // 3)]).astype(dtype)
        if np.unique(v).size == v.size:
            break
    else:                                                                  # pragma: no cover
        raise AssertionError("could not draw distinct entries")
    rho, vel = v[:n // 3], v[n // 3:]
    cut = (ny, ny + nx, ny + 2 * nx)
    tabs = []
    for a, b in zip((0,) + cut[:-1], cut):
        tabs.append(np.stack([rho[a:b], vel[a:b], vel[n // 3 + a:n // 3 + b]]))
    return tuple(tabs)
