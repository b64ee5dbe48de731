"""NumPy reference of the surface loads of a batched sweep, written from the definitions in include/wt_polar.h alone.

Cell (i, j) (column i, row j, row 0 = bottom) covers [i, i+1) x [j, j+1).  Every fluid cell with a solid 4-neighbour
inside the grid in direction d adds a face with p = (double)rho / 3 and force F = p d on the body, at the face centre
r = (i + 0.5 + 0.5 dx, j + 0.5 + 0.5 dy).  Mz = sum (r.x - xref) F.y - (r.y - yref) F.x, counter-clockwise positive.
"""
import math

import numpy as np

DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1))
U = 2.0 ** -53          # unit roundoff of a double


class Loads:
    """fx, fy, mz (sums by math.fsum), n faces, and the terms themselves (tx, ty, tm: one entry per face)."""

    def __init__(self, tx, ty, tm):
        self.tx, self.ty, self.tm = tx, ty, tm
        self.n = int(tm.size)
        self.fx, self.fy, self.mz = math.fsum(tx), math.fsum(ty), math.fsum(tm)

    @staticmethod
    def _bound(n, terms):
        # each term carries at most three roundings of a double, and a sum of n terms in any order n - 1 more: the error of
        # one side is below (n + 2) u sum|t_i| to first order, and two sides that add the same terms in different orders
        # differ by at most twice that
        return 2.0 * (n + 2) * U * math.fsum(np.abs(terms))

    @property
    def mz_bound(self):
        return self._bound(self.n, self.tm)

    @property
    def fx_bound(self):
        return self._bound(self.n, self.tx)

    @property
    def fy_bound(self):
        return self._bound(self.n, self.ty)


def loads_reference(rho, mask, xref, yref) -> Loads:
    """rho [NY][NX] (any float dtype), mask [NY][NX] (non-zero = solid), reference point in lattice units."""
    rho = np.asarray(rho)
    solid = np.asarray(mask) != 0
    ny, nx = solid.shape
    p = rho.astype(np.float64) / 3.0
    jj, ii = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    tx, ty, tm = [], [], []
    for dx, dy in DIRS:
        nb = np.zeros_like(solid)                      # the neighbour in direction d is inside the grid and solid
        src = solid[max(dy, 0):ny + min(dy, 0), max(dx, 0):nx + min(dx, 0)]
        nb[max(-dy, 0):ny + min(-dy, 0), max(-dx, 0):nx + min(-dx, 0)] = src
        face = ~solid & nb
        pf = p[face]
        fx, fy = pf * dx, pf * dy
        rx = ii[face] + 0.5 + 0.5 * dx
        ry = jj[face] + 0.5 + 0.5 * dy
        tx.append(fx)
        ty.append(fy)
        tm.append((rx - xref) * fy - (ry - yref) * fx)
    return Loads(np.concatenate(tx), np.concatenate(ty), np.concatenate(tm))


def surface_rows(mask):
    """(j_upper, j_lower) [NX] int32: the row of the fluid cell directly above the highest / below the lowest solid cell of each
    column; -1 where the column holds no solid cell or that cell touches row NY-1 / row 0."""
    solid = np.asarray(mask) != 0
    ny, nx = solid.shape
    ju = np.full(nx, -1, np.int32)
    jl = np.full(nx, -1, np.int32)
    for i in range(nx):
        rows = np.flatnonzero(solid[:, i])
        if rows.size:
            if rows[-1] + 1 < ny:
                ju[i] = rows[-1] + 1
            if rows[0] - 1 >= 0:
                jl[i] = rows[0] - 1
    return ju, jl


def surface_sums(rhos, mask):
    """Sums of (double)rho at the upper / lower sample of every column over the fields `rhos`, added in that order, and the
    counts: (rho_upper, rho_lower, n_upper, n_lower), zeros where there is no sample."""
    ju, jl = surface_rows(mask)
    nx = ju.size
    cols = np.arange(nx)
    su, sl = np.zeros(nx), np.zeros(nx)
    nu, nl = np.zeros(nx, np.int64), np.zeros(nx, np.int64)
    hu, hl = ju >= 0, jl >= 0
    for rho in rhos:
        su[hu] += np.asarray(rho)[ju[hu], cols[hu]].astype(np.float64)
        sl[hl] += np.asarray(rho)[jl[hl], cols[hl]].astype(np.float64)
        nu[hu] += 1
        nl[hl] += 1
    return su, sl, nu, nl
