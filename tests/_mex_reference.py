"""NumPy reference of the momentum exchange of a batched sweep, written from the definition in include/wt_polar.h alone.

Directions e_k, k = 1..8, as d2q9.hpp / html:238-248.  Cell (i, j) (column i, row j, row 0 = bottom) covers
[i, i+1) x [j, j+1).  The lattice holds, in every interior fluid cell x (not solid, 1 <= i <= NX-2, 1 <= j <= NY-2), the
post-collision populations f*_k(x).  A link is a pair (interior fluid cell x, direction k) whose neighbour x + e_k is solid; the
body receives 2 f*_k(x) e_k per step from it.  All in double from the stored values converted exactly:
  F = sum over the links of 2 (double)f*_k(x) e_k,
  Mz = sum over the links of (r.x - xref) F_link.y - (r.y - yref) F_link.x, r = (i + 0.5 + 0.5 e_kx, j + 0.5 + 0.5 e_ky),
  links = the number of links.
No rest-state term is subtracted; boundary cells own no link.
"""
import math

import numpy as np

E = ((0, 0), (1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))
U = 2.0 ** -53          # unit roundoff of a double


class Mex:
    """fx, fy, mz (sums by math.fsum), the number of links, and the terms themselves, one entry per link: tx, ty (the link's
    force), ta, tb (the two products of its moment term ta - tb)."""

    def __init__(self, tx, ty, ta, tb):
        self.tx, self.ty, self.ta, self.tb = tx, ty, ta, tb
        self.links = int(tx.size)
        self.fx, self.fy, self.mz = math.fsum(tx), math.fsum(ty), math.fsum(ta - tb)

    # A force term 2 f e is exact in double, so two sides that add the same n terms in different orders differ by the
    # summation errors alone, each below (n - 1) u sum|t| to first order.
    def _force_bound(self, t):
        return 2.0 * max(self.links - 1, 0) * U * math.fsum(np.abs(t))

    @property
    def fx_bound(self):
        return self._force_bound(self.tx)

    @property
    def fy_bound(self):
        return self._force_bound(self.ty)

    @property
    def mz_bound(self):
        # a term is a - b with a = (r.x - xref) F.y, b = (r.y - yref) F.x: two roundings in each product and one in the
        # difference, each relative to |a| + |b| at most (not to |a - b|: a diagonal link's products can cancel), then the sum
        # of n terms: one side is below (n + 2) u sum(|a| + |b|) to first order, two sides differ by at most twice that
        return 2.0 * (self.links + 2) * U * math.fsum(np.abs(self.ta) + np.abs(self.tb))


def link_masks(mask):
    """owner[k] [NY][NX] bool for k = 0..8 (owner[0] is empty): cell (j, i) is an interior fluid cell whose neighbour in
    direction k is solid."""
    solid = np.asarray(mask) != 0
    ny, nx = solid.shape
    interior = np.zeros_like(solid)
    interior[1:ny - 1, 1:nx - 1] = True
    out = [np.zeros_like(solid)]
    for ex, ey in E[1:]:
        nb = np.zeros_like(solid)                      # the neighbour in direction k (inside the grid for every interior cell)
        nb[1:ny - 1, 1:nx - 1] = solid[1 + ey:ny - 1 + ey, 1 + ex:nx - 1 + ex]
        out.append(interior & ~solid & nb)
    return out


def count_links(mask) -> int:
    return int(sum(int(o.sum()) for o in link_masks(mask)))


def mex_reference(f, mask, xref, yref) -> Mex:
    """f [9][NY][NX] (any float dtype), mask [NY][NX] (non-zero = solid), reference point in lattice units."""
    f = np.asarray(f)
    ny, nx = f.shape[1:]
    jj, ii = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    tx, ty, ta, tb = [], [], [], []
    for k, own in enumerate(link_masks(mask)):
        if k == 0:
            continue
        ex, ey = E[k]
        t = 2.0 * f[k][own].astype(np.float64)
        flx, fly = t * ex, t * ey
        rx = (ii[own] + 0.5) + 0.5 * ex
        ry = (jj[own] + 0.5) + 0.5 * ey
        tx.append(flx)
        ty.append(fly)
        ta.append((rx - xref) * fly)
        tb.append((ry - yref) * flx)
    return Mex(*(np.concatenate(v) for v in (tx, ty, ta, tb)))
