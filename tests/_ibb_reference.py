"""Interpolated bounce-back of batched sweeps (include/wt_polar.h, wtp_enable_ibb) in NumPy: test infrastructure only.

The boundary and solid branches are oracle.lbm_numpy.step's own, taken by calling it; only the interior fluid cells are recomputed
here, in the header's order of operations, one rounding per operation in the lattice's dtype:

  The directions e_k, k = 1..8, and opp(k) are those of d2q9.hpp.  Member m holds, per cell (i, j) and direction k, a wall distance
  q_k(i, j) with 0 < q <= 1, used only where x = (i, j) is an interior fluid cell and x + e_k is solid: a link.  The incoming
  population fin[opp(k)] of x, which half-way bounce-back sets to s[k](x), becomes, with a = s[k](x), g = s[k](x - e_k),
  h = s[opp(k)](x) and s the source lattice,
      two = 2*q
      q <  0.5:  fin = two*a + (1 - two)*g      if x - e_k is not solid, else fin = a
      q >= 0.5:  inv = 1/two;  fin = inv*a + (1 - inv)*h
  Everything else in the step is unchanged.

The collision is BGK (c is None) or the Smagorinsky one of tests/_les_reference.py (the header's formulas, restated here because
that module streams for itself).  With q = 0.5 everywhere every population comes out as lbm_numpy.step's (tests/test_polar_ibb_host.py).

The momentum exchange with the model on: the link's term is ((double)a + (double)b) e_k with b the value the next step will reflect
(the formulas above on the current lattice, in T), and the link's point is r = (i + 0.5 + q e_kx, j + 0.5 + q e_ky).
"""
import math

import numpy as np

import lbm_numpy
from lbm_numpy import E, OPP, RHO_MAX, RHO_MIN, U_MAX, feq
from _mex_reference import U, Mex, link_masks


def wall_incoming(q, a, g, g_solid, h):
    """The header's formulas, elementwise; every array of one dtype T."""
    T = a.dtype.type
    with np.errstate(all="ignore"):
        two = T(2.0) * q
        low = np.where(g_solid, a, two * a + (T(1.0) - two) * g)
        inv = T(1.0) / two
        high = inv * a + (T(1.0) - inv) * h
    out = np.where(q < T(0.5), low, high)
    assert out.dtype == a.dtype
    return out


def step(f, solid, tau, u0, q, c=None):
    """One step with interpolated bounce-back.  q [8][NY][NX] of f's dtype, plane k - 1 for direction k; c: None for BGK, else the
    Smagorinsky constant c = (T)(18 sqrt(2) Cs^2) (_les_reference.les_constant).  Returns (f_out, (rho, ux, uy))."""
    T = f.dtype.type
    _, ny, nx = f.shape
    assert q.shape == (8, ny, nx) and q.dtype == f.dtype
    sol = solid != 0
    fo, (rho_o, ux_o, uy_o) = lbm_numpy.step(f, solid, tau, u0)
    tau = T(tau)
    inner = (slice(1, ny - 1), slice(1, nx - 1))
    fluid = ~sol[inner]
    fin = []
    for i, (ex, ey) in enumerate(E):                                     # pull-stream (html:324-333)
        src = f[i, 1 - ey:ny - 1 - ey, 1 - ex:nx - 1 - ex]                # f_i(x - e_i)
        if i == 0:
            fin.append(src)
            continue
        src_solid = sol[1 - ey:ny - 1 - ey, 1 - ex:nx - 1 - ex]
        k = OPP[i]                                                        # the link's direction: x + e_k = x - e_i is solid
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
        if c is None:
            out = [fin[i] - (fin[i] - feq(i, rho, ux, uy, T)) / tau for i in range(9)]
        else:
            c = T(c)
            n = [fin[i] - feq(i, rho, ux, uy, T) for i in range(9)]
            pxx = n[1] + n[3] + n[5] + n[6] + n[7] + n[8]
            pyy = n[2] + n[4] + n[5] + n[6] + n[7] + n[8]
            pxy = n[5] - n[6] + n[7] - n[8]
            qq = np.sqrt((pxx * pxx + T(2.0) * (pxy * pxy)) + pyy * pyy)
            te = T(0.5) * (tau + np.sqrt(tau * tau + (c * qq) / rho))
            out = [fin[i] - n[i] / te for i in range(9)]
    for i in range(9):
        fo[i][inner] = np.where(fluid, out[i], fo[i][inner])
    for dst, v in ((rho_o, rho), (ux_o, ux), (uy_o, uy)):
        dst[inner] = np.where(fluid, v, dst[inner])
    assert fo.dtype == f.dtype and rho_o.dtype == f.dtype
    return fo, (rho_o, ux_o, uy_o)


def run(solid, steps, tau, u0, q, c=None, dtype=np.float32, f=None):
    """`steps` steps from `f` (default: the uniform equilibrium at u0).  Returns (f, (rho, ux, uy)) of the last step."""
    ny, nx = solid.shape
    macro = None
    if f is None:
        f, macro = lbm_numpy.equilibrium_init(nx, ny, u0, dtype)
    q = np.ascontiguousarray(q, dtype=f.dtype)
    for _ in range(steps):
        f, macro = step(f, solid, tau, u0, q, c)
    return f, macro


def fallback_links(mask, q):
    """The number of links with q < 0.5 whose cell behind, x - e_k, is solid: the ones that fall back to fin = a."""
    sol = np.asarray(mask) != 0
    ny, nx = sol.shape
    n = 0
    for k, own in enumerate(link_masks(mask)):
        if k == 0:
            continue
        ex, ey = E[k]
        behind = np.zeros_like(sol)
        behind[1:ny - 1, 1:nx - 1] = sol[1 - ey:ny - 1 - ey, 1 - ex:nx - 1 - ex]
        n += int((own & behind & (q[k - 1] < 0.5)).sum())
    return n


class MexIbb(Mex):
    """_mex_reference.Mex with the bounds of the interpolated term.  Kernel and reference evaluate a link's term by the same
    operations, so in fact they differ by the order of the sums alone; the bounds below nevertheless allow for the roundings that
    the interpolated definition adds to a term, as the half-way bounds allow for theirs:
      * the link's momentum (double)a + (double)b rounds once (2 f was exact): one more relative u on every term, so the force sums
        get n in place of n - 1, and the moment products three roundings in place of two (n + 3 in place of n + 2);
      * the wall point (i + 0.5) + q e rounds once (the midpoint was exact): an absolute error of at most u (NX + 1) in r.x and
        u (NY + 1) in r.y, i.e. at most u ((NX + 1) |F.y| + (NY + 1) |F.x|) in a link's moment term, summed over the links.
    Two sides differ by at most twice the one-sided bound, as there."""

    def __init__(self, tx, ty, ta, tb, nx, ny):
        super().__init__(tx, ty, ta, tb)
        self.nx, self.ny = nx, ny

    def _force_bound(self, t):
        return 2.0 * self.links * U * math.fsum(np.abs(t))

    @property
    def mz_bound(self):
        point = U * math.fsum((self.nx + 1) * np.abs(self.ty) + (self.ny + 1) * np.abs(self.tx))
        return 2.0 * ((self.links + 3) * U * math.fsum(np.abs(self.ta) + np.abs(self.tb)) + point)


def mex_reference(f, mask, q, xref, yref) -> MexIbb:
    """f [9][NY][NX], mask [NY][NX] (non-zero = solid), q [8][NY][NX] of f's dtype, reference point in lattice units."""
    f = np.asarray(f)
    T = f.dtype.type
    q = np.asarray(q)
    assert q.dtype == f.dtype
    sol = np.asarray(mask) != 0
    ny, nx = sol.shape
    jj, ii = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    tx, ty, ta, tb = [], [], [], []
    for k, own in enumerate(link_masks(mask)):
        if k == 0:
            continue
        ex, ey = E[k]
        js, is_ = np.nonzero(own)
        a = f[k][js, is_]
        b = wall_incoming(q[k - 1][js, is_], a, f[k][js - ey, is_ - ex], sol[js - ey, is_ - ex], f[OPP[k]][js, is_])
        assert b.dtype == T
        t = a.astype(np.float64) + b.astype(np.float64)
        flx, fly = t * ex, t * ey
        hq = q[k - 1][js, is_].astype(np.float64)
        rx = (ii[own] + 0.5) + hq * ex
        ry = (jj[own] + 0.5) + hq * ey
        tx.append(flx)
        ty.append(fly)
        ta.append((rx - xref) * fly)
        tb.append((ry - yref) * flx)
    return MexIbb(*(np.concatenate(v) for v in (tx, ty, ta, tb)), nx, ny)
