"""Host-side geometry of the wind tunnel: airfoil generators, AoA rotation, cosine
re-panelling and the scanline rasterisation of the solid mask.

Mirrors the JS geometry block of the reference component,
``pages/airfoil_flow_lbm_aerolab.html`` (``html:LINE`` below): ``naca4`` html:99-116,
``clarkY`` html:118-121, ``SHAPES`` html:123-129, ``rotate`` html:133-140,
``panelise`` html:142-157 (``NP`` html:131), ``rasterMask`` html:160-182,
``buildGeometry`` html:559-577.  In the reference this code runs on the host
(single JS thread) as well; it is O(NY x 160) and stays on the host here.

Arithmetic is IEEE double in the reference's evaluation order so that masks are
identical cell for cell (tests/test_geometry_golden.py compares against the
reference's own JS run under Node).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

# html:73 — world window of the tunnel.  The reference fixes DY to +-0.46 (a 2:1
# lattice); for other aspect ratios the build keeps square cells by scaling the
# y half-height with NY/NX (SURVEY.md §7 "Grid-size generalisation").
DX0, DX1 = -0.42, 1.42
DY_HALF_REF = 0.46
NP = 160  # html:131

Coords = List[Tuple[float, float]]


def domain_y_half(nx: int, ny: int) -> float:
    """Half-height of the tunnel window: the reference's 0.46 on 2:1 lattices."""
    if nx == 2 * ny:
        return DY_HALF_REF
    return 0.5 * (DX1 - DX0) * ny / nx


def naca4(m: float, p: float, t: float, n: int) -> Coords:
    """html:99-116: NACA 4-digit, closed trailing edge (-0.1036), cosine spacing,
    returned in Selig order TE -> upper -> LE -> lower -> TE (2n+1 points)."""
    m /= 100
    p /= 10
    t /= 100
    up: Coords = []
    lo: Coords = []
    for i in range(n + 1):
        b = math.pi * i / n
        x = 0.5 * (1 - math.cos(b))
        yt = 5 * t * (0.2969 * math.sqrt(x) - 0.126 * x - 0.3516 * x * x + 0.2843 * x ** 3 - 0.1036 * x ** 4)
        yc = 0.0
        dyc = 0.0
        if m > 0:
            if x < p:
                yc = m / p / p * (2 * p * x - x * x)
                dyc = 2 * m / p / p * (p - x)
            else:
                yc = m / (1 - p) ** 2 * ((1 - 2 * p) + 2 * p * x - x * x)
                dyc = 2 * m / (1 - p) ** 2 * (p - x)
        th = math.atan(dyc)
        up.append((x - yt * math.sin(th), yc + yt * math.cos(th)))
        lo.append((x + yt * math.sin(th), yc - yt * math.cos(th)))
    up.reverse()
    return up + lo[1:]


_CLARK_Y = [[100, .44], [95, 1.46], [90, 2.22], [80, 3.69], [70, 5.07], [60, 6.23], [50, 7.1], [40, 7.62],
            [30, 7.79], [25, 7.67], [20, 7.35], [15, 6.79], [10, 5.88], [7.5, 5.23], [5, 4.39], [2.5, 3.18],
            [1.25, 2.17], [0, 0], [1.25, -1.35], [2.5, -1.93], [5, -2.55], [7.5, -2.9], [10, -3.05],
            [15, -3.01], [20, -2.75], [25, -2.41], [30, -2.06], [40, -1.38], [50, -.85], [60, -.44],
            [70, -.16], [80, 0], [90, 0], [95, 0], [100, -.44]]


def clark_y() -> Coords:
    """html:118-121: tabulated Clark-Y ordinates in percent chord."""
    return [(x / 100, y / 100) for x, y in _CLARK_Y]


# html:123-129
SHAPES: Dict[str, Callable[[], Coords]] = {
    "naca0012": lambda: naca4(0, 0, 12, 50),
    "naca2412": lambda: naca4(2, 4, 12, 50),
    "naca4412": lambda: naca4(4, 4, 12, 50),
    "naca6409": lambda: naca4(6, 4, 9, 50),
    "clark_y": clark_y,
}


def rotate(coords: Sequence[Tuple[float, float]], a_deg: float) -> Coords:
    """html:133-140: rotate by -a_deg about the quarter chord (0.25, 0):
    positive AoA = nose up, the free stream stays along +x."""
    a = -a_deg * math.pi / 180
    ca, sa = math.cos(a), math.sin(a)
    px, py = 0.25, 0.0
    out: Coords = []
    for x, y in coords:
        dx, dy = x - px, y - py
        out.append((px + dx * ca - dy * sa, py + dx * sa + dy * ca))
    return out


def panelise(coords: Sequence[Tuple[float, float]]) -> Tuple[np.ndarray, np.ndarray]:
    """html:142-157: arc-length cosine resampling to NP+1 = 161 points."""
    xs = [p[0] for p in coords]
    ys = [p[1] for p in coords]
    arc = [0.0]
    for i in range(1, len(coords)):
        arc.append(arc[i - 1] + math.hypot(xs[i] - xs[i - 1], ys[i] - ys[i - 1]))
    L = arc[-1]
    xp = np.empty(NP + 1)
    yp = np.empty(NP + 1)
    for i in range(NP + 1):
        s = L * 0.5 * (1 - math.cos(math.pi * i / NP))
        j = 0
        while j < len(arc) - 2 and arc[j + 1] < s:
            j += 1
        t = (s - arc[j]) / (arc[j + 1] - arc[j] + 1e-12)
        xp[i] = xs[j] + (xs[j + 1] - xs[j]) * t
        yp[i] = ys[j] + (ys[j + 1] - ys[j]) * t
    return xp, yp


def raster_mask(xp: np.ndarray, yp: np.ndarray, nx: int, ny: int, y_half: Optional[float] = None) -> np.ndarray:
    """html:160-182: even-odd scanline fill of the (open) panel polyline at row
    centres; returns uint8 [NY][NX] with 255 = solid, row 0 = bottom.

    Quirks kept on purpose: no closing segment, an
    unpaired last crossing is dropped, the x test is on the integer cell index
    (ceil/floor of the crossing in cell units), the y test on row centres."""
    if y_half is None:
        y_half = domain_y_half(nx, ny)
    dy0, dy1 = -y_half, y_half
    mask = np.zeros((ny, nx), dtype=np.uint8)
    x1, x2 = xp[:-1], xp[1:]
    y1, y2 = yp[:-1], yp[1:]
    for iy in range(ny):
        wy = dy0 + (iy + 0.5) / ny * (dy1 - dy0)
        cross = (y1 > wy) != (y2 > wy)
        if not cross.any():
            continue
        xs = x1[cross] + (x2[cross] - x1[cross]) * (wy - y1[cross]) / (y2[cross] - y1[cross])
        xs = np.sort(xs, kind="stable")
        for k in range(0, len(xs) - 1, 2):
            ix0 = math.ceil((xs[k] - DX0) / (DX1 - DX0) * nx)
            ix1 = math.floor((xs[k + 1] - DX0) / (DX1 - DX0) * nx)
            ix0 = max(0, ix0)
            ix1 = min(nx - 1, ix1)
            if ix1 >= ix0:
                mask[iy, ix0:ix1 + 1] = 255
    return mask


@dataclass
class Geometry:
    """html:556 `sol`: what buildGeometry returns (panel mid-points/normals are
    unused by the LBM path and omitted)."""
    xp: np.ndarray
    yp: np.ndarray
    mask: np.ndarray      # uint8 [NY][NX], 255 = solid
    a_deg: float


def round_coords(coords) -> Coords:
    """The 6-decimal rounding of build_lbm_component (pages/Airfoil_Analysis.py:34-36),
    applied before the coordinates reach the component."""
    return [(round(float(x), 6), round(float(y), 6)) for x, y in coords]


def build_geometry(nx: int, ny: int, a_deg: float, user_coords=None, shape: str = "naca2412",
                   y_half: Optional[float] = None) -> Geometry:
    """html:559-577: injected user coordinates win over the built-in shape."""
    if user_coords is not None and len(user_coords) > 0:
        base = [(float(x), float(y)) for x, y in user_coords]
    else:
        if shape not in SHAPES:
            raise ValueError(f"unknown shape {shape!r}; choose from {sorted(SHAPES)}")
        base = SHAPES[shape]()
    xp, yp = panelise(rotate(base, a_deg))
    return Geometry(xp=xp, yp=yp, mask=raster_mask(xp, yp, nx, ny, y_half), a_deg=float(a_deg))


# D2Q9 directions 1..8 (csrc/d2q9.hpp, html:238-248)
_LINK_DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))


def wall_distances(xp: np.ndarray, yp: np.ndarray, mask: np.ndarray, nx: int, ny: int, y_half: Optional[float] = None) -> np.ndarray:
    """The wall distances of interpolated bounce-back (include/wt_polar.h): float64 [8][NY][NX], plane k - 1 for direction k.

    A link is an interior fluid cell (i, j) (1 <= i <= NX-2, 1 <= j <= NY-2, not solid) and a direction k whose neighbour
    (i, j) + e_k is solid in `mask`.  Its entry is the fraction q in (0, 1] of the link at which the ray P + t e_k from the
    cell centre P = (i + 0.5, j + 0.5) first crosses the panel polygon: the 160 panels of (xp, yp) plus the closing segment
    from the last point to the first, in lattice units as raster_mask maps them, X = (x - DX0) / (DX1 - DX0) * nx,
    Y = (y + y_half) / (2 y_half) * ny.  A crossing with segment A + u (B - A) counts with a non-zero denominator,
    0 < t <= 1 and 0 <= u <= 1; q is the smallest such t.  A link without a crossing keeps 0.5, half-way bounce-back: the
    rasteriser tests row centres and integer cell indices, so its staircase is not exactly "centre inside the polygon".
    Entries that are no link are 0.5."""
    if y_half is None:
        y_half = domain_y_half(nx, ny)
    solid = np.asarray(mask) != 0
    if solid.shape != (ny, nx):
        raise ValueError(f"mask must have shape [NY][NX] = {(ny, nx)}, got {solid.shape}")
    X = (np.asarray(xp, np.float64) - DX0) / (DX1 - DX0) * nx
    Y = (np.asarray(yp, np.float64) + y_half) / (2 * y_half) * ny
    ax, ay = X, Y                                           # segment s runs from point s to point s + 1, the last one to point 0
    dx, dy = np.roll(X, -1) - X, np.roll(Y, -1) - Y
    q = np.full((8, ny, nx), 0.5)
    interior = np.zeros_like(solid)
    interior[1:ny - 1, 1:nx - 1] = True
    for k, (ex, ey) in enumerate(_LINK_DIRS):
        nb = np.zeros_like(solid)
        nb[1:ny - 1, 1:nx - 1] = solid[1 + ey:ny - 1 + ey, 1 + ex:nx - 1 + ex]
        jj, ii = np.nonzero(interior & ~solid & nb)
        if jj.size == 0:
            continue
        # P + t e = A + u d:  t = ((A - P) x d) / (e x d),  u = ((A - P) x e) / (e x d),  [links][segments]
        rx, ry = ax[None, :] - (ii[:, None] + 0.5), ay[None, :] - (jj[:, None] + 0.5)
        den = ex * dy - ey * dx
        ok = den != 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (rx * dy[None, :] - ry * dx[None, :]) / den[None, :]
            u = (rx * ey - ry * ex) / den[None, :]
        hit = ok[None, :] & (t > 0.0) & (t <= 1.0) & (u >= 0.0) & (u <= 1.0)
        first = np.where(hit, t, np.inf).min(axis=1)
        q[k, jj, ii] = np.where(np.isfinite(first), first, 0.5)
    return q


def to_lattice(x, y, nx: int, ny: int, y_half: Optional[float] = None):
    """World coordinates in lattice units, as raster_mask maps them: X = (x - DX0) / (DX1 - DX0) * nx, Y = (y + y_half) / (2 y_half) * ny,
    so that cell (i, j) covers [i, i+1) x [j, j+1)."""
    if y_half is None:
        y_half = domain_y_half(nx, ny)
    return (np.asarray(x, np.float64) - DX0) / (DX1 - DX0) * nx, (np.asarray(y, np.float64) + y_half) / (2 * y_half) * ny


def surface_stations(geom: Geometry, nx: int, ny: int, y_half: Optional[float] = None) -> Dict[str, object]:
    """One station per panel of the member's panel polyline (geom.xp, geom.yp: NP = 160 panels), for read-outs along the wall (the
    boundary-layer rakes of polar.boundary_layer_points).  All arrays are [NP] float64 in panel order unless said otherwise:
      x, y          the panel's midpoint in lattice units, mapped as raster_mask maps it (to_lattice)
      nrm_x, nrm_y  the unit outward normal in lattice units: the panel's direction turned by -90 degrees where the polyline runs
                    counter-clockwise (its shoelace area is positive, as for Selig order: trailing edge, upper side, leading edge,
                    lower side), by +90 degrees where it runs clockwise
      tan_x, tan_y  the unit tangent pointing from the leading edge to the trailing edge on each side, so that attached flow has a
                    positive tangential speed on both surfaces: against the panel's direction on the side the polyline walks first
                    (trailing edge to leading edge), along it on the other
      upper         bool: the panel lies on the upper side.  The leading edge is the polyline point of smallest x in the body's own
                    axes; the panels before it are the first side, which is the upper one of a counter-clockwise polyline
      x_over_c      x of the midpoint in the body's own axes, rotated back by the member's angle geom.a_deg about (0.25, 0)
      lattice       (nx, ny), and chord_cells = nx / (DX1 - DX0), the cells of one chord
    A panel of zero length has NaN normal and tangent."""
    xp, yp = np.asarray(geom.xp, np.float64), np.asarray(geom.yp, np.float64)
    X, Y = to_lattice(xp, yp, nx, ny, y_half)
    dx, dy = np.diff(X), np.diff(Y)
    length = np.hypot(dx, dy)
    with np.errstate(invalid="ignore", divide="ignore"):
        ux, uy = dx / length, dy / length
    area = 0.5 * float(np.sum(X * np.roll(Y, -1) - np.roll(X, -1) * Y))     # shoelace, the closing segment included
    ccw = area > 0
    nrm_x, nrm_y = (uy, -ux) if ccw else (-uy, ux)
    body = rotate(list(zip(xp.tolist(), yp.tolist())), -geom.a_deg)         # back into the body's own axes
    bx = np.array([p[0] for p in body])
    le = int(np.argmin(bx))
    first = np.arange(xp.size - 1) < le                                     # the side walked from the trailing edge to the leading edge
    sign = np.where(first, -1.0, 1.0)
    return {"x": 0.5 * (X[:-1] + X[1:]), "y": 0.5 * (Y[:-1] + Y[1:]), "nrm_x": nrm_x, "nrm_y": nrm_y, "tan_x": sign * ux, "tan_y": sign * uy,
            "upper": first if ccw else ~first, "x_over_c": 0.5 * (bx[:-1] + bx[1:]), "lattice": (int(nx), int(ny)),
            "chord_cells": nx / (DX1 - DX0)}


def _links(solid: np.ndarray):
    """(k, jj, ii) for every direction k = 0..7 (direction k + 1 of _LINK_DIRS): the interior fluid cells (1 <= i <= NX-2, 1 <= j <= NY-2,
    not solid) whose neighbour (i, j) + e_k is solid, the links of interpolated bounce-back."""
    ny, nx = solid.shape
    interior = np.zeros_like(solid)
    interior[1:ny - 1, 1:nx - 1] = True
    for k, (ex, ey) in enumerate(_LINK_DIRS):
        nb = np.zeros_like(solid)
        nb[1:ny - 1, 1:nx - 1] = solid[1 + ey:ny - 1 + ey, 1 + ex:nx - 1 + ex]
        jj, ii = np.nonzero(interior & ~solid & nb)
        yield k, jj, ii


def _check_link_planes(mask, q):
    solid = np.asarray(mask) != 0
    q = np.asarray(q, np.float64)
    if solid.ndim != 2 or q.shape != (8,) + solid.shape:
        raise ValueError(f"mask must be [NY][NX] and q [8][NY][NX], got {solid.shape} and {q.shape}")
    return solid, q


def rigid_wall_velocity(mask: np.ndarray, q: np.ndarray, ux: float, uy: float, omega: float, px: float, py: float) -> np.ndarray:
    """The wall-normal velocities (include/wt_polar.h "Wall velocity") of a body that moves rigidly: float64 [8][NY][NX], plane k - 1 for
    direction k.  The body translates with (ux, uy) and turns counter-clockwise with `omega` (radians per step) about (px, py), all in
    lattice units, so that the wall's velocity at a point r is u_w = (ux - omega (r_y - py), uy + omega (r_x - px)).  On every link of
    `mask` (wall_distances' links) with wall distance q = q[k - 1][j][i],
        un_k = e_kx (ux - omega (r_y - py)) + e_ky (uy + omega (r_x - px))   at the wall point   r = (i + 0.5 + q e_kx, j + 0.5 + q e_ky);
    every other entry is +0.  The mask itself does not move: a spinning circle, or a small-amplitude motion applied by transpiration."""
    solid, q = _check_link_planes(mask, q)
    un = np.zeros(q.shape)
    for k, jj, ii in _links(solid):
        ex, ey = _LINK_DIRS[k]
        rx, ry = ii + 0.5 + q[k, jj, ii] * ex, jj + 0.5 + q[k, jj, ii] * ey
        un[k, jj, ii] = ex * (ux - omega * (ry - py)) + ey * (uy + omega * (rx - px))
    return un


def slot_wall_velocity(geom: Geometry, mask: np.ndarray, q: np.ndarray, nx: int, ny: int, surface: str, x0: float, x1: float, vn: float,
                       y_half: Optional[float] = None) -> np.ndarray:
    """The wall-normal velocities of blowing (vn > 0, into the fluid) or suction (vn < 0) through a slot of the surface: float64
    [8][NY][NX], plane k - 1 for direction k.  A link of `mask` belongs to the slot when the station of surface_stations(geom, nx, ny)
    nearest to its wall point r = (i + 0.5 + q e_kx, j + 0.5 + q e_ky) lies on `surface` ("upper" or "lower") with x0 <= x_over_c <= x1;
    there u_w = vn (nrm_x, nrm_y) of that station, in lattice units, and un_k = e_k . u_w.  Every other entry is +0.  Stations of
    zero-length panels are not candidates."""
    if surface not in ("upper", "lower"):
        raise ValueError(f'surface must be "upper" or "lower", got {surface!r}')
    solid, q = _check_link_planes(mask, q)
    if solid.shape != (ny, nx):
        raise ValueError(f"mask must have shape [NY][NX] = {(ny, nx)}, got {solid.shape}")
    st = surface_stations(geom, nx, ny, y_half)
    ok = np.isfinite(st["nrm_x"]) & np.isfinite(st["nrm_y"])
    sx, sy, nrx, nry = st["x"][ok], st["y"][ok], st["nrm_x"][ok], st["nrm_y"][ok]
    side = st["upper"][ok] if surface == "upper" else ~st["upper"][ok]
    slot = side & (st["x_over_c"][ok] >= x0) & (st["x_over_c"][ok] <= x1)
    un = np.zeros(q.shape)
    for k, jj, ii in _links(solid):
        if jj.size == 0:
            continue
        ex, ey = _LINK_DIRS[k]
        rx, ry = ii + 0.5 + q[k, jj, ii] * ex, jj + 0.5 + q[k, jj, ii] * ey
        near = np.argmin((rx[:, None] - sx[None, :]) ** 2 + (ry[:, None] - sy[None, :]) ** 2, axis=1)
        un[k, jj, ii] = np.where(slot[near], vn * (ex * nrx[near] + ey * nry[near]), 0.0)
    return un
