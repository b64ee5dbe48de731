"""The probe points and the boundary-layer read-out of batched sweeps (wtp_enable_probes and its three companions, PolarEngine.enable_probes,
probe_weights, geometry.surface_stations, boundary_layer_points, boundary_layer, run_polar(boundary_layer=)): what needs no GPU.  The weight
rule on hand values, that the NumPy reference of tests/_probe_reference.py can tell a misread, the boundary-layer arithmetic on an analytic
profile within a derived tolerance, the stations of a NACA 2412, the C-ABI's declaration, export and binding, and run_polar's argument checks.
"""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _probe_reference as pr
from _rough_start import rough_state

WT_ERR_ARG = -1
GPU_CASE = pr.GPU_CASE


# ---- 1. the weight rule ------------------------------------------------------------------------
def test_probe_weights_on_hand_values(pkg):
    from airfoil_cfd_tool_amd.polar import probe_weights
    nx, ny = 12, 7
    # a cell centre: weight 1 on that cell
    i0, j0, w = probe_weights(np.array([3.5]), np.array([2.5]), nx, ny)
    assert (i0[0], j0[0]) == (3, 2) and w[:, 0].tolist() == [1.0, 0.0, 0.0, 0.0]
    # the borders of the valid rectangle: x = 0.5 is cell 0; x = NX - 0.5 has base NX - 2 and tx = 1, y likewise
    i0, j0, w = probe_weights(np.array([0.5, nx - 0.5, 0.5, nx - 0.5]), np.array([0.5, 0.5, ny - 0.5, ny - 0.5]), nx, ny)
    assert i0.tolist() == [0, nx - 2, 0, nx - 2] and j0.tolist() == [0, 0, ny - 2, ny - 2]
    assert w.T.tolist() == [[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]]
    # a point on a vertical face, a quarter above a row of centres: half and half in x, 3/4 and 1/4 in y
    i0, j0, w = probe_weights(np.array([5.0]), np.array([3.75]), nx, ny)
    assert (i0[0], j0[0]) == (4, 3) and w[:, 0].tolist() == [0.375, 0.375, 0.125, 0.125]
    # the order of operations: gx = x - 0.5, tx = gx - i0, sx = 1.0 - tx, w00 = sx * sy
    x, y = 7.3, 4.9
    tx, ty = (x - 0.5) - 6, (y - 0.5) - 4
    i0, j0, w = probe_weights(x, y, nx, ny)
    assert (int(i0), int(j0)) == (6, 4) and w.tolist() == [(1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty]
    # NaN x is inactive, whatever y holds
    i0, j0, w = probe_weights(np.array([np.nan, np.nan, 1.5]), np.array([np.nan, 1e9, 1.5]), nx, ny)
    assert i0.tolist() == [-1, -1, 1] and j0.tolist() == [-1, -1, 1] and not w[:, :2].any() and w[0, 2] == 1.0
    assert i0.dtype == np.int64 and w.dtype == np.float64 and w.shape == (4, 3)
    # everything else outside the rectangle raises
    for bx, by in ((0.49, 3.0), (nx - 0.49, 3.0), (3.0, 0.49), (3.0, ny - 0.49), (3.0, np.nan), (np.inf, 3.0), (-np.inf, 3.0), (3.0, np.inf)):
        with pytest.raises(ValueError, match="outside"):
            probe_weights(np.array([2.5, bx]), np.array([2.5, by]), nx, ny)
    with pytest.raises(ValueError):
        probe_weights(np.zeros(3), np.zeros(2), nx, ny)


# ---- 2. the reference can tell a misread -------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_reference_can_tell_a_misread(pkg, dtype):
    """On a field with no two cells alike, a base cell shifted by one row or one column, w10 and w01 exchanged and a wrong plane each
    change bits at every tested point."""
    nx, ny, P = 97, 53, 257
    f = rough_state(nx, ny, 0.06, np.dtype(dtype), 5).astype(np.float64)
    rho = f.sum(axis=0)
    macro = tuple(a.astype(dtype) for a in (rho, (f[1] + f[5] + f[8] - f[3] - f[6] - f[7]) / rho, (f[2] + f[5] + f[6] - f[4] - f[7] - f[8]) / rho))
    for a in macro:                                                        # no cell like another within the reach of a shifted stencil
        mid = a[2:ny - 2, 2:nx - 2]
        assert all((mid != a[2 + dj:ny - 2 + dj, 2 + di:nx - 2 + di]).all() for di in range(-2, 3) for dj in range(-2, 3) if (di, dj) != (0, 0))
    assert not any((a == b).any() for a, b in ((macro[0], macro[1]), (macro[0], macro[2]), (macro[1], macro[2])))
    rng = np.random.default_rng(9)
    # interior points off the centres and off the faces (every weight non-zero, a shifted stencil stays inside), tx != ty
    x, y = rng.uniform(2.6, nx - 2.6, P), rng.uniform(2.6, ny - 2.6, P)
    good = pr.sample(macro, x, y)
    assert all(np.isfinite(good[k]).all() for k in pr.PLANES)
    misreads = {"column + 1": dict(di=1), "column - 1": dict(di=-1), "row + 1": dict(dj=1), "row - 1": dict(dj=-1), "w10 <-> w01": dict(swap=True)}
    for name, kw in misreads.items():
        bad = pr.sample(macro, x, y, **kw)
        for k in pr.PLANES:
            assert (bad[k].view(np.uint64) != good[k].view(np.uint64)).all(), (name, k)
    for planes in ((1, 0, 2), (0, 2, 1), (2, 1, 0)):
        bad = pr.sample(macro, x, y, planes=planes)
        for k, p in zip(pr.PLANES, planes):
            assert (bad[k].view(np.uint64) != good[k].view(np.uint64)).all() == (pr.PLANES[p] != k), (planes, k)
    # the sums follow the samples: two samples, added in order; inactive points stay +0 and NaN
    xs, ys = pr.point_set(nx, ny, P, np.zeros((ny, nx), np.uint8), 3)
    two = pr.accumulate([macro, tuple(a[::-1].copy() for a in macro)], xs, ys)
    first, second = pr.sample(macro, xs, ys), pr.sample(tuple(a[::-1].copy() for a in macro), xs, ys)
    off = np.isnan(xs)
    assert off.sum() == 3 and two["n"] == 2
    for k in pr.PLANES:
        assert np.isnan(first[k][off]).all() and (two[k][off] == 0).all() and not np.signbit(two[k][off]).any()
        assert np.array_equal(two[k][~off], first[k][~off] + second[k][~off])


# ---- 3. the boundary-layer arithmetic ----------------------------------------------------------
def _flat_stations(n, nx=400, ny=200):
    """n stations on a flat wall along y = 20, the flow along +x: all on the upper side, x/c rising."""
    x = np.linspace(60.0, 300.0, n)
    return {"x": x, "y": np.full(n, 20.0), "nrm_x": np.zeros(n), "nrm_y": np.ones(n), "tan_x": np.ones(n), "tan_y": np.zeros(n),
            "upper": np.ones(n, bool), "x_over_c": (x - 60.0) / 240.0, "lattice": (nx, ny), "chord_cells": 240.0}


def test_boundary_layer_on_an_analytic_profile(pkg):
    """u_t/Ue = sin(pi h / 2 delta) below delta and 1 above, delta = 20 cells, spacing 0.5.  Exact: delta*/delta = 1 - 2/pi,
    theta/delta = (4 - pi)/(2 pi), H = 2.660, wall slope pi Ue / (2 delta).  The tolerance is the sum of three bounds:
      trapezoid   spacing^2/12 * max|f''| * h_e on the intervals of one spacing, with |f''| <= (pi/2 delta)^2 for f = 1 - r and
                  <= 3 (pi/2 delta)^2 for f = r(1 - r) = sin - sin^2 (|(sin)''| <= k^2, |(sin^2)''| = |2 k^2 cos 2kh| <= 2 k^2);
      0.99 cut    the integral stops at h_e, the first rake height with r >= 0.99, not at delta: the integrand there is at most 0.01
                  (1 - r <= 0.01 and r(1 - r) <= 0.01), so at most 0.01 (delta - h_e) is missing;
      first cell  the samples below one cell are left out, so [0, 1] is one trapezoid of width 1 and not two of width 0.5: its error is at
                  most 1^2/12 * max|f''| * 1 in place of the two small intervals' share of the first bound (counted there too; kept)."""
    from airfoil_cfd_tool_amd.polar import BL_EDGE, boundary_layer, boundary_layer_points
    delta, spacing, ue_lat, u0, tau = 20.0, 0.5, 0.07, 0.05, 0.6
    st = _flat_stations(4)
    x, y, h = boundary_layer_points(st, 30.0, spacing)
    assert h.size == 60 and h[0] == 0.5 and h[-1] == 30.0 and x.shape == (240,) and not np.isnan(x).any()
    assert np.array_equal(x.reshape(4, 60)[:, 7], st["x"]) and np.array_equal(y.reshape(4, 60)[2], 20.0 + h)       # station-major, along the normal
    r = np.where(h < delta, np.sin(np.pi * h / (2 * delta)), 1.0)
    means = {"ux": np.tile(ue_lat * r, 4), "uy": np.tile(0.3 * r, 4)}         # (uy is normal to the wall: not in u_t)
    bl = boundary_layer(st, means, h, u0, tau)
    side = bl["upper"]
    assert len(bl["lower"]["station"]) == 0 and side["station"].tolist() == [0, 1, 2, 3] and np.array_equal(bl["heights"], h)
    k = np.pi / (2 * delta)
    h_e = float(h[np.nonzero((h >= 1.0) & (r >= BL_EDGE))[0][0]])
    assert delta - 2.0 < h_e < delta
    chord = st["chord_cells"]
    for name, exact, curv in (("dstar", delta * (1 - 2 / np.pi), k * k), ("theta", delta * (4 - np.pi) / (2 * np.pi), 3 * k * k)):
        tol = spacing ** 2 / 12 * curv * h_e + 0.01 * (delta - h_e) + 1.0 / 12 * curv
        err = np.abs(side[name] * chord - exact).max()
        print(f"{name}: {side[name][0] * chord:.5f} cells, exact {exact:.5f}, error {err:.3g}, tolerance {tol:.3g}")
        assert err <= tol and tol < 0.01 * exact
    H = (1 - 2 / np.pi) / ((4 - np.pi) / (2 * np.pi))
    assert abs(H - 2.660) < 5e-4
    # H = dstar/theta: the relative errors of the two add (first order), each at most its tolerance over its exact value
    tol_h = H * ((spacing ** 2 / 12 * k * k * h_e + 0.01 * (delta - h_e) + k * k / 12) / (delta * (1 - 2 / np.pi))
                 + (spacing ** 2 / 12 * 3 * k * k * h_e + 0.01 * (delta - h_e) + 3 * k * k / 12) / (delta * (4 - np.pi) / (2 * np.pi))) * 1.01
    print(f"H: {side['H'][0]:.5f}, exact {H:.5f}, tolerance {tol_h:.3g}")
    assert np.abs(side["H"] - H).max() <= tol_h and np.array_equal(side["H"], side["dstar"] / side["theta"])
    assert np.array_equal(side["ue"], np.full(4, ue_lat * 1.0 / u0))
    # Cf: the one-sided difference at h_1 = 1 cell against the exact wall slope: sin(k)/k - 1 >= -k^2/6 relative
    nu = (tau - 0.5) / 3
    cf_exact = 2 * nu * (np.pi * ue_lat / (2 * delta)) / u0 ** 2
    assert np.array_equal(side["cf"], np.full(4, 2 * nu * ((ue_lat * r[1]) / h[1]) / (u0 * u0))) and h[1] == 1.0
    assert 0 <= (cf_exact - side["cf"][0]) / cf_exact <= k * k / 6
    assert np.isnan(side["x_sep"]) and np.isnan(side["x_reattach"])            # attached
    # a station whose rake holds an inactive point is NaN throughout, and is skipped by the sign search
    means["ux"] = means["ux"].copy()
    means["ux"][60 + 17] = np.nan
    hole = boundary_layer(st, means, h, u0, tau)["upper"]
    for name in ("ue", "dstar", "theta", "cf", "H"):
        assert np.isnan(hole[name][1]) and np.array_equal(hole[name][[0, 2, 3]], side[name][[0, 2, 3]]), name
    # the rake that runs towards the leading edge is read in its own direction: the same thicknesses, Ue and Cf negative
    back = boundary_layer(st, {"ux": -np.tile(ue_lat * r, 4), "uy": means["uy"]}, h, u0, tau)["upper"]
    assert np.array_equal(back["dstar"], side["dstar"]) and np.array_equal(back["ue"], -side["ue"]) and np.array_equal(back["cf"], -side["cf"])
    with pytest.raises(ValueError):
        boundary_layer(st, {"ux": np.zeros(4), "uy": np.zeros(4)}, np.array([0.5]), u0, tau)           # no height of one cell
    for height, sp in ((0.4, 0.5), (3.0, 0.0), (3.0, -1.0), (np.inf, 0.5), (np.nan, 0.5)):
        with pytest.raises(ValueError):
            boundary_layer_points(st, height, sp)


def test_separation_and_reattachment_are_the_interpolated_sign_changes(pkg):
    from airfoil_cfd_tool_amd.polar import boundary_layer
    n, u0, tau = 9, 0.05, 0.8
    st = _flat_stations(n)
    st["upper"] = np.array([True] * 9)
    h = np.array([0.5, 1.0, 1.5, 2.0, 2.5, 3.0])
    # the speed at h_1 = 1 cell per station; the outer flow stays forward: a reversed stretch between stations 3 and 6
    wall = np.array([0.03, 0.02, 0.01, -0.01, -0.02, -0.005, 0.015, 0.02, 0.03])
    ux = np.tile(np.array([0.0, 0.0, 0.03, 0.04, 0.05, 0.05]), (n, 1))
    ux[:, 0], ux[:, 1] = 0.5 * wall, wall
    bl = boundary_layer(st, {"ux": ux, "uy": np.zeros_like(ux)}, h, u0, tau)["upper"]
    xc = st["x_over_c"]
    nu = (tau - 0.5) / 3
    assert np.array_equal(bl["cf"], 2.0 * nu * (wall / 1.0) / (u0 * u0))
    assert bl["x_sep"] == xc[2] + (xc[3] - xc[2]) * (bl["cf"][2] / (bl["cf"][2] - bl["cf"][3])) and xc[2] < bl["x_sep"] < xc[3]
    assert abs(bl["x_sep"] - (xc[2] + 0.5 * (xc[3] - xc[2]))) < 1e-15         # 0.01 to -0.01: half-way
    assert bl["x_reattach"] == xc[5] + (xc[6] - xc[5]) * (bl["cf"][5] / (bl["cf"][5] - bl["cf"][6])) and xc[5] < bl["x_reattach"] < xc[6]
    assert abs(bl["x_reattach"] - (xc[5] + 0.25 * (xc[6] - xc[5]))) < 1e-15   # -0.005 to 0.015: a quarter of the way
    assert np.isfinite(bl["dstar"]).all() and (bl["ue"] == 0.05 / u0).all()
    # reversed to the last station: separated, never reattached; the sides are ordered from the leading edge whatever the panel order
    ux[6:, 1] = -0.01
    flipped = {k: (v[::-1].copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    lo = boundary_layer(flipped, {"ux": ux[::-1].copy(), "uy": np.zeros_like(ux)}, h, u0, tau)["upper"]
    assert lo["x_sep"] == bl["x_sep"] and np.isnan(lo["x_reattach"]) and lo["station"].tolist() == list(range(8, -1, -1))
    # negative from the first station on (leading edge to stagnation point), then positive: no separation
    ux[:, 1] = np.where(np.arange(n) < 2, -0.01, 0.02)
    stag = boundary_layer(st, {"ux": ux, "uy": np.zeros_like(ux)}, h, u0, tau)["upper"]
    assert np.isnan(stag["x_sep"]) and np.isnan(stag["x_reattach"]) and (stag["cf"][:2] < 0).all()


# ---- 4. the stations ---------------------------------------------------------------------------
def test_surface_stations_of_a_naca_2412(pkg):
    geo = pkg.geometry
    nx, ny = 320, 160
    st0 = None
    for alpha in (0.0, 8.0):
        g = geo.build_geometry(nx, ny, alpha, [], "naca2412")
        st = geo.surface_stations(g, nx, ny)
        assert all(np.shape(st[k]) == (geo.NP,) for k in ("x", "y", "nrm_x", "nrm_y", "tan_x", "tan_y", "upper", "x_over_c"))
        assert st["lattice"] == (nx, ny) and st["chord_cells"] == nx / (geo.DX1 - geo.DX0)
        # midpoints, mapped as raster_mask maps them
        X, Y = geo.to_lattice(g.xp, g.yp, nx, ny)
        assert np.array_equal(st["x"], 0.5 * (X[:-1] + X[1:])) and np.array_equal(st["y"], 0.5 * (Y[:-1] + Y[1:]))
        assert X[0] == (g.xp[0] - geo.DX0) / (geo.DX1 - geo.DX0) * nx and Y[3] == (g.yp[3] + 0.46) / 0.92 * ny
        # unit vectors, normal across tangent
        assert np.abs(np.hypot(st["nrm_x"], st["nrm_y"]) - 1).max() < 1e-15 and np.abs(np.hypot(st["tan_x"], st["tan_y"]) - 1).max() < 1e-15
        assert np.abs(st["nrm_x"] * st["tan_x"] + st["nrm_y"] * st["tan_y"]).max() < 1e-15
        # outward: the point one cell along the normal is not solid, the one a cell inwards is or lies in the thin tail
        for sign, want in ((1.0, False), (-1.0, True)):
            px, py = st["x"] + sign * st["nrm_x"], st["y"] + sign * st["nrm_y"]
            solid = g.mask[np.floor(py).astype(int), np.floor(px).astype(int)] != 0
            assert not solid.any() if not want else solid[(st["x_over_c"] > 0.05) & (st["x_over_c"] < 0.7)].all()
        # 80 panels per side; the tangent runs from the leading edge to the trailing edge on both: x/c rises along it, in body axes
        assert st["upper"].sum() == 80 and st["upper"][:80].all() and not st["upper"][80:].any()
        a = math.radians(alpha)                                              # the body's x axis in lattice axes: rotate() turns it by -alpha
        along = st["tan_x"] * math.cos(a) + st["tan_y"] * -math.sin(a)
        assert (along[(st["x_over_c"] > 0.02)] > 0).all()
        assert (st["nrm_y"][st["upper"] & (st["x_over_c"] > 0.1)] > 0).all() and (st["nrm_y"][~st["upper"] & (st["x_over_c"] > 0.1)] < 0).all()
        assert st["x_over_c"].min() >= 0 and st["x_over_c"].max() <= 1
        if st0 is None:
            st0 = st
        else:                                                                # x/c does not move with the angle (panelise resamples by arc length: rounding only)
            assert np.abs(st["x_over_c"] - st0["x_over_c"]).max() < 1e-12 and np.array_equal(st["upper"], st0["upper"])
    # a clockwise polyline (the points in the other order): the same outward normals, the sides exchanged in order
    g = geo.build_geometry(nx, ny, 4.0, [], "naca2412")
    st = geo.surface_stations(g, nx, ny)
    rev = geo.surface_stations(geo.Geometry(xp=g.xp[::-1].copy(), yp=g.yp[::-1].copy(), mask=g.mask, a_deg=4.0), nx, ny)
    for k in ("x", "y", "nrm_x", "nrm_y", "tan_x", "tan_y", "upper", "x_over_c"):
        assert np.allclose(rev[k][::-1], st[k], atol=1e-15) if rev[k].dtype != bool else np.array_equal(rev[k][::-1], st[k]), k


def test_no_rake_point_of_the_gpu_case_is_inactive(pkg):
    """The geometry of the GPU run_polar test: every rake point is valid, so every station there may be required to be finite."""
    from airfoil_cfd_tool_amd.polar import BL_HEIGHT_DEFAULT, BL_SPACING_DEFAULT, boundary_layer_points, probe_weights
    from airfoil_cfd_tool_amd.windtunnel import chord_cells
    nx, ny = GPU_CASE["nx"], GPU_CASE["ny"]
    for alpha in GPU_CASE["alphas"]:
        st = pkg.geometry.surface_stations(pkg.geometry.build_geometry(nx, ny, alpha, [], "naca2412"), nx, ny)
        x, y, h = boundary_layer_points(st, BL_HEIGHT_DEFAULT * chord_cells(nx), BL_SPACING_DEFAULT)
        assert h.size == 26 and x.size == 160 * 26 and not np.isnan(x).any() and not np.isnan(y).any()
        i0, _, _ = probe_weights(x, y, nx, ny)
        assert (i0 >= 0).all()
    # a rake that leaves the lattice: its points are inactive, not an error
    st = pkg.geometry.surface_stations(pkg.geometry.build_geometry(nx, ny, 0.0, [], "naca2412"), nx, ny)
    x, y, h = boundary_layer_points(st, 60.0, 0.5)
    assert np.isnan(x).any() and np.array_equal(np.isnan(x), np.isnan(y)) and (probe_weights(x, y, nx, ny)[0][np.isnan(x)] == -1).all()


# ---- 5. the C-ABI without a GPU ----------------------------------------------------------------
NEW = {
    "wtp_enable_probes": r"wtp_batch \* b , int npoints",
    "wtp_set_probes": r"wtp_batch \* b , int first , int count , const double \* x , const double \* y",
    "wtp_probe_sums": r"wtp_batch \* b , int member , int64_t \* n , double \* rho , double \* ux , double \* uy",
    "wtp_probe_sample": r"wtp_batch \* b , int member , double \* rho , double \* ux , double \* uy",
}


def test_entry_points_are_declared_exported_and_bound(pkg):
    from airfoil_cfd_tool_amd.polar import EXPORTS, POLAR_LIB_PATH, WTP_MAX_PROBES
    with open(os.path.join(ROOT, "include", "wt_polar.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    spaced = " ".join(re.sub(r"([(),*])", r" \1 ", header).split())          # every token apart, one blank between
    for name, args in NEW.items():
        assert re.search(r"\bint " + name + r" \( " + args + r" \)", spaced), name
        assert name in EXPORTS
    assert re.search(r"#define WTP_MAX_PROBES \(1 << 20\)", header) and WTP_MAX_PROBES == 1 << 20
    out = subprocess.run(["nm", "-D", "--defined-only", POLAR_LIB_PATH], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {s for s in syms if s.startswith("wtp_")} == set(EXPORTS) and len(set(EXPORTS)) == len(EXPORTS)
    assert set(re.findall(r"\b(wtp_\w+)\s*\(", header)) == set(EXPORTS)
    lib = pkg.polar.load_polar_library()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    want = {"wtp_enable_probes": [vp, ci], "wtp_set_probes": [vp, ci, ci, dp, dp], "wtp_probe_sums": [vp, ci, ip, dp, dp, dp],
            "wtp_probe_sample": [vp, ci, dp, dp, dp]}
    for name, argtypes in want.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes == argtypes, name
    version = lib.wtp_version()
    for phrase in (b"probe points", b"device-side far-field vortex", b"prescribed far-field profile", b"two-relaxation-time collision",
                   b"state upload and restart", b"half-precision population storage", b"inclined free stream", b"interpolated bounce-back",
                   b"Smagorinsky subgrid viscosity", b"mean fields", b"momentum exchange", b"surface loads"):
        assert phrase in version, phrase
    # a null batch is an argument error in every one of them
    one = np.ones(4)
    p = one.ctypes.data_as(dp)
    n = np.zeros(1, np.int64).ctypes.data_as(ip)
    calls = [lambda: lib.wtp_enable_probes(None, 4), lambda: lib.wtp_enable_probes(None, 0), lambda: lib.wtp_set_probes(None, 0, 1, p, p),
             lambda: lib.wtp_probe_sums(None, 0, n, p, p, p), lambda: lib.wtp_probe_sample(None, 0, p, p, p)]
    for k, call in enumerate(calls):
        assert call() == WT_ERR_ARG and b"null batch" in lib.wtp_last_error(), k
    for name in ("enable_probes", "set_probes", "probe_sums", "probe_sample"):
        assert callable(getattr(pkg.PolarEngine, name)), name
    assert isinstance(pkg.PolarEngine.probes_enabled, property)
    doc = " ".join(" ".join(re.sub(r"^\s*/?\*+/?", "", line) for line in text.splitlines()).split())
    for needle in ("gx = x - 0.5; i0 = min(max((int)floor(gx), 0), NX - 2); tx = gx - i0; sx = 1.0 - tx",
                   "w00 = sx*sy (cell (i0, j0)) w10 = tx*sy (cell (i0+1, j0))", "v = ((w00*a00 + w10*a10) + w01*a01) + w11*a11",
                   "A point whose x is NaN is inactive", "The points themselves survive all of these",
                   "A batch that never calls wtp_enable_probes launches the kernels it always launched and returns the bits it always returned"):
        assert needle in doc, needle


# ---- 6. run_polar ------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(bl_height=0.0), dict(bl_height=-0.1), dict(bl_height=float("nan")), dict(bl_height=float("inf")),
                                 dict(bl_spacing=0.0), dict(bl_spacing=-0.5), dict(bl_spacing=float("nan")), dict(bl_height=0.005),
                                 dict(bl_height=0.02, bl_spacing=3.0), dict(bl_height=0.4, bl_spacing=1e-4)])
def test_run_polar_refuses_a_bad_rake_before_an_engine_exists(pkg, monkeypatch, bad):
    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(pkg.polar, "PolarEngine", no_engine)
    with pytest.raises(ValueError, match="bl_|boundary-layer"):
        pkg.run_polar([2.0], nx=96, ny=48, samples=2, boundary_layer=True, **bad)


def test_run_polar_signature_and_rows(pkg):
    import dataclasses
    from airfoil_cfd_tool_amd.polar import PolarPoint, PolarResult, polar_rows
    sig = inspect.signature(pkg.run_polar).parameters
    assert (sig["boundary_layer"].default, sig["bl_height"].default, sig["bl_spacing"].default) == (False, 0.15, 0.5)
    doc = " ".join(pkg.run_polar.__doc__.split())
    assert "Cf uses the molecular viscosity" in doc and "polar_rows then carries x_sep_upper and x_sep_lower" in doc
    assert "no transition detection" in " ".join(pkg.polar.boundary_layer.__doc__.split())
    # a plain attribute: the constructor and the fields are what they were
    assert PolarPoint.boundary_layer is None and "boundary_layer" not in [f.name for f in dataclasses.fields(PolarPoint)]
    assert list(inspect.signature(PolarPoint).parameters)[-1] == "mean"

    def point(alpha, finite=True):
        return PolarPoint(alpha=alpha, cl_mean=0.5, cl_std=0.0, cd_mean=0.05, cd_std=0.0, sep_frac=0.0, separation="attached", samples=4,
                          finite=finite, clamp_events=(0, 0), cm_mean=-0.05)

    res = PolarResult(points=[point(0.0), point(4.0), point(8.0, finite=False)], nx=96, ny=48, tau=0.58, u0=0.06, warmup_steps=0, sample_every=12)
    plain = polar_rows(res)
    assert all(list(r) == ["α (°)", "CL", "CD", "L/D", "Cm", "Status"] for r in plain)
    side = {"x_sep": float("nan"), "x_reattach": float("nan")}
    res.points[0].boundary_layer = {"upper": dict(side), "lower": dict(side)}
    assert polar_rows(res) == plain                                          # not every point carries one: the rows as they were
    res.points[1].boundary_layer = {"upper": {"x_sep": 0.61234, "x_reattach": float("nan")}, "lower": dict(side)}
    res.points[2].boundary_layer = {"upper": {"x_sep": 0.3, "x_reattach": 0.5}, "lower": dict(side)}
    rows = polar_rows(res)
    assert all(list(r) == ["α (°)", "CL", "CD", "L/D", "Cm", "x_sep_upper", "x_sep_lower", "Status"] for r in rows)
    assert [(r["x_sep_upper"], r["x_sep_lower"]) for r in rows] == [("—", "—"), (0.612, "—"), ("—", "—")]
    assert all({k: v for k, v in r.items() if not k.startswith("x_sep")} == p for r, p in zip(rows, plain))
