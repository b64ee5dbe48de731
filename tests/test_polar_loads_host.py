"""Surface loads of batched sweeps (wtp_enable_loads, polar.py): what needs no GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import _polar_isa
from _loads_reference import loads_reference, surface_rows, surface_sums

WT_ERR_ARG = -1


# ---- the NumPy reference itself ----------------------------------------------------------------
def _blob_mask(rng, nx, ny):
    """A ragged solid blob that keeps two cells away from the border, with a hole and a detached cell."""
    m = np.zeros((ny, nx), np.uint8)
    for _ in range(12):
        i0, j0 = rng.integers(4, nx - 12), rng.integers(4, ny - 10)
        m[j0:j0 + rng.integers(1, 7), i0:i0 + rng.integers(1, 9)] = 255
    m[:2] = m[-2:] = 0
    m[:, :2] = m[:, -2:] = 0
    return m


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_uniform_density_has_no_load(seed):
    rng = np.random.default_rng(seed)
    nx, ny = 61, 37
    mask = _blob_mask(rng, nx, ny)
    for rho0 in (1.0, np.float32(1.0371), 0.9):
        r = loads_reference(np.full((ny, nx), rho0), mask, 17.3, 20.9)
        assert r.n > 20
        assert abs(r.fx) <= r.fx_bound and abs(r.fy) <= r.fy_bound, (r.fx, r.fy, r.fx_bound, r.fy_bound)
        assert abs(r.mz) <= r.mz_bound, (r.mz, r.mz_bound)
        assert r.mz_bound < 1e-9                      # (the bound itself is tight: it would not hide a missing face)


def test_reference_one_cell_in_a_linear_density_field():
    """One solid cell (i0, j0) in rho = 1 + a i: the faces above and below see the same rho and cancel, the left and right ones
    give Mz = (j0 + 0.5 - yref) (p_right - p_left) = (j0 + 0.5 - yref) 2 a / 3."""
    nx, ny, i0, j0, a = 20, 14, 8, 5, 0.375
    mask = np.zeros((ny, nx), np.uint8)
    mask[j0, i0] = 1
    rho = np.broadcast_to(1.0 + a * np.arange(nx), (ny, nx))
    for xr, yr in ((0.0, 0.0), (8.5, 9.25), (-3.0, 5.5)):
        r = loads_reference(rho, mask, xr, yr)
        assert r.n == 4
        assert abs(r.mz - (j0 + 0.5 - yr) * 2 * a / 3) <= r.mz_bound, (xr, yr, r.mz)
        assert abs(r.fx - (-2 * a / 3)) <= r.fx_bound and abs(r.fy) <= r.fy_bound      # the pressure rises with x: the force points upstream
    assert loads_reference(rho, mask, 0.0, j0 + 0.5).mz == 0.0                       # the x faces have no arm, the y faces cancel exactly


def test_reference_moving_the_reference_point():
    rng = np.random.default_rng(5)
    nx, ny = 61, 37
    mask = _blob_mask(rng, nx, ny)
    rho = (1.0 + 0.05 * rng.standard_normal((ny, nx))).astype(np.float32)
    r0 = loads_reference(rho, mask, 20.0, 18.0)
    for ddx, ddy in ((1.0, 0.0), (0.0, -2.5), (7.25, 3.5)):
        r1 = loads_reference(rho, mask, 20.0 + ddx, 18.0 + ddy)
        want = r0.mz - ddx * r0.fy + ddy * r0.fx
        assert abs(r1.mz - want) <= r0.mz_bound + r1.mz_bound + abs(ddx) * r0.fy_bound + abs(ddy) * r0.fx_bound, (ddx, ddy)
        assert r1.mz != r0.mz


def test_reference_ignores_neighbours_outside_the_grid():
    """A solid cell on the border has no face towards the outside, and the surface rows skip a column whose body touches the border."""
    mask = np.zeros((6, 5), np.uint8)
    mask[0, 2] = mask[5, 4] = mask[2:4, 1] = 1
    r = loads_reference(np.ones((6, 5)), mask, 0.0, 0.0)
    assert r.n == 3 + 2 + 6
    ju, jl = surface_rows(mask)
    assert list(ju) == [-1, 4, 1, -1, -1] and list(jl) == [-1, 1, -1, -1, 4]
    su, sl, nu, nl = surface_sums([np.full((6, 5), 2.0), np.full((6, 5), 3.0)], mask)
    assert list(su) == [0, 5, 5, 0, 0] and list(nl) == [0, 2, 0, 0, 2]


# ---- the C-ABI without a GPU -------------------------------------------------------------------
def test_null_arguments_are_argument_errors(pkg):
    import ctypes
    lib = pkg.polar.load_polar_library()
    x = (ctypes.c_double * 4)()
    n = (ctypes.c_int64 * 4)()
    j = (ctypes.c_int32 * 4)()
    assert lib.wtp_enable_loads(None, x, x) == WT_ERR_ARG
    assert b"null batch" in lib.wtp_last_error()
    assert lib.wtp_enable_loads(None, None, None) == WT_ERR_ARG
    assert lib.wtp_history_moment(None, 0, 0, x) == WT_ERR_ARG
    assert lib.wtp_moment(None, x) == WT_ERR_ARG
    assert lib.wtp_moment(None, None) == WT_ERR_ARG
    assert lib.wtp_surface(None, 0, x, x, n, n, j, j) == WT_ERR_ARG
    assert lib.wtp_surface(None, -1, None, None, None, None, None, None) == WT_ERR_ARG


def test_new_entry_points_are_exported_and_bound(pkg):
    from airfoil_cfd_tool_amd.polar import EXPORTS
    lib = pkg.polar.load_polar_library()
    for name in ("wtp_enable_loads", "wtp_history_moment", "wtp_moment", "wtp_surface"):
        assert name in EXPORTS and getattr(lib, name).argtypes is not None


# ---- polar.py ----------------------------------------------------------------------------------
def _history(n=30):
    rng = np.random.default_rng(11)
    surf = rng.integers(150, 170, n)
    surf[4] = 0
    return np.arange(1, n + 1) * 12, rng.normal(0.3, 0.05, n), rng.normal(2.0, 0.3, n), surf, rng.integers(0, 40, n), rng.normal(-40.0, 5.0, n)


def test_polar_point_without_a_moment_is_todays_point(pkg):
    import dataclasses
    from airfoil_cfd_tool_amd.polar import polar_point, raw_coefficients
    step, fx, fy, surf, rev, _ = _history()
    u0, nx = 0.05, 320
    p = polar_point(4.0, step, fx, fy, surf, rev, u0, nx, (0, 0))
    cl, cd, sep = raw_coefficients(fx, fy, surf, rev, u0, nx)
    want = dict(alpha=4.0, cl_mean=float(cl.mean()), cl_std=float(cl.std()), cd_mean=float(cd.mean()), cd_std=float(cd.std()),
                sep_frac=float(sep.mean()), separation=pkg.stall_label(float(sep.mean())), samples=29, finite=True, clamp_events=(0, 0))
    got = {f.name: getattr(p, f.name) for f in dataclasses.fields(p)}
    for k, v in want.items():
        assert got.pop(k) == v, k
    hist = got.pop("history")
    assert list(hist) == ["step", "fx", "fy", "surf", "rev"]
    assert got == {"cm_mean": None, "cm_std": None, "surface": None}
    assert p.converged


def test_polar_point_with_a_moment(pkg):
    from airfoil_cfd_tool_amd.polar import polar_point
    from airfoil_cfd_tool_amd.windtunnel import chord_cells
    step, fx, fy, surf, rev, mz = _history()
    u0, nx = 0.05, 320
    p = polar_point(4.0, step, fx, fy, surf, rev, u0, nx, (0, 0), mz=mz)
    q = polar_point(4.0, step, fx, fy, surf, rev, u0, nx, (0, 0))
    keep = surf != 0
    c = chord_cells(nx)
    assert p.cm_mean == -mz[keep].mean() / (0.5 * u0 * u0 * (c * c)) and p.cm_mean > 0      # Mz < 0 is clockwise: nose up
    assert p.cm_std == mz[keep].std() / (0.5 * u0 * u0 * (c * c))
    assert (p.cl_mean, p.cl_std, p.cd_mean, p.cd_std, p.sep_frac, p.samples) == (q.cl_mean, q.cl_std, q.cd_mean, q.cd_std, q.sep_frac, q.samples)
    assert list(p.history) == ["step", "fx", "fy", "surf", "rev", "mz"]
    empty = polar_point(0.0, step[:2], fx[:2], fy[:2], [0, 0], [0, 0], u0, nx, mz=mz[:2])
    assert empty.samples == 0 and np.isnan(empty.cm_mean) and not empty.converged


def test_polar_rows_show_cm_only_for_a_converged_point_that_carries_one(pkg):
    from airfoil_cfd_tool_amd.polar import PolarPoint, PolarResult
    base = dict(cl_mean=0.71, cl_std=0.01, cd_mean=0.04, cd_std=0.001, sep_frac=0.02, separation="Attached", samples=10, finite=True)
    pts = [PolarPoint(alpha=2.0, clamp_events=(0, 0), cm_mean=-0.0512345, cm_std=0.002, **base),
           PolarPoint(alpha=4.0, clamp_events=(0, 0), **base),
           PolarPoint(alpha=6.0, clamp_events=(1, 0), cm_mean=-0.06, cm_std=0.002, **base)]
    rows = pkg.polar_rows(PolarResult(points=pts, nx=320, ny=160, tau=0.58, u0=0.06, warmup_steps=0, sample_every=12))
    assert [r["Cm"] for r in rows] == [-0.0512, "—", "—"]
    assert all(list(r) == ["α (°)", "CL", "CD", "L/D", "Cm", "Status"] for r in rows)
    assert rows[2]["Status"] == "❌ Failed" and rows[0]["CL"] == rows[1]["CL"] == 0.71


def test_quarter_chord_and_surface_cp(pkg):
    from airfoil_cfd_tool_amd import geometry as geo
    from airfoil_cfd_tool_amd.polar import quarter_chord, surface_cp
    nx, ny, u0 = 320, 160, 0.06
    xr, yr = quarter_chord(nx, ny)
    assert yr == 80 and abs(geo.DX0 + xr / nx * (geo.DX1 - geo.DX0) - 0.25) < 1e-12
    s = {"rho_upper": np.zeros(nx), "rho_lower": np.zeros(nx), "n_upper": np.zeros(nx, np.int64), "n_lower": np.zeros(nx, np.int64),
         "j_upper": np.full(nx, -1, np.int32), "j_lower": np.full(nx, -1, np.int32)}
    s["j_upper"][100:110] = 90
    s["j_lower"][100:109] = 70
    s["rho_upper"][100:110], s["n_upper"][100:110] = 4 * 0.99, 4
    s["rho_lower"][100:109], s["n_lower"][100:109] = 4 * 1.01, 4
    cp = surface_cp(s, 0.0, u0)
    assert cp["x_over_c"].shape == cp["cp_upper"].shape == cp["cp_lower"].shape == (10,)
    assert np.allclose(cp["x_over_c"], geo.DX0 + (np.arange(100, 110) + 0.5) / nx * (geo.DX1 - geo.DX0))
    assert np.allclose(cp["cp_upper"], -0.01 / (1.5 * u0 * u0)) and np.allclose(cp["cp_lower"][:9], 0.01 / (1.5 * u0 * u0))
    assert np.isnan(cp["cp_lower"][9])
    # at an angle the chord line is foreshortened about the pivot (0.25, 0): a column's distance from it grows by 1 / cos
    rot = surface_cp(s, 10.0, u0)["x_over_c"]
    assert np.allclose(rot - 0.25, (cp["x_over_c"] - 0.25) / np.cos(np.radians(10.0)), rtol=1e-14, atol=0)


# ---- the kernel's code object ------------------------------------------------------------------
@pytest.fixture(scope="module")
def polar_isa():
    return _polar_isa.polar_isa()


def test_loads_kernel_has_no_scratch(polar_isa):
    chk, files = polar_isa
    seen = []
    for f in files:
        for name, r in chk.resources(f).items():
            if "k_loads_batch" in name:
                seen.append(name)
                assert r.get("private_seg_size", 0) == 0, (name, r)
    assert len(seen) == 2, seen                     # float and double
