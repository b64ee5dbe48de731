"""Interpolated bounce-back of batched sweeps (wtp_enable_ibb, geometry.wall_distances, polar.py): what needs no GPU."""
import ctypes
import dataclasses
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _ibb_reference as ibb
import _les_reference as les
import _polar_isa
from _mex_reference import link_masks

WT_ERR_ARG = -1

# (nx, ny, shape, angle, links, links without a crossing): the three geometries the feature was prototyped on
GEOMETRIES = [(160, 80, "naca2412", 6.0, 544, 57), (320, 160, "naca2412", 10.0, 1096, 179), (96, 48, "naca0012", 0.0, 304, 20)]


# ---- the C-ABI without a GPU -------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound(pkg):
    from airfoil_cfd_tool_amd.polar import EXPORTS, POLAR_LIB_PATH
    with open(os.path.join(ROOT, "include", "wt_polar.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", POLAR_LIB_PATH], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = pkg.polar.load_polar_library()
    assert re.search(r"\bint\s+wtp_enable_ibb\s*\(\s*wtp_batch\s*\*\s*b\s*,\s*int\s+on\s*\)", header)
    assert re.search(r"\bint\s+wtp_set_wall_q\s*\(\s*wtp_batch\s*\*\s*b\s*,\s*int\s+first\s*,\s*int\s+count\s*,\s*const\s+void\s*\*\s*q\s*\)", header)
    for name in ("wtp_enable_ibb", "wtp_set_wall_q"):
        assert name in syms and name in EXPORTS
    assert lib.wtp_enable_ibb.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert lib.wtp_set_wall_q.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    # the header, the kernel comment and the reference carry one definition, word for word
    def words(path):
        with open(path) as fh:
            return " ".join(" ".join(re.sub(r"^\s*(/?\*+/?|//)", "", line) for line in fh.read().splitlines()).split())
    for path in (os.path.join(ROOT, "include", "wt_polar.h"), os.path.join(ROOT, "airfoil-cfd-tool_amd", "csrc", "d2q9.hpp"),
                 os.path.join(ROOT, "tests", "_ibb_reference.py")):
        doc = words(path)
        for needle in ("two = 2*q", "q < 0.5: fin = two*a + (1 - two)*g if x - e_k is not solid, else fin = a",
                       "q >= 0.5: inv = 1/two; fin = inv*a + (1 - inv)*h"):
            assert needle in doc, (path, needle)
    assert "bytes per member" in words(os.path.join(ROOT, "include", "wt_polar.h"))
    v = lib.wtp_version()
    assert b"interpolated bounce-back" in v and b"Smagorinsky" in v


def test_null_batch_is_an_argument_error(pkg):
    lib = pkg.polar.load_polar_library()
    q = np.full((1, 8, 4, 4), 0.5, np.float32)
    assert lib.wtp_enable_ibb(None, 1) == WT_ERR_ARG
    assert b"null batch" in lib.wtp_last_error()
    assert lib.wtp_enable_ibb(None, 0) == WT_ERR_ARG
    assert lib.wtp_set_wall_q(None, 0, 1, q.ctypes.data_as(ctypes.c_void_p)) == WT_ERR_ARG


# ---- run_polar, PolarEngine, PolarResult -------------------------------------------------------
@pytest.mark.parametrize("bad", ["curved", "", None, 1, "Interpolated"])
def test_run_polar_validates_walls_before_creating_the_engine(pkg, monkeypatch, bad):
    def no_engine(*a, **k):
        raise AssertionError("the engine was created")
    monkeypatch.setattr(pkg.polar, "PolarEngine", no_engine)
    with pytest.raises(ValueError, match="walls"):
        pkg.run_polar([4.0], nx=96, ny=48, walls=bad)


def test_run_polar_engine_and_result_expose_the_switch(pkg):
    from airfoil_cfd_tool_amd.polar import PolarResult
    sig = inspect.signature(pkg.run_polar)
    assert sig.parameters["walls"].default == "staircase" and sig.parameters["walls"].kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(pkg.PolarEngine.enable_interpolated_walls) and callable(pkg.PolarEngine.set_wall_distances)
    assert inspect.signature(pkg.PolarEngine.enable_interpolated_walls).parameters["on"].default is True
    assert inspect.signature(pkg.PolarEngine.set_wall_distances).parameters["first"].default == 0
    r = PolarResult(points=[], nx=320, ny=160, tau=0.58, u0=0.06, warmup_steps=0, sample_every=12)
    assert r.walls == "staircase" and r.les is None
    r = PolarResult(points=[], nx=320, ny=160, tau=0.58, u0=0.06, warmup_steps=0, sample_every=12, walls="interpolated")
    assert r.walls == "interpolated"
    assert "walls" not in [f.name for f in dataclasses.fields(PolarResult)]       # (the fields callers enumerate are unchanged)
    assert inspect.signature(pkg.polar_rows).parameters.keys() == {"result", "forces"}


# ---- the wall distances ------------------------------------------------------------------------
def _links(mask):
    return np.stack(link_masks(mask)[1:])                                          # [8][NY][NX], plane k - 1 for direction k


@pytest.mark.parametrize("nx,ny,shape,alpha,links,missed", GEOMETRIES)
def test_wall_distances_of_an_airfoil(pkg, nx, ny, shape, alpha, links, missed):
    g = pkg.geometry.build_geometry(nx, ny, alpha, None, shape)
    q = pkg.geometry.wall_distances(g.xp, g.yp, g.mask, nx, ny)
    own = _links(g.mask)
    assert q.shape == (8, ny, nx) and q.dtype == np.float64
    assert (q > 0.0).all() and (q <= 1.0).all()
    assert (q[~own] == 0.5).all()
    n, fell_back = int(own.sum()), int((own & (q == 0.5)).sum())
    print(f"{nx}x{ny} {shape} {alpha}: {n} links, {fell_back} without a crossing ({100.0 * fell_back / n:.1f} %), q in [{q[own].min():.4f}, {q[own].max():.4f}]")
    assert (n, fell_back) == (links, missed)
    assert 5 * fell_back <= n                       # the fallback must not swallow the feature: at most one link in five
    below, above = int((q[own] < 0.5).sum()), int((q[own] > 0.5).sum())
    assert below > n // 5 and above > n // 5         # (distances on both branches of the rule)
    # y_half: the default is the lattice's own window
    assert np.array_equal(q, pkg.geometry.wall_distances(g.xp, g.yp, g.mask, nx, ny, pkg.geometry.domain_y_half(nx, ny)))


def test_wall_distances_of_a_circle_are_the_ray_circle_distances(pkg):
    """A 64-gon inscribed in a circle of radius R lies inside the circle by at most its sagitta R (1 - cos(pi / 64)), measured along the
    normal.  So the wall point P + q e_k found on the polygon lies within the sagitta of the circle, on its inside, and q is never
    below the analytic ray-circle distance t.  Along the link the two differ by more than the sagitta where the link crosses the gap
    obliquely, and that is bounded too: the polygon lies between the circle and its incircle (radius R cos(pi / 64)), so q lies between
    t and the ray's distance t_in to the incircle.  Along a straight ray the radius falls at the rate cos(angle to the inward normal),
    which is smallest where the ray meets the incircle (cos = sqrt(r^2 - h^2) / r with h the ray's distance from the centre), so
    (t_in - t) |e_k| <= sagitta / cos(incidence on the incircle), and with it |q - t| |e_k|: the sagitta, seen along the link.
    The mask is unambiguous: no cell centre lies between the polygon's incircle and the circle, so every link starts outside the
    circle and ends inside the incircle."""
    geo = pkg.geometry
    nx, ny, R, n = 96, 48, 7.77, 64
    cx, cy = 30.13, 20.9
    y_half = geo.domain_y_half(nx, ny)
    th = 2.0 * math.pi * np.arange(n) / n
    X, Y = cx + R * np.cos(th), cy + R * np.sin(th)
    xp = X / nx * (geo.DX1 - geo.DX0) + geo.DX0                  # the inverse of the rasteriser's map
    yp = Y / ny * (2 * y_half) - y_half
    jj, ii = np.meshgrid(np.arange(ny) + 0.5, np.arange(nx) + 0.5, indexing="ij")
    apothem = R * math.cos(math.pi / n)
    sagitta = R - apothem
    radius = np.hypot(ii - cx, jj - cy)
    assert not ((radius >= apothem) & (radius <= R)).any()
    mask = np.where(radius < apothem, 255, 0).astype(np.uint8)
    q = geo.wall_distances(xp, yp, mask, nx, ny)
    own = _links(mask)
    assert int(own.sum()) > 100 and (q[~own] == 0.5).all() and (q > 0).all() and (q <= 1).all()
    worst_normal = worst_link = 0.0
    for k, (ex, ey) in enumerate(ibb.E[1:]):
        px, py = ii[own[k]] - cx, jj[own[k]] - cy                  # the links' fluid centres, relative to the circle's
        qk = q[k][own[k]]
        a, b, c = ex * ex + ey * ey, px * ex + py * ey, px * px + py * py - R * R
        t = (-b - np.sqrt(b * b - a * c)) / a                      # |P + t e - centre| = R, the first root
        assert ((t > 0) & (t <= 1)).all()
        normal = np.abs(np.hypot(px + qk * ex, py + qk * ey) - R)  # the wall point's distance from the circle
        assert (normal <= sagitta + 1e-12).all(), (k, normal.max())
        along = np.abs(qk - t)
        assert (qk >= t - 1e-12).all(), k                          # (the polygon lies inside the circle: the ray meets the circle first)
        disc_in = b * b - a * (px * px + py * py - apothem * apothem)
        assert (disc_in > 0).all(), k                              # (every link ends inside the incircle)
        t_in = (-b - np.sqrt(disc_in)) / a                         # the ray's distance to the incircle
        assert (qk <= t_in + 1e-12).all(), (k, float((qk - t_in).max()))
        cos_in = np.sqrt(disc_in / a) / apothem                    # the incidence on the incircle
        assert (along * math.sqrt(a) <= sagitta / cos_in + 1e-12).all(), (k, float((along * math.sqrt(a) * cos_in).max()))
        worst_normal, worst_link = max(worst_normal, float(normal.max())), max(worst_link, float(along.max()))
    print(f"64-gon, R {R}: sagitta {sagitta:.5f}, wall points within {worst_normal:.5f} of the circle, worst |q - analytic| {worst_link:.5f} "
          f"over {int(own.sum())} links")


# ---- the reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_with_half_everywhere_is_the_bgk_oracle(pkg, oracle_np, dtype):
    nx, ny, u0, tau = 96, 48, 0.06, 0.58
    mask = pkg.geometry.build_geometry(nx, ny, 6.0, None, "naca2412").mask
    q = np.full((8, ny, nx), 0.5, dtype)
    f, _ = oracle_np.equilibrium_init(nx, ny, u0, dtype)
    g = f.copy()
    for _ in range(40):
        f, mf = oracle_np.step(f, mask, tau, u0)
        g, mg = ibb.step(g, mask, tau, u0, q)
    assert np.array_equal(f, g) and all(np.array_equal(a, b) for a, b in zip(mf, mg))
    assert np.ptp(f[1]) > 1e-3                                           # (a flow, not the initial state)


def test_reference_with_half_everywhere_and_the_les_collision_is_the_les_reference(pkg):
    nx, ny, u0, tau = 96, 48, 0.06, 0.5008
    mask = pkg.geometry.build_geometry(nx, ny, 6.0, None, "naca2412").mask
    c = les.les_constant(0.17, np.float32)
    q = np.full((8, ny, nx), 0.5, np.float32)
    f, mf, _ = les.run(mask, 40, tau, u0, c)
    g, mg = ibb.run(mask, 40, tau, u0, q, c)
    assert np.array_equal(f, g) and all(np.array_equal(a, b) for a, b in zip(mf, mg))
    assert not np.array_equal(g, ibb.run(mask, 40, tau, u0, q)[0])          # (the collision is not BGK)


def test_reference_with_true_distances_differs_at_the_body_and_stays_off_the_net(pkg, oracle_np):
    """96x48 NACA 0012 at 0 deg, tau 0.9, 400 steps: finite, zero clamp events, and not the staircase's flow."""
    nx, ny, u0, tau = 96, 48, 0.06, 0.9
    g = pkg.geometry.build_geometry(nx, ny, 0.0, None, "naca0012")
    q = pkg.geometry.wall_distances(g.xp, g.yp, g.mask, nx, ny).astype(np.float32)
    f, _ = oracle_np.equilibrium_init(nx, ny, u0, np.float32)
    first = None
    for s in range(400):
        f, macro = ibb.step(f, g.mask, tau, u0, q)
        if s == 0:
            first = f
        if (s + 1) % 50 == 0:
            assert np.isfinite(f).all() and oracle_np.clamp_events(*macro, g.mask) == (0, 0), s + 1
    plain, _ = oracle_np.run(g.mask, 400, tau, u0, np.float32)
    # the first step differs from the oracle's in cells that own a link, and nowhere else
    one, _ = oracle_np.run(g.mask, 1, tau, u0, np.float32)
    diff = (first != one).any(axis=0)
    assert diff.any() and not diff[~_links(g.mask).any(axis=0)].any()
    assert float(np.abs(f - plain).max()) > 1e-4
    xr, yr = 0.25 * nx, 0.5 * ny
    a, b = ibb.mex_reference(f, g.mask, q, xr, yr), ibb.mex_reference(f, g.mask, np.full_like(q, 0.5), xr, yr)
    from _mex_reference import mex_reference
    c = mex_reference(f, g.mask, xr, yr)
    assert (b.fx, b.fy, b.mz, b.links) == (c.fx, c.fy, c.mz, c.links)       # at q = 0.5 the term is the half-way one
    assert a.links == b.links == 304 and a.fx != b.fx and a.fx > 0
    print(f"drag by momentum exchange, interpolated term {a.fx:.6f}, half-way term on the same lattice {b.fx:.6f}")


# ---- the kernels' code object ------------------------------------------------------------------
@pytest.fixture(scope="module")
def polar_isa():
    return _polar_isa.polar_isa()


def test_ibb_kernels_have_their_instantiations_and_no_scratch(polar_isa):
    """The step: fp32 and fp64, emitting and not, BGK and Smagorinsky; the momentum exchange: fp32 and fp64.  No spill."""
    chk, files = polar_isa
    family = lambda v: v[0] == "native" and v[4:] == (_polar_isa.INTERP, _polar_isa.AXIAL)      # noqa: E731
    step = {name: r for name, (_, r) in _polar_isa.step_kernels(chk, files, family).items()}
    mex = {name: r for f in files for name, r in chk.resources(f).items() if _polar_isa.mex_variant(name) in (("f", "Interp"), ("d", "Interp"))}
    for name, r in {**step, **mex}.items():
        assert r.get("private_seg_size", 0) == 0, (name, r)
    print({k: v.get("num_vgpr") for k, v in {**step, **mex}.items()})
    assert len(step) == 8 and len(mex) == 2, (sorted(step), sorted(mex))
