"""Momentum-exchange forces of batched sweeps (wtp_enable_mex, polar.py): what needs no GPU."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import _polar_isa
from _mex_reference import E, count_links, link_masks, mex_reference

WT_ERR_ARG = -1
W = (4 / 9, 1 / 9, 1 / 9, 1 / 9, 1 / 9, 1 / 36, 1 / 36, 1 / 36, 1 / 36)


def _feq(rho, ux, uy):
    return [W[k] * rho * (1 + 3 * (ex * ux + ey * uy) + 4.5 * (ex * ux + ey * uy) ** 2 - 1.5 * (ux * ux + uy * uy)) for k, (ex, ey) in enumerate(E)]


def _uniform(nx, ny, vals, dtype=np.float64):
    f = np.empty((9, ny, nx), dtype)
    for k in range(9):
        f[k] = vals[k]
    return f


# ---- the NumPy reference itself ----------------------------------------------------------------
def _blob_mask(rng, nx, ny):
    """A ragged solid blob that keeps two cells away from the border, with holes and detached cells."""
    m = np.zeros((ny, nx), np.uint8)
    for _ in range(12):
        i0, j0 = rng.integers(4, nx - 12), rng.integers(4, ny - 10)
        m[j0:j0 + rng.integers(1, 7), i0:i0 + rng.integers(1, 9)] = 255
    m[:2] = m[-2:] = 0
    m[:, :2] = m[:, -2:] = 0
    return m


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_state_at_rest_exerts_no_force(seed):
    """f_k = w_k around a closed body clear of the border: every link k has its partner opp(k) on the other side of the body with
    the same weight, so F vanishes to the bound, and the links come in pairs."""
    rng = np.random.default_rng(seed)
    nx, ny = 61, 37
    mask = _blob_mask(rng, nx, ny)
    for dtype in (np.float64, np.float32):
        r = mex_reference(_uniform(nx, ny, W, dtype), mask, 17.3, 20.9)
        assert r.links > 40 and r.links % 2 == 0 and r.links == count_links(mask)
        assert abs(r.fx) <= r.fx_bound and abs(r.fy) <= r.fy_bound, (r.fx, r.fy, r.fx_bound, r.fy_bound)
        assert abs(r.mz) <= r.mz_bound, (r.mz, r.mz_bound)
        assert r.fx_bound < 1e-11 and r.mz_bound < 1e-9          # (the bounds are tight: they would not hide a missing link)


def test_reference_one_cell_in_a_uniform_stream():
    """One solid cell in feq(1, u0, 0): eight links, one per direction, the link of direction k owned by the cell at -e_k, so
    Fx = 2 sum_k f_k e_kx = 2 (f1 - f3 + f5 - f6 - f7 + f8) and Fy = 2 (f2 - f4 + f5 + f6 - f7 - f8) = 0."""
    nx, ny, i0, j0, u0 = 20, 14, 8, 5, 0.06
    mask = np.zeros((ny, nx), np.uint8)
    mask[j0, i0] = 1
    fe = _feq(1.0, u0, 0.0)
    f = _uniform(nx, ny, fe)
    r = mex_reference(f, mask, i0 + 0.5, j0 + 0.5)
    assert r.links == 8
    want = 2 * (fe[1] - fe[3] + fe[5] - fe[6] - fe[7] + fe[8])
    assert abs(r.fx - want) <= r.fx_bound and want > 0            # feq's first moment: Fx = 2 rho u0 (the stream pushes downstream)
    assert abs(want - 2 * u0) < 1e-15
    assert abs(r.fy) <= r.fy_bound
    assert abs(r.mz) <= r.mz_bound                                # symmetric about the cell's centre
    # each link's midpoint lies half a step from the solid cell's centre towards its owner
    owners = link_masks(mask)
    for k in range(1, 9):
        jj, ii = np.nonzero(owners[k])
        assert (list(ii), list(jj)) == ([i0 - E[k][0]], [j0 - E[k][1]])


def test_reference_moving_the_reference_point():
    rng = np.random.default_rng(5)
    nx, ny = 61, 37
    mask = _blob_mask(rng, nx, ny)
    f = (np.array(W)[:, None, None] * (1.0 + 0.05 * rng.standard_normal((9, ny, nx)))).astype(np.float32)
    r0 = mex_reference(f, mask, 20.0, 18.0)
    for ddx, ddy in ((1.0, 0.0), (0.0, -2.5), (7.25, 3.5)):
        r1 = mex_reference(f, mask, 20.0 + ddx, 18.0 + ddy)
        want = r0.mz - ddx * r0.fy + ddy * r0.fx
        assert abs(r1.mz - want) <= r0.mz_bound + r1.mz_bound + abs(ddx) * r0.fy_bound + abs(ddy) * r0.fx_bound + 4 * 2.0 ** -53 * abs(want), (ddx, ddy)
        assert r1.mz != r0.mz and (r1.fx, r1.fy) == (r0.fx, r0.fy)


def test_reference_only_interior_fluid_cells_own_links():
    """A solid block that reaches into row 1 and column 1: the border cells beside it own nothing, and a solid cell ON the border
    still gives its interior neighbours their links."""
    mask = np.zeros((8, 9), np.uint8)
    mask[0:3, 3:5] = 1                                            # rows 0-2, columns 3-4: touches the bottom border
    r = mex_reference(_uniform(9, 8, W), mask, 0.0, 0.0)
    # column 2: row 1 sees (3,0), (3,1), (3,2): 3 links; row 2 sees (3,1), (3,2): 2; row 3 sees (3,2): 1.  Column 5 likewise: 6 + 6.
    # row 3 above the block: column 3 sees (3,2) and (4,2), column 4 likewise: 4.  Row 0 beside the block owns nothing.
    assert r.links == 6 + 6 + 4
    mask2 = np.zeros((8, 9), np.uint8)
    mask2[3:5, 0:2] = 1                                           # columns 0-1: touches the inlet column
    r2 = mex_reference(_uniform(9, 8, W), mask2, 0.0, 0.0)
    # column 2, rows 2..5: 1 + 2 + 2 + 1 = 6; column 1, rows 2 and 5: the cell of column 1 above / below and the one of column 0
    # diagonally: 2 each.  Column 0 beside the block owns nothing.
    assert r2.links == 6 + 4
    assert count_links(np.ones((8, 9), np.uint8)) == 0 and count_links(np.zeros((8, 9), np.uint8)) == 0


@pytest.mark.parametrize("shape,aoa,links", [("naca0012", 0.0, 852), ("naca2412", 6.0, 870)])
def test_known_link_counts(pkg, shape, aoa, links):
    assert count_links(pkg.geometry.build_geometry(256, 128, aoa, None, shape).mask) == links


def test_oracle_flow_has_positive_friction_drag(pkg, oracle_np):
    """The NumPy oracle, 256x128 fp32, tau 0.58, U0 0.06, 2000 steps: the momentum exchange holds the wall shear that the
    pressure read-out does not see (friction 0.231 and 0.229 against pressure 0.111 and 0.171), and the two lifts agree."""
    from airfoil_cfd_tool_amd.windtunnel import chord_cells
    nx, ny, tau, u0 = 256, 128, 0.58, 0.06
    q = 0.5 * u0 * u0 * chord_cells(nx)
    for shape, aoa in (("naca0012", 0.0), ("naca2412", 6.0)):
        mask = pkg.geometry.build_geometry(nx, ny, aoa, None, shape).mask
        f, (rho, ux, uy) = oracle_np.run(mask, 2000, tau, u0, np.float32)
        r = mex_reference(f, mask, *pkg.polar.quarter_chord(nx, ny))
        fxp, fyp, surf, _ = oracle_np.compute_forces_raw(rho, ux, mask)
        cdp, cdt, clp, clt = fxp / q, r.fx / q, fyp / q, r.fy / q
        print(f"{shape} at {aoa}: CD pressure {cdp:.4f}, total {cdt:.4f}, friction {cdt - cdp:.4f}; CL pressure {clp:.5f}, total {clt:.5f}; {r.links} links")
        assert surf > 0 and cdp > 0
        assert cdt - cdp > 0.5 * cdp
        if aoa == 0.0:
            assert abs(clt) < 1e-3
        else:
            assert abs(clt - clp) < 0.05 * abs(clp)


# ---- the C-ABI without a GPU -------------------------------------------------------------------
def test_null_arguments_are_argument_errors(pkg):
    lib = pkg.polar.load_polar_library()
    x = (ctypes.c_double * 4)()
    n = (ctypes.c_int64 * 4)()
    assert lib.wtp_enable_mex(None, x, x) == WT_ERR_ARG
    assert b"null batch" in lib.wtp_last_error()
    assert lib.wtp_enable_mex(None, None, None) == WT_ERR_ARG
    assert lib.wtp_history_mex(None, 0, 0, x, x, x, n) == WT_ERR_ARG
    assert lib.wtp_history_mex(None, 0, 0, None, None, None, None) == WT_ERR_ARG
    assert lib.wtp_mex(None, x, x, x, n) == WT_ERR_ARG
    assert lib.wtp_mex(None, None, None, None, None) == WT_ERR_ARG


def test_new_entry_points_are_exported_and_bound(pkg):
    from airfoil_cfd_tool_amd.polar import EXPORTS
    lib = pkg.polar.load_polar_library()
    for name in ("wtp_enable_mex", "wtp_history_mex", "wtp_mex"):
        assert name in EXPORTS and getattr(lib, name).argtypes is not None
    assert len(lib.wtp_history_mex.argtypes) == 7 and len(lib.wtp_mex.argtypes) == 5 and len(lib.wtp_enable_mex.argtypes) == 3
    assert b"momentum exchange" in lib.wtp_version()


# ---- polar.py ----------------------------------------------------------------------------------
TOTALS = ("cl_total_mean", "cl_total_std", "cd_total_mean", "cd_total_std", "cm_total_mean", "cm_total_std", "cd_friction_mean")


def _history(n=30):
    rng = np.random.default_rng(11)
    surf = rng.integers(150, 170, n)
    surf[4] = 0
    return dict(step=np.arange(1, n + 1) * 12, fx=rng.normal(0.3, 0.05, n), fy=rng.normal(2.0, 0.3, n), surf=surf, rev=rng.integers(0, 40, n),
                mz=rng.normal(-40.0, 5.0, n), fx_mex=rng.normal(0.9, 0.05, n), fy_mex=rng.normal(2.05, 0.3, n), mz_mex=rng.normal(-42.0, 5.0, n),
                links=np.full(n, 870))


def test_polar_point_with_the_momentum_exchange(pkg):
    from airfoil_cfd_tool_amd.polar import polar_point
    from airfoil_cfd_tool_amd.windtunnel import chord_cells
    h = _history()
    u0, nx = 0.05, 320
    args = (4.0, h["step"], h["fx"], h["fy"], h["surf"], h["rev"], u0, nx, (0, 0))
    q = polar_point(*args, mz=h["mz"])
    assert all(getattr(q, k) is None for k in TOTALS)
    assert list(q.history) == ["step", "fx", "fy", "surf", "rev", "mz"]
    p = polar_point(*args, mz=h["mz"], fx_mex=h["fx_mex"], fy_mex=h["fy_mex"], mz_mex=h["mz_mex"], links=h["links"])
    keep = h["surf"] != 0
    c = chord_cells(nx)
    qd = 0.5 * u0 * u0 * c
    assert p.cl_total_mean == (h["fy_mex"][keep] / qd).mean() and p.cl_total_std == (h["fy_mex"][keep] / qd).std()
    assert p.cd_total_mean == (h["fx_mex"][keep] / qd).mean() and p.cd_total_std == (h["fx_mex"][keep] / qd).std()
    assert p.cm_total_mean == -h["mz_mex"][keep].mean() / (0.5 * u0 * u0 * (c * c)) and p.cm_total_mean > 0      # as cm_mean: nose up
    assert p.cm_total_std == h["mz_mex"][keep].std() / (0.5 * u0 * u0 * (c * c))
    assert p.cd_friction_mean == p.cd_total_mean - p.cd_mean and p.cd_friction_mean > 0
    # everything that existed is what it was
    for f in dataclasses.fields(p):
        if f.name != "history":
            assert getattr(p, f.name) == getattr(q, f.name), f.name
    assert list(p.history) == ["step", "fx", "fy", "surf", "rev", "mz", "fx_mex", "fy_mex", "mz_mex", "links"]
    empty = polar_point(0.0, h["step"][:2], h["fx"][:2], h["fy"][:2], [0, 0], [0, 0], u0, nx, fx_mex=h["fx_mex"][:2], fy_mex=h["fy_mex"][:2],
                        mz_mex=h["mz_mex"][:2])
    assert empty.samples == 0 and np.isnan(empty.cd_total_mean) and np.isnan(empty.cd_friction_mean) and not empty.converged
    with pytest.raises(ValueError):
        polar_point(*args, fx_mex=h["fx_mex"])
    with pytest.raises(TypeError):
        polar_point(*args, None, None, h["fx_mex"])              # the new histories are keyword-only


def test_polar_point_takes_the_totals_after_the_existing_fields(pkg):
    from airfoil_cfd_tool_amd.polar import PolarPoint
    base = dict(alpha=2.0, cl_mean=0.71, cl_std=0.01, cd_mean=0.04, cd_std=0.001, sep_frac=0.02, separation="Attached", samples=10, finite=True,
                clamp_events=(0, 0))
    p = PolarPoint(**base)
    assert all(getattr(p, k) is None for k in TOTALS)
    p = PolarPoint(**base, cd_total_mean=0.11, cd_friction_mean=0.07)
    assert (p.cd_total_mean, p.cd_friction_mean, p.cl_total_mean) == (0.11, 0.07, None)
    p = PolarPoint(*base.values(), {}, None, None, None, 0.7, 0.01, 0.11, 0.002, -0.05, 0.001, 0.07)
    assert [getattr(p, k) for k in TOTALS] == [0.7, 0.01, 0.11, 0.002, -0.05, 0.001, 0.07]


def test_polar_rows_with_total_forces(pkg):
    from airfoil_cfd_tool_amd.polar import PolarPoint, PolarResult
    base = dict(cl_mean=0.71, cl_std=0.01, cd_mean=0.0412345, cd_std=0.001, sep_frac=0.02, separation="Attached", samples=10, finite=True,
                cm_mean=-0.0512345, cm_std=0.002)
    tot = dict(cl_total_mean=0.7234567, cl_total_std=0.01, cd_total_mean=0.1098765, cd_total_std=0.002, cm_total_mean=-0.0498765,
               cm_total_std=0.002, cd_friction_mean=0.1098765 - 0.0412345)
    pts = [PolarPoint(alpha=2.0, clamp_events=(0, 0), **base, **tot), PolarPoint(alpha=6.0, clamp_events=(1, 0), **base, **tot)]

    def result(points):
        return PolarResult(points=points, nx=320, ny=160, tau=0.58, u0=0.06, warmup_steps=0, sample_every=12)

    rows = pkg.polar_rows(result(pts), forces="total")
    assert all(list(r) == ["α (°)", "CL", "CD", "CDp", "CDf", "L/D", "Cm", "Status"] for r in rows)
    assert rows[0] == {"α (°)": 2.0, "CL": 0.7235, "CD": 0.10988, "CDp": 0.04123, "CDf": round(0.1098765 - 0.0412345, 5),
                       "L/D": round(0.7234567 / 0.1098765, 2), "Cm": -0.0499, "Status": "✅ Converged"}
    assert rows[1] == {"α (°)": 6.0, "CL": "—", "CD": "—", "CDp": "—", "CDf": "—", "L/D": "—", "Cm": "—", "Status": "❌ Failed"}
    # the default is today's table, whether or not the points carry totals
    plain = [PolarPoint(alpha=p.alpha, clamp_events=p.clamp_events, **base) for p in pts]
    assert pkg.polar_rows(result(pts)) == pkg.polar_rows(result(plain)) == pkg.polar_rows(result(pts), forces="pressure")
    assert list(pkg.polar_rows(result(pts))[0]) == ["α (°)", "CL", "CD", "L/D", "Cm", "Status"]
    assert pkg.polar_rows(result(pts))[0]["CD"] == 0.04123
    with pytest.raises(ValueError):
        pkg.polar_rows(result([pts[0], plain[1]]), forces="total")
    with pytest.raises(ValueError):
        pkg.polar_rows(result(pts), forces="viscous")


def test_run_polar_and_engine_expose_the_switch(pkg):
    import inspect
    sig = inspect.signature(pkg.run_polar)
    assert sig.parameters["total_forces"].default is False and sig.parameters["total_forces"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(pkg.polar_rows).parameters["forces"].default == "pressure"
    assert callable(pkg.PolarEngine.enable_momentum_exchange) and callable(pkg.PolarEngine.momentum_exchange)


# ---- the kernel's code object ------------------------------------------------------------------
@pytest.fixture(scope="module")
def polar_isa():
    return _polar_isa.polar_isa()


def test_mex_kernel_has_no_scratch(polar_isa):
    chk, files = polar_isa
    seen = []
    for f in files:
        for name, r in chk.resources(f).items():
            if _polar_isa.mex_variant(name) in (("f", "Halfway"), ("d", "Halfway")):
                seen.append(name)
                assert r.get("private_seg_size", 0) == 0, (name, r)
    assert len(seen) == 2, seen                     # float and double


def test_the_mex_kernels_are_exactly_the_built_variants(polar_isa):
    """k_mex_batch<E, Link> holds the seven kernels that a sample can select, each once, and the momentum exchange has no kernel of another
    name; the two moving-wall ones, which no other test looks at, have no scratch."""
    chk, files = polar_isa
    res = {n: r for f in files for n, r in chk.resources(f).items() if "k_mex" in n}
    variants = [_polar_isa.mex_variant(n) for n in res]
    assert None not in variants, [n for n, v in zip(res, variants) if v is None]
    assert len(variants) == 7 and set(variants) == _polar_isa.mex_variants_built(), sorted(res)
    moving = [n for n in res if _polar_isa.mex_variant(n)[1] == "Moving"]
    assert len(moving) == 2
    for n in moving:
        assert res[n].get("private_seg_size", 0) == 0, (n, res[n])
