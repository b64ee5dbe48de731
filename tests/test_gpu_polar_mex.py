"""GPU: momentum-exchange forces of batched sweeps (k_mex_batch) against the NumPy reference of tests/_mex_reference.py, evaluated on
the batch's own populations (read_f after every sampled call).

The tolerances are derived, not measured (Mex.fx_bound / fy_bound / mz_bound): a force term 2 f e is exact in double, so the two
sides differ by summation order alone, |F - F_ref| <= 2 (n - 1) 2^-53 sum|t|; a moment term a - b carries five roundings relative to
|a| + |b|, so |Mz - Mz_ref| <= 2 (n + 2) 2^-53 sum(|a| + |b|).
"""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal
from _mex_reference import count_links, mex_reference
from test_gpu_polar_loads import MEMBERS

pytestmark = pytest.mark.gpu

WT_ERR_ARG, WT_ERR_STATE = -1, -5
EVERY = 12
MEX_KEYS = ("fx_mex", "fy_mex", "mz_mex", "links")


def _mask(pkg, nx, ny, shape, aoa):
    return pkg.geometry.build_geometry(nx, ny, aoa, None, shape).mask


def _masks(pkg, nx, ny, members):
    return np.stack([_mask(pkg, nx, ny, s, a) for s, a, _, _ in members])


def _border_mask(nx, ny):
    """Solid rectangles that touch each of the four borders and reach into column 1 / row 1 / column NX-2 / row NY-2, and one
    detached block in the middle."""
    m = np.zeros((ny, nx), np.uint8)
    m[0:ny // 5, nx // 4:nx // 4 + 7] = 1                      # on the bottom row
    m[ny // 2 - 3:ny // 2 + 4, 0:5] = 1                        # on the inlet column
    m[ny - ny // 6:ny, nx // 2:nx // 2 + 9] = 1                # on the top row
    m[ny // 3:ny // 3 + 5, nx - 4:nx] = 1                      # on the outlet column
    m[ny // 2:ny // 2 + 6, nx // 2 + 20:nx // 2 + 26] = 1
    return m


def _refs(nx, ny, n):
    """A different off-centre reference point per member, none on a cell centre or a face."""
    return [0.3641 * nx + 1.7 * m for m in range(n)], [0.5 * ny - 0.85 * m - 3.3 for m in range(n)]


def _sampled_run(pkg, nx, ny, masks, tau, u0, dtype, calls, mex=True, loads=False, reference=True):
    """`calls` calls of EVERY steps, each ending in a sample and followed by read_f of every member, on which the reference is
    evaluated at once."""
    B = len(masks)
    xr, yr = _refs(nx, ny, B)
    out = {"masks": masks, "xr": xr, "yr": yr, "ref": []}
    with pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=calls) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        if loads:
            b.enable_loads(yr, xr)                                      # (other points than the momentum exchange's)
        if mex:
            b.enable_momentum_exchange(xr, yr)
        for _ in range(calls):
            b.step(EVERY, tau, u0, sample_every=EVERY)
            if reference:
                out["ref"].append([mex_reference(b.read_f(m), masks[m], xr[m], yr[m]) for m in range(B)])
        out["h"] = b.history()
        if mex:
            out["mex"] = b.momentum_exchange()
            out["h_after"] = b.history()
        if loads:
            out["surface"] = [b.surface(m) for m in range(B)]
            out["moment"] = b.moment()
        out["forces"] = b.forces()
        out["f"] = [b.read_f(m) for m in range(B)]
        out["macro"] = [b.read_macro(m) for m in range(B)]
    return out


def _assert_matches(run, min_links=100):
    h = run["h"]
    rows, B = len(run["ref"]), len(run["masks"])
    assert list(h["step"]) == [EVERY * (k + 1) for k in range(rows)]
    for k in MEX_KEYS:
        assert h[k].shape == (rows, B), k
    worst = [0.0, 0.0, 0.0]
    for r in range(rows):
        for m in range(B):
            ref = run["ref"][r][m]
            assert int(h["links"][r, m]) == ref.links == count_links(run["masks"][m]) and ref.links >= min_links, (r, m, h["links"][r, m], ref.links)
            for q, (got, want, bound) in enumerate(((h["fx_mex"][r, m], ref.fx, ref.fx_bound), (h["fy_mex"][r, m], ref.fy, ref.fy_bound),
                                                    (h["mz_mex"][r, m], ref.mz, ref.mz_bound))):
                err = abs(got - want)
                worst[q] = max(worst[q], err / bound)
                assert err <= bound, (r, m, "fx fy mz".split()[q], got, want, bound)
    print(f"momentum exchange: worst |x - ref| / bound = {worst[0]:.3g} (fx), {worst[1]:.3g} (fy), {worst[2]:.3g} (mz) over {rows} rows x {B} members")
    # wtp_mex on the current lattice = the state of the last sample; it added no row
    fx, fy, mz, links = run["mex"]
    assert bits_equal(fx, h["fx_mex"][-1]) and bits_equal(fy, h["fy_mex"][-1]) and bits_equal(mz, h["mz_mex"][-1])
    assert np.array_equal(links, h["links"][-1])
    assert len(run["h_after"]["step"]) == rows
    for m in range(B):                                                   # (a comparison of signal, not of noise against noise)
        ref = run["ref"][-1][m]
        assert np.hypot(ref.fx, ref.fy) > 1e3 * max(ref.fx_bound, ref.fy_bound), (m, ref.fx, ref.fy, ref.fx_bound, ref.fy_bound)
        assert abs(ref.mz) > 1e3 * ref.mz_bound, (m, ref.mz, ref.mz_bound)


def _tau_u0(members):
    return [m[2] for m in members], [m[3] for m in members]


@pytest.fixture(scope="module")
def run_320(pkg):
    return _sampled_run(pkg, 320, 160, _masks(pkg, 320, 160, MEMBERS), *_tau_u0(MEMBERS), "float32", 20)


def test_matches_the_reference(run_320):
    _assert_matches(run_320)
    assert list(run_320["h"]) == ["step", "fx", "fy", "surf", "rev", "fx_mex", "fy_mex", "mz_mex", "links"]


def test_ragged_lattice(pkg):
    """301x150 fp32: pitch != NY, a partial chunk of 64 rows, an odd NX against the sixteen-column blocks; member 2's body reaches
    into column 1 and row 1 (and NX-2, NY-2): the reference alone decides which cells own links."""
    nx, ny = 301, 150
    members = MEMBERS[:2] + [("border", 0.0, 0.6, 0.05)]
    masks = np.stack([_mask(pkg, nx, ny, *MEMBERS[0][:2]), _mask(pkg, nx, ny, *MEMBERS[1][:2]), _border_mask(nx, ny)])
    run = _sampled_run(pkg, nx, ny, masks, *_tau_u0(members), "float32", 10)
    _assert_matches(run)
    bm = _border_mask(nx, ny)
    assert bm[1, :].any() and bm[:, 1].any() and bm[ny - 2, :].any() and bm[:, nx - 2].any()


def test_fp64_batch(pkg):
    nx, ny = 96, 48
    members = [("naca4412", 14.0, 0.56, 0.08), ("naca0012", 4.0, 0.58, 0.06), ("border", 0.0, 0.9, 0.03)]
    masks = np.stack([_mask(pkg, nx, ny, "naca4412", 14.0), _mask(pkg, nx, ny, "naca0012", 4.0), _border_mask(nx, ny)])
    run = _sampled_run(pkg, nx, ny, masks, *_tau_u0(members), "float64", 12)
    _assert_matches(run, min_links=60)


@pytest.mark.parametrize("shape,aoa,links", [("naca0012", 0.0, 852), ("naca2412", 6.0, 870)])
def test_known_link_counts(pkg, shape, aoa, links):
    nx, ny = 256, 128
    mask = _mask(pkg, nx, ny, shape, aoa)
    assert count_links(mask) == links
    with pkg.PolarEngine(nx, ny, 1) as b:
        b.set_masks(mask)
        b.init_equilibrium(0.06)
        b.enable_momentum_exchange(*pkg.polar.quarter_chord(nx, ny))
        assert list(b.momentum_exchange()[3]) == [links]


def test_two_runs_give_the_same_bits(pkg, run_320):
    again = _sampled_run(pkg, 320, 160, run_320["masks"], *_tau_u0(MEMBERS), "float32", 20, reference=False)
    for k in ("fx_mex", "fy_mex", "mz_mex"):
        assert bits_equal(again["h"][k], run_320["h"][k]), k
    assert np.array_equal(again["h"]["links"], run_320["h"]["links"])
    for a, b in zip(again["mex"], run_320["mex"]):
        assert a.tobytes() == b.tobytes()


def test_the_sampling_changes_nothing_else(pkg, run_320):
    nx, ny = 320, 160
    args = (pkg, nx, ny, run_320["masks"], *_tau_u0(MEMBERS), "float32", 20)
    on = _sampled_run(*args, mex=True, loads=True, reference=False)
    off = _sampled_run(*args, mex=False, loads=True, reference=False)
    assert list(off["h"]) == ["step", "fx", "fy", "surf", "rev", "mz"]
    assert list(on["h"]) == ["step", "fx", "fy", "surf", "rev", "mz", "fx_mex", "fy_mex", "mz_mex", "links"]
    for k in ("fx", "fy", "mz"):
        assert bits_equal(on["h"][k], off["h"][k]), k
    for k in ("step", "surf", "rev"):
        assert np.array_equal(on["h"][k], off["h"][k]), k
    assert bits_equal(on["moment"], off["moment"])
    for a, b in zip(on["forces"], off["forces"]):
        assert a.tobytes() == b.tobytes()
    for m in range(len(MEMBERS)):
        for k, v in on["surface"][m].items():
            assert v.tobytes() == off["surface"][m][k].tobytes(), (m, k)
        assert bits_equal(on["f"][m], off["f"][m])
        assert all(bits_equal(a, b) for a, b in zip(on["macro"][m], off["macro"][m]))
    # with loads on beside it the momentum exchange is what it is alone, and the pressure forces are those of a plain batch
    for k in ("fx_mex", "fy_mex", "mz_mex"):
        assert bits_equal(on["h"][k], run_320["h"][k]), k
    for k in ("fx", "fy"):
        assert bits_equal(on["h"][k], run_320["h"][k]), k


def test_momentum_exchange_without_loads(pkg):
    nx, ny = 96, 48
    members = MEMBERS[:2]
    with pkg.PolarEngine(nx, ny, 2, history_cap=2) as b:
        b.set_masks(_masks(pkg, nx, ny, members))
        b.init_equilibrium(0.06)
        b.enable_momentum_exchange(30.0, 24.0)
        b.step(EVERY, 0.58, 0.06, sample_every=EVERY)
        h = b.history()
        assert "mz" not in h and np.isfinite(h["fx_mex"]).all() and (h["links"] > 0).all()
        mz = np.empty((1, 2))
        assert b._lib.wtp_history_moment(b._b, 0, 1, mz.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == WT_ERR_STATE
        with pytest.raises(pkg.WTError) as ei:
            b.moment()
        assert ei.value.code == WT_ERR_STATE and "wtp_enable_loads" in str(ei.value)


def test_members_do_not_leak_into_each_other(pkg):
    nx, ny = 320, 160
    members = MEMBERS[:3]
    masks = _masks(pkg, nx, ny, members)
    other = masks.copy()
    other[1] = _mask(pkg, nx, ny, "naca0012", 9.0)
    a = _sampled_run(pkg, nx, ny, masks, *_tau_u0(members), "float32", 4, reference=False)
    b = _sampled_run(pkg, nx, ny, other, *_tau_u0(members), "float32", 4, reference=False)
    for k in ("fx_mex", "fy_mex", "mz_mex"):
        assert bits_equal(a["h"][k][:, [0, 2]], b["h"][k][:, [0, 2]]), k
        assert (a["h"][k][:, 1] != b["h"][k][:, 1]).all(), k
    assert np.array_equal(a["h"]["links"][:, [0, 2]], b["h"]["links"][:, [0, 2]])
    assert (b["h"]["links"][:, 1] == count_links(other[1])).all() and count_links(other[1]) != count_links(masks[1])


def test_life_cycle(pkg):
    nx, ny = 320, 160
    members = MEMBERS[:3]
    tau, u0 = _tau_u0(members)
    masks = _masks(pkg, nx, ny, members)
    xr, yr = _refs(nx, ny, 3)
    with pkg.PolarEngine(nx, ny, 3, history_cap=8) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        b.step(EVERY, tau, u0, sample_every=EVERY)                      # a sample before the sampling is enabled
        b.enable_momentum_exchange(xr, yr)
        b.step(2 * EVERY, tau, u0, sample_every=EVERY)
        h = b.history()
        assert np.isnan(h["fx_mex"][0]).all() and np.isnan(h["fy_mex"][0]).all() and np.isnan(h["mz_mex"][0]).all() and (h["links"][0] == -1).all()
        assert np.isfinite(h["fx_mex"][1:]).all() and np.isfinite(h["mz_mex"][1:]).all() and (h["links"][1:] > 0).all()
        b.enable_momentum_exchange(yr, xr)                              # again: other points; earlier rows keep F and lose Mz
        b.step(EVERY, tau, u0, sample_every=EVERY)
        h2 = b.history()
        assert bits_equal(h2["fx_mex"][:3], h["fx_mex"]) and bits_equal(h2["fy_mex"][:3], h["fy_mex"]) and np.array_equal(h2["links"][:3], h["links"])
        assert np.isnan(h2["mz_mex"][:3]).all() and np.isfinite(h2["mz_mex"][3]).all()
        for m in range(3):
            ref = mex_reference(b.read_f(m), masks[m], yr[m], xr[m])
            assert abs(h2["mz_mex"][3, m] - ref.mz) <= ref.mz_bound and abs(h2["fx_mex"][3, m] - ref.fx) <= ref.fx_bound
        b.clear_history()
        assert all(len(b.history()[k]) == 0 for k in MEX_KEYS)
        b.step(EVERY, tau, u0, sample_every=EVERY)
        assert np.isfinite(b.history()["mz_mex"]).all() and len(b.history()["step"]) == 1
        # a new mask moves the member's window with it: only its links change
        new = _mask(pkg, nx, ny, "naca0012", 9.0)
        before = b.momentum_exchange()[3]
        b.set_masks(new, first=1)
        after = b.momentum_exchange()
        assert list(after[3]) == [before[0], count_links(new), before[2]] and count_links(new) != before[1]
        ref = mex_reference(b.read_f(1), new, yr[1], xr[1])
        assert abs(after[0][1] - ref.fx) <= ref.fx_bound and abs(after[2][1] - ref.mz) <= ref.mz_bound
        b.init_equilibrium(u0)                                          # restarts the count and empties the history; the sampling stays on
        assert len(b.history()["fx_mex"]) == 0
        b.step(EVERY, tau, u0, sample_every=EVERY)
        assert np.isfinite(b.history()["fx_mex"]).all() and list(b.history()["step"]) == [EVERY]


def test_argument_and_state_errors(pkg):
    nx, ny = 96, 48
    members = MEMBERS[:2]
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    x, n = np.empty((4, 2)), np.empty((4, 2), np.int64)
    with pkg.PolarEngine(nx, ny, 2, history_cap=2) as b:
        b.set_masks(_masks(pkg, nx, ny, members))
        b.init_equilibrium(0.06)
        with pytest.raises(pkg.WTError) as ei:
            b.momentum_exchange()
        assert ei.value.code == WT_ERR_STATE and "wtp_enable_mex" in str(ei.value)
        assert b._lib.wtp_history_mex(b._b, 0, 0, None, None, None, None) == WT_ERR_STATE
        assert not set(MEX_KEYS) & set(b.history())
        for bad in (float("nan"), float("inf")):
            with pytest.raises(pkg.WTError) as ei:
                b.enable_momentum_exchange([1.0, bad], [2.0, 3.0])
            assert ei.value.code == WT_ERR_ARG and "finite" in str(ei.value)
        assert b._lib.wtp_enable_mex(b._b, None, x.ctypes.data_as(dp)) == WT_ERR_ARG
        assert not b.mex_enabled
        b.enable_momentum_exchange(30.0, 24.0)
        b.step(EVERY, 0.58, 0.06, sample_every=EVERY)
        for first, count in ((0, 2), (-1, 1), (1, 1), (0, -1)):          # one row held
            assert b._lib.wtp_history_mex(b._b, first, count, x.ctypes.data_as(dp), None, None, None) == WT_ERR_ARG, (first, count)
        assert b._lib.wtp_history_mex(b._b, 0, 1, None, None, None, n.ctypes.data_as(ip)) == 0 and (n[0] > 0).all()
        assert b._lib.wtp_mex(b._b, x.ctypes.data_as(dp), x.ctypes.data_as(dp), None, n.ctypes.data_as(ip)) == WT_ERR_ARG
        assert np.isfinite(b.momentum_exchange()[0]).all()
    with pkg.PolarEngine(nx, ny, 2) as b:                               # no mask yet: nothing to reduce
        b.init_equilibrium(0.06)
        b.enable_momentum_exchange(30.0, 24.0)
        with pytest.raises(pkg.WTError) as ei:
            b.momentum_exchange()
        assert ei.value.code == WT_ERR_STATE


def test_developed_flow_has_friction_drag_and_the_same_lift(pkg):
    """256x128 fp32, tau 0.58, U0 0.06, 6000 steps, NACA 0012 at 0 deg and NACA 2412 at 6 deg.  The NumPy oracle gives, at that step,
    CD 0.1106 (pressure) / 0.3288 (total) and CL -0.00000 / -0.00001 for the first, CD 0.1564 / 0.3738 and CL 0.6785 / 0.6908 for the
    second.  The thresholds are conditions with margins over those figures (4x and 2.8x on the friction, 2.8x on the lift), not
    tolerances on the kernel."""
    from airfoil_cfd_tool_amd.windtunnel import chord_cells
    nx, ny, tau, u0 = 256, 128, 0.58, 0.06
    masks = np.stack([_mask(pkg, nx, ny, "naca0012", 0.0), _mask(pkg, nx, ny, "naca2412", 6.0)])
    with pkg.PolarEngine(nx, ny, 2) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        b.enable_momentum_exchange(*pkg.polar.quarter_chord(nx, ny))
        b.step(6000, tau, u0)
        fxp, fyp, surf, _ = b.forces()
        fx, fy, mz, links = b.momentum_exchange()
    q = 0.5 * u0 * u0 * chord_cells(nx)
    cdp, clp, cdt, clt = fxp / q, fyp / q, fx / q, fy / q
    for m, name in enumerate(("NACA 0012 at 0", "NACA 2412 at 6")):
        print(f"{name}: CD pressure {cdp[m]:.4f}, total {cdt[m]:.4f}, friction {cdt[m] - cdp[m]:.4f}; CL pressure {clp[m]:.5f}, total {clt[m]:.5f}; "
              f"Cm total {-mz[m] / (q * chord_cells(nx)):.4f}; {links[m]} links")
    assert list(links) == [852, 870] and (surf > 0).all()
    assert abs(clt[0]) < 1e-3
    assert (cdt - cdp > 0.5 * cdp).all() and (cdp > 0).all()
    assert abs(clt[1] - clp[1]) < 0.05 * abs(clp[1])


def test_run_polar_reports_total_forces(pkg):
    alphas = [0, 4, 8]
    kw = dict(nx=160, ny=80, samples=8, warmup_steps=600)
    res = pkg.run_polar(alphas, total_forces=True, **kw)
    totals = ("cl_total_mean", "cl_total_std", "cd_total_mean", "cd_total_std", "cm_total_mean", "cm_total_std", "cd_friction_mean")
    for p in res.points:
        assert all(isinstance(getattr(p, k), float) and np.isfinite(getattr(p, k)) for k in totals), p
        assert p.cd_friction_mean == p.cd_total_mean - p.cd_mean
        assert all(p.history[k].shape == (8,) for k in MEX_KEYS) and p.converged
    rows = pkg.polar_rows(res, forces="total")
    assert all(list(r) == ["α (°)", "CL", "CD", "CDp", "CDf", "L/D", "Cm", "Status"] for r in rows)
    for r, p in zip(rows, res.points):
        assert (r["CL"], r["CD"], r["CDp"], r["CDf"]) == (round(p.cl_total_mean, 4), round(p.cd_total_mean, 5), round(p.cd_mean, 5), round(p.cd_friction_mean, 5))
        assert r["Cm"] == round(p.cm_total_mean, 4) and r["Status"] == "✅ Converged"
    off = pkg.run_polar(alphas, total_forces=False, **kw)
    assert pkg.polar_rows(res) == pkg.polar_rows(off) and all(list(r) == ["α (°)", "CL", "CD", "L/D", "Cm", "Status"] for r in pkg.polar_rows(off))
    for p, q in zip(res.points, off.points):
        assert (p.cl_mean, p.cl_std, p.cd_mean, p.cd_std, p.sep_frac, p.cm_mean, p.cm_std) == (q.cl_mean, q.cl_std, q.cd_mean, q.cd_std, q.sep_frac, q.cm_mean, q.cm_std)
        assert all(getattr(q, k) is None for k in totals) and not set(MEX_KEYS) & set(q.history)
    with pytest.raises(ValueError):
        pkg.polar_rows(off, forces="total")
