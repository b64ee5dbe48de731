"""GPU: the on-demand readouts (k_ranges, k_forces / forces_block / k_forces_batch, k_clamp_events, k_field, k_render,
k_advect) on ragged lattices, against the NumPy references of oracle/lbm_numpy.py computed from the handle's own
read_macro(), so that only the readout is under test (step parity is pinned elsewhere).

The lattices reach what the round shapes of the other files do not: partial 32x32 transpose tiles on both axes, pitch == ny
(no pad rows between columns: only the row guards keep row 0 from reading the previous column's top row), grids capped at
1024 blocks whose threads loop over several sites, solids on every border, a fully solid column, states at the stability
clamp, parameters under the 1e-6 floors and colour-map inputs outside [0, 1]; tracers on the window edges, outside the
lattice's cell centres and in and beside bodies; slabs cut by the caller; and batched sweeps."""
import numpy as np
import pytest

from conftest import bits_equal
from lbm_numpy import clamp_events

pytestmark = pytest.mark.gpu

TAU, U0 = 0.58, 0.06
CLAMP_TAU, CLAMP_U0 = 0.5004, 0.10             # low viscosity, fast inlet: the stability net (html:344-350) fires
VORT_SCALE = 0.06                               # html:528
GRID_SITES = 1024 * 256                         # sites one pass of a capped reduction grid covers
STEPS = 90

# nx, ny, dtype, shape, aoa, at the clamp
LATTICES = [
    (3, 3, "float32", None, 0.0, False),                    # the smallest lattice wt_create accepts, hand mask
    (37, 29, "float32", "naca4412", 24.0, False),           # partial tiles on both axes
    (200, 131, "float32", "clark_y", -7.5, False),
    (511, 256, "float32", "naca2412", 16.0, False),         # pitch == ny
    (731, 389, "float32", "naca4412", 18.0, True),          # 284 359 sites: the grid is capped, some threads loop twice
    (2049, 1031, "float32", "naca0012", 15.0, False),       # about 8 turns of the grid-stride loop
    (65, 130, "float64", "naca4412", 20.0, True),
    (300, 512, "float64", "naca2412", 16.0, False),         # pitch == ny
    (1111, 487, "float64", "naca6409", 14.0, False),
]


def _ids(lat):
    return f"{lat[0]}x{lat[1]}-{'f32' if lat[2] == 'float32' else 'f64'}" + ("-clamp" if lat[5] else "")


def _mask(pkg, nx, ny, shape, aoa, seed=0):
    """An airfoil, solid runs on row 0, row ny-1, column 0 and column nx-1, and one fully solid column behind the body.
    The runs end inside the rows, so that the first fluid site after a top-row run sits in row 0 of the next column."""
    if shape is None:                                                       # 3x3: row 0 / column 0 corner, a 2x2 block on the top right
        return np.array([[1, 0, 0], [0, 1, 1], [0, 1, 1]], np.uint8)
    rng = np.random.default_rng(1000 + nx + 7 * ny + seed)
    m = pkg.geometry.build_geometry(nx, ny, aoa, None, shape).mask.copy()
    m[m != 0] = 1
    for row in (0, ny - 1):
        for _ in range(3):
            x0 = int(rng.integers(1, nx - 2))
            m[row, x0:x0 + int(rng.integers(1, max(2, nx // 8)))] = 1
    for col in (0, nx - 1):
        y0 = int(rng.integers(1, ny - 2))
        m[y0:y0 + int(rng.integers(1, max(2, ny // 6))), col] = 1
    m[:, nx - 4] = 1                                                         # a fully solid column
    return m


def _run(e, mask, tau, u0, clamp):
    """Steps a fresh handle; at the clamp, until the reference counts sites at both kinds of bound."""
    e.set_mask(mask)
    e.init_equilibrium(u0)
    if not clamp:
        e.step(STEPS, tau, u0)
        return
    for _ in range(60):
        e.step(50, tau, u0)
        ev = clamp_events(*e.read_macro(), mask)
        if ev[0] > 0 and ev[1] > 0:
            break


def _check_field_and_render(e, oracle_np, macro, mask, u0, params):
    """wt_field bits (NaN pattern included) and wt_render_rgba bytes in all three modes; returns the reference scalars."""
    rho, ux, uy = macro
    ts = []
    for mode in (0, 1, 2):
        t = e.field(mode, u0, *params)
        ref = oracle_np.field_scalar(mode, rho, ux, uy, mask, u0, *params)
        assert t.dtype == ref.dtype and t.shape == ref.shape
        assert np.array_equal(np.isnan(t), np.isnan(ref)) and np.array_equal(np.isnan(ref), mask != 0), (mode, params)
        assert bits_equal(np.nan_to_num(t), np.nan_to_num(ref)), (mode, params)
        img = e.render_rgba(mode, u0, *params)
        want = oracle_np.render_rgba8(mode, ref, mask)
        bad = np.argwhere((img != want).any(axis=-1))
        assert bad.size == 0, (mode, params, len(bad), bad[:4].tolist())
        ts.append(ref)
    return ts


def _forces_close(got, ref):
    fx, fy, surf, rev = got
    rfx, rfy, rsurf, rrev = ref
    assert (surf, rev) == (rsurf, rrev), (got, ref)
    np.testing.assert_allclose([fx, fy], [rfx, rfy], rtol=1e-12, atol=1e-14 * max(1, surf))


@pytest.mark.parametrize("lat", LATTICES, ids=_ids)
def test_readouts_on_ragged_lattices(pkg, oracle_np, lat):
    nx, ny, dtype, shape, aoa, clamp = lat
    mask = _mask(pkg, nx, ny, shape, aoa)
    tau, u0 = (CLAMP_TAU, CLAMP_U0) if clamp else (TAU, U0)
    with pkg.Engine(nx, ny, dtype=dtype) as e:
        _run(e, mask, tau, u0, clamp)
        macro = e.read_macro()
        rho, ux, uy = macro
        assert np.isfinite(rho).all() and np.isfinite(ux).all() and np.isfinite(uy).all()
        ranges = oracle_np.ranges_from_macro(rho, ux, uy, mask, u0)
        np.testing.assert_allclose(e.reduce_ranges(u0), ranges, rtol=1e-13, atol=0)
        ref_f = oracle_np.compute_forces_raw(rho, ux, mask)
        _forces_close(e.forces(), ref_f)
        ref_ev = oracle_np.clamp_events(rho, ux, uy, mask)
        assert e.clamp_events() == ref_ev
        _check_field_and_render(e, oracle_np, macro, mask, u0, ranges + (VORT_SCALE,))
    # each lattice reached what it is here for
    if shape is not None:
        assert ref_f[3] > 0, "no reversed face: the angle is too low for this state"
        assert (mask[:, nx - 4] != 0).all() and mask[0].any() and mask[ny - 1].any() and mask[:, 0].any() and mask[:, nx - 1].any()
    if ny % 256 == 0:                                                       # pitch == ny: a top-row solid beside a row-0 fluid site
        assert (mask[ny - 1, :-1].astype(bool) & (mask[0, 1:] == 0)).any()
    if nx >= 700:                                                           # the capped grid loops
        assert nx * ny > GRID_SITES
    if clamp:
        assert ref_ev[0] > 0 and ref_ev[1] > 0, ref_ev


@pytest.mark.parametrize("dtype,nx,ny", [("float32", 731, 389), ("float64", 65, 130)])
def test_clamp_events_at_every_bound(pkg, oracle_np, dtype, nx, ny):
    """Populations written by hand, one step: patches of sites whose density sum is above 2, below 0.5, and whose speed is
    above 0.35, so that the net stores rho == 2.0, rho == 0.5 and |u| == 0.35 (up to rounding) on known sites."""
    mask = _mask(pkg, nx, ny, "naca2412", 6.0)
    with pkg.Engine(nx, ny, dtype=dtype) as e:
        e.set_mask(mask)
        e.init_equilibrium(U0)
        f = e.read_f()
        T = f.dtype.type
        y0, x0 = ny // 5, 2
        f[:, y0:y0 + 4, x0:x0 + 6] *= T(3.0)                                   # rho 3 -> 2.0
        f[:, y0 + 8:y0 + 11, x0:x0 + 5] *= T(0.25)                             # rho 0.25 -> 0.5
        f[1, y0 + 16:y0 + 19, x0:x0 + 5] += T(0.6)                             # fast in +x: |u| -> 0.35
        e.write_f(f)
        e.step(1, TAU, U0)
        rho, ux, uy = e.read_macro()
        ref = oracle_np.clamp_events(rho, ux, uy, mask)
        assert e.clamp_events() == ref
    fluid = mask == 0
    assert (rho[fluid] == T(2.0)).sum() > 0 and (rho[fluid] == T(0.5)).sum() > 0 and ref[1] > 0, ref


# --------------------------------------------------------------------------------------------------------------------------------------------
# parameters under the 1e-6 floors of field_value and colour-map inputs outside [0, 1] / [-1, 1]
# --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nx,ny,shape,aoa", [("float32", 37, 29, "naca4412", 24.0), ("float64", 65, 130, "naca4412", 20.0)])
def test_floors_and_clamps(pkg, oracle_np, dtype, nx, ny, shape, aoa):
    mask = _mask(pkg, nx, ny, shape, aoa)
    fluid = mask == 0
    with pkg.Engine(nx, ny, dtype=dtype) as e:
        _run(e, mask, TAU, U0, False)
        macro = e.read_macro()
        T = macro[0].dtype.type
        mx, cmin, cmax = oracle_np.ranges_from_macro(*macro, mask, U0)
        cmid = float(np.median(((macro[0].astype(np.float64) - 1) / (1.5 * U0 * U0))[fluid]))
        floor = T(1e-6)
        cases = [  # (max_s, cp_min, cp_max, vort_scale), what the case asserts
            ((0.0, cmid, cmid, 0.0), "floor"),                        # max_s 0, cpMax == cpMin, vortScale 0
            ((1e-7, cmax, cmin, 1e-9), "floor"),                      # max_s 1e-7, cpMax < cpMin, tiny vortScale
            ((2e-6, cmin + 0.6 * (cmax - cmin), cmax + 1.0, 1e-3), "clamp"),    # no floor: t >> 1, t < 0, |t| > 1
        ]
        lo, hi = [False] * 3, [False] * 3                                    # some t below 0 (-1 for vort) / above 1, per mode
        for params, what in cases:
            max_s, cp_min, cp_max, vs = params
            dens = (T(max_s) * T(0.92), T(cp_max) - T(cp_min), T(U0) * T(vs))
            ts = _check_field_and_render(e, oracle_np, macro, mask, U0, params)
            ts = [t[fluid] for t in ts]
            assert all(np.isfinite(t).all() for t in ts), params              # (no NaN t on fluid sites)
            if what == "floor":
                assert all(d < floor for d in dens), (params, dens)
            else:
                assert all(d > floor for d in dens), (params, dens)
                assert ts[0].min() > 1 and (ts[1] < 0).any() and (np.abs(ts[2]) > 1).any()
            for k, t in enumerate(ts):
                lo[k] |= bool((t < (-1 if k == 2 else 0)).any())
                hi[k] |= bool((t > 1).any())
        assert hi == [True] * 3 and lo[1:] == [True, True], (lo, hi)     # both clamps of every map; t == 1 -> stop index nseg - 1


# --------------------------------------------------------------------------------------------------------------------------------------------
# tracers: sampleUV / advect (html:616-639, 758-771)
# --------------------------------------------------------------------------------------------------------------------------------------------
def _particles(rng, mask, window):
    """~10 k uniform particles over a box 5 % larger than the window, and crafted ones, each with its category."""
    ny, nx = mask.shape
    dx0, dx1, dy0, dy1 = window
    cw, ch = (dx1 - dx0) / nx, (dy1 - dy0) / ny
    pts, cat = [], []

    def add(x, y, name):
        x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
        pts.append(np.stack([x.ravel(), y.ravel()], 1))
        cat.extend([name] * x.size)

    mx, my = 0.05 * (dx1 - dx0), 0.05 * (dy1 - dy0)
    add(rng.uniform(dx0 - mx, dx1 + mx, 10_000), rng.uniform(dy0 - my, dy1 + my, 10_000), "random")
    ys, xs = rng.uniform(dy0, dy1, 24), rng.uniform(dx0, dx1, 24)
    add(dx0, ys, "edge"); add(dx1, ys, "edge"); add(xs, dy0, "edge"); add(xs, dy1, "edge")
    add(np.nextafter(dx0, -np.inf), ys, "ulp_out"); add(np.nextafter(dx1, np.inf), ys, "ulp_out")
    add(xs, np.nextafter(dy0, -np.inf), "ulp_out"); add(xs, np.nextafter(dy1, np.inf), "ulp_out")
    add(np.nextafter(dx0, np.inf), ys, "ulp_in"); add(np.nextafter(dx1, -np.inf), ys, "ulp_in")
    add(dx0 + rng.uniform(0, 0.5, 24) * cw, ys, "fx_below_0")                    # fx in [-0.5, 0)
    add(dx1 - rng.uniform(0, 0.5, 24) * cw, ys, "fx_above_nx1")                  # fx in (NX-1, NX-0.5]
    add(xs, dy0 + rng.uniform(0, 0.5, 24) * ch, "fy_below_0")
    add(xs, dy1 - rng.uniform(0, 0.5, 24) * ch, "fy_above_ny1")
    # cells by their solid corners: (ix, iy) .. (ix+1, iy+1)
    s = mask != 0
    corners = s[:-1, :-1].astype(int) + s[:-1, 1:] + s[1:, :-1] + s[1:, 1:]
    for name, sel in (("in_body", corners == 4), ("beside_body", (corners > 0) & (corners < 4))):
        iy, ix = np.nonzero(sel)
        k = rng.permutation(iy.size)[:200]
        fx = ix[k] + rng.uniform(0.05, 0.95, k.size)
        fy = iy[k] + rng.uniform(0.05, 0.95, k.size)
        add(dx0 + (fx + 0.5) / nx * (dx1 - dx0), dy0 + (fy + 0.5) / ny * (dy1 - dy0), name)
    return np.concatenate(pts), np.array(cat)


TRACER_LATTICES = [(3, 3, "float32", None, 0.0), (37, 29, "float32", "naca4412", 24.0), (200, 131, "float32", "clark_y", -7.5),
                   (3, 3, "float64", None, 0.0), (65, 130, "float64", "naca4412", 20.0)]


@pytest.mark.parametrize("lat", TRACER_LATTICES, ids=lambda lat: f"{lat[0]}x{lat[1]}-{lat[2]}")
def test_tracers(pkg, oracle_np, lat):
    nx, ny, dtype, shape, aoa = lat
    mask = _mask(pkg, nx, ny, shape, aoa)
    rng = np.random.default_rng(nx * 131 + ny)
    yh = 1.84 * ny / nx / 2
    windows = [(oracle_np.DX0, oracle_np.DX1, -yh, yh), (-1.1, 2.3, -0.35, 0.8)]
    seen = set()
    with pkg.Engine(nx, ny, dtype=dtype) as e:
        _run(e, mask, TAU, U0, False)
        ux, uy = e.read_macro()[1:]
        for window in windows:
            pts, cat = _particles(rng, mask, window)
            for dt in (16.0, 400.0):
                xn, yn, sp, ok = e.advect_tracers(pts[:, 0], pts[:, 1], dt, U0, window)
                rx, ry, rs, rok = oracle_np.advect(ux, uy, mask, U0, window, pts[:, 0], pts[:, 1], dt)
                assert np.array_equal(ok, rok), (window, dt, np.unique(cat[ok != rok]))
                np.testing.assert_allclose(np.stack([xn, yn, sp], 1)[ok], np.stack([rx, ry, rs], 1)[ok], rtol=1e-12, atol=1e-14)
                assert np.array_equal(xn[~ok], pts[~ok, 0]) and np.array_equal(yn[~ok], pts[~ok, 1]) and (sp[~ok] == 0).all()
                u1, v1, _ = oracle_np.sample_uv(ux, uy, mask, U0, window, pts[:, 0], pts[:, 1])
                capped = rok & (np.hypot(u1, v1) * 0.00105 * dt > 0.05)
                seen |= {("capped", dt)} if capped.any() else set()
                seen |= {("uncapped", dt)} if (rok & ~capped).any() else set()
            seen |= {(c, "ok") for c in np.unique(cat[rok])} | {(c, "null") for c in np.unique(cat[~rok])}
    want = {("edge", "ok"), ("ulp_in", "ok"), ("ulp_out", "null"), ("fx_below_0", "ok"), ("fx_above_nx1", "ok"),
            ("fy_below_0", "ok"), ("fy_above_ny1", "ok"), ("in_body", "null"), ("beside_body", "ok"),
            ("random", "ok"), ("random", "null"), ("capped", 400.0), ("uncapped", 16.0)}
    assert want <= seen, sorted(want - seen)
    assert ("ulp_out", "ok") not in seen and ("in_body", "ok") not in seen


# --------------------------------------------------------------------------------------------------------------------------------------------
# slabs cut by the caller
# --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nx,ny,edges,block", [
    ("float32", 333, 200, [0, 101, 104, 251, 292, 297, 333], (290, 300)),
    ("float64", 200, 131, [0, 45, 48, 120, 163, 170, 200], (160, 173)),
], ids=["f32", "f64"])
def test_slab_readouts(pkg, oracle_np, dtype, nx, ny, edges, block):
    halo = 2
    mask = _mask(pkg, nx, ny, "naca2412", 12.0)
    mask[:, block[0]:block[1]] = 1                                              # a slab lies wholly inside this block
    widths = np.diff(edges)
    assert all(w % 32 for w in widths) and min(widths) >= max(2, halo)
    assert any(block[0] <= a and b <= block[1] for a, b in zip(edges[:-1], edges[1:]))
    es = [pkg.Engine(nx, ny, dtype=dtype, rank=r, nranks=len(edges) - 1, halo=halo, edges=edges) for r in range(len(edges) - 1)]
    try:
        pkg.Engine.link_local(es)
        for e in es:
            e.set_mask(mask)
            e.init_equilibrium(U0)
        pkg.Engine.step_group(es, STEPS, TAU, U0)
        macro = tuple(np.concatenate(parts, axis=1) for parts in zip(*[e.read_macro() for e in es]))
        rho, ux, uy = macro
        with pkg.Engine(nx, ny, dtype=dtype) as whole:                      # (the slabs hold the whole lattice's state)
            whole.set_mask(mask)
            whole.init_equilibrium(U0)
            whole.step(STEPS, TAU, U0)
            assert all(bits_equal(a, c) for a, c in zip(whole.read_macro(), macro))
        ranges = oracle_np.ranges_from_macro(rho, ux, uy, mask, U0)
        rr = [e.reduce_ranges(U0) for e in es]
        got = (max(r[0] for r in rr), min(r[1] for r in rr), max(r[2] for r in rr))
        np.testing.assert_allclose(got, ranges, rtol=1e-13, atol=0)
        ff = [e.forces() for e in es]
        _forces_close(tuple(sum(x[k] for x in ff) for k in range(4)), oracle_np.compute_forces_raw(rho, ux, mask))
        ev = [e.clamp_events() for e in es]
        assert (sum(a for a, _ in ev), sum(b for _, b in ev)) == oracle_np.clamp_events(rho, ux, uy, mask)
        params = ranges + (VORT_SCALE,)
        for mode in (0, 1, 2):
            t = np.concatenate([e.field(mode, U0, *params) for e in es], axis=1)
            ref = oracle_np.field_scalar(mode, rho, ux, uy, mask, U0, *params)
            assert np.array_equal(np.isnan(t), np.isnan(ref)) and bits_equal(np.nan_to_num(t), np.nan_to_num(ref)), mode
            img = np.concatenate([e.render_rgba(mode, U0, *params) for e in es], axis=1)
            assert np.array_equal(img, oracle_np.render_rgba8(mode, ref, mask)), mode
    finally:
        for e in es:
            e.close()


# --------------------------------------------------------------------------------------------------------------------------------------------
# batched sweeps (libwtpolar): k_forces_batch and wtp_clamp_events
# --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nx,ny", [("float32", 731, 389), ("float64", 65, 130)])
def test_batched_readouts(pkg, oracle_np, dtype, nx, ny):
    # (mask, tau, u0): a member at the stability clamp, a healthy one, and (fp32) one whose body touches the borders
    members = [(_mask(pkg, nx, ny, "naca4412", 18.0, seed=1), CLAMP_TAU, CLAMP_U0),
               (pkg.geometry.build_geometry(nx, ny, 6.0, None, "naca2412").mask, TAU, U0)]
    if dtype == "float32":
        members.append((_mask(pkg, nx, ny, "clark_y", 10.0, seed=2), 0.62, 0.07))
    B = len(members)
    tau, u0 = [m[1] for m in members], [m[2] for m in members]
    with pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=1) as b:
        b.set_masks(np.stack([m[0] for m in members]))
        b.init_equilibrium(u0)
        done = 0
        while done < 3000:                                                  # until the clamp member sits at both kinds of bound
            b.step(50, tau, u0)
            done += 50
            ev = clamp_events(*b.read_macro(0), members[0][0])
            if ev[0] > 0 and ev[1] > 0:
                break
        b.step(1, tau, u0, sample_every=done + 1)                           # one sample, at the last step
        done += 1
        h = b.history()
        got_f = b.forces()
        got_ev = b.clamp_events()
        macros = [b.read_macro(m) for m in range(B)]
    assert list(h["step"]) == [done]
    for m, ((mask, t, u), macro) in enumerate(zip(members, macros)):
        ref = oracle_np.compute_forces_raw(macro[0], macro[1], mask)
        row = (h["fx"][0, m], h["fy"][0, m], int(h["surf"][0, m]), int(h["rev"][0, m]))
        _forces_close(row, ref)
        assert row == (got_f[0][m], got_f[1][m], int(got_f[2][m]), int(got_f[3][m]))
        ref_ev = oracle_np.clamp_events(*macro, mask)
        assert (int(got_ev[0][m]), int(got_ev[1][m])) == ref_ev, m
        if m == 0:
            assert ref_ev[0] > 0 and ref_ev[1] > 0
        else:
            assert ref_ev == (0, 0)
        with pkg.Engine(nx, ny, dtype=dtype) as e:                          # a single handle at the same state: the same bits
            e.set_mask(mask)
            e.init_equilibrium(u)
            e.step(done, t, u)
            assert all(bits_equal(a, c) for a, c in zip(e.read_macro(), macro)), m
            single = e.forces()
        assert np.float64(row[0]).tobytes() == np.float64(single[0]).tobytes()
        assert np.float64(row[1]).tobytes() == np.float64(single[1]).tobytes() and row[2:] == single[2:], (m, row, single)
    if dtype == "float32":
        assert nx * ny > GRID_SITES                                         # wt_forces' block count is capped at 1024
        assert members[2][0][0].any() and members[2][0][-1].any() and members[2][0][:, 0].any() and members[2][0][:, -1].any()
