"""GPU: half-precision population storage of batched sweeps (k_step_half_batch, k_fill_half, k_mex_half_batch, wtp_create_stored)
against its definition in NumPy (tests/_half_reference.py).

There is no tolerance on the state: the kernel and the reference load, compute and store by the same operations, rounded once each,
so the stored halves and the macroscopic planes are the same bits, with either collision and either far field.  The read-outs on
top of a half state are held to their own features' references and bounds.  Every batch has three members that mix tau 0.52 to 0.9
and U0 0.01 to 0.08; the member with U0 = 0.01 fills the k = 2 and k = 4 planes with subnormal halves.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import bits_equal
import lbm_numpy
import _half_reference as half
import _les_reference as les
import _wind_reference as wind
from _loads_reference import loads_reference, surface_sums
from _mean_reference import SUMS, accumulate
from _mex_reference import mex_reference
from test_gpu_polar_mean import _block_masks

pytestmark = pytest.mark.gpu

WT_ERR_ARG, WT_ERR_STATE = -1, -5
WT_F32, WT_F64 = 0, 1
STEPS = 60
EVERY = 12

# Members: (shape, aoa, tau, u0, v0 / u0, cs); v0 and cs are used by the variants only.  The lattices: 96x48 has NY below one wave;
# 40x300 and 37x299 more than one 256-row block (one member's body lies across row 256), a ragged end, odd NX and NY; 24x256 has NY equal to the pitch, so no pad row
# hides an overrun.
CASES = {
    "96x48": (96, 48, [("naca0012", 0.0, 0.52, 0.08, 0.6, 0.17), ("naca2412", 6.0, 0.9, 0.01, -0.25, 0.1), ("naca4412", -4.0, 0.6, 0.06, 0.0, 0.0)]),
    "40x300": (40, 300, [("block", 0.0, 0.52, 0.08, 0.6, 0.17), ("block", 0.0, 0.7, 0.01, 0.0, 0.0), ("block", 0.0, 0.9, 0.03, -0.25, 0.1)]),
    "37x299": (37, 299, [("block", 0.0, 0.9, 0.01, -0.25, 0.17), ("block", 0.0, 0.6, 0.06, 0.6, 0.1), ("block", 0.0, 0.52, 0.08, 0.0, 0.0)]),
    "24x256": (24, 256, [("block", 0.0, 0.52, 0.07, 0.6, 0.1), ("block", 0.0, 0.9, 0.01, -0.25, 0.0), ("block", 0.0, 0.6, 0.05, 0.0, 0.17)]),
}
VARIANT_CASES = ("96x48", "37x299")
VARIANTS = ("les", "wind", "les+wind")


def _masks(nx, ny, members):
    import airfoil_cfd_tool_amd as pkg
    if members[0][0] == "block":
        masks = _block_masks(nx, ny, len(members))
        if ny > 280:                                                        # the last member's block lies across row 256, the end of the first run
            masks[-1] = 0
            masks[-1, 241:272, nx // 3 + 2:nx // 3 + 9] = 1
        return masks
    return np.stack([pkg.geometry.build_geometry(nx, ny, a, None, s).mask for s, a, *_ in members])


def _params(members):
    tau, u0 = [m[2] for m in members], [m[3] for m in members]
    return tau, u0, [m[3] * m[4] for m in members], [m[5] for m in members]


def _model(variant, v0, cs):
    """(base step, its extra arguments, the v0 of the start state) of one member."""
    c = les.les_constant(cs, np.float32)
    if variant == "plain":
        return lbm_numpy.step, (), 0.0
    if variant == "les":
        return les.step, (c,), 0.0
    if variant == "wind":
        return half.windy(lbm_numpy.step), (v0,), v0
    return half.windy(les.step), (v0, c), v0


def _frozen(out):
    for a in (out[0], *out[1]):
        a.setflags(write=False)
    return out[0], out[1]


def _subnormals(h):
    a = np.abs(h.astype(np.float32))
    return int(((a > 0) & (a < 2.0 ** -14)).sum())


def _interior_fluid(mask):
    ny, nx = mask.shape
    inner = np.zeros((ny, nx), bool)
    inner[1:ny - 1, 1:nx - 1] = True
    return inner & (mask == 0)


@functools.lru_cache(maxsize=None)
def _reference(name, variant="plain"):
    """(masks, per member ((h, macro) after STEPS steps, (h, macro) after STEPS + 1, the fp32-storage populations after STEPS))."""
    nx, ny, members = CASES[name]
    masks = _masks(nx, ny, members)
    tau, u0, v0, cs = _params(members)
    out = []
    for m in range(len(members)):
        base, extra, start_v0 = _model(variant, v0[m], cs[m])
        a = half.run(masks[m], STEPS, tau[m], u0[m], *extra, base_step=base, v0=start_v0)
        b = half.half_step(base, a[0], masks[m], tau[m], u0[m], *extra)
        f, _ = wind.wind_init(nx, ny, u0[m], start_v0, np.float32)
        for _ in range(STEPS):
            f = base(f, masks[m], tau[m], u0[m], *extra)[0]
        f.setflags(write=False)
        out.append((_frozen(a), _frozen(b), f))
    return masks, out


def _assert_reference_is_not_vacuous(name, variant):
    """On the reference alone: it holds subnormal stored values, and it differs from fp32 storage in every interior fluid cell."""
    masks, ref = _reference(name, variant)
    for m, ((h, _), _, f32) in enumerate(ref):
        n = _subnormals(h)
        differ = (half.load(h) != f32).any(axis=0)[_interior_fluid(masks[m])]
        print(f"{name} {variant} member {m}: {n} subnormal halves, max |h| {float(np.abs(h.astype(np.float32)).max()):.4g}, "
              f"{float(differ.mean()):.3f} of the interior fluid cells differ from fp32 storage")
        assert n > 0 and differ.all(), (name, variant, m, n)
        assert np.isfinite(h).all()
    u0 = _params(CASES[name][2])[1]
    slow = u0.index(0.01)
    h = ref[slow][0][0]
    if variant in ("plain", "les"):       # without a cross-flow more than a quarter of its k = 2 and k = 4 planes is subnormal (0.29 to 0.72)
        for k in (2, 4):
            a = np.abs(h[k].astype(np.float32))
            assert ((a > 0) & (a < 2.0 ** -14)).mean() > 0.25, (name, k)


def _assert_state(b, ref, which, what):
    for m, pair in enumerate(ref):
        want_h, want_macro = pair[which]
        got = b.read_stored(m)
        assert got.dtype == np.uint16 and got.shape == want_h.shape
        bad = int((got != want_h.view(np.uint16)).any(axis=(0, 2)).sum())
        assert np.array_equal(got, want_h.view(np.uint16)), (what, m, bad, "rows differ")
        for g, w, plane in zip(b.read_macro(m), want_macro, ("rho", "ux", "uy")):
            assert bits_equal(g, w), (what, m, plane)
        f = b.read_f(m)
        assert f.dtype == np.float32 and bits_equal(f, half.load(want_h)), (what, m, "read_f")


def _run_and_check(pkg, name, variant):
    nx, ny, members = CASES[name]
    tau, u0, v0, cs = _params(members)
    masks, ref = _reference(name, variant)
    with pkg.PolarEngine(nx, ny, len(members), storage="half") as b:
        assert b.storage == "half" and b.dtype == np.float32
        b.set_masks(masks)
        if "wind" in variant:
            b.enable_wind(v0)
        if "les" in variant:
            b.enable_les(cs)
        b.init_equilibrium(u0)
        for m in range(len(members)):                                       # the start state: Store of the fp32 start values
            h0, macro0 = half.half_init(nx, ny, u0[m], v0[m] if "wind" in variant else 0.0)
            assert np.array_equal(b.read_stored(m), h0.view(np.uint16)), (name, variant, m, "start")
            assert all(bits_equal(g, w) for g, w in zip(b.read_macro(m), macro0)), (name, variant, m, "start")
        b.step(STEPS, tau, u0)
        _assert_state(b, ref, 0, (name, variant, STEPS))
        b.step(1, tau, u0)
        _assert_state(b, ref, 1, (name, variant, STEPS + 1))


# ---- 1. bit identity ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_stored_halves_and_macroscopic_planes_are_the_references_bits(pkg, name):
    members = CASES[name][2]
    assert min(m[2] for m in members) <= 0.55 and max(m[2] for m in members) == 0.9 and sorted(m[3] for m in members)[0] == 0.01
    _assert_reference_is_not_vacuous(name, "plain")
    _run_and_check(pkg, name, "plain")


# ---- 2. with the other collision and the other far field ---------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", VARIANT_CASES)
def test_stored_halves_are_the_references_bits_with_les_and_inclined_stream(pkg, name, variant):
    members = CASES[name][2]
    assert sorted(m[5] for m in members) == [0.0, 0.1, 0.17] and sorted(m[4] for m in members) == [-0.25, 0.0, 0.6]
    _assert_reference_is_not_vacuous(name, variant)
    _, ref = _reference(name, variant)
    _, plain = _reference(name, "plain")
    for m, (s, a, tau, u0, vr, cs) in enumerate(members):                   # the model under the wrapper acts
        acts = ("les" in variant and cs > 0) or ("wind" in variant and vr != 0)
        assert (ref[m][0][0].tobytes() != plain[m][0][0].tobytes()) == acts, (name, variant, m)
    _run_and_check(pkg, name, variant)


# ---- 3. the read-outs stand on the half state --------------------------------------------------
def test_readouts_of_a_sampled_half_run(pkg):
    """Forces, moment, surface sums and mean sums against the existing references applied to the batch's own read_macro, the
    momentum exchange (history rows and wtp_mex) against _mex_reference on the batch's own read_f, all within those references' own
    bounds (Loads.fx_bound / fy_bound / mz_bound, Mex.fx_bound / fy_bound / mz_bound; the sums bit for bit)."""
    name, calls = "96x48", 6
    nx, ny, members = CASES[name]
    tau, u0, _, _ = _params(members)
    masks = _masks(nx, ny, members)
    B = len(members)
    xr, yr = [0.3641 * nx + 1.7 * m for m in range(B)], [0.5 * ny - 0.85 * m - 3.3 for m in range(B)]
    macros, fs, forces, moments, mex = [[] for _ in range(B)], [[] for _ in range(B)], [], [], []
    with pkg.PolarEngine(nx, ny, B, history_cap=calls, storage="half") as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        b.enable_loads(xr, yr)
        b.enable_momentum_exchange(xr, yr)
        b.enable_mean_fields()
        for _ in range(calls):
            b.step(EVERY, tau, u0, sample_every=EVERY)
            forces.append(b.forces())
            moments.append(b.moment())
            mex.append(b.momentum_exchange())
            for m in range(B):
                macros[m].append(b.read_macro(m))
                fs[m].append(b.read_f(m))
        stored = [b.read_stored(m) for m in range(B)]
        h = b.history()
        surface = [b.surface(m) for m in range(B)]
        sums = [b.mean_sums(m) for m in range(B)]
    assert list(h["step"]) == [EVERY * (k + 1) for k in range(calls)]
    # the state under the read-outs is the half model's, and not the fp32 oracle's
    ref = half.run(masks[0], EVERY, tau[0], u0[0])
    assert bits_equal(fs[0][0], half.load(ref[0])) and all(bits_equal(g, w) for g, w in zip(macros[0][0], ref[1]))
    assert not bits_equal(fs[0][0], lbm_numpy.run(masks[0], EVERY, tau[0], u0[0], np.float32)[0])
    for m in range(B):
        assert bits_equal(fs[m][-1], half.load(stored[m]))
    worst = [0.0] * 7
    for m in range(B):
        for r in range(calls):
            rho, ux, _ = macros[m][r]
            lo = loads_reference(rho, masks[m], xr[m], yr[m])
            assert lo.n == int(h["surf"][r, m]) == int(forces[r][2][m]) > 0
            assert int(h["rev"][r, m]) == int(forces[r][3][m]) == lbm_numpy.compute_forces_raw(rho, ux, masks[m])[3]
            mx = mex_reference(fs[m][r], masks[m], xr[m], yr[m])
            assert mx.links == int(h["links"][r, m]) == int(mex[r][3][m]) > 100
            rows = ((h["fx"][r, m], forces[r][0][m], lo.fx, lo.fx_bound), (h["fy"][r, m], forces[r][1][m], lo.fy, lo.fy_bound),
                    (h["mz"][r, m], moments[r][m], lo.mz, lo.mz_bound), (h["fx_mex"][r, m], mex[r][0][m], mx.fx, mx.fx_bound),
                    (h["fy_mex"][r, m], mex[r][1][m], mx.fy, mx.fy_bound), (h["mz_mex"][r, m], mex[r][2][m], mx.mz, mx.mz_bound))
            for q, (row, on_demand, want, bound) in enumerate(rows):
                assert row.tobytes() == on_demand.tobytes(), (m, r, q)      # a history row is the on-demand call on that state
                err = abs(row - want)
                worst[q] = max(worst[q], err / bound)
                assert err <= bound, (m, r, q, row, want, bound)
        su, sl, nu, nl = surface_sums([mac[0] for mac in macros[m]], masks[m])
        assert np.array_equal(surface[m]["n_upper"], nu) and np.array_equal(surface[m]["n_lower"], nl) and int((nu > 0).sum()) > 30
        assert bits_equal(surface[m]["rho_upper"], su) and bits_equal(surface[m]["rho_lower"], sl)
        want = accumulate(macros[m])
        assert sums[m]["n"] == want["n"] == calls
        for k in SUMS:
            assert bits_equal(sums[m][k], want[k]), (m, k)
    print("worst |x - ref| / bound: fx %.3g, fy %.3g, Mz %.3g, mex fx %.3g, fy %.3g, mz %.3g; surface and mean sums bit-identical" % tuple(worst[:6]))


# ---- 4. WTP_STORE_NATIVE is wtp_create ---------------------------------------------------------
def test_create_stored_native_is_create(pkg):
    name = "40x300"
    nx, ny, members = CASES[name]
    tau, u0, _, _ = _params(members)
    masks = _masks(nx, ny, members)
    B = len(members)
    state = []
    for stored in (False, True):
        with pkg.PolarEngine(nx, ny, B) as b:
            if stored:                                                      # the same engine around a batch of wtp_create_stored
                assert b._lib.wtp_destroy(b._b) == 0
                b._b = ctypes.c_void_p()
                assert b._lib.wtp_create_stored(nx, ny, WT_F32, pkg.polar.WTP_STORE_NATIVE, B, 0, 0, ctypes.byref(b._b)) == 0
            b.set_masks(masks)
            b.init_equilibrium(u0)
            b.step(STEPS, tau, u0)
            state.append([(b.read_f(m), b.read_macro(m)) for m in range(B)])
            with pytest.raises(pkg.WTError) as ei:
                b.read_stored(0)
            assert ei.value.code == WT_ERR_STATE
    for m in range(B):
        assert state[0][m][0].tobytes() == state[1][m][0].tobytes(), m
        assert all(a.tobytes() == c.tobytes() for a, c in zip(state[0][m][1], state[1][m][1])), m
        assert bits_equal(state[1][m][0], lbm_numpy.run(masks[m], STEPS, tau[m], u0[m], np.float32)[0]), m


# ---- 5. error paths ----------------------------------------------------------------------------
def test_error_paths_leave_the_batch_working(pkg):
    name = "96x48"
    nx, ny, members = CASES[name]
    tau, u0, _, _ = _params(members)
    masks, ref = _reference(name)
    B = len(members)
    lib = pkg.polar.load_polar_library()
    h = ctypes.c_void_p()
    assert lib.wtp_create_stored(nx, ny, WT_F64, pkg.polar.WTP_STORE_HALF, B, 0, 0, ctypes.byref(h)) == WT_ERR_ARG and not h
    assert b"WT_F32" in lib.wtp_last_error()
    for bad in (2, -1, 100):
        assert lib.wtp_create_stored(nx, ny, WT_F32, bad, B, 0, 0, ctypes.byref(h)) == WT_ERR_ARG and not h
        assert b"storage" in lib.wtp_last_error()
    with pkg.PolarEngine(nx, ny, B) as native:
        native.set_masks(masks)
        native.init_equilibrium(u0)
        with pytest.raises(pkg.WTError) as ei:
            native.read_stored(0)
        assert ei.value.code == WT_ERR_STATE
        buf = np.zeros((9, ny, nx), np.uint16)
        assert lib.wtp_read_stored(native._b, 0, buf.ctypes.data_as(ctypes.c_void_p)) == WT_ERR_STATE and not buf.any()
    with pkg.PolarEngine(nx, ny, B, storage="half") as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        b.step(24, tau, u0)
        for on in (True, False):
            with pytest.raises(pkg.WTError) as ei:
                b.enable_interpolated_walls(on)
            assert ei.value.code == WT_ERR_STATE and "half" in str(ei.value)
        with pytest.raises(pkg.WTError) as ei:
            b.set_wall_distances(np.full((B, 8, ny, nx), 0.5, np.float32))
        assert ei.value.code == WT_ERR_STATE
        with pytest.raises(pkg.WTError) as ei:
            b.read_stored(B)
        assert ei.value.code == WT_ERR_ARG
        b.step(STEPS - 24, tau, u0)                                         # ... and steps on correctly
        _assert_state(b, ref, 0, "after the refused calls")


# ---- 6. run_polar ------------------------------------------------------------------------------
def test_run_polar_with_half_storage_stays_within_the_measured_bound_of_the_native_sweep(pkg):
    """96x48 NACA 2412 at 4 and 6 degrees, tau 0.58, U0 0.06, warm-up 200 steps, 8 samples every 12 steps.  The same configuration
    measured on the CPU with the reference wrapper against the oracle (mean over the 8 samples): at 4 degrees CL 0.402642 against
    0.402295 (3.47e-4) and CD 0.244410 against 0.244544 (1.34e-4); at 6 degrees CL 0.542411 against 0.542818 (4.07e-4) and CD 0.266608
    against 0.266668 (6.0e-5).  The bounds are four times the larger of the two: |dCL| <= 1.63e-3, |dCD| <= 5.4e-4."""
    alphas = [4.0, 6.0]
    kw = dict(shape="naca2412", nx=96, ny=48, warmup_steps=200, samples=8)
    hres = pkg.run_polar(alphas, storage="half", **kw)
    nres = pkg.run_polar(alphas, **kw)
    assert hres.storage == "half" and nres.storage == "native" and hres.tau == nres.tau == 0.58 and hres.u0 == nres.u0 == 0.06
    for p, q in zip(hres.points, nres.points):
        assert p.converged and q.converged and p.samples == q.samples == 8, (p, q)
        print(f"alpha {p.alpha}: CL half {p.cl_mean:.6f} native {q.cl_mean:.6f} (d {abs(p.cl_mean - q.cl_mean):.3g}), "
              f"CD half {p.cd_mean:.6f} native {q.cd_mean:.6f} (d {abs(p.cd_mean - q.cd_mean):.3g})")
        assert p.cl_mean != q.cl_mean
        assert abs(p.cl_mean - q.cl_mean) <= 4 * 4.07e-4
        assert abs(p.cd_mean - q.cd_mean) <= 4 * 1.34e-4
        assert p.cm_mean is not None and np.isfinite(p.cm_mean)
