"""GPU: state upload and restart of batched sweeps (wtp_write_f, wtp_write_stored, wtp_step_count, wtp_set_step_count, k_half_rows_to_cols,
PolarEngine.state / restore, run_polar(start=, keep_state=)), and with it every batch step kernel from a start state in which no two sites
are alike (tests/_restart_cases.py; tests/test_polar_restart_host.py shows on the references that the cases are sensitive).

Everything is compared as bits; the one bound is that of _mex_reference for the momentum exchange, whose sums the device adds in another
order.
"""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal
import lbm_numpy
import _half_reference as half
import _restart_cases as rc
from _mex_reference import mex_reference

pytestmark = pytest.mark.gpu

WT_ERR_ARG, WT_ERR_STATE = -1, -5
ROWS = ("fx", "fy", "surf", "rev", "mz", "fx_mex", "fy_mex", "mz_mex", "links")


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _engine(pkg, lattice, variant, stored=False, **kw):
    nx, ny, dtype = rc.LATTICES[lattice]
    return pkg.PolarEngine(nx, ny, rc.B, dtype=dtype, storage="half" if stored else "native", **kw)


def _ref_points(nx, ny):
    return [0.3641 * nx + 1.7 * m for m in range(rc.B)], [0.5 * ny - 0.85 * m - 3.3 for m in range(rc.B)]


# ---- 1. round trip -----------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", list(rc.LATTICES))
def test_write_f_then_read_f_returns_the_bits_written(pkg, lattice):
    nx, ny, dtype = rc.LATTICES[lattice]
    masks, _ = rc.setup(lattice, "halfway")
    f = rc.starts(lattice)[1].copy()
    odd = np.array([np.nan, -0.0, np.inf, -np.inf, 5e-324 if dtype == "float64" else 1e-45], dtype=dtype)      # values are not inspected
    f[3, ny - 1, nx - 5:] = odd
    f[8, 0, :5] = -odd
    with _engine(pkg, lattice, "bgk") as b:
        rc.configure(b, "bgk", masks, None)
        before = [b.read_f(m) for m in range(rc.B)]
        b.write_f(1, f)
        assert _same(b.read_f(1), f)
        assert _same(b.read_f(0), before[0]) and _same(b.read_f(2), before[2])       # the other members still read their previous bits
        assert not _same(before[1], f) and b.step_count == 0
        b.write_f(1, before[1])                                            # and a second write replaces the first
        assert _same(b.read_f(1), before[1])


@pytest.mark.parametrize("lattice", rc.HALF_LATTICES)
def test_half_batch_round_trips_raw_halves_and_stores_fp32_values(pkg, lattice):
    nx, ny, _ = rc.LATTICES[lattice]
    masks, _ = rc.setup(lattice, "halfway")
    rng = np.random.default_rng(77)
    raw = rng.integers(0, 65536, size=(9, ny, nx)).astype(np.uint16)       # every kind of pattern: subnormals, both zeros, infinities, NaNs
    raw[0, 0, :4] = (0x8000, 0x0001, 0x7C01, 0xFFFF)
    f = rc.starts(lattice)[2]
    with _engine(pkg, lattice, "bgk", stored=True) as b:
        rc.configure(b, "bgk", masks, None)
        before = [b.read_stored(m) for m in range(rc.B)]
        b.write_stored(0, raw)
        assert _same(b.read_stored(0), raw)
        b.write_f(2, f)
        want = (f - half.W).astype(np.float16)
        assert want.tobytes() == half.store(f).tobytes()
        assert _same(b.read_stored(2), want.view(np.uint16))
        assert _same(b.read_f(2), half.load(want))
        assert _same(b.read_stored(1), before[1]) and not _same(before[0], raw)
        # read_f then write_f keeps the values but not the bits: the -0 written above comes back as +0
        b.write_f(0, np.nan_to_num(b.read_f(0), nan=1.0, posinf=1.0, neginf=1.0))
        assert b.read_stored(0)[0, 0, 0] == 0x0000 and raw[0, 0, 0] == 0x8000


# ---- 2. every step kernel from a rough start ---------------------------------------------------
def _step_calls(b):
    for n in rc.CALLS:
        b.step(n, rc.TAU, rc.U0)
    assert b.step_count == rc.STEPS


def _rows_differ(got, want):
    g, w = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    return int((g != w).reshape(9, got.shape[1], -1).any(axis=(0, 2)).sum())


@pytest.mark.parametrize("lattice,variant", rc.NATIVE_CASES, ids=[f"{lat}-{v}" for lat, v in rc.NATIVE_CASES])
def test_native_step_kernels_from_a_rough_start_are_the_references_bits(pkg, lattice, variant):
    masks, q, start, ref = rc.reference(lattice, variant)
    with _engine(pkg, lattice, variant) as b:
        rc.configure(b, variant, masks, q)
        assert b.les_enabled is ("les" in variant) and b.interpolated_walls is ("ibb" in variant) and b.wind_enabled is ("wind" in variant)
        for m in range(rc.B):
            b.write_f(m, start[m])
        for m in range(rc.B):
            assert _same(b.read_f(m), start[m]), (lattice, variant, m, "start")
        _step_calls(b)
        for m, (want_f, want_macro, _, _) in enumerate(ref):
            got = b.read_f(m)
            assert bits_equal(got, want_f), (lattice, variant, m, _rows_differ(got, want_f), "rows differ")
            for g, w, plane in zip(b.read_macro(m), want_macro, ("rho", "ux", "uy")):
                assert bits_equal(g, w), (lattice, variant, m, plane)
        assert b.clamp_events()[0].tolist() == [0] * rc.B and b.clamp_events()[1].tolist() == [0] * rc.B


@pytest.mark.parametrize("lattice,variant", rc.HALF_CASES, ids=[f"{lat}-{v}" for lat, v in rc.HALF_CASES])
def test_half_step_kernels_from_a_rough_start_are_the_references_bits(pkg, lattice, variant):
    masks, _, start, ref = rc.reference(lattice, variant, True)
    rough = rc.starts(lattice)
    with _engine(pkg, lattice, variant, stored=True) as b:
        rc.configure(b, variant, masks, None)
        for m in range(rc.B):
            b.write_f(m, rough[m])                                          # through Store, on the device
        for m in range(rc.B):
            assert _same(b.read_stored(m), start[m].view(np.uint16)), (lattice, variant, m, "start")
        _step_calls(b)
        for m, (want_h, want_macro, _, _) in enumerate(ref):
            got = b.read_stored(m)
            assert _same(got, want_h.view(np.uint16)), (lattice, variant, m, _rows_differ(got, want_h), "rows differ")
            for g, w, plane in zip(b.read_macro(m), want_macro, ("rho", "ux", "uy")):
                assert bits_equal(g, w), (lattice, variant, m, plane)


# ---- 3. the state rules ------------------------------------------------------------------------
def test_a_write_invalidates_the_macroscopic_planes_and_empties_the_members_sums_only(pkg):
    lattice = "96x48-f32"
    nx, ny, dtype = rc.LATTICES[lattice]
    masks, _ = rc.setup(lattice, "halfway")
    rough = rc.starts(lattice)
    xr, yr = _ref_points(nx, ny)
    with _engine(pkg, lattice, "bgk", history_cap=8) as b:
        rc.configure(b, "bgk", masks, None)
        b.enable_loads(xr, yr)
        b.enable_momentum_exchange(xr, yr)
        b.enable_mean_fields()
        b.step(12, rc.TAU, rc.U0, sample_every=6)
        hist, surf0, mean0, f0 = b.history(), b.surface(0), b.mean_sums(0), b.read_f(0)
        assert list(hist["step"]) == [6, 12] and mean0["n"] == 2 and int(surf0["n_upper"].max()) == 2
        assert b.surface(1)["n_upper"].max() == 2 and b.mean_sums(1)["n"] == 2
        b.write_f(1, rough[1])
        for call in (lambda: b.read_macro(0), lambda: b.read_macro(1), b.forces, b.moment):      # one flag per batch
            with pytest.raises(pkg.WTError) as ei:
                call()
            assert ei.value.code == WT_ERR_STATE
        fx, fy, mz, links = b.momentum_exchange()                           # reads populations: still defined
        for m, f in ((0, f0), (1, rough[1])):
            want = mex_reference(f, masks[m], xr[m], yr[m])
            assert want.links == int(links[m]) > 20
            for got, ref, bound in ((fx[m], want.fx, want.fx_bound), (fy[m], want.fy, want.fy_bound), (mz[m], want.mz, want.mz_bound)):
                assert abs(got - ref) <= bound, (m, got, ref, bound)
        after = b.history()                                                 # the rows held before the write are the same bytes
        assert list(after) == list(hist) and all(_same(after[k], hist[k]) for k in hist)
        s1, m1 = b.surface(1), b.mean_sums(1)
        assert not s1["n_upper"].any() and not s1["n_lower"].any() and not s1["rho_upper"].any() and not s1["rho_lower"].any()
        assert m1["n"] == 0 and not any(m1[k].any() for k in pkg.polar.MEAN_SUMS)
        s0, m0 = b.surface(0), b.mean_sums(0)                               # another member's are untouched
        assert all(_same(s0[k], surf0[k]) for k in surf0) and m0["n"] == 2 and all(_same(m0[k], mean0[k]) for k in pkg.polar.MEAN_SUMS)
        assert b.step_count == 12 and _same(b.read_f(0), f0) and _same(b.read_f(1), rough[1])
        b.step(1, rc.TAU, rc.U0)                                            # after one step all of them work
        want_f, want_macro = lbm_numpy.step(rough[1], masks[1], rc.TAU[1], rc.U0[1])
        assert bits_equal(b.read_f(1), want_f)
        assert all(bits_equal(g, w) for g, w in zip(b.read_macro(1), want_macro))
        assert all(np.isfinite(v).all() for v in b.forces()[:2]) and np.isfinite(b.moment()).all()
        assert list(b.history()["step"]) == [6, 12]


# ---- 4. restart is invisible -------------------------------------------------------------------
@pytest.mark.parametrize("stored", [False, True], ids=["native-les-wind", "half"])
def test_a_restart_from_a_state_is_invisible(pkg, stored):
    lattice, variant = "96x48-f32", "wind+les"
    nx, ny, _ = rc.LATTICES[lattice]
    masks, _ = rc.setup(lattice, "halfway")
    rough = rc.starts(lattice)
    xr, yr = _ref_points(nx, ny)

    def engine():
        b = _engine(pkg, lattice, variant, stored=stored, history_cap=8)
        rc.configure(b, variant, masks, None)
        b.enable_loads(xr, yr)
        b.enable_momentum_exchange(xr, yr)
        return b

    def read(b):
        pops = [b.read_stored(m) if stored else b.read_f(m) for m in range(rc.B)]
        return pops, [b.read_macro(m) for m in range(rc.B)], b.history()

    with engine() as a:
        for m in range(rc.B):
            a.write_f(m, rough[m])
        a.step(36, rc.TAU, rc.U0, sample_every=6)
        pops_a, macro_a, hist_a = read(a)
    with engine() as b:
        for m in range(rc.B):
            b.write_f(m, rough[m])
        b.step(18, rc.TAU, rc.U0, sample_every=6)
        state = b.state()
    assert state["steps"] == 18 and state["f"].shape == (rc.B, 9, ny, nx) and state["f"].dtype == (np.uint16 if stored else np.float32)
    assert (state["nx"], state["ny"], state["dtype"], state["storage"], state["members"]) == (nx, ny, "float32", "half" if stored else "native", rc.B)
    with engine() as c:
        c.restore(state)
        assert c.step_count == 18 and len(c.history()["step"]) == 0
        c.step(18, rc.TAU, rc.U0, sample_every=6)
        assert c.step_count == 36
        pops_c, macro_c, hist_c = read(c)
        with pytest.raises(ValueError):
            c.restore({**state, "members": rc.B + 1})
    for m in range(rc.B):
        assert _same(pops_c[m], pops_a[m]), m
        assert all(_same(g, w) for g, w in zip(macro_c[m], macro_a[m])), m
    assert list(hist_a["step"]) == [6, 12, 18, 24, 30, 36] and list(hist_c["step"]) == [24, 30, 36]
    for k in ROWS:
        assert _same(hist_c[k], hist_a[k][3:]), k
        assert np.isfinite(hist_c[k].astype(np.float64)).all(), k          # (sampled rows, not the "never sampled" fill)
    assert (hist_c["links"] > 20).all() and (hist_c["surf"] > 0).all()


# ---- 5. step-count rules -----------------------------------------------------------------------
def test_step_count_rules(pkg):
    lattice = "96x48-f32"
    masks, _ = rc.setup(lattice, "halfway")
    with _engine(pkg, lattice, "bgk", history_cap=4) as b:
        rc.configure(b, "bgk", masks, None)
        assert b.step_count == 0
        b.step(12, rc.TAU, rc.U0, sample_every=6)
        hist, f, macro = b.history(), b.read_f(2), b.read_macro(2)
        for bad, code in ((-1, WT_ERR_ARG), (11, WT_ERR_STATE), (0, WT_ERR_STATE)):
            with pytest.raises(pkg.WTError) as ei:
                b.set_step_count(bad)
            assert ei.value.code == code
            after = b.history()                                             # a refused call changes nothing
            assert b.step_count == 12 and all(_same(after[k], hist[k]) for k in hist) and _same(b.read_f(2), f)
        assert b._lib.wtp_step_count(b._b, None) == WT_ERR_ARG
        b.set_step_count(12)
        b.set_step_count(20)
        assert b.step_count == 20 and _same(b.read_f(2), f) and all(_same(g, w) for g, w in zip(b.read_macro(2), macro))      # nothing else changed
        b.step(4, rc.TAU, rc.U0, sample_every=6)                            # the cadence follows the count: 24 samples
        assert b.step_count == 24 and list(b.history()["step"]) == [6, 12, 24]
        b.clear_history()
        b.set_step_count(0)                                                 # no row held: any count >= 0
        assert b.step_count == 0


# ---- 6. argument errors leave the batch usable -------------------------------------------------
def test_refused_writes_leave_the_batch_usable(pkg, oracle_np):
    nx, ny = 96, 48
    mask = pkg.geometry.build_geometry(nx, ny, 6.0, None, "naca2412").mask
    tau, u0 = 0.58, 0.06
    f = rc.starts("96x48-f32")[0]
    vp = ctypes.c_void_p
    with pkg.PolarEngine(nx, ny, 2) as b:
        b.set_masks(np.stack([mask, mask]))
        with pytest.raises(pkg.WTError) as ei:                              # before init_equilibrium: pad columns hold nothing defined
            b.write_f(0, f)
        assert ei.value.code == WT_ERR_STATE and "wtp_init_equilibrium" in str(ei.value)
        b.init_equilibrium(u0)
        for member in (-1, 2):
            with pytest.raises(pkg.WTError) as ei:
                b.write_f(member, f)
            assert ei.value.code == WT_ERR_ARG
        with pytest.raises(pkg.WTError) as ei:
            b.write_stored(0, np.zeros((9, ny, nx), np.uint16))
        assert ei.value.code == WT_ERR_STATE and "natively" in str(ei.value)
        assert b._lib.wtp_write_f(b._b, 0, None) == WT_ERR_ARG and b._lib.wtp_write_stored(b._b, 0, None) == WT_ERR_ARG
        for bad in (f[:, :-1], f.astype(np.float64), f[:8]):
            with pytest.raises(ValueError):
                b.write_f(0, bad)
        with pytest.raises(ValueError):
            b.write_stored(0, np.zeros((9, ny, nx), np.int16))
        assert all(np.isfinite(a).all() for a in b.read_macro(0))           # nothing was written: the planes are still the start's
        b.step(10, tau, u0)
        want_f, want_macro = oracle_np.run(mask, 10, tau, u0, np.float32)
        for m in range(2):
            assert bits_equal(b.read_f(m), want_f), m
            assert all(bits_equal(g, w) for g, w in zip(b.read_macro(m), want_macro)), m
    with pkg.PolarEngine(nx, ny, 2, storage="half") as b:
        b.set_masks(np.stack([mask, mask]))
        with pytest.raises(pkg.WTError) as ei:
            b.write_stored(1, np.zeros((9, ny, nx), np.uint16))
        assert ei.value.code == WT_ERR_STATE and "wtp_init_equilibrium" in str(ei.value)
        with pytest.raises(ValueError):
            b.write_f(0, f.astype(np.float16))


# ---- 7. run_polar continuation -----------------------------------------------------------------
def test_run_polar_continues_from_a_kept_state(pkg):
    alphas = [2.0, 6.0]
    kw = dict(nx=96, ny=48, total_forces=True)
    first = pkg.run_polar(alphas, warmup_steps=60, samples=4, keep_state=True, **kw)
    second = pkg.run_polar(alphas, start=first.state, samples=4, **kw)
    whole = pkg.run_polar(alphas, warmup_steps=60, samples=8, **kw)
    assert whole.state is None and second.state is None and first.state["steps"] == 60 + 4 * 12
    assert second.warmup_steps == 0 and first.warmup_steps == whole.warmup_steps == 60
    for m in range(len(alphas)):
        h, h1, h2 = whole.points[m].history, first.points[m].history, second.points[m].history
        assert list(h) == list(h1) == list(h2) and {"step", "fx", "fy", "surf", "rev", "mz", "fx_mex", "links"} <= set(h)
        assert list(h["step"]) == [60 + 12 * (r + 1) for r in range(8)]
        for k in h:
            assert _same(h[k][:4], h1[k]) and _same(h[k][4:], h2[k]), (m, k)
        assert whole.points[m].samples == 8 and second.points[m].samples == 4
    with pytest.raises(ValueError, match="nx"):
        pkg.run_polar(alphas, nx=128, ny=48, start=first.state, samples=4)
