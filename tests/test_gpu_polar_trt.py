"""GPU: the two-relaxation-time collision of batched sweeps (k_step_batch and k_step_half_batch with COLLIDE_TRT / COLLIDE_TRT_LES, wtp_enable_trt) against its
definition in NumPy (tests/_trt_reference.py), on the cases of tests/_trt_cases.py (tests/test_polar_trt_host.py shows on the references
that they are sensitive).

There is no tolerance on the state: the kernels and the reference round every operation of the collision once, in the same order, so
populations and macroscopic fields are compared as bits.  The read-outs on a TRT state are held to their own features' checks: bits for a
history row against the on-demand calls, the derived summation bound of _mex_reference for the momentum exchange.  The channel test
asserts the two facts the collision is for, with the bounds of the host test.
"""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal
import lbm_numpy
import _half_reference as half
import _les_reference as les
import _restart_cases as rc
import _trt_cases as tc
import _trt_reference as trt
from _mex_reference import mex_reference

pytestmark = pytest.mark.gpu

WT_ERR_ARG, WT_ERR_STATE = -1, -5
EVERY = 6


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rows_differ(got, want):
    g, w = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    return int((g != w).reshape(9, got.shape[1], -1).any(axis=(0, 2)).sum())


def _engine(pkg, lattice, stored=False, **kw):
    nx, ny, dtype = rc.LATTICES[lattice]
    return pkg.PolarEngine(nx, ny, rc.B, dtype=dtype, storage="half" if stored else "native", **kw)


def _step_calls(b):
    for n in rc.CALLS:
        b.step(n, rc.TAU, rc.U0)
    assert b.step_count == rc.STEPS


# ---- 1. from equilibrium -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.EQ_CASES))
def test_state_from_equilibrium_is_the_references_bits(pkg, name):
    nx, ny, dtype, members = tc.EQ_CASES[name]
    tau, u0, magic = ([m[k] for m in members] for k in (2, 3, 4))
    masks, ref = tc.eq_reference(name)
    with pkg.PolarEngine(nx, ny, len(members), dtype=dtype) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        assert not b.trt_enabled
        b.enable_trt(magic)
        assert b.trt_enabled and not b.les_enabled and not b.wind_enabled
        b.step(tc.EQ_STEPS, tau, u0)
        for m, (want_f, want_macro, bgk) in enumerate(ref):
            f = b.read_f(m)
            assert bits_equal(f, want_f), (name, m, _rows_differ(f, want_f), "rows differ")
            assert not bits_equal(f, bgk), (name, m)
            for got, want, what in zip(b.read_macro(m), want_macro, ("rho", "ux", "uy")):
                assert bits_equal(got, want), (name, m, what)
        assert b.clamp_events()[0].tolist() == [0] * len(members)


# ---- 2. every kernel from the rough start ------------------------------------------------------
@pytest.mark.parametrize("lattice,variant", tc.NATIVE_CASES, ids=[f"{lat}-{v}" for lat, v in tc.NATIVE_CASES])
def test_native_kernels_from_a_rough_start_are_the_references_bits(pkg, lattice, variant):
    masks, q, start, ref = tc.reference(lattice, variant)
    with _engine(pkg, lattice) as b:
        tc.configure(b, variant, masks, q)
        assert b.trt_enabled
        assert b.les_enabled is ("les" in variant) and b.interpolated_walls is ("ibb" in variant) and b.wind_enabled is ("wind" in variant)
        for m in range(rc.B):
            b.write_f(m, start[m])
        _step_calls(b)
        for m, (want_f, want_macro, _) in enumerate(ref):
            got = b.read_f(m)
            assert bits_equal(got, want_f), (lattice, variant, m, _rows_differ(got, want_f), "rows differ")
            for g, w, plane in zip(b.read_macro(m), want_macro, ("rho", "ux", "uy")):
                assert bits_equal(g, w), (lattice, variant, m, plane)
        assert b.clamp_events()[0].tolist() == [0] * rc.B and b.clamp_events()[1].tolist() == [0] * rc.B


@pytest.mark.parametrize("lattice,variant", tc.HALF_CASES, ids=[f"{lat}-{v}" for lat, v in tc.HALF_CASES])
def test_half_kernels_from_a_rough_start_are_the_references_bits(pkg, lattice, variant):
    masks, _, start, ref = tc.reference(lattice, variant, True)
    rough = rc.starts(lattice)
    with _engine(pkg, lattice, stored=True) as b:
        tc.configure(b, variant, masks, None)
        for m in range(rc.B):
            b.write_f(m, rough[m])                                          # through Store, on the device
        for m in range(rc.B):
            assert _same(b.read_stored(m), start[m].view(np.uint16)), (lattice, variant, m, "start")
        _step_calls(b)
        for m, (want_h, want_macro, _) in enumerate(ref):
            got = b.read_stored(m)
            assert _same(got, want_h.view(np.uint16)), (lattice, variant, m, _rows_differ(got, want_h), "rows differ")
            assert _same(b.read_f(m), half.load(want_h)), (lattice, variant, m)
            for g, w, plane in zip(b.read_macro(m), want_macro, ("rho", "ux", "uy")):
                assert bits_equal(g, w), (lattice, variant, m, plane)


# ---- 3. the Smagorinsky model at cs = 0 ----------------------------------------------------------
@pytest.mark.parametrize("lattice", ["37x299-f32", "24x140-f64"])
def test_les_with_cs_zero_has_the_bits_of_trt_alone(pkg, lattice):
    masks, _, start, ref = tc.reference(lattice, "trt")
    state = {}
    for on in (False, True):
        with _engine(pkg, lattice) as b:
            tc.configure(b, "trt", masks, None)
            if on:
                b.enable_les(0.0)
            assert b.les_enabled is on and b.trt_enabled
            for m in range(rc.B):
                b.write_f(m, start[m])
            _step_calls(b)
            state[on] = [(b.read_f(m), b.read_macro(m)) for m in range(rc.B)]
    for m in range(rc.B):
        assert _same(state[True][m][0], state[False][m][0]), m
        assert all(_same(g, w) for g, w in zip(state[True][m][1], state[False][m][1])), m
        assert bits_equal(state[True][m][0], ref[m][0]), m                   # (and both are the reference's)


# ---- 4. on and off in mid-run ------------------------------------------------------------------
def test_switching_on_and_off_in_mid_run_composes_the_references(pkg):
    lattice = "96x48-f32"
    nx, ny, dtype = rc.LATTICES[lattice]
    masks, _ = rc.setup(lattice, "halfway")
    start = rc.starts(lattice)
    with _engine(pkg, lattice, history_cap=8) as b:
        rc.configure(b, "bgk", masks, None)
        for m in range(rc.B):
            b.write_f(m, start[m])
        b.step(2 * EVERY, rc.TAU, rc.U0, sample_every=EVERY)                 # BGK
        b.enable_trt(tc.MAGIC)
        assert b.trt_enabled and b.step_count == 2 * EVERY and list(b.history()["step"]) == [EVERY, 2 * EVERY]
        b.step(2 * EVERY, rc.TAU, rc.U0, sample_every=EVERY)                 # TRT
        first = b.history()
        at_switch = [b.read_f(m) for m in range(rc.B)]
        for m in range(rc.B):
            f, _ = lbm_numpy.run(masks[m], 2 * EVERY, rc.TAU[m], rc.U0[m], np.dtype(dtype), f=start[m])
            only_bgk, _ = lbm_numpy.run(masks[m], 2 * EVERY, rc.TAU[m], rc.U0[m], np.dtype(dtype), f=f)
            f, macro = trt.run(masks[m], 2 * EVERY, rc.TAU[m], rc.U0[m], tc.MAGIC[m], f=f)
            assert bits_equal(at_switch[m], f) and not bits_equal(at_switch[m], only_bgk), m
            assert all(bits_equal(g, w) for g, w in zip(b.read_macro(m), macro)), m
        b.enable_trt(None)
        assert not b.trt_enabled and list(b.history()["step"]) == [EVERY * k for k in (1, 2, 3, 4)]
        b.step(2 * EVERY, rc.TAU, rc.U0, sample_every=EVERY)                 # BGK again
        h = b.history()
        assert list(h["step"]) == [EVERY * k for k in (1, 2, 3, 4, 5, 6)]   # the step count went on, the rows stayed
        for k in ("fx", "fy", "surf", "rev"):
            assert h[k][:4].tobytes() == first[k].tobytes(), k
        for m in range(rc.B):
            want_f, want_macro = lbm_numpy.run(masks[m], 2 * EVERY, rc.TAU[m], rc.U0[m], np.dtype(dtype), f=at_switch[m])
            assert bits_equal(b.read_f(m), want_f), m
            assert all(bits_equal(g, w) for g, w in zip(b.read_macro(m), want_macro)), m


# ---- 5. the read-outs stand on the new state ---------------------------------------------------
def test_readouts_are_defined_on_the_trt_state(pkg):
    name, calls = "96x48-f32", 4
    nx, ny, dtype, members = tc.EQ_CASES[name]
    tau, u0, magic = ([m[k] for m in members] for k in (2, 3, 4))
    masks = tc.eq_masks(name)
    B = len(members)
    xr, yr = [0.3641 * nx + 1.7 * m for m in range(B)], [0.5 * ny - 0.85 * m - 3.3 for m in range(B)]
    forces, mex, fs = [], [], [[] for _ in range(B)]
    with pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=calls) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        b.enable_momentum_exchange(xr, yr)
        b.enable_trt(magic)
        for _ in range(calls):
            b.step(12, tau, u0, sample_every=12)
            forces.append(b.forces())
            mex.append(b.momentum_exchange())
            for m in range(B):
                fs[m].append(b.read_f(m))
        h = b.history()
    assert list(h["step"]) == [12 * (k + 1) for k in range(calls)]
    f_trt, _ = trt.run(masks[0], 12, tau[0], u0[0], magic[0])                 # the state under the read-outs is the model's
    assert bits_equal(fs[0][0], f_trt) and not bits_equal(fs[0][0], lbm_numpy.run(masks[0], 12, tau[0], u0[0], np.float32)[0])
    worst = [0.0, 0.0, 0.0]
    for r in range(calls):
        for k, v in zip(("fx", "fy", "surf", "rev"), forces[r]):              # a history row is the on-demand call on that state
            assert h[k][r].tobytes() == v.tobytes(), (r, k)
        for k, v in zip(("fx_mex", "fy_mex", "mz_mex", "links"), mex[r]):
            assert h[k][r].tobytes() == v.tobytes(), (r, k)
        for m in range(B):
            mx = mex_reference(fs[m][r], masks[m], xr[m], yr[m])
            assert mx.links == int(h["links"][r, m]) > 20
            for q, (got, want, bound) in enumerate(((h["fx_mex"][r, m], mx.fx, mx.fx_bound), (h["fy_mex"][r, m], mx.fy, mx.fy_bound),
                                                    (h["mz_mex"][r, m], mx.mz, mx.mz_bound))):
                err = abs(got - want)
                worst[q] = max(worst[q], err / bound)
                assert err <= bound, (m, r, q, got, want, bound)
    print(f"worst |x - ref| / bound: mex fx {worst[0]:.3g}, fy {worst[1]:.3g}, mz {worst[2]:.3g}")


# ---- 6. errors ---------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_leave_the_batch_as_it_was(pkg, oracle_np):
    nx, ny = 96, 48
    mask = pkg.geometry.build_geometry(nx, ny, 6.0, None, "naca2412").mask
    tau, u0 = 0.56, 0.06
    dp = ctypes.POINTER(ctypes.c_double)
    with pkg.PolarEngine(nx, ny, 2, history_cap=4) as b:
        b.set_masks(np.stack([mask, mask]))
        b.init_equilibrium(u0)
        for bad in (0.0, -0.25, 1.0000001, float("nan")):
            with pytest.raises(pkg.WTError) as ei:
                b.enable_trt([0.25, bad])
            assert ei.value.code == WT_ERR_ARG and "magic[1]" in str(ei.value)
            assert not b.trt_enabled
        inf = np.array([0.25, float("inf")])
        assert b._lib.wtp_enable_trt(b._b, inf.ctypes.data_as(dp)) == WT_ERR_ARG
        b.step(6, tau, u0, sample_every=6)                                    # still a BGK batch, with the bits of an undisturbed one
        assert bits_equal(b.read_f(1), oracle_np.run(mask, 6, tau, u0, np.float32)[0])
        b.step(6, 0.5, u0, sample_every=6)                                    # with the model off tau = 0.5 is accepted, as always
        at = b.read_f(0)
        b.enable_trt([1.0, 1.0 / 12.0])                                       # the upper bound itself is allowed
        with pytest.raises(pkg.WTError):
            b.enable_trt([0.25, 2.0])
        assert b.trt_enabled                                                  # a refused call changes nothing: the magic numbers stay
        hist = b.history()
        for bad_tau in (0.5, [0.56, 0.5 + 1e-9], 0.4):                        # (0.5 + 1e-9 is 0.5 in float32)
            with pytest.raises(pkg.WTError) as ei:
                b.step(6, bad_tau, u0, sample_every=6)
            assert ei.value.code == WT_ERR_ARG and "tau[" in str(ei.value)
            after = b.history()
            assert b.step_count == 12 and list(after["step"]) == [6, 12] and all(_same(after[k], hist[k]) for k in hist)
            assert _same(b.read_f(0), at)
        b.step(6, tau, u0, sample_every=6)
        for m, lam in ((0, 1.0), (1, 1.0 / 12.0)):
            assert bits_equal(b.read_f(m), trt.run(mask, 6, tau, u0, lam, f=at)[0]), m
        b.enable_trt(None)
        b.step(6, 0.5, u0, sample_every=6)                                    # off again: accepted again
        assert b.step_count == 24 and list(b.history()["step"]) == [6, 12, 18, 24]
    with pkg.PolarEngine(nx, ny, 2, storage="half") as b:                    # interpolated walls stay out of a half batch
        b.set_masks(np.stack([mask, mask]))
        b.init_equilibrium(u0)
        b.enable_trt(0.1875)
        with pytest.raises(pkg.WTError) as ei:
            b.enable_interpolated_walls()
        assert ei.value.code == WT_ERR_STATE and b.trt_enabled and not b.interpolated_walls
        b.step(4, tau, u0)
        want = half.run(mask, 4, tau, u0, 0.1875, base_step=trt.step)
        assert _same(b.read_stored(0), want[0].view(np.uint16))


# ---- 7. the wall position ----------------------------------------------------------------------
def test_channel_walls_sit_half_way_under_trt_and_not_under_bgk(pkg):
    """The channel of tests/test_polar_trt_host.py on the device: fp64, 64x14, rows 0 and NY-1 solid, tau = 2.0, U0 = 0.04, 7264 steps from
    equilibrium, a parabola fitted to ux over rows 1 .. NY-2 of column 48.  BGK's zeros lie more than 0.15 cells outside the walls at y = 1
    and y = NY-1 (theory 0.225, the reference measures 0.32); TRT's at Lambda = 3/16 less than 0.1 cells from them (theory 0, reference 0.035)."""
    C = trt.CHANNEL
    mask = trt.channel_mask()
    offsets = {}
    for magic in (None, 3.0 / 16.0):
        with pkg.PolarEngine(C["nx"], C["ny"], 1, dtype="float64") as b:
            b.set_masks(mask)
            b.init_equilibrium(C["u0"])
            if magic is not None:
                b.enable_trt(magic)
            b.step(C["steps"], C["tau"], C["u0"])
            offsets[magic] = trt.wall_offsets(b.read_macro(0)[1][:, C["column"]])
    print(f"wall offsets (cells outside y = 1, y = NY - 1): BGK {offsets[None]}, TRT 3/16 {offsets[3.0 / 16.0]}")
    assert all(v > 0.15 for v in offsets[None])
    assert all(abs(v) < 0.1 for v in offsets[3.0 / 16.0])


# ---- 8. run_polar ------------------------------------------------------------------------------
def test_run_polar_with_trt_is_an_engine_driven_by_hand(pkg):
    alphas = [2.0, 4.0, 6.0]
    nx, ny, warmup, samples, every, magic = 96, 48, 36, 4, 12, 0.25
    kw = dict(nx=nx, ny=ny, warmup_steps=warmup, samples=samples, sample_every=every)
    res = pkg.run_polar(alphas, collision="trt", magic=magic, **kw)
    assert res.collision == "trt" and res.magic == magic and res.les is None
    masks = np.stack([pkg.geometry.build_geometry(nx, ny, a, [], "naca2412").mask for a in alphas])
    with pkg.PolarEngine(nx, ny, len(alphas), history_cap=samples) as b:
        b.set_masks(masks)
        b.init_equilibrium(res.u0)
        b.enable_loads(*pkg.polar.quarter_chord(nx, ny))
        b.enable_trt(magic)
        b.step(warmup, res.tau, res.u0)
        b.step(samples * every, res.tau, res.u0, sample_every=every)
        h = b.history()
    assert list(h["step"]) == [warmup + every * (r + 1) for r in range(samples)]
    for m in range(len(alphas)):
        got = res.points[m].history
        assert list(got["step"]) == list(h["step"])
        for k in ("fx", "fy", "surf", "rev", "mz"):
            assert _same(got[k], np.ascontiguousarray(h[k][:, m])), (m, k)
        assert np.isfinite(got["fx"]).all() and (got["surf"] > 0).all()
    plain, bgk = pkg.run_polar(alphas, **kw), pkg.run_polar(alphas, collision="bgk", **kw)
    assert plain.collision == bgk.collision == "bgk" and plain.magic is None and bgk.magic is None
    for m in range(len(alphas)):
        for k in plain.points[m].history:
            assert _same(plain.points[m].history[k], bgk.points[m].history[k]), (m, k)
        assert not _same(plain.points[m].history["fx"], res.points[m].history["fx"]), m      # (and TRT is another flow)
