"""GPU: the inclined free stream of batched sweeps (k_step_batch with FAR_INCLINED, k_fill_wind, wtp_enable_wind) against its definition in NumPy
(tests/_wind_reference.py).

There is no tolerance on the state: the kernel and the reference form the far field by the same operations, rounded once each, so
populations and macroscopic fields are the same bits, with either collision and either wall rule.  The read-outs on top of a wind state
are held to their own features' checks.  The sweep test asserts what tests/test_polar_wind_host.py asserts of the reference: the
second differences of the polar shrink by more than a factor of ten, and the lift-curve slope stays.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from conftest import bits_equal
import lbm_numpy
import _ibb_reference as ibb
import _les_reference as les
import _wind_reference as wind
from _loads_reference import loads_reference, surface_sums
from _mean_reference import SUMS, accumulate
from _mex_reference import mex_reference
from test_gpu_polar_ibb import _setup as _ibb_setup
from test_gpu_polar_mean import _block_masks

pytestmark = pytest.mark.gpu

WT_ERR_ARG = -1
STEPS = 60
EVERY = 12

# Members: (shape, aoa, tau, u0, v0 / u0, cs); cs is used by the Smagorinsky variants only.  The lattices are chosen by step_tile's
# classes: 96x48 has ragged tiles only, so site_general holds the far field; 40x300 and 37x299 fp32 a FAST or INLET tile of 256 rows
# that holds row 0 and a ragged one that holds row NY-1 (and an odd NY); 24x256 fp32 FAST and INLET tiles only, so the top row sits
# inside a FAST tile; 24x140 fp64 tiles of 128 rows.
CASES = {
    "96x48-f32": (96, 48, "float32", [("naca0012", 0.0, 0.52, 0.08, 0.0, 0.17), ("naca2412", 6.0, 0.9, 0.03, 0.6, 0.1), ("naca4412", -4.0, 0.6, 0.06, -0.25, 0.0)]),
    "40x300-f32": (40, 300, "float32", [("block", 0.0, 0.52, 0.08, 0.6, 0.17), ("block", 0.0, 0.7, 0.05, 0.0, 0.0), ("block", 0.0, 0.9, 0.03, -0.25, 0.1)]),
    "37x299-f32": (37, 299, "float32", [("block", 0.0, 0.55, 0.08, -0.25, 0.17), ("block", 0.0, 0.6, 0.06, 0.6, 0.1), ("block", 0.0, 0.52, 0.03, 0.0, 0.0)]),
    "24x256-f32": (24, 256, "float32", [("block", 0.0, 0.52, 0.07, 0.6, 0.1), ("block", 0.0, 0.9, 0.03, -0.25, 0.0), ("block", 0.0, 0.6, 0.05, 0.0, 0.17)]),
    "24x140-f64": (24, 140, "float64", [("block", 0.0, 0.52, 0.08, -0.25, 0.1), ("block", 0.0, 0.9, 0.03, 0.0, 0.17), ("block", 0.0, 0.6, 0.06, 0.6, 0.0)]),
}
# the interpolated walls of test_gpu_polar_ibb: member 0 an airfoil with its true distances, the others random blobs with random ones
COMBINED = {"96x48-f32": "96x48-f32", "24x140-f64": "24x140-f64"}
VARIANTS = ("les", "ibb", "les+ibb")


def _masks(nx, ny, members):
    import airfoil_cfd_tool_amd as pkg
    if members[0][0] == "block":
        return _block_masks(nx, ny, len(members))
    return np.stack([pkg.geometry.build_geometry(nx, ny, a, None, s).mask for s, a, *_ in members])


def _params(members):
    tau, u0 = [m[2] for m in members], [m[3] for m in members]
    return tau, u0, [m[3] * m[4] for m in members], [m[5] for m in members]


def _frozen(out):
    for a in (out[0], *out[1]):
        a.setflags(write=False)
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def _reference(name, steps=STEPS):
    """(masks, per member (f, (rho, ux, uy)) of the wrapped oracle after `steps` steps from wind_init)."""
    nx, ny, dtype, members = CASES[name]
    masks = _masks(nx, ny, members)
    tau, u0, v0, _ = _params(members)
    return masks, [_frozen(wind.run(masks[m], steps, tau[m], u0[m], v0[m], dtype=np.dtype(dtype))) for m in range(len(members))]


@functools.lru_cache(maxsize=None)
def _combined_reference(name, variant):
    """The same with the Smagorinsky collision, interpolated walls, or both: (masks, q, per member (f, macro))."""
    nx, ny, dtype, members = CASES[name]
    tau, u0, v0, cs = _params(members)
    masks, q = _ibb_setup(COMBINED[name])
    out = []
    for m in range(len(members)):
        c = les.les_constant(cs[m], dtype)
        if variant == "les":
            base, extra = les.step, (c,)
        else:
            base, extra = ibb.step, (q[m], c if variant == "les+ibb" else None)
        out.append(_frozen(wind.run(masks[m], STEPS, tau[m], u0[m], v0[m], *extra, base_step=base, dtype=np.dtype(dtype))))
    return masks, q, out


def _assert_state(b, ref, what):
    for m, (want_f, want_macro) in enumerate(ref):
        f, macro = b.read_f(m), b.read_macro(m)
        bad = int((f.view(np.uint8) != want_f.view(np.uint8)).reshape(9, f.shape[1], -1).any(axis=(0, 2)).sum())
        assert bits_equal(f, want_f), (what, m, bad, "rows differ")
        for got, want, plane in zip(macro, want_macro, ("rho", "ux", "uy")):
            assert bits_equal(got, want), (what, m, plane)


# ---- 1. bit identity ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_state_is_the_references_bits(pkg, name):
    nx, ny, dtype, members = CASES[name]
    tau, u0, v0, _ = _params(members)
    masks, ref = _reference(name)
    # the comparison is not vacuous, on the reference itself
    assert sorted(m[4] for m in members) == [-0.25, 0.0, 0.6]
    for m in range(len(members)):
        axial = lbm_numpy.run(masks[m], STEPS, tau[m], u0[m], np.dtype(dtype))[0]
        far = wind.far_field(masks[m])
        diff = (ref[m][0] != axial).any(axis=0)
        if v0[m] == 0:
            assert ref[m][0].tobytes() == axial.tobytes()                  # a V0 = 0 member of the reference is the oracle
            continue
        inner = ~far & (masks[m] == 0)
        inner[:, nx - 1] = False
        print(f"{name} member {m}: {int(far.sum())} far-field cells, all differ from the axial oracle: {bool(diff[far].all())}; "
              f"so do {float(diff[inner].mean()):.3f} of the interior fluid cells")
        assert diff[far].all() and diff[inner].mean() > 0.25
    with pkg.PolarEngine(nx, ny, len(members), dtype=dtype) as b:
        b.set_masks(masks)
        b.enable_wind(v0)
        assert b.wind_enabled
        b.init_equilibrium(u0)
        b.step(STEPS, tau, u0)
        _assert_state(b, ref, name)


# ---- 2. with the other collision and the other wall rule ---------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(COMBINED))
def test_state_is_the_references_bits_with_les_and_interpolated_walls(pkg, name, variant):
    nx, ny, dtype, members = CASES[name]
    tau, u0, v0, cs = _params(members)
    masks, q, ref = _combined_reference(name, variant)
    assert sorted(cs) == [0.0, 0.1, 0.17]
    for m in range(len(members)):                                           # the model under the wrapper acts: not the plain wind reference
        plain = wind.run(masks[m], STEPS, tau[m], u0[m], v0[m], dtype=np.dtype(dtype))[0]
        if variant != "les" or cs[m] > 0:
            assert not np.array_equal(ref[m][0], plain), (name, variant, m)
    with pkg.PolarEngine(nx, ny, len(members), dtype=dtype) as b:
        b.set_masks(masks)
        if "ibb" in variant:
            b.enable_interpolated_walls()
            b.set_wall_distances(q)
        if "les" in variant:
            b.enable_les(cs)
        b.enable_wind(v0)
        b.init_equilibrium(u0)
        b.step(STEPS, tau, u0)
        _assert_state(b, ref, (name, variant))


# ---- 3. V0 = 0 is today's batch ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["40x300-f32", "24x140-f64"])
def test_v0_zero_is_a_plain_batch(pkg, name):
    nx, ny, dtype, members = CASES[name]
    tau, u0, v0, _ = _params(members)
    masks = _masks(nx, ny, members)
    B = len(members)
    zero = v0.index(0.0)
    state = {}
    for mode, values in (("never", None), ("zeros", [0.0] * B), ("mixed", v0)):
        with pkg.PolarEngine(nx, ny, B, dtype=dtype) as b:
            b.set_masks(masks)
            if values is not None:
                b.enable_wind(values)
            assert b.wind_enabled is (values is not None)
            b.init_equilibrium(u0)
            start = [(b.read_f(m), b.read_macro(m)) for m in range(B)]
            b.step(STEPS, tau, u0)
            state[mode] = (start, [(b.read_f(m), b.read_macro(m)) for m in range(B)])

    def same(x, y):
        return x[0].tobytes() == y[0].tobytes() and all(a.tobytes() == c.tobytes() for a, c in zip(x[1], y[1]))
    for part in (0, 1):                                                     # the start state, and the state after the steps
        for m in range(B):
            assert same(state["zeros"][part][m], state["never"][part][m]), (part, m)
        assert same(state["mixed"][part][zero], state["never"][part][zero]), part
        other = (zero + 1) % B
        assert not same(state["mixed"][part][other], state["never"][part][other]), part      # (while a member with V0 != 0 is not)


# ---- 4. the start state ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_start_state_is_wind_init(pkg, dtype):
    nx, ny = 37, 299
    u0, v0 = [0.0598, 0.03, 0.08], [0.0042, -0.0075, 0.0]
    with pkg.PolarEngine(nx, ny, 3, dtype=dtype) as b:
        b.set_masks(_block_masks(nx, ny, 3))
        b.init_equilibrium(u0)
        b.enable_wind(v0)                                                   # the start state changes from the next init_equilibrium
        assert bits_equal(b.read_f(0), lbm_numpy.equilibrium_init(nx, ny, u0[0], dtype)[0])
        b.init_equilibrium(u0)
        for m in range(3):
            want_f, want_macro = wind.wind_init(nx, ny, u0[m], v0[m], dtype)
            assert bits_equal(b.read_f(m), want_f), m
            assert all(bits_equal(a, c) for a, c in zip(b.read_macro(m), want_macro)), m
        assert not bits_equal(b.read_f(0), lbm_numpy.equilibrium_init(nx, ny, u0[0], dtype)[0])
        b.enable_wind(None)
        b.init_equilibrium(u0)
        assert bits_equal(b.read_f(0), lbm_numpy.equilibrium_init(nx, ny, u0[0], dtype)[0])


# ---- 5. off again ------------------------------------------------------------------------------
def test_switching_off_returns_to_the_axial_far_field_and_keeps_the_history(pkg, oracle_np):
    name = "96x48-f32"
    nx, ny, dtype, members = CASES[name]
    tau, u0, v0, _ = _params(members)
    masks, _ = _reference(name)
    B = len(members)
    with pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=8) as b:
        b.set_masks(masks)
        b.enable_wind(v0)
        b.init_equilibrium(u0)
        b.step(24, tau, u0, sample_every=EVERY)
        first = b.history()
        at_switch = [b.read_f(m) for m in range(B)]
        _assert_state(b, _reference(name, 24)[1], "first half")             # the first half was the model's
        b.enable_wind(None)
        assert not b.wind_enabled
        assert list(b.history()["step"]) == [12, 24]
        b.step(24, tau, u0, sample_every=EVERY)
        h = b.history()
        assert list(h["step"]) == [12, 24, 36, 48]                          # the step count went on, the rows stayed
        for k in ("fx", "fy", "surf", "rev"):
            assert h[k][:2].tobytes() == first[k].tobytes(), k
        after = [b.read_f(m) for m in range(B)]
        for m in range(B):
            want_f, want_macro = oracle_np.run(masks[m], 24, tau[m], u0[m], np.float32, f=at_switch[m])
            assert bits_equal(after[m], want_f), m
            assert all(bits_equal(a, c) for a, c in zip(b.read_macro(m), want_macro)), m
        # on again with other values: takes effect from the next step, the state is kept
        other = [0.01, 0.0, -0.02]
        b.enable_wind(other)
        assert b.wind_enabled
        b.step(12, tau, u0)
        for m in range(B):
            want_f, want_macro = wind.run(masks[m], 12, tau[m], u0[m], other[m], f=after[m])
            assert bits_equal(b.read_f(m), want_f), m
            assert all(bits_equal(a, c) for a, c in zip(b.read_macro(m), want_macro)), m
        assert not bits_equal(b.read_f(0), oracle_np.run(masks[0], 12, tau[0], u0[0], np.float32, f=after[0])[0])


# ---- 6. the read-outs stand on the new state ---------------------------------------------------
def test_readouts_are_defined_on_the_wind_state(pkg):
    nx, ny, calls = 160, 80, 6
    members = [("naca0012", 0.0, 0.53, 0.06, 0.1), ("naca2412", 0.0, 0.58, 0.05, -0.07), ("naca4412", 3.0, 0.7, 0.07, 0.15)]
    tau, u0 = [m[2] for m in members], [m[3] for m in members]
    v0 = [m[3] * m[4] for m in members]
    masks = np.stack([pkg.geometry.build_geometry(nx, ny, a, None, s).mask for s, a, *_ in members])
    B = len(members)
    xr, yr = [0.3641 * nx + 1.7 * m for m in range(B)], [0.5 * ny - 0.85 * m - 3.3 for m in range(B)]
    macros, fs, forces = [[] for _ in range(B)], [[] for _ in range(B)], []
    with pkg.PolarEngine(nx, ny, B, history_cap=calls) as b:
        b.set_masks(masks)
        b.enable_wind(v0)
        b.init_equilibrium(u0)
        b.enable_loads(xr, yr)
        b.enable_momentum_exchange(xr, yr)
        b.enable_mean_fields()
        for _ in range(calls):
            b.step(EVERY, tau, u0, sample_every=EVERY)
            forces.append(b.forces())
            for m in range(B):
                macros[m].append(b.read_macro(m))
                fs[m].append(b.read_f(m))
        h = b.history()
        surface = [b.surface(m) for m in range(B)]
        sums = [b.mean_sums(m) for m in range(B)]
    assert list(h["step"]) == [EVERY * (k + 1) for k in range(calls)]
    for r in range(calls):                                                  # a history row is wtp_forces on that state
        for k, v in zip(("fx", "fy", "surf", "rev"), forces[r]):
            assert h[k][r].tobytes() == v.tobytes(), (r, k)
    # the state under the read-outs is the model's: member 0 is the wind reference, and not the axial oracle
    assert bits_equal(fs[0][0], wind.run(masks[0], EVERY, tau[0], u0[0], v0[0])[0])
    assert not bits_equal(fs[0][0], lbm_numpy.run(masks[0], EVERY, tau[0], u0[0], np.float32)[0])
    worst = [0.0, 0.0, 0.0, 0.0]
    for m in range(B):
        for r in range(calls):
            lo = loads_reference(macros[m][r][0], masks[m], xr[m], yr[m])
            assert lo.n == int(h["surf"][r, m]) > 0
            mx = mex_reference(fs[m][r], masks[m], xr[m], yr[m])
            assert mx.links == int(h["links"][r, m]) > 100
            for q, (got, want, bound) in enumerate(((h["mz"][r, m], lo.mz, lo.mz_bound), (h["fx_mex"][r, m], mx.fx, mx.fx_bound),
                                                    (h["fy_mex"][r, m], mx.fy, mx.fy_bound), (h["mz_mex"][r, m], mx.mz, mx.mz_bound))):
                err = abs(got - want)
                worst[q] = max(worst[q], err / bound)
                assert err <= bound, (m, r, q, got, want, bound)
        su, sl, nu, nl = surface_sums([mac[0] for mac in macros[m]], masks[m])
        assert np.array_equal(surface[m]["n_upper"], nu) and np.array_equal(surface[m]["n_lower"], nl) and int((nu > 0).sum()) > 60
        assert bits_equal(surface[m]["rho_upper"], su) and bits_equal(surface[m]["rho_lower"], sl)
        want = accumulate(macros[m])
        assert sums[m]["n"] == want["n"] == calls
        for k in SUMS:
            assert bits_equal(sums[m][k], want[k]), (m, k)
    print(f"worst |x - ref| / bound: Mz {worst[0]:.3g}, mex fx {worst[1]:.3g}, fy {worst[2]:.3g}, mz {worst[3]:.3g}; surface and mean sums bit-identical")


# ---- 7. run_polar ------------------------------------------------------------------------------
def _rms_second_difference(v):
    v = np.asarray(v, np.float64)
    d2 = v[:-2] - 2.0 * v[1:-1] + v[2:]
    return float(np.sqrt((d2 * d2).mean()))


def test_run_polar_in_the_wind_frame_has_no_saw_tooth(pkg):
    """160x80 NACA 2412, 4 to 6 degrees in steps of 0.25, warm-up 5400 steps, 100 samples.  On the NumPy reference the r.m.s. second
    difference of CL is 0.00013 with the free stream turned against 0.0763 with the body turned, that of CD 0.00015 against 0.00818, and
    the slopes are 0.0952 and 0.1047 per degree."""
    alphas = pkg.sweep_alphas(4.0, 6.0, 0.25)
    assert len(alphas) == 9
    kw = dict(shape="naca2412", nx=160, ny=80, warmup_steps=5400, samples=100, total_forces=True)
    w = pkg.run_polar(alphas, frame="wind", **kw)
    b = pkg.run_polar(alphas, **kw)
    assert w.frame == "wind" and b.frame == "body" and w.tau == b.tau and w.u0 == b.u0 == 0.06
    for p in w.points + b.points:
        assert p.converged and p.samples == 100, p
    assert [p.alpha for p in w.points] == alphas
    cl = {k: [p.cl_mean for p in r.points] for k, r in (("wind", w), ("body", b))}
    cd = {k: [p.cd_mean for p in r.points] for k, r in (("wind", w), ("body", b))}
    rms_cl = {k: _rms_second_difference(v) for k, v in cl.items()}
    rms_cd = {k: _rms_second_difference(v) for k, v in cd.items()}
    slope = {k: (v[-1] - v[0]) / 2.0 for k, v in cl.items()}
    print(f"CL wind {np.round(cl['wind'], 4).tolist()}, body {np.round(cl['body'], 4).tolist()}")
    print(f"CD wind {np.round(cd['wind'], 5).tolist()}, body {np.round(cd['body'], 5).tolist()}")
    print(f"r.m.s. second difference: CL wind {rms_cl['wind']:.5f}, body {rms_cl['body']:.5f}; CD wind {rms_cd['wind']:.5f}, body {rms_cd['body']:.5f}; "
          f"slopes wind {slope['wind']:.4f}, body {slope['body']:.4f} per degree")
    assert rms_cl["wind"] < 0.1 * rms_cl["body"]
    assert rms_cd["wind"] < 0.1 * rms_cd["body"]
    assert abs(slope["wind"] - slope["body"]) <= 0.2 * min(abs(slope["wind"]), abs(slope["body"]))
    for p in w.points:
        assert all(math.isfinite(v) for v in (p.cl_total_mean, p.cd_total_mean, p.cm_total_mean, p.cm_mean))
        assert p.cd_total_mean > p.cd_mean
        assert set(p.history) >= {"fx", "fy", "fx_mex", "fy_mex", "mz", "links"}
    # one body: every member of the wind sweep has the unrotated body's surface, the body sweep's do not
    assert len({int(p.history["surf"][0]) for p in w.points}) == 1 and len({int(p.history["links"][0]) for p in w.points}) == 1
    assert len({int(p.history["links"][0]) for p in b.points}) > 1


# ---- 8. argument errors ------------------------------------------------------------------------
def test_bad_values_are_argument_errors_and_leave_the_batch_usable(pkg, oracle_np):
    nx, ny = 96, 48
    mask = pkg.geometry.build_geometry(nx, ny, 0.0, None, "naca2412").mask
    tau, u0 = 0.58, 0.06
    with pkg.PolarEngine(nx, ny, 2) as b:
        b.set_masks(np.stack([mask, mask]))
        b.init_equilibrium(u0)
        for bad in (float("nan"), float("inf"), -float("inf"), 0.36, -0.36):
            with pytest.raises(pkg.WTError) as ei:
                b.enable_wind([0.01, bad])
            assert ei.value.code == WT_ERR_ARG and "v0[1]" in str(ei.value), bad
            assert not b.wind_enabled
        v = np.array([float("nan"), 0.0])
        assert b._lib.wtp_enable_wind(b._b, v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == WT_ERR_ARG
        assert b"v0[0]" in b._lib.wtp_last_error()
        b.step(10, tau, u0)                                                 # still an axial batch
        assert bits_equal(b.read_f(1), oracle_np.run(mask, 10, tau, u0, np.float32)[0])
        b.enable_wind([0.35, -0.35])                                        # the bounds themselves are allowed
        assert b.wind_enabled
        first = [0.004, -0.006]
        b.enable_wind(first)                                                # calling it again replaces the values
        b.step(10, tau, u0)
        with pytest.raises(pkg.WTError):
            b.enable_wind([0.02, 0.5])
        assert b.wind_enabled                                               # a refused call changes nothing
        b.step(10, tau, u0)
        for m in range(2):
            f = oracle_np.run(mask, 10, tau, u0, np.float32)[0]
            f = wind.run(mask, 20, tau, u0, first[m], f=f)[0]
            assert bits_equal(b.read_f(m), f), m
