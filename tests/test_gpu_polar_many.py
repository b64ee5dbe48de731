"""GPU: batched sweeps (libwtpolar.so) at many members, every member against its own reference: batches of 67 (prime, above 64), 35
(odd) and 1024 (WTP_MAX_MEMBERS) members whose masks, tau, U0, Cs, V0, wall distances and reference points all differ
(tests/_many_cases.py; tests/test_polar_many_host.py shows on the references alone that a member which ran with another member's
value of anything would be seen).  What is exercised is every lookup the kernels and the host loops make by the member index:
params, cles, vwind, the reference points, the windows, the member strides of every array, the surface and column partials, the
three ticket arrays, the rows of the sample tables, the reversed member walk, and the (first, count) loops of wtp_set_masks and
wtp_set_wall_q.

The references and the tolerances are those of the tests of each feature: states are the references' bits (the C oracle for a plain
batch, _wind_reference over _ibb_reference / _les_reference with the models on), the force sums are held to the derived bounds of
Loads, Mex and MexIbb, the surface and mean sums are the references' bits.

The lookups by member index of the features that came after this file live in tests/test_gpu_polar_many_models.py, on the same
batches (tests/_many_model_cases.py): the member walk of the half kernels (k_step_half_batch, init_half,
k_mex_half_batch) and the lattice counted in halves, lam[m], zero_v and the per-member tau check of the two-relaxation-time collision,
prof + m * p_stride, the (first, count) loop of wtp_set_far_profile and prof_set[m] of the far-field profile, and the member offsets of
wtp_write_f / wtp_write_stored, of the sums they clear and of state() / restore().  That file imports this one's assertion helpers.
"""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal
import lbm_numpy
import _ibb_reference as ibb
import _many_cases as mc
import _wind_reference as wind
from _loads_reference import loads_reference, surface_rows, surface_sums
from _mean_reference import SUMS, accumulate
from _mex_reference import mex_reference

pytestmark = pytest.mark.gpu

WT_ERR_ARG = -1
PLANES = ("rho", "ux", "uy")


def _assert_member_state(got_f, got_macro, want, what):
    """Bit identity of one member's populations and planes; the failure names the member, the plane and the first differing row."""
    want_f, want_macro = want
    if not bits_equal(got_f, want_f):
        rows = np.flatnonzero((got_f.view(np.uint8) != want_f.view(np.uint8)).reshape(9, got_f.shape[1], -1).any(axis=(0, 2)))
        raise AssertionError((what, "f", f"{rows.size} rows differ, the first is row {int(rows[0])}"))
    for got, ref, plane in zip(got_macro, want_macro, PLANES):
        assert bits_equal(got, ref), (what, plane)


def _assert_batch_state(b, ref, what, members=None):
    for m in (range(b.members) if members is None else members):
        _assert_member_state(b.read_f(m), b.read_macro(m), ref[m], (what, "member", m))


def _ratio(err, bound):
    return err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))


def _engine(pkg, name, cap=0):
    nx, ny, dtype, B, _, _ = mc.CASES[name]
    return pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=cap)


# ---- 1. a plain batch ---------------------------------------------------------------------------
def _plain_batch(pkg, oracle_c, name, b):
    """Steps a fresh plain batch through plain_marks(name), reading every member back at each; asserts states, history rows, the
    on-demand forces and the clamp events of every member.  Returns the worst |x - ref| / bound of fx, fy."""
    nx, ny, dtype, B, steps, every = mc.CASES[name]
    mem = mc.members(name)
    ref = mc.plain_reference(name, oracle_c)
    marks = mc.plain_marks(name)
    b.init_equilibrium(mem.u0)
    done, got = 0, []
    for k, mark in enumerate(marks):
        b.step(mark - done, mem.tau, mem.u0, sample_every=every)
        done = mark
        got.append([(b.read_f(m), b.read_macro(m)) for m in range(B)])
    h = b.history()
    forces = b.forces()
    events = b.clamp_events()
    for k, mark in enumerate(marks):
        for m in range(B):
            _assert_member_state(*got[k][m], ref[k][m], (name, "step", mark, "member", m))
    assert list(h["step"]) == list(marks[1:]) and h["fx"].shape == (len(marks) - 1, B)
    worst = [0.0, 0.0]
    for r in range(len(marks) - 1):
        for m in range(B):
            rho, ux, _ = got[r + 1][m][1]
            lo = loads_reference(rho, mem.masks[m], 0.0, 0.0)
            assert int(h["surf"][r, m]) == lo.n > 0, (name, "row", r, "member", m, "surf", int(h["surf"][r, m]), lo.n)
            assert int(h["rev"][r, m]) == lbm_numpy.compute_forces_raw(rho, ux, mem.masks[m])[3], (name, "row", r, "member", m, "rev")
            for q, (key, want, bound) in enumerate((("fx", lo.fx, lo.fx_bound), ("fy", lo.fy, lo.fy_bound))):
                err = abs(float(h[key][r, m]) - want)
                worst[q] = max(worst[q], _ratio(err, bound))
                assert err <= bound, (name, "row", r, "member", m, key, float(h[key][r, m]), want, bound)
    for key, v in zip(("fx", "fy", "surf", "rev"), forces):                 # the last step was a sample: forces() is the last row
        assert v.tobytes() == h[key][-1].tobytes(), key
    for m in range(B):
        want = lbm_numpy.clamp_events(*got[-1][m][1], mem.masks[m])
        assert (int(events[0][m]), int(events[1][m])) == want == (0, 0), m
    print(f"{name}: {B} members x {len(marks)} read-backs bit-identical; worst |x - ref| / bound: fx {worst[0]:.3g}, fy {worst[1]:.3g}")
    return worst


@pytest.mark.parametrize("name", list(mc.BODY))
def test_every_member_of_a_plain_batch_is_its_oracle(pkg, oracle_c, name):
    mem = mc.members(name)
    with _engine(pkg, name, cap=3) as b:
        b.set_masks(mem.masks)
        _plain_batch(pkg, oracle_c, name, b)


# ---- 2. all models and all read-outs on ---------------------------------------------------------
def _models_on(b, mem, ibb_on=True, les_on=True, wind_on=True):
    if ibb_on:
        b.enable_interpolated_walls()
        b.set_wall_distances(mem.q)
    if les_on:
        b.enable_les(mem.cs)
    if wind_on:
        b.enable_wind(mem.v0)


class _Worst:
    KEYS = ("mz", "fx_mex", "fy_mex", "mz_mex")

    def __init__(self):
        self.v = dict.fromkeys(self.KEYS, 0.0)

    def check(self, key, got, want, bound, what):
        err = abs(float(got) - want)
        self.v[key] = max(self.v[key], _ratio(err, bound))
        assert err <= bound, (what, key, float(got), want, bound)

    def __str__(self):
        return "worst |x - ref| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in self.v.items())


def _assert_rows(h, r, m, f, rho, mask, q, xr, yr, worst, what):
    """History row r of member m against the references on the member's own read-back state."""
    lo = loads_reference(rho, mask, xr, yr)
    mx = ibb.mex_reference(f, mask, q, xr, yr) if q is not None else mex_reference(f, mask, xr, yr)
    assert int(h["surf"][r, m]) == lo.n > 0, (what, "surf", int(h["surf"][r, m]), lo.n)
    assert int(h["links"][r, m]) == mx.links > 0, (what, "links", int(h["links"][r, m]), mx.links)
    worst.check("mz", h["mz"][r, m], lo.mz, lo.mz_bound, what)
    worst.check("fx_mex", h["fx_mex"][r, m], mx.fx, mx.fx_bound, what)
    worst.check("fy_mex", h["fy_mex"][r, m], mx.fy, mx.fy_bound, what)
    worst.check("mz_mex", h["mz_mex"][r, m], mx.mz, mx.mz_bound, what)


def _assert_sums(surface, sums, macros, mask, what):
    """A member's surface and mean sums against the references over the list of its read-back planes, in sample order: bits."""
    ju, jl = surface_rows(mask)
    assert np.array_equal(surface["j_upper"], ju) and np.array_equal(surface["j_lower"], jl), what
    su, sl, nu, nl = surface_sums([mac[0] for mac in macros], mask)
    assert np.array_equal(surface["n_upper"], nu) and np.array_equal(surface["n_lower"], nl), what
    assert int(nu.max()) == int(nl.max()) == len(macros), what
    assert bits_equal(surface["rho_upper"], su) and bits_equal(surface["rho_lower"], sl), what
    want = accumulate(macros)
    assert sums["n"] == want["n"] == len(macros), what
    for k in SUMS:
        assert bits_equal(sums[k], want[k]), (what, k)


@pytest.mark.parametrize("name", list(mc.BODY))
def test_every_member_with_all_models_and_read_outs_on(pkg, name):
    nx, ny, dtype, B, steps, every = mc.CASES[name]
    mem = mc.members(name)
    ref = mc.model_reference(name)
    marks = mc.model_marks(name)
    got = []
    with _engine(pkg, name, cap=len(marks)) as b:
        b.set_masks(mem.masks)
        _models_on(b, mem)
        b.init_equilibrium(mem.u0)
        b.enable_loads(mem.xref, mem.yref)
        b.enable_momentum_exchange(mem.xref, mem.yref)
        b.enable_mean_fields()
        for _ in marks:
            b.step(every, mem.tau, mem.u0, sample_every=every)
            got.append([(b.read_f(m), b.read_macro(m)) for m in range(B)])
        h = b.history()
        moment, exchange = b.moment(), b.momentum_exchange()
        surface = [b.surface(m) for m in range(B)]
        sums = [b.mean_sums(m) for m in range(B)]
    assert list(h["step"]) == list(marks)
    worst = _Worst()
    for m in range(B):
        for r, mark in enumerate(marks):
            what = (name, "step", mark, "member", m)
            _assert_member_state(*got[r][m], ref[r][m], what)
            _assert_rows(h, r, m, got[r][m][0], got[r][m][1][0], mem.masks[m], mem.q[m], float(mem.xref[m]), float(mem.yref[m]), worst, what)
        _assert_sums(surface[m], sums[m], [got[r][m][1] for r in range(len(marks))], mem.masks[m], (name, "member", m))
    assert moment.tobytes() == h["mz"][-1].tobytes()                        # the on-demand calls on the last sampled state: the last row
    for key, v in zip(("fx_mex", "fy_mex", "mz_mex", "links"), exchange):
        assert v.tobytes() == h[key][-1].tobytes(), key
    print(f"{name}: {B} members x {len(marks)} samples bit-identical in state, surface sums and mean sums; {worst}")


# ---- 3. each model alone ------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(mc.VARIANTS))
def test_every_member_with_one_model_alone(pkg, variant):
    name = mc.SUB_CASE
    mem = mc.members(name)
    ref = mc.variant_reference(variant)
    with _engine(pkg, name) as b:
        b.set_masks(mem.masks)
        _models_on(b, mem, ibb_on=variant == "ibb", les_on="les" in variant, wind_on="wind" in variant)
        b.init_equilibrium(mem.u0)
        b.step(mc.VARIANT_STEPS - 7, mem.tau, mem.u0)                       # (two calls: the second starts on an odd count)
        b.step(7, mem.tau, mem.u0)
        _assert_batch_state(b, ref, (name, variant))


# ---- 4. sub-ranges in the middle of a batch -----------------------------------------------------
def test_sub_ranges_in_the_middle_of_a_batch(pkg):
    name = mc.SUB_CASE
    nx, ny, dtype, B, _, every = mc.CASES[name]
    mem = mc.members(name)
    ref = mc.model_reference(name)
    new_masks, new_q = mc.sub_inputs()
    (first, count), (qfirst, qcount) = mc.SUB_MASKS, mc.SUB_Q
    touched = range(first, first + count)
    got = []
    with _engine(pkg, name, cap=2) as b:
        b.set_masks(mem.masks)
        _models_on(b, mem)
        b.init_equilibrium(mem.u0)
        b.enable_loads(mem.xref, mem.yref)
        b.enable_momentum_exchange(mem.xref, mem.yref)
        b.enable_mean_fields()
        b.step(every, mem.tau, mem.u0, sample_every=every)
        got.append([(b.read_f(m), b.read_macro(m)) for m in range(B)])
        b.set_masks(new_masks, first=first)
        b.set_wall_distances(new_q, first=qfirst)
        after_upload = {m: (b.surface(m), b.mean_sums(m)) for m in (first - 1, *touched, first + count)}
        b.step(every, mem.tau, mem.u0, sample_every=every)
        got.append([(b.read_f(m), b.read_macro(m)) for m in range(B)])
        h = b.history()
        surface = [b.surface(m) for m in range(B)]
        sums = [b.mean_sums(m) for m in range(B)]
    assert list(h["step"]) == [every, 2 * every]
    # the uploads zeroed the sums of the members they touched, and of no neighbour
    for m, (s, mean) in after_upload.items():
        zero = not s["rho_upper"].any() and not s["n_upper"].any() and not s["rho_lower"].any() and not s["n_lower"].any()
        assert zero == (m in touched) and mean["n"] == (0 if m in touched else 1), \
            (f"member {m} and the uploads to [{first}, {first + count})", "surface sums zero:", zero, "mean n:", mean["n"])
    half = np.full((8, ny, nx), 0.5, np.dtype(dtype))
    worst = _Worst()
    for m in range(B):
        what = (name, "member", m)
        _assert_member_state(*got[0][m], ref[0][m], (*what, "before the uploads"))
        if m in touched:
            mask = new_masks[m - first]
            q = new_q[m - qfirst] if qfirst <= m < qfirst + qcount else half
            # the flow was kept: the member goes on from its own state under the new mask, with the distances reset or uploaded
            want = mc.run_member("all", mask, every, *mem.params(m), q, dtype, f=got[0][m][0])
            _assert_member_state(*got[1][m], want, (*what, "after the uploads"))
            _assert_sums(surface[m], sums[m], [got[1][m][1]], mask, what)   # the sums restarted: one sample
            assert sums[m]["n"] == 1 and int(surface[m]["n_upper"].max()) <= 1 and int(surface[m]["n_lower"].max()) <= 1
        else:
            mask, q = mem.masks[m], mem.q[m]
            _assert_member_state(*got[1][m], ref[1][m], (*what, "uninterrupted"))
            _assert_sums(surface[m], sums[m], [got[0][m][1], got[1][m][1]], mask, what)
        _assert_rows(h, 0, m, got[0][m][0], got[0][m][1][0], mem.masks[m], mem.q[m], float(mem.xref[m]), float(mem.yref[m]), worst, (*what, "row 0"))
        _assert_rows(h, 1, m, got[1][m][0], got[1][m][1][0], mask, q, float(mem.xref[m]), float(mem.yref[m]), worst, (*what, "row 1"))
    for m in (first - 1, first + count):                                    # either end of the range, by name
        assert got[1][m][0].tobytes() == ref[1][m][0].tobytes(), f"member {m}, next to the range [{first}, {first + count}), was touched"
        assert sums[m]["n"] == 2 and int(surface[m]["n_upper"].max()) == 2, m
    for m in (qfirst - 1, qfirst + qcount):                                 # and of the range of the distances: reset ones, not uploaded ones
        old = mc.run_member("all", new_masks[m - first], every, *mem.params(m), mem.q[m], dtype, f=got[0][m][0])
        assert got[1][m][0].tobytes() != old[0].tobytes(), m
    print(f"{name}: members {first}..{first + count - 1} restarted, {B - count} uninterrupted; {worst}")


# ---- 5. history sub-reads -----------------------------------------------------------------------
def test_history_sub_reads_are_slices_of_the_whole(pkg):
    name = mc.SUB_CASE
    nx, ny, dtype, B, steps, every = mc.CASES[name]
    mem = mc.members(name)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)

    def d(a):
        return a.ctypes.data_as(dp)

    def i(a):
        return a.ctypes.data_as(ip)

    with _engine(pkg, name, cap=3) as b:
        b.set_masks(mem.masks)
        b.init_equilibrium(mem.u0)
        b.enable_loads(mem.xref, mem.yref)
        b.enable_momentum_exchange(mem.xref, mem.yref)
        b.step(steps, mem.tau, mem.u0, sample_every=every)
        h = b.history()
        assert list(h["step"]) == [every, 2 * every, 3 * every] and np.isfinite(h["mz"]).all() and np.isfinite(h["mz_mex"]).all()
        for first, count in ((1, 2), (2, 1)):
            step = np.zeros(count, np.int64)
            f64 = {k: np.full((count, B), -7.0) for k in ("fx", "fy", "mz", "fx_mex", "fy_mex", "mz_mex")}
            i64 = {k: np.full((count, B), -7, np.int64) for k in ("surf", "rev", "links")}
            assert b._lib.wtp_history(b._b, first, count, i(step), d(f64["fx"]), d(f64["fy"]), i(i64["surf"]), i(i64["rev"])) == 3
            assert b._lib.wtp_history_moment(b._b, first, count, d(f64["mz"])) == 0
            assert b._lib.wtp_history_mex(b._b, first, count, d(f64["fx_mex"]), d(f64["fy_mex"]), d(f64["mz_mex"]), i(i64["links"])) == 0
            assert list(step) == list(h["step"][first:first + count])
            for k, v in {**f64, **i64}.items():
                assert v.tobytes() == np.ascontiguousarray(h[k][first:first + count]).tobytes(), (first, count, k)
        for m in range(B):                                                  # the rows are the members', not copies of one another
            assert len({h["fx"][r, m] for r in range(3)}) == 3, m
        assert len(set(h["fx"][2].tolist())) == B and len(set(h["mz"][2].tolist())) == B
        b.enable_loads(mem.yref, mem.xref)                                  # again: the rows held carry no Mz about these points
        again = b.history()
        assert np.isnan(again["mz"]).all() and again["mz"].shape == (3, B)
        for k in ("fx", "fy", "surf", "rev", "fx_mex", "fy_mex", "mz_mex", "links"):
            assert again[k].tobytes() == h[k].tobytes(), k


# ---- 6. WTP_MAX_MEMBERS -------------------------------------------------------------------------
def test_the_largest_batch(pkg, oracle_c):
    from airfoil_cfd_tool_amd._capi import WT_F32
    from airfoil_cfd_tool_amd.polar import load_polar_library
    name = mc.MAX
    nx, ny, dtype, B, steps, every = mc.CASES[name]
    mem = mc.members(name)
    T = np.dtype(dtype).type
    assert B == 1024
    handle = ctypes.c_void_p()
    lib = load_polar_library()
    assert lib.wtp_create(nx, ny, WT_F32, B + 1, 0, 0, ctypes.byref(handle)) == WT_ERR_ARG and not handle
    with _engine(pkg, name, cap=3) as b:
        b.set_masks(mem.masks)
        _plain_batch(pkg, oracle_c, name, b)                                # every member, every row
        # the same batch with an inclined free stream and the Smagorinsky collision, from a new start
        b.enable_les(mem.cs)
        b.enable_wind(mem.v0)
        b.init_equilibrium(mem.u0)
        b.enable_loads(mem.xref, mem.yref)
        b.enable_momentum_exchange(mem.xref, mem.yref)
        b.step(2 * every, mem.tau, mem.u0, sample_every=every)
        b.step(steps - 2 * every, mem.tau, mem.u0, sample_every=every)
        _assert_batch_state(b, mc.listed_reference(), (name, "wind+les"), mc.listed_members())
        events = b.clamp_events()
        assert not events[0].any() and not events[1].any()
        h = b.history()
        assert list(h["step"]) == list(mc.model_marks(name))
        worst = _Worst()
        for m in range(B):
            rho, ux, uy = b.read_macro(m)
            far = wind.far_field(mem.masks[m])                              # every member's far field is its own (U0, V0)
            want = (T(1.0), T(mem.u0[m]), T(mem.v0[m]))
            for plane, got, v in zip(PLANES, (rho, ux, uy), want):
                assert (got[far] == v).all() and (got[far].view(np.uint32) == np.array(v).view(np.uint32)).all(), (m, plane)
            assert int(far.sum()) == 2 * nx + ny - 4
            # and the last row of its moment and momentum exchange is the references' on its own state, about its own point
            _assert_rows(h, 2, m, b.read_f(m), rho, mem.masks[m], None, float(mem.xref[m]), float(mem.yref[m]), worst, (name, "wind+les", "member", m))
        assert np.isfinite(h["mz"]).all() and np.isfinite(h["mz_mex"]).all() and (h["links"] == 26).all() and (h["surf"] == 10).all()
        print(f"{name}: wind + LES: {len(mc.listed_members())} states bit-identical, {B} far fields exact; {worst}")
