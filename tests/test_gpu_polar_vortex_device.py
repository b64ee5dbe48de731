"""GPU: the device-side far-field vortex of batched sweeps (k_far_vortex behind k_forces_batch, wtp_enable_far_vortex and its
read-backs, run_polar(vortex_on="device")) against the host loop it replaces and against the NumPy functions that define it
(far_profile, vortex_update(norm="sqrt")), on the cases of tests/_vortex_cases.py.

No tolerance appears: every comparison is of bits.  The device forms the tables and the update by the operations of the NumPy
functions, rounded once each, and reads the forces that wtp_forces returns; a step reads tables and does not know who wrote them.  So a
run updated on the device and the same run updated by the host (forces, vortex_update, far_profile, set_far_profile) are one run, as
long as no update clips, which the cases avoid (tests/_vortex_cases.py) and every comparison asserts.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import bits_equal
import _profile_cases as pc
import _vortex_cases as vc
from test_gpu_polar_ibb import _setup as ibb_setup

pytestmark = pytest.mark.gpu

WT_ERR_ARG, WT_ERR_STATE = -1, -5
EVERY, AFTER, STEPS, SAMPLE_EVERY = vc.EVERY, vc.AFTER, vc.STEPS, vc.SAMPLE_EVERY
VARIANT = "trt+les+ibb"


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _masks(name, variant=""):
    return ibb_setup(pc.COMBINED[name]) if "ibb" in variant else (pc.masks_of(name), None)


def _engine(pkg, name, variant="", **kw):
    """A batch of the lattice `name` with its masks, the members' start state of (u0, v0), `variant`'s models and the profile on."""
    nx, ny, dtype, B = pc.lattice(name)
    _, u0, v0, cs = pc.params(name)
    masks, q = _masks(name, variant)
    b = pkg.PolarEngine(nx, ny, B, dtype=dtype.name, **kw)
    b.set_masks(masks)
    b.enable_wind(v0)
    b.init_equilibrium(u0)
    pc.configure(b, variant, q, cs)
    b.enable_far_profile()
    return b


def _enable(b, name, log_cap, every=EVERY, after=AFTER, relax=vc.RELAX, u_ref=None, with_source=True):
    s = vc.settings(name)
    b.enable_far_vortex(every, after, relax, s["u_ref"] if u_ref is None else u_ref, with_source, s["xc"], s["yc"], s["u_far"], s["v_far"],
                        s["alpha"], log_cap=log_cap)


def _result(b):
    B = b.members
    return {"f": [b.read_f(m) for m in range(B)], "macro": [b.read_macro(m) for m in range(B)], "history": b.history(),
            "tables": b.read_far_profile(), "steps": b.step_count}


def _assert_same_run(got, want, what):
    assert got["steps"] == want["steps"], what
    for m, (f, g) in enumerate(zip(got["f"], want["f"])):
        assert bits_equal(f, g), (what, m, "populations")
        for a, c, plane in zip(got["macro"][m], want["macro"][m], ("rho", "ux", "uy")):
            assert bits_equal(a, c), (what, m, plane)
    assert sorted(got["history"]) == sorted(want["history"])
    for k in got["history"]:
        assert _same(got["history"][k], want["history"][k]), (what, "history", k)
    for a, c, tab in zip(got["tables"], want["tables"], ("left", "bottom", "top")):
        assert bits_equal(a, c), (what, tab)


@functools.lru_cache(maxsize=None)
def _device_run(name, variant="", split=(STEPS,)):
    """STEPS steps on the device schedule, issued as the calls of `split`: the final state, the history, the log and the strengths."""
    import airfoil_cfd_tool_amd as pkg
    tau, u0, _, _ = pc.params(name)
    with _engine(pkg, name, variant, history_cap=STEPS // SAMPLE_EVERY) as b:
        _enable(b, name, log_cap=len(vc.UPDATE_STEPS))
        assert b.far_vortex_enabled
        for n in split:
            b.step(n, tau, u0, sample_every=SAMPLE_EVERY)
        out = _result(b)
        out["log"] = b.far_vortex_log()
        out["vortex"] = b.far_vortex()
    return out


@functools.lru_cache(maxsize=None)
def _host_run(name, variant=""):
    """The same run driven by the host loop: chunks of EVERY steps, and after each chunk that ends at or beyond AFTER forces(),
    vortex_update, far_profile and set_far_profile.  Also the list of updates, and whether one clipped."""
    import airfoil_cfd_tool_amd as pkg
    from airfoil_cfd_tool_amd.polar import vortex_update
    tau, u0, _, _ = pc.params(name)
    _, _, _, B = pc.lattice(name)
    s = vc.settings(name)
    strength, source = np.zeros(B), np.zeros(B)
    updates = []
    with _engine(pkg, name, variant, history_cap=STEPS // SAMPLE_EVERY) as b:
        b.set_far_profile(*pc.stack(vc.tables(name, strength, source)))
        done = 0
        while done < STEPS:
            n = min(EVERY, STEPS - done)
            b.step(n, tau, u0, sample_every=SAMPLE_EVERY)
            done += n
            if done % EVERY == 0 and done >= AFTER:
                fx, fy, _, _ = b.forces()
                strength, source, clipped = vortex_update(strength, source, fx, fy, s["alpha"], s["u_ref"], vc.RELAX, s["bound"])
                b.set_far_profile(*pc.stack(vc.tables(name, strength, source)))
                updates.append((done, fx, fy, strength, source, clipped))
        out = _result(b)
    out["updates"] = updates
    out["vortex"] = (strength, source)
    return out


# ---- 1. the tables ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.LATTICES)
def test_tables_are_far_profiles_bits(pkg, name):
    nx, ny, dtype, B = pc.lattice(name)
    _, u0, v0, _ = pc.params(name)
    T = dtype.type
    with _engine(pkg, name) as b:
        random = pc.stack(pc.random_tables(name))                           # the read-back returns what the host uploaded
        b.set_far_profile(*random)
        for got, want in zip(b.read_far_profile(), random):
            assert bits_equal(got, want), name
        for got, want in zip(b.read_far_profile(1, 1), random):
            assert bits_equal(got, want[1:2]), name
        _enable(b, name, log_cap=0)                                         # zero strengths: the uniform tables, entry for entry
        for tab in b.read_far_profile():
            assert tab.dtype == dtype
            for m in range(B):
                assert (tab[m, 0] == T(1.0)).all() and (tab[m, 1] == T(u0[m])).all() and (tab[m, 2] == T(v0[m])).all(), (name, m)
        strength, source = (np.array(v) for v in zip(*pc.VORTEX[name]))
        b.set_far_vortex(strength, source)
        for got, want in zip(b.read_far_profile(), pc.stack(pc.vortex_tables(name))):
            assert bits_equal(got, want), name
        s, q = b.far_vortex()
        assert _same(s, strength) and _same(q, source)
        assert any(not bits_equal(a, c) for a, c in zip(b.read_far_profile(), pc.stack(pc.tables_of(name, "uniform"))))


# ---- 2. one update ------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [False, True], ids=["u_ref=u0", "u_ref=0.002"])
@pytest.mark.parametrize("name", vc.LATTICES)
def test_one_update_is_vortex_updates_bits(pkg, name, clip):
    from airfoil_cfd_tool_amd.polar import VORTEX_SPEED_MAX, vortex_update
    tau, u0, _, _ = pc.params(name)
    _, _, _, B = pc.lattice(name)
    s = vc.settings(name)
    u_ref, relax = (vc.U_REF_CLIP, vc.RELAX_CLIP) if clip else (s["u_ref"], vc.RELAX)
    with _engine(pkg, name) as b:
        _enable(b, name, log_cap=1, every=1000, u_ref=u_ref, relax=relax)   # no scheduled update in 20 steps
        b.step(20, tau, u0)
        b.far_vortex_update()
        fx, fy, _, _ = b.forces()
        log = b.far_vortex_log()
        got_s, got_q = b.far_vortex()
        tables = b.read_far_profile()
        with pytest.raises(pkg.WTError) as ei:                              # the log is full
            b.far_vortex_update()
        assert ei.value.code == WT_ERR_STATE
    assert list(log["step"]) == [20] and log["fx"].shape == (1, B)
    assert _same(log["fx"][0], fx) and _same(log["fy"][0], fy) and np.abs(fx).min() > 0
    want_s, want_q, clipped = vortex_update(np.zeros(B), np.zeros(B), fx, fy, s["alpha"], u_ref, relax, s["bound"], norm="sqrt")
    print(name, clip, want_s, want_q, clipped)
    assert _same(log["strength"][0], want_s) and _same(log["source"][0], want_q) and _same(got_s, want_s) and _same(got_q, want_q)
    assert list(log["clipped"][0]) == list(clipped) == [clip] * B            # every member has a body
    if clip:
        assert (np.abs(np.sqrt(got_s * got_s + got_q * got_q) / s["bound"] - VORTEX_SPEED_MAX) <= 1e-15).all()
    for got, want in zip(tables, pc.stack(vc.tables(name, want_s, want_q))):
        assert bits_equal(got, want), name


# ---- 3. a whole run against the host loop ------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("96x48-f32", ""), ("24x140-f64", ""), ("96x48-f32", VARIANT)])
def test_a_run_on_the_device_schedule_is_the_host_loops(pkg, name, variant):
    dev, host = _device_run(name, variant), _host_run(name, variant)
    assert not any(u[5].any() for u in host["updates"])                      # else the comparison is not defined
    assert [u[0] for u in host["updates"]] == vc.UPDATE_STEPS and list(dev["log"]["step"]) == vc.UPDATE_STEPS
    _assert_same_run(dev, host, (name, variant))
    assert list(dev["history"]["step"]) == list(range(SAMPLE_EVERY, STEPS + 1, SAMPLE_EVERY))
    for r, (_, fx, fy, strength, source, _) in enumerate(host["updates"]):
        for k, want in (("fx", fx), ("fy", fy), ("strength", strength), ("source", source)):
            assert _same(dev["log"][k][r], want), (name, variant, r, k)
    assert not dev["log"]["clipped"].any()
    assert _same(dev["vortex"][0], host["vortex"][0]) and _same(dev["vortex"][1], host["vortex"][1])
    # not vacuous: the same run with the uniform profile throughout is another state
    tau, u0, _, _ = pc.params(name)
    with _engine(pkg, name, variant) as b:
        b.set_far_profile(*pc.stack(pc.tables_of(name, "uniform")))
        b.step(STEPS, tau, u0)
        for m in range(b.members):
            assert not bits_equal(b.read_f(m), dev["f"][m]), (name, variant, m)


# ---- 4. the schedule ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["96x48-f32", "24x140-f64"])
def test_call_boundaries_do_not_move_the_schedule(pkg, name):
    one, split, host = _device_run(name), _device_run(name, "", (5, 7, 48)), _host_run(name)
    _assert_same_run(split, one, name)
    for k in one["log"]:
        assert _same(split["log"][k], one["log"][k]), (name, k)
    assert split["log"]["step"].min() >= AFTER and list(split["log"]["step"]) == vc.UPDATE_STEPS
    both = [n for n in vc.UPDATE_STEPS if n % SAMPLE_EVERY == 0]              # steps that sample and update: the sample comes first
    assert both == [16, 24, 32, 40, 48, 56]
    rows = [list(split["history"]["step"]).index(n) for n in both]
    for k in ("fx", "fy", "surf", "rev"):
        assert _same(split["history"][k][rows], host["history"][k][rows]), (name, k)
    # the sample of step 16 precedes the update of step 16: it is the force the update read
    assert _same(split["history"]["fx"][rows[0]], split["log"]["fx"][0]) and _same(split["history"]["fy"][rows[0]], split["log"]["fy"][0])


def test_a_log_that_is_too_small_refuses_the_call(pkg):
    name = "96x48-f32"
    tau, u0, _, _ = pc.params(name)
    with _engine(pkg, name, history_cap=STEPS // SAMPLE_EVERY) as b:
        _enable(b, name, log_cap=2)
        b.step(10, tau, u0, sample_every=SAMPLE_EVERY)
        held = b.history()
        with pytest.raises(pkg.WTError) as ei:                              # steps 11 .. 60 hold six updates
            b.step(STEPS - 10, tau, u0, sample_every=SAMPLE_EVERY)
        assert ei.value.code == WT_ERR_STATE and "log" in str(ei.value)
        assert b.step_count == 10 and list(b.history()["step"]) == list(held["step"]) == [4, 8]
        assert b.far_vortex_log()["step"].size == 0
        b.step(14, tau, u0, sample_every=SAMPLE_EVERY)                      # two updates fit: steps 16 and 24
        assert list(b.far_vortex_log()["step"]) == [16, 24] and b.step_count == 24
        one = _device_run(name)
        assert _same(b.far_vortex_log()["strength"], one["log"]["strength"][:2])
        b.clear_history()                                                   # empties the log too
        assert b.far_vortex_log()["step"].size == 0
        b.step(16, tau, u0, sample_every=SAMPLE_EVERY)
        assert list(b.far_vortex_log()["step"]) == [32, 40]
        assert _same(b.far_vortex_log()["strength"], one["log"]["strength"][2:4])


# ---- 5. errors and switches --------------------------------------------------------------------
def test_errors_leave_the_batch_working(pkg):
    name = "96x48-f32"
    nx, ny, dtype, B = pc.lattice(name)
    tau, u0, _, _ = pc.params(name)
    s = vc.settings(name)
    good = dict(every=EVERY, after=AFTER, relax=vc.RELAX, u_ref=s["u_ref"], with_source=True, xc=s["xc"], yc=s["yc"], u_far=s["u_far"],
                v_far=s["v_far"], alpha=s["alpha"], log_cap=len(vc.UPDATE_STEPS))
    nan, inf = float("nan"), float("inf")
    bad = [dict(every=-1), dict(after=-1), dict(relax=0.0), dict(relax=1.5), dict(relax=nan), dict(u_ref=0.0), dict(u_ref=inf), dict(u_ref=nan),
           dict(xc=nan), dict(yc=inf), dict(xc=1.2), dict(yc=1.0), dict(yc=ny - 1.0), dict(log_cap=-1), dict(u_far=[0.2, 0.2, 0.2], v_far=[0.2, 0.0, 0.0]),
           dict(u_far=[0.05, nan, 0.05]), dict(v_far=[0.0, 0.0, inf]), dict(alpha=[0.0, nan, 0.0])]
    with _engine(pkg, name, history_cap=STEPS // SAMPLE_EVERY) as b:
        with pytest.raises(pkg.WTError) as ei:                              # before the first enable
            b.far_vortex()
        assert ei.value.code == WT_ERR_STATE
        for call in (b.far_vortex_update, lambda: b.set_far_vortex(0.0, 0.0)):
            with pytest.raises(pkg.WTError) as ei:
                call()
            assert ei.value.code == WT_ERR_STATE
        b.enable_far_vortex(**good)
        for change in bad:
            with pytest.raises(pkg.WTError) as ei:
                b.enable_far_vortex(**{**good, **change})
            assert ei.value.code == WT_ERR_ARG, change
            assert b.far_vortex_enabled
        lib, dp = b._lib, ctypes.POINTER(ctypes.c_double)
        p = np.zeros(B).ctypes.data_as(dp)
        assert lib.wtp_enable_far_vortex(b._b, 8, 16, 0.3, 0.08, 2, s["xc"], s["yc"], p, p, p, p, 4) == WT_ERR_ARG          # with_source is 0 or 1
        assert lib.wtp_enable_far_vortex(b._b, 8, 16, 0.3, 0.08, 1, s["xc"], s["yc"], p, None, p, p, 4) == WT_ERR_ARG       # a null pointer
        assert lib.wtp_set_far_vortex(b._b, p, None) == WT_ERR_ARG and lib.wtp_far_vortex(b._b, None, p) == WT_ERR_ARG
        assert lib.wtp_far_vortex_log(b._b, 0, 1, None, None, None, None, None, None) == WT_ERR_ARG                           # no row is held
        for pair in ((0.1 * s["bound"] * 1.01, 0.0), (0.0, -0.11 * s["bound"]), (nan, 0.0), (0.0, inf)):
            with pytest.raises(pkg.WTError) as ei:
                b.set_far_vortex([0.0, pair[0], 0.0], [0.0, pair[1], 0.0])
            assert ei.value.code == WT_ERR_ARG, pair
        tabs = pc.stack(pc.tables_of(name, "uniform"))
        with pytest.raises(pkg.WTError) as ei:                              # the device owns the tables
            b.set_far_profile(*tabs)
        assert ei.value.code == WT_ERR_STATE
        b.step(STEPS, tau, u0, sample_every=SAMPLE_EVERY)                   # after every refusal: the settings last accepted
        got = _result(b)
        got_log = b.far_vortex_log()
    one = _device_run(name)
    _assert_same_run(got, one, "after the refusals")
    for k in one["log"]:
        assert _same(got_log[k], one["log"][k]), k
    with pkg.PolarEngine(nx, ny, B, storage="half") as b:                   # a half batch
        b.set_masks(pc.masks_of(name))
        b.init_equilibrium(u0)
        with pytest.raises(pkg.WTError) as ei:
            b.enable_far_vortex(**good)
        assert ei.value.code == WT_ERR_STATE and not b.far_vortex_enabled
        b.step(4, tau, u0)
    with pkg.PolarEngine(nx, ny, B) as b:                                   # without the profile on
        b.set_masks(pc.masks_of(name))
        b.init_equilibrium(u0)
        with pytest.raises(pkg.WTError) as ei:
            b.enable_far_vortex(**good)
        assert ei.value.code == WT_ERR_STATE
        with pytest.raises(pkg.WTError) as ei:
            b.read_far_profile()
        assert ei.value.code == WT_ERR_STATE
        b.enable_far_profile()
        with pytest.raises(pkg.WTError) as ei:                              # no member has a profile
            b.read_far_profile()
        assert ei.value.code == WT_ERR_STATE


def test_switching_off_leaves_a_profile_batch(pkg):
    name = "96x48-f32"
    tau, u0, _, _ = pc.params(name)
    with _engine(pkg, name) as a:
        _enable(a, name, log_cap=4)
        a.step(24, tau, u0)                                                 # updates behind steps 16 and 24
        assert list(a.far_vortex_log()["step"]) == [16, 24]
        tables = a.read_far_profile()
        f24 = [a.read_f(m) for m in range(a.members)]
        a.enable_far_vortex(0, 0, 0.0, 0.0, False, 0.0, 0.0, 0.0, 0.0)       # off: the other arguments are not read
        assert not a.far_vortex_enabled and a.far_profile_enabled
        a.step(20, tau, u0)                                                 # would have updated behind steps 32 and 40
        assert list(a.far_vortex_log()["step"]) == [16, 24]
        for got, want in zip(a.read_far_profile(), tables):
            assert bits_equal(got, want)
        a.set_far_profile(*tables)                                          # the host owns the tables again
        with _engine(pkg, name) as b:                                       # a batch given those tables by hand, from the same state
            for m in range(b.members):
                b.write_f(m, f24[m])
            b.set_step_count(24)
            b.set_far_profile(*tables)
            b.step(20, tau, u0)
            for m in range(b.members):
                assert bits_equal(a.read_f(m), b.read_f(m)), m
                assert all(bits_equal(x, y) for x, y in zip(a.read_macro(m), b.read_macro(m))), m
            _enable(b, name, log_cap=2)
            b.write_f(0, f24[0])
            with pytest.raises(pkg.WTError) as ei:                          # the macroscopic planes are stale
                b.far_vortex_update()
            assert ei.value.code == WT_ERR_STATE and b.far_vortex_log()["step"].size == 0
            b.step(1, tau, u0)
            b.far_vortex_update()
            assert list(b.far_vortex_log()["step"]) == [45]


# ---- 6. run_polar -------------------------------------------------------------------------------
# vortex_relax: the impulsive start of these 64 to 88 steps has pressure forces near 1, whose target induces 0.11 at the bound (23.5 cells,
# u0 = 0.06); at the default 0.3 eleven updates would come within a few per cent of the clip, at 0.05 they reach less than half of it.
RUN = dict(shape="naca2412", nx=96, ny=48, frame="wind", far_field="vortex+source", sample_every=4, vortex_every=8, vortex_after=16,
           vortex_relax=0.05)
ALPHAS = [2.0, 4.0, 6.0]


def _assert_same_polar(a, b, what):
    assert not a.vortex_history["clipped"].any() and not b.vortex_history["clipped"].any(), what
    for m, (p, q) in enumerate(zip(a.points, b.points)):
        assert sorted(p.history) == sorted(q.history)
        for k in p.history:
            assert _same(p.history[k], q.history[k]), (what, m, k)
        assert (p.vortex_strength, p.vortex_source) == (q.vortex_strength, q.vortex_source), (what, m)
    assert sorted(a.vortex_history) == sorted(b.vortex_history) == ["clipped", "fx", "fy", "source", "step", "strength"]
    for k in a.vortex_history:
        assert _same(a.vortex_history[k], b.vortex_history[k]), (what, k)


def _assert_same_state(a, b, what):
    assert sorted(a) == sorted(b) and a["steps"] == b["steps"], what
    assert bits_equal(a["f"], b["f"]), what
    for k in ("left", "bottom", "top"):
        assert bits_equal(a["far_profile"][k], b["far_profile"][k]), (what, k)
    for k in ("strength", "source"):
        assert _same(a["vortex"][k], b["vortex"][k]), (what, k)


def test_run_polar_on_the_device_is_run_polar_on_the_host(pkg):
    kw = dict(warmup_steps=40, samples=6, keep_state=True, **RUN)            # 64 steps
    host = pkg.run_polar(ALPHAS, vortex_on="host", **kw)
    dev = pkg.run_polar(ALPHAS, vortex_on="device", **kw)
    assert list(dev.vortex_history["step"]) == [16, 24, 32, 40, 48, 56, 64] and dev.far_field == "vortex+source"
    assert all(p.vortex_strength > 0 for p in dev.points)
    _assert_same_polar(dev, host, "64 steps")
    _assert_same_state(dev.state, host.state, "64 steps")
    # continued from the state: the two runs together are one run of the combined length
    two = pkg.run_polar(ALPHAS, vortex_on="device", samples=6, start=dev.state, keep_state=True, **RUN)
    both = pkg.run_polar(ALPHAS, vortex_on="device", warmup_steps=40, samples=12, keep_state=True, **RUN)
    assert list(two.vortex_history["step"]) == [72, 80, 88]
    for m in range(len(ALPHAS)):
        for k in ("step", "fx", "fy", "surf", "rev", "mz"):
            joined = np.concatenate([dev.points[m].history[k], two.points[m].history[k]])
            assert _same(joined, both.points[m].history[k]), (m, k)
    for k in both.vortex_history:
        assert _same(np.concatenate([dev.vortex_history[k], two.vortex_history[k]]), both.vortex_history[k]), k
    _assert_same_state(two.state, both.state, "continued")
    # a total that is no multiple of vortex_every: the last row is the explicit final update
    kw = dict(warmup_steps=40, samples=7, keep_state=True, **RUN)            # 68 steps
    host, dev = pkg.run_polar(ALPHAS, vortex_on="host", **kw), pkg.run_polar(ALPHAS, vortex_on="device", **kw)
    assert list(dev.vortex_history["step"]) == [16, 24, 32, 40, 48, 56, 64, 68]
    _assert_same_polar(dev, host, "68 steps")
    _assert_same_state(dev.state, host.state, "68 steps")
