"""GPU: the wall velocity of batched sweeps (k_step_batch with WALL_MOVING, k_mex_batch with LinkMoving, wtp_enable_wall_velocity,
wtp_set_wall_velocity) against its definition in NumPy (tests/_wallvel_reference.py).

There is no tolerance on the state: the kernel and the reference round every operation of the wall rule once, in the same order, so
populations and macroscopic fields are compared with np.array_equal.  The momentum exchange is held to _ibb_reference.MexIbb's bounds.
The sensitivity check at the end of the matrix section runs on the references alone, without a GPU.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import lbm_numpy
import _half_reference as half
import _ibb_reference as ibb
import _les_reference as les
import _many_cases as mc
import _many_model_cases as mm
import _profile_reference as prof
import _wallvel_reference as wv
from _mex_reference import link_masks

gpu = pytest.mark.gpu

WT_ERR_ARG, WT_ERR_STATE = -1, -5
MEMBERS = (0, 1, 2)
CALLS = (1, 4, 3)
EVERY = 8
NAMES = ("67-24x300-f32", "35-24x140-f64")                  # one whole tile and a ragged one; below one tile
FARS = ("axial", "wind", "profile")
RUNS = [(name, lesq, trt, far) for name in NAMES for lesq, trt, far in itertools.product((False, True), (False, True), FARS)]


def _run_id(run):
    name, lesq, trt, far = run
    return "+".join(["les"] * lesq + ["trt"] * trt + [far]) + "-" + name.split("-")[-1]


@functools.lru_cache(maxsize=None)
def _velocities(name):
    """[3][8][NY][NX] of the case's dtype, read-only: within +-0.05 on the links of each member's mask and +-0.5 everywhere else, so that
    a kernel that reads an entry that is no link shows."""
    nx, ny, dtype, *_ = mc.CASES[name]
    mem = mc.members(name)
    rng = np.random.default_rng((9127, NAMES.index(name)))
    out = []
    for m in MEMBERS:
        links = np.stack(link_masks(mem.masks[m])[1:])
        on = rng.uniform(-0.05, 0.05, links.shape)
        off = np.where(rng.random(links.shape) < 0.5, -0.5, 0.5)
        out.append(np.where(links, on, off).astype(dtype))
        assert int(links.sum()) > 100 and (np.abs(out[-1][links]) <= 0.05).all() and (np.abs(out[-1][~links]) == 0.5).all()
    un = np.stack(out)
    un.setflags(write=False)
    return un


def _advance(run, m, state, steps, un):
    """`steps` steps of member m's reference under the run's models with the velocity planes `un`."""
    name, lesq, trt, far = run
    mem = mc.members(name)
    dtype = np.dtype(mc.CASES[name][2])
    tau, u0, cs, v0 = mem.params(m)
    extra = (mem.q[m], un, les.les_constant(cs, dtype) if lesq else None, float(mm.magic(name)[m]) if trt else None)
    out = None
    for _ in range(steps):
        if far == "profile":
            out = prof.profile_step(wv.step, state, mem.masks[m], tau, u0, mm.tables(name, m), *extra)
        elif far == "wind":
            out = half.windy(wv.step)(state, mem.masks[m], tau, u0, v0, *extra)
        else:
            out = wv.step(state, mem.masks[m], tau, u0, *extra)
        state = out[0]
    return mc.frozen(out)


@functools.lru_cache(maxsize=None)
def _reference(run, swapped=False):
    """{step: [(f, (rho, ux, uy)) of members 0..2]} after each call.  swapped: the planes of direction opp(k) in the place of k."""
    name = run[0]
    marks = [int(v) for v in np.cumsum(CALLS)]
    out = {mark: [] for mark in marks}
    for m in MEMBERS:
        un = _velocities(name)[m]
        if swapped:
            un = wv.opposite_planes(un)
        state, done = mm.start(name, m), 0
        for mark in marks:
            state, macro = _advance(run, m, state, mark - done, un)
            done = mark
            out[mark].append((state, macro))
    return out


def _assert_member(b, m, want, what):
    f, macro = want
    assert np.array_equal(b.read_f(m), f), what
    for got, ref, field in zip(b.read_macro(m), macro, ("rho", "ux", "uy")):
        assert np.array_equal(got, ref), (what, field)


def _moving_batch(pkg, name, **kw):
    """A batch of members 0..2 of the case with interpolated walls, their wall distances, the model on and their velocity planes."""
    nx, ny, dtype, *_ = mc.CASES[name]
    mem, B = mc.members(name), len(MEMBERS)
    b = pkg.PolarEngine(nx, ny, B, dtype=dtype, **kw)
    b.set_masks(mem.masks[:B])
    b.enable_interpolated_walls()
    b.set_wall_distances(mem.q[:B])
    b.enable_wall_velocity()
    b.set_wall_velocity(_velocities(name))
    return b


def _start(b, name):
    mem, B = mc.members(name), len(MEMBERS)
    b.init_equilibrium(mem.u0[:B])
    for m in MEMBERS:
        b.write_f(m, mm.start(name, m))


# ---- 1. bit identity on the step matrix ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("run", RUNS, ids=[_run_id(r) for r in RUNS])
def test_every_moving_wall_variant_is_its_reference(pkg, run):
    name, lesq, trt, far = run
    mem, B = mc.members(name), len(MEMBERS)
    want = _reference(run)
    with _moving_batch(pkg, name, history_cap=2) as b:
        assert b.wall_velocity_enabled and b.interpolated_walls
        if lesq:
            b.enable_les(mem.cs[:B])
        if far == "wind":
            b.enable_wind(mem.v0[:B])
        if trt:
            b.enable_trt(mm.magic(name)[:B])
        if far == "profile":
            b.enable_far_profile()
            b.set_far_profile(*mm.stacked_tables(name, MEMBERS))
        _start(b, name)
        done = 0
        for n in CALLS:
            b.step(n, mem.tau[:B], mem.u0[:B], sample_every=EVERY)
            done += n
            for m in MEMBERS:
                _assert_member(b, m, want[done][m], (_run_id(run), "step", done, "member", m))
        assert list(b.history()["step"]) == [EVERY]


@pytest.mark.parametrize("run", RUNS, ids=[_run_id(r) for r in RUNS])
def test_the_matrix_inputs_tell_direction_k_from_its_opposite(run):
    """On the references alone: with the planes of direction opp(k) handed over in the place of k every run computes another state, and so
    does every run with the interpolating rule alone."""
    want, other = _reference(run), _reference(run, swapped=True)
    last = max(want)
    for m in MEMBERS:
        assert not np.array_equal(want[last][m][0], other[last][m][0]), m
    name = run[0]
    mem = mc.members(name)
    for m in MEMBERS:
        at_rest = _advance(run, m, mm.start(name, m), 1, np.zeros_like(mem.q[m]))
        assert not np.array_equal(at_rest[0], want[1][m][0]), m


# ---- 2. zero planes and switching ------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", NAMES)
def test_zero_planes_and_switching_off_are_interpolated_walls(pkg, name):
    nx, ny, dtype, *_ = mc.CASES[name]
    mem, B = mc.members(name), len(MEMBERS)
    tau, u0 = mem.tau[:B], mem.u0[:B]
    with pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=4) as a, pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=4) as b:
        for e in (a, b):
            e.set_masks(mem.masks[:B])
            e.enable_interpolated_walls()
            e.set_wall_distances(mem.q[:B])
            _start(e, name)
        a.enable_wall_velocity()                                            # on, every plane +0
        for e in (a, b):
            e.step(5, tau, u0, sample_every=4)
        for m in MEMBERS:
            assert np.array_equal(a.read_f(m), b.read_f(m)), m
            assert all(np.array_equal(x, y) for x, y in zip(a.read_macro(m), b.read_macro(m))), m
        a.set_wall_velocity(_velocities(name))
        a.enable_wall_velocity(False)                                       # the planes are kept and not read
        assert not a.wall_velocity_enabled and a.interpolated_walls
        for e in (a, b):
            e.step(4, tau, u0, sample_every=4)
        state = []
        for m in MEMBERS:
            state.append(a.read_f(m))
            assert np.array_equal(state[m], b.read_f(m)), m
            assert all(np.array_equal(x, y) for x, y in zip(a.read_macro(m), b.read_macro(m))), m
        ha, hb = a.history(), b.history()
        assert list(ha["step"]) == list(hb["step"]) == [4, 8]
        for k in ("fx", "fy", "surf", "rev"):
            assert ha[k].tobytes() == hb[k].tobytes(), k
        a.enable_wall_velocity()                                            # on again: the planes kept their values
        a.step(3, tau, u0)
        b.step(3, tau, u0)
        run = (name, False, False, "axial")
        for m in MEMBERS:
            _assert_member(a, m, _advance(run, m, state[m], 3, _velocities(name)[m]), ("on again", m))
            assert not np.array_equal(a.read_f(m), b.read_f(m)), m
        a.enable_interpolated_walls(False)                                  # switches the wall velocity off too
        assert not a.wall_velocity_enabled and not a.interpolated_walls
        state = [a.read_f(m) for m in MEMBERS]
        a.step(2, tau, u0)
        for m in MEMBERS:
            assert np.array_equal(a.read_f(m), lbm_numpy.run(mem.masks[m], 2, tau[m], u0[m], np.dtype(dtype), f=state[m])[0]), m
        with pytest.raises(pkg.WTError) as ei:                              # and it needs them again
            a.enable_wall_velocity()
        assert ei.value.code == WT_ERR_STATE


# ---- 3. circular Couette flow on the device --------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_couette_members_are_the_reference(pkg, dtype):
    """Three members: the inner wall turning with +omega, with -omega, and at rest.  Every member is bit-identical to the reference.  The
    resting member keeps (1, 0, 0) up to rounding: the rest state is a fixed point of the exact step, and a step's roundings move a
    moment by at most 12 eps (nine populations of at most 4/9, at most six roundings of eps/2 each on a link), 1000 steps at most by
    12 000 eps; the reference itself drifts by 8.3e-7 in rho and 1.5e-7 in the velocity in fp32, 3.1e-14 and 9.3e-16 in fp64."""
    C = wv.COUETTE
    n, mask, signs = C["n"], wv.couette_mask(), (+1, -1, 0)
    q = wv.couette_q(mask)
    with pkg.PolarEngine(n, n, 3, dtype=dtype) as b:
        b.set_masks(np.stack([mask] * 3))
        b.enable_interpolated_walls()
        b.set_wall_distances(np.stack([q] * 3))
        b.enable_wall_velocity()
        b.set_wall_velocity(np.stack([wv.couette_un(s) for s in signs[:2]]))     # the third member keeps its +0
        b.init_equilibrium(0.0)
        b.step(C["steps"], C["tau"], 0.0)
        for m, s in enumerate(signs):
            _assert_member(b, m, wv.couette_run(dtype, s), ("couette", dtype, s))
        rho, ux, uy = b.read_macro(2)
        turn = b.read_macro(0)
    omega = C["rim"] / C["r1"]
    err = wv.couette_error(mask, turn[1], turn[2], omega)
    print(f"couette on the device, {dtype}: relative L2 error {err:.4g}")
    assert err <= 1e-2
    bound = 12 * C["steps"] * float(np.finfo(dtype).eps)
    fluid = mask == 0
    assert np.abs(rho[fluid] - 1).max() <= bound and np.abs(ux[fluid]).max() <= bound and np.abs(uy[fluid]).max() <= bound
    assert (rho[~fluid] == 1).all() and (ux[~fluid] == 0).all() and (uy[~fluid] == 0).all()


# ---- 4. the momentum exchange ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", NAMES)
def test_momentum_exchange_uses_the_moving_wall_term(pkg, name):
    nx, ny, dtype, *_ = mc.CASES[name]
    mem, B = mc.members(name), len(MEMBERS)
    xr, yr = mem.xref[:B], mem.yref[:B]
    fs, on_demand = [], []
    with _moving_batch(pkg, name, history_cap=2) as b:
        b.enable_momentum_exchange(xr, yr)
        _start(b, name)
        for _ in range(2):
            b.step(EVERY, mem.tau[:B], mem.u0[:B], sample_every=EVERY)
            on_demand.append(b.momentum_exchange())
            fs.append([b.read_f(m) for m in MEMBERS])
        h = b.history()
    worst = [0.0, 0.0, 0.0]
    for r in range(2):
        for m in MEMBERS:
            ref = wv.mex_reference(fs[r][m], mem.masks[m], mem.q[m], _velocities(name)[m], xr[m], yr[m])
            assert ref.links == int(h["links"][r, m]) == int(on_demand[r][3][m]) > 100
            rows = ((h["fx_mex"][r, m], on_demand[r][0][m], ref.fx, ref.fx_bound), (h["fy_mex"][r, m], on_demand[r][1][m], ref.fy, ref.fy_bound),
                    (h["mz_mex"][r, m], on_demand[r][2][m], ref.mz, ref.mz_bound))
            for k, (row, call, want, bound) in enumerate(rows):
                assert row.tobytes() == call.tobytes(), (r, m, k)               # a history row is wtp_mex on that lattice
                err = abs(float(row) - want)
                worst[k] = max(worst[k], err / bound)
                assert err <= bound, (r, m, k, float(row), want, bound)
            resting = ibb.mex_reference(fs[r][m], mem.masks[m], mem.q[m], xr[m], yr[m])     # and it is not the term of a wall at rest
            assert abs(resting.fx - ref.fx) > 1e3 * ref.fx_bound and abs(resting.mz - ref.mz) > 1e3 * ref.mz_bound, (r, m)
    print(f"{name}: worst |x - ref| / bound: fx {worst[0]:.3g}, fy {worst[1]:.3g}, mz {worst[2]:.3g}")


# ---- 5. a velocity belongs to a mask ---------------------------------------------------------------
@gpu
def test_set_masks_zeroes_the_velocities_of_the_members_it_touches_and_no_others(pkg):
    name = NAMES[0]
    mem, B = mc.members(name), len(MEMBERS)
    run = (name, False, False, "axial")
    with _moving_batch(pkg, name) as b:
        b.set_masks(mem.masks[1], first=1)                                  # the same mask again: member 1's distances and velocities are gone
        b.set_wall_distances(mem.q[1], first=1)                             # ... the distances come back
        _start(b, name)
        b.step(3, mem.tau[:B], mem.u0[:B])
        for m in MEMBERS:
            un = np.zeros_like(mem.q[m]) if m == 1 else _velocities(name)[m]
            _assert_member(b, m, _advance(run, m, mm.start(name, m), 3, un), ("after set_masks", m))
        assert not np.array_equal(b.read_f(1), _advance(run, 1, mm.start(name, 1), 3, _velocities(name)[1])[0])
        b.set_wall_velocity(_velocities(name)[1], first=1)                  # one member's velocities, by its index
        state = [b.read_f(m) for m in MEMBERS]
        b.step(2, mem.tau[:B], mem.u0[:B])
        for m in MEMBERS:
            _assert_member(b, m, _advance(run, m, state[m], 2, _velocities(name)[m]), ("after set_wall_velocity", m))


# ---- 6. error paths --------------------------------------------------------------------------------
@gpu
def test_error_paths_leave_a_working_batch(pkg):
    name = NAMES[0]
    nx, ny, dtype, *_ = mc.CASES[name]
    mem, B = mc.members(name), len(MEMBERS)
    un = _velocities(name)
    vp = ctypes.c_void_p
    run = (name, False, False, "axial")
    with pkg.PolarEngine(nx, ny, B, dtype=dtype) as b:
        b.set_masks(mem.masks[:B])
        with pytest.raises(pkg.WTError) as ei:                              # enabling without interpolated walls
            b.enable_wall_velocity()
        assert ei.value.code == WT_ERR_STATE and "wtp_enable_ibb" in str(ei.value) and not b.wall_velocity_enabled
        b.enable_interpolated_walls()
        b.set_wall_distances(mem.q[:B])
        with pytest.raises(pkg.WTError) as ei:                              # setting before the first enable
            b.set_wall_velocity(un)
        assert ei.value.code == WT_ERR_STATE and "wtp_enable_wall_velocity" in str(ei.value)
        b.enable_wall_velocity()
        b.set_wall_velocity(un)
        for bad in (0.5000001, -0.5000001, float("nan"), float("inf")):
            wrong = un.copy()
            wrong[2, 5, 7, 9] = bad                                         # one value, in the last member
            with pytest.raises(pkg.WTError) as ei:
                b.set_wall_velocity(wrong)
            assert ei.value.code == WT_ERR_ARG and "member 2" in str(ei.value), bad
        for first, count in ((-1, 1), (B, 1), (1, B), (0, 0)):
            assert b._lib.wtp_set_wall_velocity(b._b, first, count, un.ctypes.data_as(vp)) == WT_ERR_ARG, (first, count)
        assert b._lib.wtp_set_wall_velocity(b._b, 0, 1, None) == WT_ERR_ARG
        with pytest.raises(ValueError):
            b.set_wall_velocity(un[:, :4])
        assert b.wall_velocity_enabled
        _start(b, name)
        b.step(3, mem.tau[:B], mem.u0[:B])                                   # no refused call changed a velocity, of any member
        for m in MEMBERS:
            _assert_member(b, m, _advance(run, m, mm.start(name, m), 3, un[m]), ("after the refusals", m))
    with pkg.PolarEngine(nx, ny, B, dtype="float32", storage="half") as h:  # a half batch
        h.set_masks(mem.masks[:B])
        h.init_equilibrium(mem.u0[:B])
        with pytest.raises(pkg.WTError) as ei:
            h.enable_wall_velocity()
        assert ei.value.code == WT_ERR_STATE and "half" in str(ei.value)
        assert h._lib.wtp_set_wall_velocity(h._b, 0, 1, un.ctypes.data_as(vp)) == WT_ERR_STATE
        h.step(2, mem.tau[:B], mem.u0[:B])
        assert np.isfinite(h.read_f(0)).all()


# ---- 7. run_polar ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("frame", ["body", "wind"])
def test_run_polar_with_a_slot(pkg, frame):
    kw = dict(shape="naca2412", nx=96, ny=48, tau=0.6, warmup_steps=300, samples=4, total_forces=True, walls="interpolated", frame=frame)
    alphas = [2.0, 6.0]
    slot = {"surface": "upper", "x0": 0.3, "x1": 0.6, "vn": 0.2}
    blown = pkg.run_polar(alphas, slot=slot, **kw)
    still = pkg.run_polar(alphas, slot=dict(slot, vn=0.0), **kw)
    plain = pkg.run_polar(alphas, **kw)
    assert plain.slot is None and slot == {"surface": "upper", "x0": 0.3, "x1": 0.6, "vn": 0.2}
    assert {k: blown.slot[k] for k in slot} == slot and blown.slot["links"].shape == (2,) and (blown.slot["links"] > 4).all()
    assert (still.slot["links"] == 0).all()
    if frame == "wind":
        assert blown.slot["links"][0] == blown.slot["links"][1]
    for p, s, d in zip(blown.points, still.points, plain.points):
        print(f"{frame} alpha {p.alpha}: CL_total {p.cl_total_mean:.5f} (no slot {d.cl_total_mean:.5f}), CD_total {p.cd_total_mean:.5f} ({d.cd_total_mean:.5f})")
        assert p.samples == 4 and p.finite
        for k in ("fx", "fy", "surf", "rev", "fx_mex", "fy_mex"):           # a slot that does not blow is no slot, bit for bit
            assert s.history[k].tobytes() == d.history[k].tobytes(), k
        assert p.history["fx"].tobytes() != d.history["fx"].tobytes() and p.cl_total_mean != d.cl_total_mean
