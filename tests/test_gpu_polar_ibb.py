"""GPU: interpolated bounce-back of batched sweeps (k_step_batch with WALL_INTERP, k_mex_ibb_batch, wtp_enable_ibb, wtp_set_wall_q) against its
definition in NumPy (tests/_ibb_reference.py).

There is no tolerance on the state: the kernel and the reference round every operation of the wall rule once, in the same order, so
populations and macroscopic fields are compared with np.array_equal.  The momentum exchange is held to the summation bounds of
_mex_reference, widened as _ibb_reference.MexIbb derives for the roundings the interpolated term adds.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import bits_equal
import lbm_numpy
import _ibb_reference as ibb
import _les_reference as les
from _mex_reference import link_masks

pytestmark = pytest.mark.gpu

WT_ERR_ARG, WT_ERR_STATE = -1, -5
STEPS = 60
EVERY = 12

# Members: (tau, u0, cs); cs is used by the Smagorinsky variants only.  Member 0 of every case is an airfoil with its true wall
# distances, the others are random blobs with random distances.  The lattices are chosen by step_tile's classes: 96x48 has ragged tiles
# only; 40x300 and 37x299 fp32 a full tile of 256 rows and a ragged one per column (and an odd NY); 24x140 fp64 a full tile of 128
# rows and a ragged one.  The bodies sit in the full tiles and reach into the ragged ones.
MEMBERS = [(0.52, 0.08, 0.1), (0.9, 0.03, 0.0), (0.6, 0.05, 0.1)]
CASES = {
    "96x48-f32": (96, 48, "float32", ("naca2412", 6.0)),
    "40x300-f32": (40, 300, "float32", ("naca0012", 10.0)),
    "37x299-f32": (37, 299, "float32", ("naca4412", -4.0)),
    "24x140-f64": (24, 140, "float64", ("naca0012", 5.0)),
}


def _blob_mask(nx, ny, rng):
    """A body of random blobs with narrow gaps: a block cut by one-cell slots (cells with a wall on either side, where a short link
    has no fluid cell behind it), sprinkled with single solid cells, and a second sprinkle near the top, in the ragged tile of the
    tall lattices.  The border cells stay fluid."""
    mask = np.zeros((ny, nx), np.uint8)
    j0, i0 = ny // 2 - 9 + int(rng.integers(0, 5)), nx // 3 + int(rng.integers(0, 3))
    h, w = 17, max(7, nx // 4)
    mask[j0:j0 + h, i0:i0 + w] = 255
    mask[j0 + 4, i0:i0 + w - 2] = 0                                    # a horizontal slot, open upstream
    mask[j0 + 9:j0 + h, i0 + 3] = 0                                    # a vertical slot, open at the top
    mask[j0 + 12, i0 + 5:i0 + w] = 0                                   # and one open downstream
    for (ja, jb) in ((j0 - 5, j0 + h + 5), (ny - 11, ny - 2)):         # sprinkles: around the block, and near the top
        ja, jb = max(ja, 2), min(jb, ny - 2)
        band = rng.random((jb - ja, nx - 4)) < 0.12
        mask[ja:jb, 2:nx - 2][band] = 255
    mask[[0, 1, ny - 2, ny - 1], :] = 0
    mask[:, [0, 1, nx - 2, nx - 1]] = 0
    return mask


def _random_q(nx, ny, dtype, rng):
    """Wall distances drawn from (0, 1] in every entry (link or not: the others are never read), with exact 0.5, exact 1, values
    close to 0 and values either side of 0.5 among them."""
    q = 1.0 - rng.random((8, ny, nx))                                  # (0, 1]
    pick = rng.random(q.shape)
    q[pick < 0.10] = 0.5
    q[(pick >= 0.10) & (pick < 0.20)] = 1.0
    q[(pick >= 0.20) & (pick < 0.25)] = 2.0 ** -12
    q[(pick >= 0.25) & (pick < 0.30)] = np.nextafter(0.5, 0.0)
    q = q.astype(dtype)
    assert (q > 0).all() and (q <= 1).all()
    return q


@functools.lru_cache(maxsize=None)
def _setup(name):
    """(masks [B][NY][NX], q [B][8][NY][NX] of the case's dtype), read-only."""
    import airfoil_cfd_tool_amd as pkg
    nx, ny, dtype, (shape, alpha) = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 11)
    g = pkg.geometry.build_geometry(nx, ny, alpha, None, shape)
    masks = [g.mask] + [_blob_mask(nx, ny, rng) for _ in MEMBERS[1:]]
    q = [pkg.geometry.wall_distances(g.xp, g.yp, g.mask, nx, ny).astype(dtype)] + [_random_q(nx, ny, dtype, rng) for _ in MEMBERS[1:]]
    masks, q = np.stack(masks), np.stack(q)
    masks.setflags(write=False)
    q.setflags(write=False)
    return masks, q


@functools.lru_cache(maxsize=None)
def _reference(name, with_les, steps=STEPS):
    """Per member: (f, (rho, ux, uy)) of _ibb_reference after `steps` steps from equilibrium."""
    nx, ny, dtype, _ = CASES[name]
    masks, q = _setup(name)
    out = []
    for m, (tau, u0, cs) in enumerate(MEMBERS):
        c = les.les_constant(cs, dtype) if with_les else None
        f, macro = ibb.run(masks[m], steps, tau, u0, q[m], c, np.dtype(dtype))
        for a in (f, *macro):
            a.setflags(write=False)
        out.append((f, macro))
    return out


def _params():
    return [m[0] for m in MEMBERS], [m[1] for m in MEMBERS], [m[2] for m in MEMBERS]


def _links_on_both_branches(mask, q):
    own = np.stack(link_masks(mask)[1:])
    return int(own.sum()), int((own & (q < 0.5)).sum()), int((own & (q > 0.5)).sum()), int((own & (q == 0.5)).sum()), int((own & (q == 1)).sum())


# ---- 1. bit identity, with either collision ----------------------------------------------------
@pytest.mark.parametrize("with_les", [False, True], ids=["bgk", "les"])
@pytest.mark.parametrize("name", list(CASES))
def test_state_is_the_references(pkg, name, with_les):
    nx, ny, dtype, _ = CASES[name]
    tau, u0, cs = _params()
    masks, q = _setup(name)
    ref = _reference(name, with_les)
    # the comparison is not vacuous, on the inputs and on the reference itself
    for m in range(len(MEMBERS)):
        n, below, above, half, one = _links_on_both_branches(masks[m], q[m])
        fallback = ibb.fallback_links(masks[m], q[m])
        print(f"{name} member {m}: {n} links, q < 0.5 at {below}, > 0.5 at {above}, = 0.5 at {half}, = 1 at {one}; {fallback} short links with a wall behind")
        assert n > 20 and below > 0 and above > 0
        if m > 0:
            assert half > 0 and one > 0 and fallback > 0          # the blob masks hold narrow gaps: the "x - e_k is solid" branch runs
        plain = lbm_numpy.run(masks[m], STEPS, tau[m], u0[m], np.dtype(dtype))[0]
        assert not np.array_equal(ref[m][0], plain)
        assert np.isfinite(ref[m][0]).all()
    with pkg.PolarEngine(nx, ny, len(MEMBERS), dtype=dtype) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        b.enable_interpolated_walls()
        b.set_wall_distances(q)
        if with_les:
            b.enable_les(cs)
        assert b.interpolated_walls
        b.step(STEPS, tau, u0)
        for m in range(len(MEMBERS)):
            f, macro = b.read_f(m), b.read_macro(m)
            want_f, want_macro = ref[m]
            bad = int((f != want_f).any(axis=(0, 2)).sum())
            assert f.dtype == want_f.dtype and np.array_equal(f, want_f), (name, m, bad, "rows differ")
            for got, want, what in zip(macro, want_macro, ("rho", "ux", "uy")):
                assert np.array_equal(got, want), (name, m, what)


# ---- 2. on, distances never set: a plain batch -------------------------------------------------
@pytest.mark.parametrize("name", ["96x48-f32", "24x140-f64"])
def test_model_on_with_no_distances_set_is_a_plain_batch(pkg, name):
    nx, ny, dtype, _ = CASES[name]
    tau, u0, _ = _params()
    masks, _ = _setup(name)
    B = len(MEMBERS)
    xr, yr = [0.3 * nx + m for m in range(B)], [0.5 * ny - m for m in range(B)]
    got = {}
    for on in (True, False):
        with pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=8) as b:
            b.set_masks(masks)
            b.init_equilibrium(u0)
            b.enable_momentum_exchange(xr, yr)
            if on:
                b.enable_interpolated_walls()
            assert b.interpolated_walls is on
            b.step(STEPS, tau, u0, sample_every=EVERY)
            got[on] = ([b.read_f(m) for m in range(B)], [b.read_macro(m) for m in range(B)], b.history(), b.clamp_events(),
                       b.momentum_exchange())
    (f1, m1, h1, c1, x1), (f0, m0, h0, c0, x0) = got[True], got[False]
    assert list(h1["step"]) == list(h0["step"]) == [EVERY * (k + 1) for k in range(STEPS // EVERY)]
    for m in range(B):
        assert bits_equal(f1[m], f0[m]), m
        assert all(bits_equal(a, c) for a, c in zip(m1[m], m0[m])), m
    for k in ("fx", "fy", "surf", "rev", "fx_mex", "fy_mex", "mz_mex", "links"):
        assert h1[k].tobytes() == h0[k].tobytes(), k
    assert all(a.tobytes() == c.tobytes() for a, c in zip(c1, c0))
    assert all(a.tobytes() == c.tobytes() for a, c in zip(x1, x0))
    assert int(h1["links"].min()) > 20


# ---- 3. off again ------------------------------------------------------------------------------
def test_switching_off_returns_to_half_way_and_keeps_the_history(pkg, oracle_np):
    name = "96x48-f32"
    nx, ny, dtype, _ = CASES[name]
    tau, u0, _ = _params()
    masks, q = _setup(name)
    B = len(MEMBERS)
    with pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=8) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        b.enable_interpolated_walls()
        b.set_wall_distances(q)
        b.step(24, tau, u0, sample_every=EVERY)
        first = b.history()
        at_switch = [b.read_f(m) for m in range(B)]
        b.enable_interpolated_walls(False)
        assert not b.interpolated_walls
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
            # and the first half was the model's: the state at the switch is the reference's, not the oracle's
            assert np.array_equal(at_switch[m], _reference(name, False, 24)[m][0])
            assert not np.array_equal(at_switch[m], oracle_np.run(masks[m], 24, tau[m], u0[m], np.float32)[0])
        # on again: the distances were kept
        b.enable_interpolated_walls()
        b.step(12, tau, u0)
        for m in range(B):
            assert np.array_equal(b.read_f(m), ibb.run(masks[m], 12, tau[m], u0[m], q[m], f=after[m])[0]), m


# ---- 4. a distance belongs to a mask -----------------------------------------------------------
def test_set_masks_resets_the_distances_of_the_members_it_touches_and_no_others(pkg):
    name = "40x300-f32"
    nx, ny, dtype, _ = CASES[name]
    tau, u0, _ = _params()
    masks, q = _setup(name)
    half = np.full_like(q[1], 0.5)
    with pkg.PolarEngine(nx, ny, len(MEMBERS), dtype=dtype) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        b.enable_interpolated_walls()
        b.set_wall_distances(q)
        b.set_masks(masks[1], first=1)                                      # the same mask again: member 1's distances are gone
        b.step(24, tau, u0)
        for m, qm in enumerate((q[0], half, q[2])):
            want = ibb.run(masks[m], 24, tau[m], u0[m], qm)[0]
            assert np.array_equal(b.read_f(m), want), m
        assert not np.array_equal(b.read_f(1), _reference(name, False, 24)[1][0])
        b.set_wall_distances(q[1], first=1)                                 # one member's distances, by its index
        state = [b.read_f(m) for m in range(len(MEMBERS))]
        b.step(12, tau, u0)
        for m in range(len(MEMBERS)):
            assert np.array_equal(b.read_f(m), ibb.run(masks[m], 12, tau[m], u0[m], q[m], f=state[m])[0]), m


# ---- 5. the momentum exchange ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["96x48-f32", "37x299-f32", "24x140-f64"])
def test_momentum_exchange_uses_the_interpolated_term(pkg, name):
    from _mex_reference import mex_reference as halfway_reference
    nx, ny, dtype, _ = CASES[name]
    tau, u0, _ = _params()
    masks, q = _setup(name)
    B, calls = len(MEMBERS), 3
    xr, yr = [0.3641 * nx + 1.7 * m for m in range(B)], [0.5 * ny - 0.85 * m - 3.3 for m in range(B)]
    fs, on_demand = [], []
    with pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=calls) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        b.enable_momentum_exchange(xr, yr)
        b.enable_interpolated_walls()
        b.set_wall_distances(q)
        for _ in range(calls):
            b.step(EVERY, tau, u0, sample_every=EVERY)
            on_demand.append(b.momentum_exchange())
            fs.append([b.read_f(m) for m in range(B)])
        h = b.history()
    worst = [0.0, 0.0, 0.0]
    for r in range(calls):
        for m in range(B):
            ref = ibb.mex_reference(fs[r][m], masks[m], q[m], xr[m], yr[m])
            assert ref.links == int(h["links"][r, m]) == int(on_demand[r][3][m]) > 20
            rows = ((h["fx_mex"][r, m], on_demand[r][0][m], ref.fx, ref.fx_bound), (h["fy_mex"][r, m], on_demand[r][1][m], ref.fy, ref.fy_bound),
                    (h["mz_mex"][r, m], on_demand[r][2][m], ref.mz, ref.mz_bound))
            for k, (row, call, want, bound) in enumerate(rows):
                assert row.tobytes() == call.tobytes(), (r, m, k)               # a history row is wtp_mex on that lattice
                err = abs(float(row) - want)
                worst[k] = max(worst[k], err / bound)
                assert err <= bound, (r, m, k, float(row), want, bound)
            # and it is not the half-way term on the same lattice
            plain = halfway_reference(fs[r][m], masks[m], xr[m], yr[m])
            assert abs(plain.fx - ref.fx) > 1e3 * ref.fx_bound and abs(plain.mz - ref.mz) > 1e3 * ref.mz_bound, (r, m)
    print(f"{name}: worst |x - ref| / bound: fx {worst[0]:.3g}, fy {worst[1]:.3g}, mz {worst[2]:.3g}")


# ---- 6. error paths ----------------------------------------------------------------------------
def test_error_paths_leave_the_batch_as_it_was(pkg):
    name = "96x48-f32"
    nx, ny, dtype, _ = CASES[name]
    tau, u0, _ = _params()
    masks, q = _setup(name)
    B = len(MEMBERS)
    vp = ctypes.c_void_p
    with pkg.PolarEngine(nx, ny, B, dtype=dtype) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        with pytest.raises(pkg.WTError) as ei:
            b.set_wall_distances(q)
        assert ei.value.code == WT_ERR_STATE and "wtp_enable_ibb" in str(ei.value)
        b.enable_interpolated_walls()
        b.set_wall_distances(q)
        for bad in (0.0, -0.25, float("nan"), np.nextafter(np.float32(1.0), np.float32(2.0)), float("inf")):
            wrong = q.copy()
            wrong[2, 5, 7, 9] = bad                                         # one value, in the last member
            with pytest.raises(pkg.WTError) as ei:
                b.set_wall_distances(wrong)
            assert ei.value.code == WT_ERR_ARG and "member 2" in str(ei.value), bad
        for first, count in ((-1, 1), (B, 1), (1, B), (0, 0)):
            assert b._lib.wtp_set_wall_q(b._b, first, count, q.ctypes.data_as(vp)) == WT_ERR_ARG, (first, count)
        assert b._lib.wtp_set_wall_q(b._b, 0, 1, None) == WT_ERR_ARG
        with pytest.raises(ValueError):
            b.set_wall_distances(q[:, :4])
        assert b.interpolated_walls
        b.step(24, tau, u0)                                                 # no refused call changed a distance, of any member
        for m in range(B):
            assert np.array_equal(b.read_f(m), _reference(name, False, 24)[m][0]), m


# ---- 7. run_polar ------------------------------------------------------------------------------
def test_run_polar_with_interpolated_walls(pkg):
    kw = dict(shape="naca2412", nx=96, ny=48, tau=0.6, warmup_steps=600, samples=8, total_forces=True)
    alphas = [2.0, 4.0, 6.0]
    curved = pkg.run_polar(alphas, walls="interpolated", **kw)
    stairs = pkg.run_polar(alphas, walls="staircase", **kw)
    default = pkg.run_polar(alphas, **kw)
    assert curved.walls == "interpolated" and stairs.walls == default.walls == "staircase"
    for p, s, d in zip(curved.points, stairs.points, default.points):
        print(f"alpha {p.alpha}: CL_total {p.cl_total_mean:.5f} (staircase {s.cl_total_mean:.5f}), CD_total {p.cd_total_mean:.5f} ({s.cd_total_mean:.5f})")
        assert p.converged and p.clamp_events == (0, 0) and p.samples == 8
        assert s.converged
        assert p.cl_total_mean != s.cl_total_mean and p.cd_total_mean != s.cd_total_mean and p.cl_mean != s.cl_mean
        assert p.cd_total_mean > 0
        for k in ("fx", "fy", "surf", "rev"):                              # the default is the staircase, bit for bit
            assert s.history[k].tobytes() == d.history[k].tobytes(), k
        assert (s.cl_total_mean, s.cd_total_mean, s.cm_total_mean) == (d.cl_total_mean, d.cd_total_mean, d.cm_total_mean)
    # ... and the staircase run is a batch stepped by hand without the model
    masks = np.stack([pkg.geometry.build_geometry(96, 48, a, None, "naca2412").mask for a in alphas])
    with pkg.PolarEngine(96, 48, 3, history_cap=8) as b:
        b.set_masks(masks)
        b.init_equilibrium(0.06)
        b.step(600, 0.6, 0.06)
        b.step(8 * 12, 0.6, 0.06, sample_every=12)
        h = b.history()
    for m, s in enumerate(stairs.points):
        assert s.history["fx"].tobytes() == h["fx"][:, m].tobytes() and s.history["fy"].tobytes() == h["fy"][:, m].tobytes()
