"""GPU: the marching kernels on windows that TILE the column (window_overlap = 0: halo lines built per pass by k_halo3 / k_halo4, seam records
and seam flags, units cut by columns or by measured time with chain blocks) on ragged lattices, bit for bit against the C oracle.

Since overlapping windows became the automatic choice for fp32 lattices of up to 7.5 M sites, the other tests run fp32 depth-3 / 4 passes on
ragged shapes on overlapping windows: here tiling windows are forced, with heights that hug the window size (a last window of a few rows, seam
rows next to the first / last row), solids on the rows next to every seam, bodies on the inlet and outlet columns inside the march, all three
division forms, the automatic plan on both sides of the size threshold, and the readouts on the ragged states those runs leave."""
import numpy as np
import pytest

from conftest import bits_equal
from lbm_numpy import clamp_events

pytestmark = pytest.mark.gpu

WIN = {"float32": 128, "float64": 64}          # rows of a tiling window: 64 lanes x 2 sites (fp32), x 1 site (fp64)
VORT_SCALE = 0.06                               # html:528
FORMS = (("float32", 2), ("float32", 3), ("float32", 4), ("float64", 3), ("float64", 4))
CLAMP_SEED = 13                                 # tau 0.5004, U0 0.10: long enough to reach the stability net
THRESHOLD = 7_500_000                           # sites: fp32 lattices up to this size plan overlapping windows by default


def _seams(ny, win):
    return [b * win for b in range(1, (ny + win - 1) // win)]


def _height(rng, seed):
    """Heights that hug the window size: a last window of 126, 128, 2 or 6 rows (fp32; the same offsets from a 64-row seam for fp64),
    one of 2 rows for fp64 only (an odd multiple of 64, plus 2), or a random even height."""
    kind = seed % 6
    if kind < 4:
        return int(rng.integers(2, 9)) * WIN["float32"] + (-2, 0, 2, 6)[kind]
    if kind == 4:
        return int(2 * rng.integers(1, 8) + 1) * WIN["float64"] + 2
    return 2 * int(rng.integers(8, 551))


def _width(rng, seed):
    kind = seed % 4
    if kind == 0:
        return int(rng.integers(16, 41))                                    # narrow
    if kind == 3:
        return int(rng.integers(600, 901))                                  # wide
    nx = int(rng.integers(41, 600))
    return nx + 1 if nx % 32 == 0 else nx                                   # not a multiple of 32


def _mask(rng, nx, ny):
    """The generator kinds of test_gpu_random.py (lines on the seams of 64- and 128-row windows, computed from the window size), then solids on
    every row next to a seam, in the top row and the last (partial) window, on the inlet and outlet columns, and rectangles across seams."""
    m = np.zeros((ny, nx), np.uint8)
    seams = _seams(ny, WIN["float64"])                                      # (every seam of 128-row windows is one of 64-row windows)
    kind = rng.integers(0, 4)
    if kind == 0:                                                           # sparse speckles
        m[rng.random((ny, nx)) < 0.002] = 1
    elif kind == 1:                                                         # a few rectangles, some touching the borders
        for _ in range(rng.integers(1, 6)):
            x0, y0 = rng.integers(0, nx), rng.integers(0, ny)
            m[y0:y0 + rng.integers(1, ny // 3 + 2), x0:x0 + rng.integers(1, nx // 3 + 2)] = 1
    elif kind == 2:                                                         # thin lines on the seam rows, one sparse column
        for s in seams:
            for r in (s - 1, s, s + 1):
                x0 = rng.integers(0, max(1, nx - 40))
                m[r, x0:x0 + rng.integers(1, 40)] = 1
        m[:, rng.integers(3, nx - 3)] = rng.random(ny) < 0.3
    for s in seams:                                                         # runs on rows s-3 .. s+2 (what the seam flags of k_seam_flags4 cover)
        for r in range(s - 3, s + 3):
            if 0 <= r < ny and rng.random() < 0.6:
                x0 = int(rng.integers(0, nx))
                m[r, x0:x0 + int(rng.integers(1, max(2, nx // 4)))] = 1
    x0 = int(rng.integers(0, nx - 2))
    m[ny - 1, x0:x0 + int(rng.integers(1, nx // 2 + 1))] = 1               # the top row
    last = (ny - 1) // WIN["float32"] * WIN["float32"]                     # the last 128-row window
    y0 = int(rng.integers(last, ny))
    x0 = int(rng.integers(3, nx - 3))
    m[y0:y0 + int(rng.integers(1, 5)), x0:x0 + int(rng.integers(1, 8))] = 1
    for cols in (slice(0, 3), slice(nx - 3, nx)):                           # inlet and outlet columns inside the march
        y0 = int(rng.integers(1, ny - 1))
        m[y0:y0 + int(rng.integers(1, ny // 4 + 2)), cols] = 1
    for _ in range(2):                                                      # rectangles across a seam
        if seams:
            s = int(rng.choice(seams))
            y0 = s - int(rng.integers(1, 9))
            x0 = int(rng.integers(0, nx - 2))
            m[max(0, y0):s + int(rng.integers(1, 12)), x0:x0 + int(rng.integers(2, max(3, nx // 3)))] = 1
    return m


def _case(seed):
    """Lattice, mask, tau, U0, step sequence and plan cut (0: by measured time; > 0: units of that many columns) of one seed."""
    rng = np.random.default_rng(7100 + seed)
    nx, ny = _width(rng, seed), _height(rng, seed)
    mask = _mask(rng, nx, ny)
    tau, u0 = float(rng.uniform(0.51, 1.2)), float(rng.uniform(0.02, 0.11))
    steps = [1] + [int(v) for v in rng.integers(2, 12, size=4)]
    rng.shuffle(steps)
    if seed == CLAMP_SEED:
        tau, u0 = 0.5004, 0.10
        steps = [1, 4, 3, 7, 2, 9] * 8
    chunk = int(rng.integers(1, 40)) if seed % 2 else 0
    return nx, ny, mask, tau, u0, steps, chunk


def _clamp_counts(mask, macro):
    """wt_clamp_events counted on the oracle's macro state (html:344-350)."""
    return clamp_events(*macro, mask)


def _assert_same(f, macro, ref_f, ref_m, what):
    assert bits_equal(f, ref_f), what
    for name, a, b in zip(("rho", "ux", "uy"), macro, ref_m):
        assert bits_equal(a, b), (what, name)


def _assert_tiling(e, depth, chain):
    """The path the case is meant to take really ran: tiling windows, a marching plan of that depth, whole passes, no downgraded chain block
    (chain blocks are four units each); `chain`: the plan holds chain blocks."""
    assert e.get_option("window_overlap") == 0.0
    assert e.get_option("fuse_active") == 1.0 and e.get_option("fuse_depth") == depth
    assert e.get_option("passes") > 0
    assert e.get_option("chain_downgrades") == 0 and e.get_option("chain_units") % 4 == 0
    if chain:
        assert e.get_option("chain_units") > 0, "a plan cut by time holds no chain block"


@pytest.mark.parametrize("seed", range(16))
def test_seeded_tiling_windows_equal_the_oracle(pkg, oracle_c, seed):
    nx, ny, mask, tau, u0, steps, chunk = _case(seed)
    refs, wrong = {}, []
    for dtype, depth in FORMS:
        if dtype not in refs:
            refs[dtype] = oracle_c.run(mask, sum(steps), tau, u0, np.dtype(dtype))
        ref_f, ref_m = refs[dtype]
        with pkg.Engine(nx, ny, dtype=dtype) as e:
            e.set_option("window_overlap", 0)
            e.set_option("fuse_depth", depth)
            e.set_option("fuse_chunk", chunk)
            e.set_option("fuse_steps", 2)
            e.set_mask(mask)
            e.init_equilibrium(u0)
            for n in steps:
                e.step(n, tau, u0)
            what = (dtype, depth, e.get_option("chain_units"))
            # (no chain block is asked for: these lattices hold fewer window-columns than the device has resident waves, so a cut by time makes
            # units of a column or two, too short for a chain; the cut by time WITH chain blocks is pinned on the larger lattices below)
            _assert_tiling(e, depth, False)
            assert e.info().steps_done == sum(steps)
            f, macro = e.read_f(), e.read_macro()
            events = e.clamp_events()
        # (every form is run before the verdict: which of them differ tells where to look)
        wrong += [what + (name,) for name, a, b in zip(("f", "rho", "ux", "uy"), (f,) + macro, (ref_f,) + ref_m) if not bits_equal(a, b)]
        if seed == CLAMP_SEED:
            want = _clamp_counts(mask, ref_m)
            assert events == want and want[1] > 0, (what, events, want)
    assert not wrong, (nx, ny, chunk, wrong)


def test_odd_height_falls_back_to_single_steps(pkg, oracle_c):
    """fp32 with an odd height: no marching plan (two sites per lane), single steps, still the oracle's bits."""
    nx, ny, mask, tau, u0, steps, _ = _case(3)
    ny -= 3
    mask = np.ascontiguousarray(mask[:ny])
    ref_f, ref_m = oracle_c.run(mask, sum(steps), tau, u0, np.float32)
    with pkg.Engine(nx, ny) as e:
        e.set_option("window_overlap", 0)
        e.set_mask(mask)
        e.init_equilibrium(u0)
        for n in steps:
            e.step(n, tau, u0)
        assert e.get_option("fuse_active") == 0.0 and e.get_option("passes") == 0
        assert e.get_option("single_steps") == sum(steps)
        _assert_same(e.read_f(), e.read_macro(), ref_f, ref_m, (nx, ny))


# --------------------------------------------------------------------------------------------------------------------------------------------
# readouts on the ragged states below (reductions in grid-stride loops, k_field's partial 32x32 tiles)
# --------------------------------------------------------------------------------------------------------------------------------------------
def _check_readouts(e, oracle_np, mask, u0, ref_m):
    rho, ux, uy = ref_m
    ranges = oracle_np.ranges_from_macro(rho, ux, uy, mask, u0)
    np.testing.assert_allclose(e.reduce_ranges(u0), ranges, rtol=1e-13, atol=0)
    fx, fy, surf, rev = e.forces()
    rfx, rfy, rsurf, rrev = oracle_np.compute_forces_raw(rho, ux, mask)
    assert (surf, rev) == (rsurf, rrev) and surf > 0
    bound = 1e-12 * surf * float(rho.max()) / 3
    assert abs(fx - rfx) <= bound and abs(fy - rfy) <= bound, (fx, rfx, fy, rfy, bound)
    assert e.clamp_events() == _clamp_counts(mask, ref_m)
    for mode in (0, 1, 2):
        t = e.field(mode, u0, *ranges, VORT_SCALE)
        ref = oracle_np.field_scalar(mode, rho, ux, uy, mask, u0, *ranges)
        assert t.dtype == ref.dtype and np.array_equal(np.isnan(t), np.isnan(ref)), mode
        assert bits_equal(np.nan_to_num(t), np.nan_to_num(ref)), mode


def _f32(bits):
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


@pytest.mark.parametrize("tau_bits,fast_div,two_op,pass_depth", [
    (0x3f147ae1, 1, 1.0, 4),            # tau 0.58: the two-operation division is proved
    (0x3f5119d3, 1, 0.0, 4),            # tau 0.8168: the two-operation form misses one significand -> the three-operation form
    (0x3f147ae1, 0, 0.0, 3),            # IEEE division: four-step tables run three-step passes
], ids=["two_op", "three_op", "ieee"])
def test_division_forms_on_tiling_windows(pkg, oracle_c, oracle_np, tau_bits, fast_div, two_op, pass_depth):
    nx, ny, u0 = 1000, 646, 0.07
    tau = _f32(tau_bits)
    mask = pkg.geometry.build_geometry(nx, ny, 35.0, None, "naca4412").mask
    rows = np.nonzero(mask.any(axis=1))[0]
    assert sum(rows[0] < s <= rows[-1] for s in _seams(ny, WIN["float32"])) >= 2          # the body crosses two seams
    steps = [1, 4, 7, 2, 9]
    ref_f, ref_m = oracle_c.run(mask, sum(steps), tau, u0, np.float32)
    with pkg.Engine(nx, ny) as e:
        e.set_option("window_overlap", 0)
        e.set_option("fuse_depth", 4)
        e.set_option("fast_div", fast_div)
        e.set_mask(mask)
        e.init_equilibrium(u0)
        for n in steps:
            e.step(n, tau, u0)
        _assert_tiling(e, 4, True)
        assert e.get_option("fast_div_active") == float(fast_div)
        assert e.get_option("fast_div_two_op_active") == two_op
        assert e.get_option("pass_depth") == pass_depth
        _assert_same(e.read_f(), e.read_macro(), ref_f, ref_m, tau_bits)
        _check_readouts(e, oracle_np, mask, u0, ref_m)


def test_automatic_plan_above_the_size_threshold(pkg, oracle_c, oracle_np):
    """2930 x 2562 (7 506 660 sites, a last window of 2 rows): the default plan takes tiling windows, four steps per pass with chain blocks,
    times its units, is cut again after an AoA change and keeps the oracle's bits; forced overlapping windows compute the same."""
    nx, ny, tau, u0 = 2930, 2562, 0.58, 0.06
    assert nx * ny > THRESHOLD and ny % WIN["float32"] == 2
    m1 = pkg.geometry.build_geometry(nx, ny, 12.0, None, "naca2412").mask
    m2 = pkg.geometry.build_geometry(nx, ny, 14.0, None, "naca2412").mask
    rows = np.nonzero(m1.any(axis=1))[0]
    assert sum(rows[0] < s <= rows[-1] for s in _seams(ny, WIN["float32"])) >= 3
    first, second = [1, 4, 7, 4], [3] + [4] * 17 + [6]
    ref_f, _ = oracle_c.run(m1, sum(first), tau, u0, np.float32)
    ref_f, ref_m = oracle_c.run(m2, sum(second), tau, u0, np.float32, f=ref_f)
    for overlap in (None, 1):
        with pkg.Engine(nx, ny) as e:
            if overlap is not None:
                e.set_option("window_overlap", overlap)
            e.set_mask(m1)
            e.init_equilibrium(u0)
            assert e.get_option("window_overlap") == (1.0 if overlap else 0.0)
            assert e.get_option("fuse_active") == 1.0 and e.get_option("fuse_depth") >= 3
            if not overlap:
                assert e.get_option("chain_units") > 0 and e.get_option("chain_downgrades") == 0
            for n in first:
                e.step(n, tau, u0)
            assert e.get_option("tune_rounds") > 0                            # the units were timed and cut again
            p0 = e.get_option("passes")
            e.set_mask(m2)                                                     # the AoA slider
            for n in second:
                e.step(n, tau, u0)
            assert e.get_option("passes") - p0 > 16 and e.get_option("tune_rounds") > 0      # (a mask after a short-lived one: timed after 16 passes)
            assert e.get_option("window_overlap") == (1.0 if overlap else 0.0) and e.get_option("chain_downgrades") == 0
            _assert_same(e.read_f(), e.read_macro(), ref_f, ref_m, "overlapping" if overlap else "automatic")
            if not overlap:
                _check_readouts(e, oracle_np, m2, u0, ref_m)


def test_automatic_plan_below_the_size_threshold(pkg):
    nx, ny = 2900, 2586                                                         # 7 499 400 sites
    assert nx * ny <= THRESHOLD
    with pkg.Engine(nx, ny) as e:
        e.set_mask(pkg.geometry.build_geometry(nx, ny, 12.0, None, "naca2412").mask)
        assert e.get_option("fuse_active") == 1.0 and e.get_option("window_overlap") == 1.0
