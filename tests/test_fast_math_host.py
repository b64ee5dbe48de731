"""CPU: the references of tests/test_gpu_fast_math_rough.py are usable (tests/_fast_math_cases.py).  For every case, call pattern and boundary:

1. the NumPy model of collide_contracted, with rcp / rsq as the rounded quotients and with either moved by a random ulp, stays within 2 d32 of the
   fp64 oracle per plane — half the bound the device is held to;
2. from a healthy state the model differs from lbm_numpy.step in bits, and in binary64 agrees with it to 1e-6: it is the same collision;
3. a read from the wrong row (row 129 takes its three upward populations from row 127; one population of one site taken from the row above),
   injected at the first or at the last step of a run, is over 8 d32 in at least one plane at the next boundary;
4. on the net cases, a collision whose omega is 64 ulps off, or that clamps the density before it takes the reciprocal, is over 4 d32 at every
   boundary.  (Off the net the non-equilibrium part that omega multiplies is a few per cent of a population and decays within a dozen steps: 64 ulps
   of omega leave 1.0 .. 5.2 d32 there — printed, not asserted; the bound does not see such an omega except on the net.)
5. net cases: the fp64 oracle, the fp32 oracle and the model count the same clamp events at every boundary, the first boundary holds density
   and speed events, and no interior fluid site of the fp64 oracle is within 1e-5 (relative) of a clamp threshold;
6. at the last boundary at most 1 in 10 000 pairs of neighbouring interior fluid sites differ by less than 100 d32 in their largest population
   difference: a read from a neighbour is far over the bound almost everywhere.

Margins measured (printed by the tests): model / d32 0.70 .. 1.70; the row misread at least 1.3e4 d32, one population at least 19 d32 (120
injections); omega +- 64 ulps on the net 28 .. 44 d32 in the worst plane, the early density clamp at least 3.3e4; pairs under 100 d32: none,
except 28 of 440 832 after the slabs' 47 steps."""
import numpy as np
import pytest

import _fast_math_cases as fm
import _rough_start as rs
from lbm_numpy import E, clamp_events
from lbm_numpy import step as ieee_step

RUNS = fm.host_runs()
IDS = [fm.run_id(*r) for r in RUNS]
SEEN, WRONG = 8.0, fm.BOUND                     # items 3 and 4
ROW = 129                                       # the row above the seam of the first two 128-row windows


def _worst(planes, ref):
    q = fm.ratios(planes, ref)
    return max(q), fm.NAMES[int(np.argmax(q))]


@pytest.mark.parametrize("case,calls", RUNS, ids=IDS)
def test_yardstick_and_model(oracle_c, case, calls):
    """Items 1 and 5."""
    refs = fm.references(oracle_c, case, calls)
    clean = fm.model_run(case, calls)
    noisy = fm.model_run(case, calls, rng=np.random.default_rng(7))
    wrong = []
    for ref, a, b in zip(refs, clean, noisy):
        fm.assert_yardstick(ref)
        print(fm.run_id(case, calls), "step", ref.steps, "d32", ["%.2e" % d for d in ref.d32], "model / d32", ["%.2f" % q for q in fm.ratios(a, ref)],
              "with ulps", ["%.2f" % q for q in fm.ratios(b, ref)], ref.events or "")
        wrong += [(ref.steps, "rounded", fm.over(a, ref, fm.MODEL_BOUND)), (ref.steps, "ulps", fm.over(b, ref, fm.MODEL_BOUND))]
        if case.net:
            mask = rs.mask_of(ref.mask, case.nx, case.ny)
            assert ref.events == ref.events32 == clamp_events(*a[1:], mask) == clamp_events(*b[1:], mask), ref.steps
            assert ref.near == 0, (ref.steps, ref.near)
    assert not [w for w in wrong if w[2]], wrong
    if case.net:
        assert refs[0].events[0] > 0 and refs[0].events[1] > 0, refs[0].events


@pytest.mark.parametrize("case", sorted({r[0] for r in RUNS if not r[0].net}, key=lambda c: c.id), ids=lambda c: c.id)
def test_model_is_the_same_collision_in_another_arithmetic(case):
    """Item 2, on the first step from the rough state."""
    mask = rs.mask_of(case.before[0] if case.before else case.mask, case.nx, case.ny)
    f32 = rs.start_of(case)
    a, b = fm.contracted_step(f32, mask, case.tau, rs.U0), ieee_step(f32, mask, case.tau, rs.U0)
    fluid = mask[1:-1, 1:-1] == 0
    differ = (rs._bits(a[0]) != rs._bits(b[0])).any(axis=0)[1:-1, 1:-1][fluid].mean()
    print(case.id, "share of interior fluid sites whose populations differ in bits", differ)
    assert differ > 0.9
    outside = np.ones(mask.shape, bool)
    outside[1:-1, 1:-1] = ~fluid
    for x, y in zip((a[0],) + a[1], (b[0],) + b[1]):                       # far field, outlet and solids are the oracle's own
        assert np.array_equal(rs._bits(x)[..., outside], rs._bits(y)[..., outside])
    f64 = f32.astype(np.float64)
    a, b = fm.contracted_step(f64, mask, case.tau, rs.U0), ieee_step(f64, mask, case.tau, rs.U0)
    worst = max(float(np.abs(x - y).max()) for x, y in zip((a[0],) + a[1], (b[0],) + b[1]))
    print(case.id, "binary64: model against lbm_numpy.step", worst)
    assert worst <= 1e-6


def _row_misread(fin, f):
    """Row ROW takes the populations that move upwards from row ROW - 2 in place of ROW - 1."""
    nx = f.shape[2]
    for k, (ex, ey) in enumerate(E):
        if ey == 1:
            fin[k][ROW - 1, :] = f[k, ROW - 2, 1 - ex:nx - 1 - ex]


def _one_population(f, mask, rng):
    """One population of one interior fluid site replaced by that of the site above."""
    ny, nx = mask.shape
    while True:
        y, x, k = int(rng.integers(2, ny - 3)), int(rng.integers(2, nx - 2)), int(rng.integers(0, 9))
        if mask[y, x] == 0:
            g = f.copy()
            g[k, y, x] = f[k, y + 1, x]
            return g, (k, y, x)


def _step(case, kind, f, **wrong):
    f, macro = fm.contracted_step(f, rs.mask_of(kind, case.nx, case.ny), case.tau, rs.U0, **wrong)
    return (f,) + tuple(macro)


@pytest.mark.parametrize("case,calls", RUNS, ids=IDS)
def test_a_misread_is_seen_at_the_next_boundary(oracle_c, case, calls):
    """Item 3."""
    refs = fm.references(oracle_c, case, calls)
    sched = fm.schedule(case, calls)
    _, last = fm.model_run(case, calls, keep_last=True)
    f0, (kind0, n0), kind1 = rs.start_of(case), sched[0], sched[-1][0]
    assert ROW + 1 < case.ny - 1
    margins = []

    def run_first(f, **wrong):
        """calls[0] steps, the first of them wrong."""
        planes = _step(case, kind0, f, **wrong)
        for _ in range(n0 - 1):
            planes = _step(case, kind0, planes[0])
        return planes
    margins.append(("row, first step",) + _worst(run_first(f0, misread=_row_misread), refs[0]))
    margins.append(("row, last step",) + _worst(_step(case, kind1, last[-1], misread=_row_misread), refs[-1]))
    rng = np.random.default_rng(31)
    for _ in range(4):
        g, where = _one_population(f0, rs.mask_of(kind0, case.nx, case.ny), rng)
        margins.append(("one population before the first step", where) + _worst(run_first(g), refs[0]))
        g, where = _one_population(last[-1], rs.mask_of(kind1, case.nx, case.ny), rng)
        margins.append(("one population before the last step", where) + _worst(_step(case, kind1, g), refs[-1]))
    print(fm.run_id(case, calls), "worst plane of every misread, in d32:", margins)
    assert all(m[-2] > SEEN for m in margins), margins


@pytest.mark.parametrize("case,calls", RUNS, ids=IDS)
def test_a_wrong_collision_is_seen(oracle_c, case, calls):
    """Item 4."""
    refs = fm.references(oracle_c, case, calls)
    om = np.array([fm.omega_of(case.tau)], np.float32)
    margins = []
    for name, wrong in (("omega + 64 ulps", {"omega": (om.view(np.int32) + 64).view(np.float32)[0]}),
                        ("omega - 64 ulps", {"omega": (om.view(np.int32) - 64).view(np.float32)[0]})) + \
            ((("density clamp before the reciprocal", {"clamp_first": True}),) if case.net else ()):
        planes = fm.model_run(case, calls, **wrong)
        margins.append((name, [round(_worst(a, ref)[0], 1) for a, ref in zip(planes, refs)]))
    print(fm.run_id(case, calls), "worst plane at every boundary, in d32:", margins)
    if case.net:
        assert all(q > WRONG for _, qs in margins for q in qs), margins


SENSITIVE = RUNS + [(fm.LARGE, fm.LARGE_CALLS)]


@pytest.mark.parametrize("case,calls", SENSITIVE, ids=[fm.run_id(*r) for r in SENSITIVE])
def test_neighbours_differ_by_far_more_than_the_bound(oracle_c, case, calls):
    """Item 6 (and the yardstick of the measured-plan case, which the model does not run)."""
    ref = fm.references(oracle_c, case, calls)[-1]
    fm.assert_yardstick(ref)
    f, ny, nx = ref.planes[0], case.ny, case.nx
    fluid = rs.mask_of(ref.mask, nx, ny) == 0
    pairs = close = 0
    for ex, ey in E[1:]:
        a, b = (slice(1, ny - 1), slice(1, nx - 1)), (slice(1 + ey, ny - 1 + ey), slice(1 + ex, nx - 1 + ex))
        both = fluid[a] & fluid[b]
        both[:, 0 if ex < 0 else nx - 3 if ex > 0 else slice(0, 0)] = False        # the neighbour is an interior site too
        both[0 if ey < 0 else ny - 3 if ey > 0 else slice(0, 0), :] = False
        d = np.abs(f[(slice(None),) + a] - f[(slice(None),) + b]).max(axis=0)
        pairs += int(both.sum())
        close += int((both & (d < 100.0 * ref.d32[0])).sum())
    print(fm.run_id(case, calls), "pairs of neighbouring interior fluid sites under 100 d32:", close, "of", pairs)
    assert pairs > 0 and close * 10000 <= pairs, (close, pairs)
