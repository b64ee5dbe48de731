"""GPU: the two velocity divisions of a site on one shared reciprocal (csrc/step_march.hpp div2_shared, collide2_shared) in the plain columns of
the four-step fp32 marching kernel.

The chain itself against the IEEE quotient on the device (option "selftest_veldiv"), and a lattice whose start state holds sites that break each
condition of the kernel's guard in turn — those waves must fall back to the IEEE divisions, every other wave must not, and the result must be that of
single steps and of the C oracle bit for bit either way."""
import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

NX, NY, TAU, U0, STEPS, CHUNK = 64, 256, 0.58, 0.06, 8, 6
E = ((0, 0), (1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))       # html:238-248
# Units of six columns: [24, 48) is a chain block (its footprint is clear of both ends of the tunnel), the rest solo units.  Columns: first / last of
# the chain units [24, 30), [30, 36), [42, 48) and of the solo units [6, 12), [12, 18), [48, 54).
COLS = (6, 11, 17, 24, 29, 36, 47)
# rows: inside either tiling window, and the four rows about their seam (127 | 128); (row, column shift, how)
ROWS = ((40, 0, "arrive"), (126, 0, "place"), (127, 3, "arrive"), (128, 0, "place"), (129, 3, "arrive"), (200, 0, "place"))
NEG0 = np.float32(-0.0)


def _crafted(feq):
    """Nine populations each, one guard condition broken (or, the last, a numerator that is exactly zero: the guard must let it through)."""
    f = np.asarray(feq, np.float32)
    big, tiny, neg, minus0, my0 = f.copy(), f.copy(), f.copy(), f.copy(), f.copy()
    big[3] = 2.5                                             # a population of 2.5
    tiny[5] = 1e-36                                          # one of 1e-36
    neg[7] = -0.01                                           # one negative
    minus0[:] = (0.5, NEG0, 0.2, 0.0, 0.25, NEG0, 0.0, 0.0, NEG0)          # mx = -0: f1 = f5 = f8 = -0, f3 = f6 = f7 = +0, the rest large
    my0[:] = (0.4375, 0.1875, 0.125, 0.0625, 0.125, 0.03125, 0.015625, 0.015625, 0.03125)      # dyadic: my = 0 exactly, rho = 1.03125
    return [big, tiny, neg, f * np.float32(0.3), f * np.float32(2.5), minus0, my0]              # (rho < 0.5; rho > 2 with every population below 2)


@pytest.fixture(scope="module")
def start(oracle_c):
    """The start state (equilibrium + 42 crafted sites) and the oracle's answer after STEPS steps, computed once."""
    f, _ = oracle_c.equilibrium_init(NX, NY, U0, np.float32)
    kinds = _crafted(f[:, 1, 1])
    assert np.signbit(kinds[5][1]) and kinds[6][2] + kinds[6][5] + kinds[6][6] - kinds[6][4] - kinds[6][7] - kinds[6][8] == 0
    n = 0
    for k, pops in enumerate(kinds):
        for j, (row, shift, how) in enumerate(ROWS):
            col = COLS[(k + j) % len(COLS)] + shift
            for i, (ex, ey) in enumerate(E):
                # "arrive": population i is put where the first step's streaming pulls it from, so that the crafted nine meet at (row, col) in a collision
                y, x = (row - ey, col - ex) if how == "arrive" else (row, col)
                f[i, y, x] = pops[i]
            n += 1
    assert n == 42
    mask = np.zeros((NY, NX), np.uint8)
    return f, mask, oracle_c.run(mask, STEPS, TAU, U0, np.float32, f=f)


def _run(pkg, f0, mask, fuse, overlap=None):
    with pkg.Engine(NX, NY) as e:
        if overlap is not None:
            e.set_option("window_overlap", overlap)
        e.set_option("fuse_depth", 4)
        e.set_option("fuse_chunk", CHUNK)
        e.set_option("fuse_steps", fuse)
        e.set_mask(mask)
        e.init_equilibrium(U0)
        if f0 is not None:
            e.write_f(f0)
        e.step(STEPS, TAU, U0)
        if fuse:
            assert e.get_option("fuse_active") == 1.0 and e.get_option("pass_depth") == 4 and e.get_option("passes") > 0
            assert e.get_option("window_overlap") == float(overlap) and e.get_option("fast_div_active") == 1.0
            chain, units = e.get_option("chain_units"), e.get_option("fuse_units")
            assert 0 < chain < units, (chain, units)         # chain blocks and solo units
        else:
            assert e.get_option("single_steps") == STEPS
        return e.read_f(), e.read_macro(), e.clamp_events()


@pytest.fixture(scope="module")
def single(pkg, start):
    """The same steps one at a time (k_step: the IEEE divisions)."""
    f0, mask, _ = start
    f, macro, _ = _run(pkg, f0, mask, 0)
    return f, macro


def test_shared_reciprocal_chain_equals_the_division(pkg):
    with pkg.Engine(NX, NY) as e:
        assert e.get_option("selftest_veldiv") == 0.0


@pytest.mark.parametrize("overlap", [0, 1], ids=["tiling", "overlapping"])
def test_sites_outside_the_guard_keep_the_bits(pkg, start, single, overlap):
    f0, mask, (ref_f, ref_m) = start
    single_f, single_m = single
    f, macro, _ = _run(pkg, f0, mask, 2, overlap)
    for name, a, b, c in zip(("f", "rho", "ux", "uy"), (f,) + macro, (single_f,) + single_m, (ref_f,) + ref_m):
        assert bits_equal(a, b), (name, "single steps")
        assert bits_equal(a, c), (name, "oracle")


def test_plain_lattice_never_touches_the_net(pkg):
    """No crafted site: no density or speed clamp anywhere — the guarded path is what an ordinary state takes."""
    _, _, events = _run(pkg, None, np.zeros((NY, NX), np.uint8), 2, 0)
    assert events == (0, 0)
