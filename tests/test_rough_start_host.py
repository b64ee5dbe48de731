"""CPU: every reference that tests/test_gpu_rough_start.py compares the stepping kernels with can tell a misplaced read (no interior fluid site
holds the bits of a fluid neighbour or of itself one step earlier: _rough_start.assert_sensitive), stays off the stability net (the shared-reciprocal
guard and the fast division by tau are the paths an ordinary state takes) — or, the net case, is on it.  And, for the record, how little of an
equilibrium start a bit comparison sees."""
import numpy as np
import pytest

import _rough_start as rs


def test_rough_state_is_the_perturbed_equilibrium():
    """The moments of a start state: density and velocity inside their amplitudes (the population noise adds at most amp_neq of either), float64
    rounded once, another seed another state, no two sites alike."""
    nx, ny = 37, 22
    f64 = rs.rough_state(nx, ny, rs.U0, np.float64, 5)
    f32 = rs.rough_state(nx, ny, rs.U0, np.float32, 5)
    assert f64.shape == (9, ny, nx) and f64.dtype == np.float64 and f32.dtype == np.float32
    assert np.array_equal(f32, f64.astype(np.float32))
    rho = f64.sum(axis=0)
    ux = sum(ex * f64[k] for k, (ex, _) in enumerate(rs.E)) / rho
    uy = sum(ey * f64[k] for k, (_, ey) in enumerate(rs.E)) / rho
    assert np.abs(rho - 1).max() < 0.03 + 0.02 * 1.04 and 0.02 < np.abs(rho - 1).max()
    assert np.abs(ux - rs.U0).max() < 0.03 + 0.025 and np.abs(uy).max() < 0.03 + 0.025 and 0.02 < np.abs(uy).max()
    assert (f64 > 0).all()
    assert rs.insensitive_counts(f64, rs.rough_state(nx, ny, rs.U0, np.float64, 6), np.zeros((ny, nx), np.uint8)) == (0, 0)
    assert rs.uniform_share(f64) == 0.0


def test_the_check_notices_a_copied_site_and_a_site_that_stood_still():
    nx, ny = 20, 12
    mask = np.zeros((ny, nx), np.uint8)
    a, b = rs.rough_state(nx, ny, rs.U0, np.float32, 1), rs.rough_state(nx, ny, rs.U0, np.float32, 2)
    rs.assert_sensitive(a, b, mask)
    c = a.copy()
    c[:, 5, 7] = c[:, 6, 8]                                                  # a diagonal neighbour's populations
    assert rs.insensitive_counts(c, b, mask) == (2, 0)                       # (seen from either side)
    with pytest.raises(AssertionError):
        rs.assert_sensitive(c, b, mask)
    solid = mask.copy()
    solid[6, 8] = 1
    assert rs.insensitive_counts(c, b, solid) == (0, 0)                      # a solid neighbour does not count
    c = a.copy()
    c[:, 3, 4] = b[:, 3, 4]
    assert rs.insensitive_counts(c, b, mask) == (0, 1)
    c[:, 0, 4], c[:, 3, 0] = b[:, 0, 4], b[:, 3, 0]                          # the outer row and column are not looked at
    assert rs.insensitive_counts(c, b, mask) == (0, 1)


def test_body_mask_holds_every_kind():
    for nx, ny in ((64, 262), (150, 390), rs.LARGE):
        m = rs.mask_of("body", nx, ny)
        assert np.array_equal(m, rs.body_mask(nx, ny, 4100 + nx + ny))       # deterministic
        assert m[0].any() and m[ny - 1].any() and m[1:-1, :3].all(axis=1).any() and m[1:-1, nx - 3:].all(axis=1).any()
        for s in range(rs.SEAM, ny, rs.SEAM):
            assert all(m[r].any() for r in range(s - 3, min(s + 3, ny))), s
        assert 0.5 < (m == 0).mean()
        assert not rs.mask_of("empty", nx, ny).any()


@pytest.mark.parametrize("case", rs.ALL_CASES, ids=[c.id for c in rs.ALL_CASES])
def test_every_reference_is_sensitive(oracle_c, case):
    _, mask, ref_f, ref_m, prev = rs.reference(oracle_c, case, with_prev=True)
    rs.assert_sensitive(ref_f, prev, mask)
    assert all(np.isfinite(a).all() for a in ref_m)
    events = rs.clamp_counts(case, ref_m)
    print(case.id, "clamp events", events, "rho", float(ref_m[0].min()), float(ref_m[0].max()))
    if not case.net:
        assert events == (0, 0)
        return
    # the net case: speed clamps after the first two calls (after the 21 steps no amplitude leaves any: _rough_start.NET_AMP_U), the same end state
    counts, f, _ = rs.net_counts(oracle_c, case)
    print(case.id, "clamp events after every call", counts)
    assert counts[0][1] > 0 and counts[1][1] > 0 and counts[-1] == events, counts
    assert np.array_equal(rs._bits(f), rs._bits(ref_f))


def test_shortest_units_share_the_small_references():
    """test_shortest_outlet_units runs on the first lattice of SMALL: its references are checked above.  The unit counts it expects: 63 marched
    columns in 3 windows of 128 or 120 rows or 5 of 64; at four steps 62 units per window; 189 and 186 units of overlapping windows are 48 and 47
    workgroups, dealt to the XCDs as 8 x 6."""
    nx, ny, chunk = rs.SHORTEST
    assert (nx, ny) == rs.SMALL[0][:2] and chunk == 1
    assert all(rs.case_small(nx, ny, m, d) in rs.ALL_CASES for m in rs.MASKS for d in rs.DTYPES)
    assert [rs.shortest_unit_count(nx, ny, depth, "float32", 0) for depth in (2, 3, 4)] == [189, 189, 186]
    assert [rs.shortest_unit_count(nx, ny, depth, "float32", 1) for depth in (3, 4)] == [192, 192]
    assert [rs.shortest_unit_count(nx, ny, depth, "float64", 0) for depth in (2, 3, 4)] == [315, 315, 310]


def test_two_part_reference_equals_the_whole_run(oracle_c):
    """reference(with_prev=True) runs the last step on its own: the same bits as one run (what the GPU file compares with)."""
    case = rs.case_small(64, 262, "body", "float32")
    _, _, f1, m1 = rs.reference(oracle_c, case)
    _, _, f2, m2, _ = rs.reference(oracle_c, case, with_prev=True)
    assert np.array_equal(rs._bits(f1), rs._bits(f2)) and all(np.array_equal(rs._bits(a), rs._bits(b)) for a, b in zip(m1, m2))


def test_an_equilibrium_start_is_mostly_uniform(oracle_c):
    """The body case of test_fused_vs_oracle_and_edge_masks (512 x 512, 17 steps from init_equilibrium): more than half of the interior sites
    hold the bits of all eight neighbours at the end — a read from the wrong neighbour there changes nothing."""
    from airfoil_cfd_tool_amd import geometry
    mask = geometry.build_geometry(512, 512, 15.0, None, "naca4412").mask
    ref_f, _ = oracle_c.run(mask, 17, 0.58, 0.06, np.float32)
    share = rs.uniform_share(ref_f)
    print("uniform share", share)
    assert share > 0.5
