"""GPU: every stepping path from a start state in which no two sites are alike (tests/_rough_start.py), bit for bit against the C oracle.

From init_equilibrium the columns in which chain blocks run, the rows about a seam away from the body and the columns about a slab edge hold the
same nine numbers in every site for as many steps as the other tests take: a column off by one in the chain blocks' hand-over, the wrong edge
column of a unit, a seam row, halo line or margin row one row off, a ghost column in the wrong order or one trimmed ghost column too many read the
right bits there.  Here every such read changes bits (tests/test_rough_start_host.py holds that of every reference used below), and every case
asserts that the path it is about really ran.  The pattern: set_mask, write_f(rough_state), step in the calls 4, 3, 7, 1, 6, compare the
populations and the three macro planes; every form of a case runs before the verdict, which names the forms that differ."""
import numpy as np
import pytest

import _rough_start as rs
from conftest import bits_equal

pytestmark = pytest.mark.gpu


def _differ(what, f, macro, ref_f, ref_m):
    return [(what, name) for name, a, b in zip(rs.NAMES, (f,) + tuple(macro), (ref_f,) + tuple(ref_m)) if not bits_equal(a, b)]


def _ref(oracle_c, case):
    assert case in rs.ALL_CASES, case                   # (the host file has checked this reference)
    return rs.reference(oracle_c, case)


def _forms():
    """(name, dtype, options): k_step; fp32 at two, three and four steps per pass on tiling windows, at three and four on overlapping ones;
    fp64 at two, three and four; from three steps per pass with and without chain blocks."""
    forms = [("f32 single steps", "float32", {"fuse_steps": 0}), ("f64 single steps", "float64", {"fuse_steps": 0})]
    for dtype, overlap, depths in (("float32", 0, (2, 3, 4)), ("float32", 1, (3, 4)), ("float64", None, (2, 3, 4))):
        for depth in depths:
            for chain in ((1, 0) if depth >= 3 else (None,)):
                opts = {"fuse_depth": depth}
                if overlap is not None:
                    opts["window_overlap"] = overlap
                if chain is not None:
                    opts["chain"] = chain
                name = f"{'f32' if dtype == 'float32' else 'f64'} depth {depth}" + ("" if overlap is None else " overlapping" if overlap else " tiling")
                forms.append((name + ("" if chain is None else f" chain {chain}"), dtype, opts))
    return forms


def _assert_marched(e, name, opts):
    """The path a form is meant to take really ran."""
    assert e.get_option("fuse_active") == 1.0 and e.get_option("passes") > 0, name
    assert e.get_option("chain_downgrades") == 0 and e.get_option("chain_units") % 4 == 0, name
    if "fuse_depth" in opts:
        assert e.get_option("fuse_depth") == opts["fuse_depth"], name
    if "window_overlap" in opts or e.dtype != np.float32:
        assert e.get_option("window_overlap") == float(opts.get("window_overlap", 0)), name
    if opts.get("chain") == 0:
        assert e.get_option("chain_units") == 0, name


def _march(pkg, case, f0, mask, opts, calls=rs.CALLS, check=None):
    """One engine through the pattern; `check(e)` asserts what is the form's own."""
    with pkg.Engine(case.nx, case.ny, dtype=case.dtype) as e:
        for k, v in opts.items():
            if k != "fuse_steps":
                e.set_option(k, v)
        e.set_option("fuse_steps", opts.get("fuse_steps", 2))
        e.set_mask(mask)
        e.write_f(f0)
        events = []
        for n in calls:
            e.step(n, case.tau, rs.U0)
            if case.net:
                events.append(e.clamp_events())
        assert e.info().steps_done == sum(calls)
        if opts.get("fuse_steps", 2):
            _assert_marched(e, case.id, opts)
        else:
            assert e.get_option("single_steps") == sum(calls) and e.get_option("passes") == 0
        if check:
            check(e)
        return e.read_f(), e.read_macro(), events


# a. --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", rs.MASKS)
@pytest.mark.parametrize("nx,ny,chunk", rs.SMALL, ids=[f"{c[0]}x{c[1]}" for c in rs.SMALL])
def test_every_kernel_form(pkg, oracle_c, nx, ny, chunk, mask_kind):
    refs = {d: _ref(oracle_c, rs.case_small(nx, ny, mask_kind, d)) for d in rs.DTYPES}
    wrong = []
    for name, dtype, opts in _forms():
        f0, mask, ref_f, ref_m = refs[dtype]

        def check(e):
            if opts.get("chain") == 1 and mask_kind == "empty":
                chain, units = e.get_option("chain_units"), e.get_option("fuse_units")
                assert 0 < chain < units, (name, chain, units)         # chain blocks and solo units
        f, macro, _ = _march(pkg, rs.case_small(nx, ny, mask_kind, dtype), f0, mask, dict(opts, fuse_chunk=chunk), check=check)
        wrong += _differ(name, f, macro, ref_f, ref_m)
    assert not wrong, (nx, ny, mask_kind, wrong)


# b. --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau_bits,fast_div,two_op,pass_depth", rs.DIVISIONS, ids=["two_op", "three_op", "ieee"])
def test_division_forms(pkg, oracle_c, tau_bits, fast_div, two_op, pass_depth):
    case = rs.case_division(tau_bits)
    f0, mask, ref_f, ref_m = _ref(oracle_c, case)

    def check(e):
        assert e.get_option("fast_div_active") == float(fast_div)
        assert e.get_option("fast_div_two_op_active") == two_op
        assert e.get_option("pass_depth") == pass_depth
        assert 0 < e.get_option("chain_units") < e.get_option("fuse_units")
    f, macro, _ = _march(pkg, case, f0, mask, {"window_overlap": 0, "fuse_depth": 4, "fuse_chunk": 6, "fast_div": fast_div}, check=check)
    assert not _differ(tau_bits, f, macro, ref_f, ref_m)


# c. --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", rs.MASKS)
def test_on_the_stability_net(pkg, oracle_c, mask_kind):
    """A start state whose velocity noise reaches the speed clamp (and, in the first steps, the density clamp; some populations are negative): the
    waves that hold such sites leave the guarded divisions.  The oracle's bits, and its clamp events after every call."""
    wrong = []
    for name, dtype, opts in (("f32 tiling", "float32", {"window_overlap": 0}), ("f32 overlapping", "float32", {"window_overlap": 1}), ("f64", "float64", {})):
        case = rs.case_net(mask_kind, dtype)
        assert case in rs.ALL_CASES
        counts, ref_f, ref_m = rs.net_counts(oracle_c, case)
        assert counts[0][1] > 0 and counts[1][1] > 0
        f, macro, events = _march(pkg, case, rs.start_of(case), rs.mask_of(mask_kind, case.nx, case.ny), dict(opts, fuse_depth=4, fuse_chunk=6))
        wrong += _differ(name, f, macro, ref_f, ref_m)
        if events != counts:
            wrong.append((name, "clamp events", events, counts))
    assert not wrong, wrong


# d. --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", rs.MASKS)
@pytest.mark.parametrize("dtype", rs.DTYPES)
def test_plan_cut_by_measured_time(pkg, oracle_c, dtype, mask_kind):
    """Default fuse_chunk and tune: units cut by modelled, then by measured time (the tuner's trial passes must leave the state as it was), with
    chain blocks where the windows tile the column."""
    case = rs.case_large(mask_kind, dtype)
    f0, mask, ref_f, ref_m = _ref(oracle_c, case)
    forms = (("tiling", {"window_overlap": 0, "fuse_depth": 4}), ("automatic", {})) if dtype == "float32" else (("f64", {"fuse_depth": 4}),)
    wrong = []
    for name, opts in forms:
        def check(e):
            assert e.get_option("tune") == 1.0 and e.get_option("tune_rounds") > 0          # the units were timed and cut again
            print(case.id, name, {k: e.get_option(k) for k in ("fuse_depth", "fuse_units", "chain_units", "tune_rounds", "passes", "single_steps", "pass_depth")})
            if name == "automatic":
                assert e.get_option("window_overlap") == 1.0
            else:
                assert e.get_option("window_overlap") == 0.0 and e.get_option("chain_units") > 0
        f, macro, _ = _march(pkg, case, f0, mask, opts, check=check)
        wrong += _differ(name, f, macro, ref_f, ref_m)
    assert not wrong, wrong


# e. --------------------------------------------------------------------------------------------------------------------------------------------
def _engine(pkg, ny, dtype, depth, overlap):
    e = pkg.Engine(rs.SWITCH_NX, ny, dtype=dtype)
    for k, v in (("fuse_steps", 2), ("fuse_depth", depth), ("tune", 0)) + ((("window_overlap", overlap),) if dtype == "float32" else ()):
        e.set_option(k, v)
    return e


def _assert_layout(e, depth, overlap):
    assert e.get_option("fuse_active") == 1.0 and e.get_option("fuse_depth") == depth and e.get_option("window_overlap") == float(overlap)
    assert e.get_option("chain_downgrades") == 0


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("ny", rs.SWITCH_NY)
def test_layout_switch_in_mid_run(pkg, oracle_c, ny, depth):
    """Passes on overlapping windows write no seam rows: after window_overlap 1 -> 0 the first pass must build its halo lines from the lattice."""
    case = rs.case_layout_switch(ny)
    f0, mask, ref_f, ref_m = _ref(oracle_c, case)
    with _engine(pkg, ny, "float32", depth, 1) as e:
        e.set_mask(mask)
        e.write_f(f0)
        e.step(rs.SWITCH_FIRST, case.tau, rs.U0)
        _assert_layout(e, depth, 1)
        assert e.get_option("passes") > 0
        p0 = e.get_option("passes")
        e.set_option("window_overlap", 0)
        _assert_layout(e, depth, 0)
        e.step(rs.SWITCH_THEN, case.tau, rs.U0)
        assert e.get_option("single_steps") == 0 and e.get_option("passes") > p0
        assert not _differ(depth, e.read_f(), e.read_macro(), ref_f, ref_m)


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("ny", rs.SWITCH_NY)
def test_write_f_in_mid_run(pkg, oracle_c, ny, depth):
    """A second state written over the first after passes on tiling windows: no seam row or halo line of the first may survive."""
    wrong = []
    for dtype in rs.DTYPES:
        case = rs.case_rewrite(ny, dtype)
        f1, mask, ref_f, ref_m = _ref(oracle_c, case)
        with _engine(pkg, ny, dtype, depth, 0) as e:
            e.set_mask(mask)
            e.write_f(rs.start_of(rs.case_layout_switch(ny, dtype)))
            e.step(rs.SWITCH_FIRST, case.tau, rs.U0)
            _assert_layout(e, depth, 0)
            assert e.get_option("passes") > 0 and e.get_option("single_steps") == 0
            e.write_f(f1)
            e.step(rs.SWITCH_THEN, case.tau, rs.U0)
            assert e.get_option("passes") > 0 and e.get_option("single_steps") == 0          # (both counted since the write)
            wrong += _differ(dtype, e.read_f(), e.read_macro(), ref_f, ref_m)
    assert not wrong, wrong


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("ny", rs.SWITCH_NY)
def test_mask_change_in_mid_run(pkg, oracle_c, ny, depth):
    """From the empty mask to the body mask: classes, bounce codes, seam flags and units are cut again, the seam rows written under the old mask
    are not the new one's."""
    wrong = []
    for dtype, overlap in (("float32", 0), ("float32", 1), ("float64", 0)):
        case = rs.case_mask_change(ny, dtype)
        f0, mask, ref_f, ref_m = _ref(oracle_c, case)
        with _engine(pkg, ny, dtype, depth, overlap) as e:
            e.set_mask(rs.mask_of("empty", case.nx, ny))
            e.write_f(f0)
            e.step(rs.SWITCH_FIRST, case.tau, rs.U0)
            _assert_layout(e, depth, overlap)
            p0 = e.get_option("passes")
            assert p0 > 0
            e.set_mask(mask)
            _assert_layout(e, depth, overlap)
            e.step(rs.SWITCH_THEN, case.tau, rs.U0)
            assert e.get_option("passes") > p0 and e.get_option("single_steps") == 0
            wrong += _differ((dtype, overlap), e.read_f(), e.read_macro(), ref_f, ref_m)
    assert not wrong, wrong


# f. --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refresh", [0, 1, 2])
@pytest.mark.parametrize("dtype,overlap", [("float32", 1), ("float32", 0), ("float64", 0)], ids=["f32-overlapping", "f32-tiling", "f64"])
def test_slabs(pkg, oracle_c, dtype, overlap, refresh):
    """Three local slabs cut by the caller, each started from its own columns of the rough state: ghost columns renewed in every refresh mode,
    with and without trimmed ghost passes; the owned columns, side by side, against the oracle."""
    case = rs.case_slabs(dtype)
    f0, mask, ref_f, ref_m = _ref(oracle_c, case)
    n = len(rs.SLAB_EDGES) - 1
    wrong = []
    for trim in (1, 0):
        es = [pkg.Engine(case.nx, case.ny, dtype=dtype, rank=r, nranks=n, halo=rs.SLAB_HALO, edges=list(rs.SLAB_EDGES)) for r in range(n)]
        try:
            assert [e.x0 for e in es] == list(rs.SLAB_EDGES[:-1])
            pkg.Engine.link_local(es)
            for e in es:
                e.set_option("fuse_steps", 2)
                if dtype == "float32":
                    e.set_option("window_overlap", overlap)
                e.set_option("refresh", refresh)
                e.set_option("trim_ghosts", trim)
                e.set_mask(mask)
                e.write_f(np.ascontiguousarray(f0[:, :, e.x0:e.x0 + e.width]))
            for k in rs.SLAB_CALLS:
                pkg.Engine.step_group(es, k, case.tau, rs.U0)
            for e in es:
                assert e.info().steps_done == case.steps
                assert e.get_option("fuse_active") == 1.0 and e.get_option("window_overlap") == float(overlap) and e.get_option("passes") > 0
                assert e.get_option("chain_downgrades") == 0
                assert (e.get_option("trimmed_passes") > 0) == bool(trim), (trim, e.get_option("trimmed_passes"))
                if refresh:
                    assert e.get_option("single_steps") == 0
                    assert (e.get_option("boundary_exchanges") > 0) == (refresh == 1) and (e.get_option("fused_renewals") > 0) == (refresh == 2)
            f = np.concatenate([e.read_f() for e in es], axis=2)
            macro = [np.concatenate(parts, axis=1) for parts in zip(*[e.read_macro() for e in es])]
        finally:
            for e in es:
                e.close()
        wrong += _differ(("trim", trim), f, macro, ref_f, ref_m)
    assert not wrong, wrong


# g. --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", rs.MASKS)
def test_shortest_outlet_units(pkg, oracle_c, mask_kind):
    """Solo units of the least length the planner allows (rs.SHORTEST): one marched column each at two and three steps per pass, at four steps
    two in a window's last unit.  At three and four steps the loop of the unit that emits the outlet column then ends, by its `break`, before it
    has stored a column of its own: what it stores is the pipeline's fill (dropped), and every column of the unit comes out of the outlet tail; at
    two steps the loop stores the unit's one column in its last trip, just before the `break`.  Every other unit is all fill and drain."""
    nx, ny, chunk = rs.SHORTEST
    refs = {d: _ref(oracle_c, rs.case_small(nx, ny, mask_kind, d)) for d in rs.DTYPES}
    wrong, ran = [], 0
    for name, dtype, opts in _forms():
        if "fuse_depth" not in opts or opts.get("chain", 0) != 0:
            continue
        f0, mask, ref_f, ref_m = refs[dtype]

        def check(e):
            want = rs.shortest_unit_count(nx, ny, opts["fuse_depth"], dtype, opts.get("window_overlap", 0))
            assert e.get_option("fuse_units") == want, (name, e.get_option("fuse_units"), want)
            assert e.get_option("chain_units") == 0, name
        f, macro, _ = _march(pkg, rs.case_small(nx, ny, mask_kind, dtype), f0, mask, dict(opts, fuse_chunk=chunk, chain=0), check=check)
        wrong += _differ(name, f, macro, ref_f, ref_m)
        ran += 1
    assert ran == 8                                     # fp32 tiling 2, 3, 4; overlapping 3, 4; fp64 2, 3, 4
    assert not wrong, (mask_kind, wrong)
