"""Half storage, TRT, far-field profiles and state upload at many members: what needs no GPU.  tests/test_gpu_polar_many_models.py
compares every member of a batch of 35, 67 or 1024 with its own reference under the families of tests/_many_model_cases.py; this file
checks, on the references alone, the conditions that comparison rests on: tests/_many_cases.py still draws the bytes it drew, every
reference state is finite and off the stability net at every step, the members of a family end in states of their own, a member run with
its neighbour's magic number, tables or start state (or, in a half family, on the fp32 lattice) computes another state by the first
mark, and the overwrites and the table changes of the GPU tests change the members they touch.
"""
import numpy as np
import pytest

import lbm_numpy
import _half_reference as half
import _many_cases as mc
import _many_model_cases as mm
import _net_cases as nc

# mc.digest of the masks and of tau of "67-96x48-f32" as tests/_many_cases.py drew them when this file was written
PINNED = {"masks": "7b0eefeb89d5ab597f00aefe9150755bc69e2bd9943e53a01601b7e1838e6904",
          "tau": "00a592cfc0cacf44e659f6904f2819af5a42be5ed52945fc5abb1e16e7263cbd"}


def test_the_many_member_inputs_are_the_bytes_they_were():
    mem = mc.members("67-96x48-f32")
    assert mc.digest(mem.masks) == PINNED["masks"]
    assert mc.digest(mem.tau) == PINNED["tau"]


def test_the_marks_cover_both_walks_and_the_families_their_cases():
    for name in mc.CASES:
        marks = mm.marks(name)
        assert marks[0] == 1 and {mc.walk_is_reversed(s) for s in marks} == {False, True}
        assert len(mm.sample_marks(name)) == 3 and mm.sample_marks(name)[-1] == marks[-1]
        assert sorted(mm.upload_order(name)) == list(range(mc.CASES[name][3])) and mm.upload_order(name)[:4] != (0, 1, 2, 3)
        assert len(mm.subset(name)) >= 8 and set(mm.subset(name)) <= set(mm.compared(name))
        B = mc.CASES[name][3]
        assert {0, B - 1} <= set(mm.subset(name)) and (B < 66 or {63, 64, 65} <= set(mm.subset(name)))
    assert mm.marks("67-96x48-f32") == (1, 5, 8, 16, 24) and mm.marks(mc.MAX) == (1, 7, 14, 21) and mm.WRITE_AFTER in mm.marks("35-24x140-f64")
    for family, (mdl, names) in mm.FAMILIES.items():
        for name in names:
            assert not mdl.stored or (mc.CASES[name][2] == "float32" and not mdl.ibb and not mdl.profile), (family, name)
    for run in (*mm.READOUT_RUNS, mm.SUB_RUN, mm.ARG_RUN, mm.RESTART_RUN):
        assert run in mm.BODY_RUNS
    first, count = mm.SUB_TABLES
    assert 0 < first and first + count < mc.CASES[mm.SUB_RUN[1]][3]
    for family, name in mm.READOUT_RUNS:
        B = mc.CASES[name][3]
        over = mm.overwritten(family, name)
        assert all(0 <= m < B for m in over) and B - 1 in over and (0 in over) == mm.model(family).stored


@pytest.mark.parametrize("name", list(mc.CASES))
def test_magic_numbers_starts_and_tables_differ_from_member_to_member(name):
    nx, ny, dtype, B, _, _ = mc.CASES[name]
    lam = mm.magic(name)
    assert lam.shape == (B,) and (lam >= 1.0 / 16.0).all() and (lam <= 0.5).all()
    assert int((lam == 3.0 / 16.0).sum()) == 2 and int((lam == 0.25).sum()) == 2 and len(set(lam.tolist())) == B - 2
    T = np.dtype(dtype).type
    for m in range(B):                                                      # no member shares its neighbour's, still after the library's rounding
        assert T(lam[m]) != T(lam[(m + 1) % B]), m
    members = range(B) if name != mc.MAX else mm.compared(name)
    starts = {mc.digest(mm.start(name, m, w)) for m in members for w in (0, 1)}
    tabs = {mc.digest(np.concatenate([t.ravel() for t in mm.tables(name, m, w)])) for m in members for w in (0, 1)}
    assert len(starts) == len(tabs) == 2 * len(members)
    f = mm.start(name, 0)
    assert f.shape == (9, ny, nx) and f.dtype == np.dtype(dtype) and np.isfinite(f).all()
    left, bottom, top = mm.tables(name, B - 1)
    assert left.shape == (3, ny) and bottom.shape == top.shape == (3, nx) and left.dtype == np.dtype(dtype)


@pytest.mark.parametrize("family,name", mm.RUNS, ids=[f"{f}-{n}" for f, n in mm.RUNS])
def test_references_are_finite_off_the_net_and_distinct(family, name):
    ref = mm.reference(family, name)
    members = mm.compared(name)
    for k, mark in enumerate(mm.marks(name)):
        assert set(ref.states[k]) == set(members)
        for m, (state, macro) in ref.states[k].items():
            assert np.isfinite(state.astype(np.float64)).all() and all(np.isfinite(p).all() for p in macro), (family, name, mark, m)
    for m in members:                                                       # summed over every step, not only the marks
        assert ref.events[m] == (0, 0), (family, name, m, ref.events[m])
    finals = {mc.digest(state) for state, _ in ref.states[-1].values()}
    print(f"{family} {name}: {len(finals)} distinct final states of {len(members)} members after {mm.marks(name)[-1]} steps")
    assert len(finals) == len(members)
    if mm.model(family).stored:
        assert all(state.dtype == np.float16 for state, _ in ref.states[0].values())


@pytest.mark.parametrize("family,name", mm.RUNS, ids=[f"{f}-{n}" for f, n in mm.RUNS])
def test_a_member_with_its_neighbours_inputs_computes_another_state(family, name):
    """Each perturbed reference is run here and must differ from the member's own at the first mark: with these references, a kernel that
    read lam, the tables or the uploaded lattice of member m + 1 for member m would fail the GPU comparison."""
    mdl = mm.model(family)
    B = mc.CASES[name][3]
    first = mm.marks(name)[0]
    own = mm.at(family, name, first)
    for m in mm.subset(name):
        n = (m + 1) % B
        want = own[m][0].tobytes()
        state = mm.start_state(family, name, m)
        again = mm.advance(family, name, m, state, first)[0][0]
        assert again.tobytes() == want, (family, name, m)                   # (the perturbed runs below differ by their input, not by chance)
        other = mm.advance(family, name, m, mm.start_state(family, name, n), first)[0][0]
        assert other.tobytes() != want, (family, name, m, "start state")
        if mdl.trt:
            other = mm.advance(family, name, m, state, first, lam=float(mm.magic(name)[n]))[0][0]
            assert other.tobytes() != want, (family, name, m, "magic number")
        if mdl.profile:
            other = mm.advance(family, name, m, state, first, tabs=mm.tables(name, n))[0][0]
            assert other.tobytes() != want, (family, name, m, "tables")
            other = mm.advance(family, name, m, state, first, which=1)[0][0]
            assert other.tobytes() != want, (family, name, m, "second tables")
        if mdl.wind and mc.members(name).v0[m] != 0:                        # the cross-flow that wtp_enable_wind(None) replaces with zero_v
            other = mm.advance(family, name, m, state, first, v0=0.0)[0][0]
            assert other.tobytes() != want, (family, name, m, "cross-flow")


HALF_RUNS = [(f, n) for f, n in mm.RUNS if mm.model(f).stored]


@pytest.mark.parametrize("family,name", HALF_RUNS, ids=[f"{f}-{n}" for f, n in HALF_RUNS])
def test_half_references_differ_from_the_stored_native_run(family, name):
    """Every member's stored state differs from Store of the fp32 lattice's state in some interior fluid cell, at the first mark already;
    on the subset, still at the last."""
    mdl = mm.model(family)
    native = mm.Model(trt=mdl.trt, wind=mdl.wind, les=mdl.les)
    mem = mc.members(name)
    ref = mm.reference(family, name)
    first, last = mm.marks(name)[0], mm.marks(name)[-1]
    for m in mm.compared(name):
        cells = nc.interior_fluid(mem.masks[m])
        f = mm.advance(family, name, m, mm.start(name, m), first, mdl=native)[0][0]
        assert f.dtype == np.float32
        differ = (half.store(f).view(np.uint16) != ref.states[0][m][0].view(np.uint16)).any(axis=0)
        assert (differ & cells).any(), (family, name, m)
        if m in mm.subset(name):
            f = mm.advance(family, name, m, f, last - first, mdl=native)[0][0]
            differ = (half.store(f).view(np.uint16) != ref.states[-1][m][0].view(np.uint16)).any(axis=0)
            assert (differ & cells).any(), (family, name, m, "last mark")


def test_overwrites_and_table_changes_change_the_members_they_touch():
    for family, name in mm.READOUT_RUNS:
        ref = mm.reference(family, name)
        k = mm.marks(name).index(mm.WRITE_AFTER) + 1
        for m, states in mm.overwrite_reference(family, name).items():
            assert len(states) == 2
            for r, (state, macro) in enumerate(states):
                assert np.isfinite(state.astype(np.float64)).all() and state.tobytes() != ref.states[k + r][m][0].tobytes(), (family, name, m, r)
                assert lbm_numpy.clamp_events(*macro, mc.members(name).masks[m]) == (0, 0), (family, name, m, r)
    family, name = mm.SUB_RUN
    ref = mm.reference(family, name)
    k = mm.marks(name).index(mm.WRITE_AFTER) + 1
    sub = mm.sub_tables_reference()
    assert sorted(sub) == list(range(mm.SUB_TABLES[0], sum(mm.SUB_TABLES)))
    for m, states in sub.items():
        for r, (state, macro) in enumerate(states):
            assert np.isfinite(state).all() and state.tobytes() != ref.states[k + r][m][0].tobytes(), (m, r)
            assert lbm_numpy.clamp_events(*macro, mc.members(name).masks[m]) == (0, 0), (m, r)
    family, name = mm.ARG_RUN
    mem = mc.members(name)
    axial = mm.axial_reference()
    for m, (state, macro) in enumerate(axial):
        assert np.isfinite(state).all() and lbm_numpy.clamp_events(*macro, mem.masks[m]) == (0, 0), m
        assert (state.tobytes() != mm.at(family, name, 24)[m][0].tobytes()) == (mem.v0[m] != 0), m
