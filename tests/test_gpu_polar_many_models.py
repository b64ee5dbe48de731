"""GPU: half storage, the two-relaxation-time collision, prescribed far-field profiles and state upload of batched sweeps
(libwtpolar.so) at many members, every member against its own reference: the batches of tests/test_gpu_polar_many.py (67, 35 and 1024
members) under the families of tests/_many_model_cases.py, every member with a magic number, a rough start state and far-field tables of
its own (tests/test_polar_many_models_host.py shows on the references alone that a member which ran with its neighbour's would be seen).
What is exercised is every lookup by the member index that these four features added: the member walk of k_step_half_batch
into params, cles, vwind, lam, the lattice counted in halves, the mask and the macro planes; init_half's and
k_mex_half_batch's; fptr<half_t>(b, cur, member) of the reads and writes of a half batch; lam[m], zero_v and the per-member tau check of
TRT; prof + m * p_stride, the (first, count) loop of wtp_set_far_profile, prof_set[m] and the Python side's tables behind state(); the
member offset of wtp_write_f / wtp_write_stored and of the sums they clear.

The references and the tolerances are those of the tests of each feature: states are the references' bits, the force sums are held to
the derived bounds of Loads, Mex and MexIbb, the surface and mean sums are the references' bits.
"""
import numpy as np
import pytest

import _half_reference as half
import _many_cases as mc
import _many_model_cases as mm
from _loads_reference import loads_reference
from _mex_reference import count_links
from test_gpu_polar_many import _assert_member_state, _assert_rows, _assert_sums, _Worst

pytestmark = pytest.mark.gpu

WT_ERR_ARG, WT_ERR_STATE = -1, -5
IDS = [f"{f}-{n}" for f, n in mm.BODY_RUNS]


def _engine(pkg, family, name, cap=3):
    nx, ny, dtype, B, _, _ = mc.CASES[name]
    return pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=cap, storage="half" if mm.model(family).stored else "native")


def _configure(b, family, name, tables=True):
    """The engine calls of a family, up to and including init_equilibrium.  tables=False: the profile on, no member given any."""
    mdl, mem = mm.model(family), mc.members(name)
    b.set_masks(mem.masks)
    if mdl.ibb:
        b.enable_interpolated_walls()
        b.set_wall_distances(mem.q)
    if mdl.les:
        b.enable_les(mem.cs)
    if mdl.wind:
        b.enable_wind(mem.v0)
    if mdl.trt:
        b.enable_trt(mm.magic(name))
    if mdl.profile:
        b.enable_far_profile()
        if tables:
            b.set_far_profile(*mm.stacked_tables(name, range(b.members)))
    b.init_equilibrium(mem.u0)


def _write(b, name, m, which, stored):
    f = mm.start(name, m, which)
    if stored:
        b.write_stored(m, half.store(f).view(np.uint16))
    else:
        b.write_f(m, f)


def _upload(b, family, name):
    """Every member started from its own rough state, in a fixed scrambled order; in a half batch the odd members by write_stored of
    Store(start), the even ones by write_f."""
    for m in mm.upload_order(name):
        _write(b, name, m, 0, mm.model(family).stored and m & 1 == 1)


def _step(b, name, n, tau=None):
    mem = mc.members(name)
    b.step(n, mem.tau if tau is None else tau, mem.u0, sample_every=mm.every(name))


def _read(b, m):
    """(read_f, read_macro, read_stored or None) of member m."""
    return b.read_f(m), b.read_macro(m), b.read_stored(m) if b.storage == "half" else None


def _assert_state(got, want, what):
    """One member's read-back against (state, macro) of its reference, bits: in a half batch the raw halves, and read_f as Load of them."""
    f, macro, stored = got
    state, want_macro = want
    if stored is not None:
        assert state.dtype == np.float16
        bits = state.view(np.uint16)
        if stored.tobytes() != bits.tobytes():
            rows = np.flatnonzero((stored != bits).any(axis=(0, 2)))
            raise AssertionError((what, "stored", f"{rows.size} rows differ, the first is row {int(rows[0])}"))
        state = half.load(state)
    _assert_member_state(f, macro, (state, want_macro), what)


def _march(b, family, name, todo, done, members=None):
    """Runs the calls `todo` from step `done`; after each, every member (or `members`) against the family's reference at that mark."""
    members = range(b.members) if members is None else members
    for n in todo:
        _step(b, name, n)
        done += n
        assert b.step_count == done
        want = mm.at(family, name, done)
        for m in members:
            _assert_state(_read(b, m), want[m], (family, name, "step", done, "member", m))
    return done


# ---- a. every member is its reference -----------------------------------------------------------
@pytest.mark.parametrize("family,name", mm.BODY_RUNS, ids=IDS)
def test_every_member_is_its_reference(pkg, family, name):
    B = mc.CASES[name][3]
    with _engine(pkg, family, name) as b:
        _configure(b, family, name)
        _upload(b, family, name)
        for m in (0, B - 1):                                                # between the upload and the first step the planes are not the lattice's
            with pytest.raises(pkg.WTError) as ei:
                b.read_macro(m)
            assert ei.value.code == WT_ERR_STATE
        done = _march(b, family, name, mm.calls(name), 0)
        assert list(b.history()["step"]) == list(mm.sample_marks(name))
    print(f"{family} {name}: {B} members x {len(mm.marks(name))} read-backs at steps {mm.marks(name)} bit-identical")
    assert done == mm.marks(name)[-1]


# ---- b, c. read-outs at many members; overwriting members in the middle of a run -------------------
def _readouts(pkg, family, name, overwrite):
    nx, ny, dtype, B, _, _ = mc.CASES[name]
    mdl, mem = mm.model(family), mc.members(name)
    over = mm.overwritten(family, name) if overwrite else {}
    new = mm.overwrite_reference(family, name) if overwrite else {}
    smarks = mm.sample_marks(name)
    later = [s for s in mm.marks(name) if s > mm.WRITE_AFTER]
    got, done = {}, 0
    with _engine(pkg, family, name) as b:
        _configure(b, family, name)
        b.enable_loads(mem.xref, mem.yref)
        b.enable_momentum_exchange(mem.xref, mem.yref)
        b.enable_mean_fields()
        _upload(b, family, name)
        for n in mm.calls(name):
            _step(b, name, n)
            done += n
            if done in smarks:
                got[done] = [_read(b, m) for m in range(B)]
            if overwrite and done == mm.WRITE_AFTER:
                for m, how in over.items():
                    _write(b, name, m, 1, how == "stored")
                for m in sorted({*over, *(k + d for k in over for d in (-1, 1) if 0 <= k + d < B)}):     # their sums were emptied, no neighbour's
                    assert b.mean_sums(m)["n"] == (0 if m in over else 1), m
                    assert bool(b.surface(m)["n_upper"].any()) == (m not in over), m
        h = b.history()
        moment, exchange, forces = b.moment(), b.momentum_exchange(), b.forces()
        surface = [b.surface(m) for m in range(B)]
        sums = [b.mean_sums(m) for m in range(B)]
    assert list(h["step"]) == list(smarks) and h["fx"].shape == (len(smarks), B)      # an overwrite leaves the rows and their step column
    worst = _Worst()
    q = mem.q if mdl.ibb else [None] * B
    for m in range(B):
        samples = []
        for r, mark in enumerate(smarks):
            what = (family, name, "step", mark, "member", m)
            restarted = m in over and mark > mm.WRITE_AFTER
            want = new[m][later.index(mark)] if restarted else mm.at(family, name, mark)[m]
            _assert_state(got[mark][m], want, what)
            f, macro, _ = got[mark][m]
            _assert_rows(h, r, m, f, macro[0], mem.masks[m], q[m], float(mem.xref[m]), float(mem.yref[m]), worst, what)
            if restarted or m not in over:
                samples.append(macro)
        assert len(samples) == (2 if m in over else 3)                      # an overwritten member holds the samples after the write only
        _assert_sums(surface[m], sums[m], samples, mem.masks[m], (family, name, "member", m))
    assert moment.tobytes() == h["mz"][-1].tobytes()                        # the on-demand calls on the last sampled state: the last row
    for key, v in zip(("fx_mex", "fy_mex", "mz_mex", "links"), exchange):
        assert v.tobytes() == h[key][-1].tobytes(), key
    for key, v in zip(("fx", "fy", "surf", "rev"), forces):
        assert v.tobytes() == h[key][-1].tobytes(), key
    print(f"{family} {name}: {B} members x {len(smarks)} samples at steps {smarks} bit-identical in state, surface sums and mean sums"
          f"{', members ' + str(sorted(over)) + ' overwritten after step ' + str(mm.WRITE_AFTER) if over else ''}; {worst}")


@pytest.mark.parametrize("family,name", mm.READOUT_RUNS, ids=[f"{f}-{n}" for f, n in mm.READOUT_RUNS])
def test_read_outs_of_every_member(pkg, family, name):
    _readouts(pkg, family, name, overwrite=False)


@pytest.mark.parametrize("family,name", mm.READOUT_RUNS, ids=[f"{f}-{n}" for f, n in mm.READOUT_RUNS])
def test_members_overwritten_in_the_middle_of_a_run(pkg, family, name):
    _readouts(pkg, family, name, overwrite=True)


# ---- d. profile sub-ranges and gating -----------------------------------------------------------
def test_profile_sub_ranges_and_gating(pkg):
    family, name = mm.SUB_RUN
    B = mc.CASES[name][3]
    mem = mc.members(name)
    last = B - 1
    first, count = mm.SUB_TABLES
    with _engine(pkg, family, name) as b:
        _configure(b, family, name, tables=False)
        b.set_far_profile(*mm.stacked_tables(name, range(last)))           # members [0, B - 1): the last one has none
        _upload(b, family, name)
        assert "far_profile" not in b.state()
        before = {m: b.read_f(m) for m in (0, last - 1, last)}
        with pytest.raises(pkg.WTError) as ei:
            _step(b, name, 1)
        assert ei.value.code == WT_ERR_STATE and f"member {last} " in str(ei.value), str(ei.value)
        assert b.step_count == 0 and all(b.read_f(m).tobytes() == f.tobytes() for m, f in before.items())
        b.set_far_profile(*mm.tables(name, last), first=last)
        done = _march(b, family, name, mm.calls(name)[:3], 0)
        assert done == mm.WRITE_AFTER
        b.set_far_profile(*mm.stacked_tables(name, range(first, first + count), 1), first=first)
        new = mm.sub_tables_reference()
        for k, n in enumerate(mm.calls(name)[3:]):
            _step(b, name, n)
            done += n
            want = mm.at(family, name, done)
            for m in range(B):
                _assert_state(_read(b, m), new[m][k] if m in new else want[m], (family, name, "step", done, "member", m))
        for m in (first - 1, first + count):                                # either end of the range, by name
            assert b.read_f(m).tobytes() == mm.at(family, name, done)[m][0].tobytes(), f"member {m}, next to the range [{first}, {first + count}), was touched"
        held = b.state()["far_profile"]
        for m in range(B):
            want = mm.tables(name, m, 1 if m in new else 0)
            for key, t in zip(("left", "bottom", "top"), want):
                assert held[key][m].dtype == t.dtype and held[key][m].tobytes() == t.tobytes(), (m, key)
    print(f"{family} {name}: {B} members bit-identical at steps {mm.marks(name)}; members {sorted(new)} on their second tables from step {mm.WRITE_AFTER}")


# ---- e. TRT argument checks at late indices -----------------------------------------------------
def test_trt_argument_checks_at_late_indices(pkg):
    family, name = mm.ARG_RUN
    B = mc.CASES[name][3]
    mem = mc.members(name)
    with _engine(pkg, family, name) as b:
        _configure(b, family, name)
        _upload(b, family, name)
        done = _march(b, family, name, mm.calls(name)[:3], 0)
        bad = mm.magic(name).copy()
        bad[65] = 0.0
        with pytest.raises(pkg.WTError) as ei:
            b.enable_trt(bad)
        assert ei.value.code == WT_ERR_ARG and "magic[65]" in str(ei.value), str(ei.value)
        assert b.trt_enabled
        done = _march(b, family, name, mm.calls(name)[3:4], done)           # the refused call changed no magic number: the next steps' bits
        hist = b.history()
        tau = mem.tau.copy()
        tau[66] = 0.5
        with pytest.raises(pkg.WTError) as ei:
            _step(b, name, 8, tau)
        assert ei.value.code == WT_ERR_ARG and "tau[66]" in str(ei.value), str(ei.value)
        after = b.history()
        assert b.step_count == done == 16 and all(after[k].tobytes() == hist[k].tobytes() for k in hist) and list(hist["step"]) == [8, 16]
        b.enable_wind(None)                                                 # under TRT the kernel now reads the [B] zeros, not a stale V0
        assert not b.wind_enabled and b.trt_enabled
        _step(b, name, 8)
        axial = mm.axial_reference()
        for m in range(B):
            _assert_state(_read(b, m), axial[m], (family, name, "axial", "member", m))
    print(f"{family} {name}: {B} members bit-identical at steps 1, 5, 8, 16 and, with the wind off, at 24")


# ---- f. checkpoint and restart of a large batch -------------------------------------------------
def test_checkpoint_and_restart_of_a_large_batch(pkg):
    family, name = mm.RESTART_RUN
    nx, ny, dtype, B, _, _ = mc.CASES[name]
    with _engine(pkg, family, name) as a:
        _configure(a, family, name)
        _upload(a, family, name)
        for n in mm.calls(name)[:3]:
            _step(a, name, n)
        state = a.state()
    assert state["steps"] == 8 and state["f"].shape == (B, 9, ny, nx) and state["f"].dtype == np.uint16 and state["storage"] == "half"
    with _engine(pkg, family, name) as b:
        _configure(b, family, name)
        b.restore(state)
        assert b.step_count == 8 and len(b.history()["step"]) == 0
        for m in (0, 41, B - 1):
            assert b.read_stored(m).tobytes() == mm.at(family, name, 8)[m][0].tobytes(), m
        done = _march(b, family, name, mm.calls(name)[3:], 8)
        assert done == b.step_count == 24 and list(b.history()["step"]) == [16, 24]
    print(f"{family} {name}: {B} members restored at step 8, bit-identical with the uninterrupted reference at 16 and 24")


# ---- g. the largest batch -----------------------------------------------------------------------
@pytest.mark.parametrize("family", mm.MAX_FAMILIES)
def test_the_largest_batch(pkg, family):
    name = mc.MAX
    nx, ny, dtype, B, _, _ = mc.CASES[name]
    mem = mc.members(name)
    listed = mm.compared(name)
    smarks = mm.sample_marks(name)
    assert B == 1024
    got, done = {}, 0
    with _engine(pkg, family, name) as b:
        _configure(b, family, name)
        b.enable_loads(mem.xref, mem.yref)
        b.enable_momentum_exchange(mem.xref, mem.yref)
        _upload(b, family, name)
        for n in mm.calls(name):
            _step(b, name, n)
            done += n
            got[done] = {m: _read(b, m) for m in listed}
        h = b.history()
        moment, exchange, forces, events = b.moment(), b.momentum_exchange(), b.forces(), b.clamp_events()
    assert list(h["step"]) == list(smarks)
    worst = _Worst()
    for mark in mm.marks(name):
        for m in listed:
            what = (family, name, "step", mark, "member", m)
            _assert_state(got[mark][m], mm.at(family, name, mark)[m], what)
            if mark in smarks:
                f, macro, _ = got[mark][m]
                _assert_rows(h, smarks.index(mark), m, f, macro[0], mem.masks[m], None, float(mem.xref[m]), float(mem.yref[m]), worst, what)
    ones = np.ones((ny, nx))
    links = np.array([count_links(mem.masks[m]) for m in range(B)])
    faces = np.array([loads_reference(ones, mem.masks[m], 0.0, 0.0).n for m in range(B)])
    assert (links == 26).all() and (faces == 10).all()                      # (what the 2x3 and 3x2 blocks have)
    for r in range(len(smarks)):                                            # all 1024 members, every row
        assert np.array_equal(h["links"][r], links) and np.array_equal(h["surf"][r], faces), r
        assert all(np.isfinite(h[k][r]).all() for k in ("fx", "fy", "mz", "fx_mex", "fy_mex", "mz_mex")), r
    assert not events[0].any() and not events[1].any()
    assert moment.tobytes() == h["mz"][-1].tobytes()
    for key, v in zip(("fx_mex", "fy_mex", "mz_mex", "links"), exchange):
        assert v.tobytes() == h[key][-1].tobytes(), key
    for key, v in zip(("fx", "fy", "surf", "rev"), forces):
        assert v.tobytes() == h[key][-1].tobytes(), key
    for k in ("mz", "mz_mex"):                                              # the rows are the members', not copies of one another (lever arms in double)
        assert len(set(h[k][-1].tolist())) == B, k
    print(f"{family} {name}: {len(listed)} states x {len(mm.marks(name))} read-backs bit-identical, links, faces and events of {B} members; {worst}")
