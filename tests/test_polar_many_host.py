"""Batched sweeps at many members: what needs no GPU.  tests/test_gpu_polar_many.py compares every member of a batch of 35, 67 or 1024
with its own reference; this file checks, on the references alone, that this comparison can tell the members apart: every member
of tests/_many_cases.py computes a state of its own, a member run with its neighbour's tau, U0, Cs and V0 computes another one, no
member sits at the stability net at a sampled step, every member has faces and links, and the tall lattices keep FAST tiles beside
every member's body.
"""
import numpy as np
import pytest

import lbm_numpy
import _many_cases as mc
import _net_cases as nc


def _span(v):
    return f"{min(v)}..{max(v)}"


@pytest.mark.parametrize("name", list(mc.CASES))
def test_inputs_differ_from_member_to_member(name):
    nx, ny, dtype, B, steps, every = mc.CASES[name]
    mem = mc.members(name)
    assert mem.masks.shape == (B, ny, nx) and mem.q.shape == (B, 8, ny, nx) and mem.q.dtype == np.dtype(dtype)
    tuples = {mem.params(m) + (float(mem.xref[m]), float(mem.yref[m])) for m in range(B)}
    assert len(tuples) == B
    for v in (mem.tau, mem.u0, mem.xref, mem.yref):                         # and in every single value that has no special one
        assert len(set(v.tolist())) == B
    T = np.dtype(dtype).type
    assert len({(T(mem.tau[m]), T(mem.u0[m])) for m in range(B)}) == B      # still after the library's rounding to the lattice's dtype
    assert (mem.tau >= 0.52).all() and (mem.tau <= 0.9).all() and (mem.u0 >= 0.03).all() and (mem.u0 <= 0.08).all()
    on = mem.cs[mem.cs != 0]
    assert (on >= 0.05).all() and (on <= 0.2).all() and B - on.size == round(B / 5)
    r = mem.v0 / mem.u0
    assert (r >= -0.3).all() and (r <= 0.6).all() and int((r == 0).sum()) == round(B / 6) and (r < 0).any() and (r > 0).any()
    assert len(set(on.tolist())) == on.size and len(set(mem.v0[mem.v0 != 0].tolist())) == int((mem.v0 != 0).sum())
    assert len({mc.digest(mem.q[m]) for m in range(B)}) == B
    masks = {mc.digest(mem.masks[m]) for m in range(B)}
    if name == mc.MAX:
        assert len(masks) == 2 * (nx - 6) * (ny - 6)                        # every position of either orientation
        assert all(int((mem.masks[m] != 0).sum()) == 6 for m in range(B))
    else:
        assert len(masks) == B
    # both walks of the members write a state that is read back
    assert {mc.walk_is_reversed(s) for s in mc.plain_marks(name)} == {False, True}
    assert mc.plain_marks(name)[-1] == mc.model_marks(name)[-1] == steps and len(mc.model_marks(name)) == 3
    fast, links, faces = mc.counts(name)
    print(f"{name}: FAST cells {_span(fast)}, links {_span(links)}, faces {_span(faces)} over {B} members")
    assert min(links) > 0 and min(faces) > 0
    if ny >= 64 * (16 // np.dtype(dtype).itemsize):
        assert min(fast) > 0                                                # a full tile beside every member's body stays FAST
        for m in range(B):                                                  # ... either side of it
            cols = np.flatnonzero((nc.fast_cells(mem.masks[m], dtype)).any(axis=0))
            body = np.flatnonzero(mem.masks[m][:ny - 12].any(axis=0))
            assert cols.min() < body.min() and cols.max() > body.max(), m
    else:
        assert max(fast) == 0


def _assert_healthy(states, masks, what):
    for k, row in enumerate(states):
        for m, (f, macro) in enumerate(row):
            assert np.isfinite(f).all(), (what, k, m)
            assert lbm_numpy.clamp_events(*macro, masks[m]) == (0, 0), (what, k, m)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_plain_references_differ_and_stay_off_the_net(name, oracle_c):
    nx, ny, dtype, B, steps, every = mc.CASES[name]
    mem = mc.members(name)
    ref = mc.plain_reference(name, oracle_c)
    _assert_healthy(ref, mem.masks, name)
    distinct = len({mc.digest(f) for f, _ in ref[-1]})
    print(f"{name}: {distinct} distinct plain states of {B} members after {steps} steps")
    assert distinct == B
    for m in range(B):                                                      # with the neighbour's tau and U0: another state
        n = (m + 1) % B
        other = oracle_c.run(mem.masks[m], mc.FIRST_READ, float(mem.tau[n]), float(mem.u0[n]), np.dtype(dtype))[0]
        assert other.tobytes() != ref[0][m][0].tobytes(), m
    if name == mc.MAX:                                                      # the C oracle is lbm_numpy's restatement: one member as a check
        want = lbm_numpy.run(mem.masks[1023], mc.FIRST_READ, float(mem.tau[1023]), float(mem.u0[1023]), np.float32)[0]
        assert want.tobytes() == ref[0][1023][0].tobytes()


@pytest.mark.parametrize("name", list(mc.BODY))
def test_model_references_differ_and_stay_off_the_net(name):
    nx, ny, dtype, B, steps, every = mc.CASES[name]
    mem = mc.members(name)
    ref = mc.model_reference(name)
    _assert_healthy(ref, mem.masks, name)
    distinct = len({mc.digest(f) for f, _ in ref[-1]})
    print(f"{name}: {distinct} distinct states of {B} members after {steps} steps with wind, LES and interpolated walls")
    assert distinct == B
    # A member that runs with its neighbour's (tau, U0, Cs, V0) computes another state, by the first sample already; and so it does
    # with only one of the four taken from the neighbour, wherever the two values differ.
    for m in range(B):
        n = (m + 1) % B
        own, nb = mem.params(m), mem.params(n)
        want = ref[0][m][0].tobytes()
        assert mc.run_member("all", mem.masks[m], every, *nb, mem.q[m], dtype)[0].tobytes() != want, m
        if m % 8 == 0:                                                      # (one in eight: each costs a reference run)
            for k in range(4):
                if own[k] == nb[k]:                                         # (both switched off)
                    continue
                mixed = own[:k] + (nb[k],) + own[k + 1:]
                assert mc.run_member("all", mem.masks[m], every, *mixed, mem.q[m], dtype)[0].tobytes() != want, (m, k)
        # ... and with its neighbour's wall distances
        if m % 8 == 1:
            assert mc.run_member("all", mem.masks[m], every, *own, mem.q[n], dtype)[0].tobytes() != want, m


def test_listed_members_of_the_largest_batch():
    nx, ny, dtype, B, steps, every = mc.CASES[mc.MAX]
    mem = mc.members(mc.MAX)
    listed = mc.listed_members()
    assert len(listed) == 40 and set(listed) >= {0, 1, 2, 63, 64, 65, 511, 512, 513, 1021, 1022, 1023} and listed == mc.listed_members()
    ref = mc.listed_reference()
    assert len({mc.digest(f) for f, _ in ref.values()}) == 40
    for m in listed:
        f, macro = ref[m]
        assert np.isfinite(f).all() and lbm_numpy.clamp_events(*macro, mem.masks[m]) == (0, 0), m
        n = (m + 1) % B
        assert mc.run_member("wind+les", mem.masks[m], steps, *mem.params(n), None, dtype)[0].tobytes() != f.tobytes(), m


def test_single_model_references_differ():
    nx, ny, dtype, B, _, _ = mc.CASES[mc.SUB_CASE]
    mem = mc.members(mc.SUB_CASE)
    finals = {}
    for variant in mc.VARIANTS:
        ref = mc.variant_reference(variant)
        finals[variant] = [mc.digest(f) for f, _ in ref]
        assert len(set(finals[variant])) == B, variant
        for m, (f, macro) in enumerate(ref):
            assert np.isfinite(f).all() and lbm_numpy.clamp_events(*macro, mem.masks[m]) == (0, 0), (variant, m)
    # the model of a variant acts in every member that has it: no two variants agree on a member, but where the difference between them is
    # a model that the member switches off (cs = 0, v0 = 0)
    for m in range(B):
        les_on, wind_on = mem.cs[m] != 0, mem.v0[m] != 0
        assert (finals["wind"][m] != finals["wind+les"][m]) == les_on, m
        assert (finals["les"][m] != finals["wind+les"][m]) == wind_on, m
        assert finals["ibb"][m] != finals["les"][m] and finals["ibb"][m] != finals["wind"][m], m


def test_the_sub_range_inputs_change_the_members_they_replace():
    nx, ny, dtype, B, _, every = mc.CASES[mc.SUB_CASE]
    mem = mc.members(mc.SUB_CASE)
    masks, q = mc.sub_inputs()
    (first, count), (qfirst, qcount) = mc.SUB_MASKS, mc.SUB_Q
    assert 0 < first and first + count < B and first <= qfirst and qfirst + qcount <= first + count
    assert masks.shape == (count, ny, nx) and q.shape == (qcount, 8, ny, nx)
    for k in range(count):
        assert not np.array_equal(masks[k], mem.masks[first + k]) and mc.counts(mc.SUB_CASE)[1][first + k] > 0
    start = mc.model_reference(mc.SUB_CASE)[0]
    half = np.full((8, ny, nx), 0.5, np.dtype(dtype))
    for k in range(count):
        m = first + k
        f = start[m][0]
        kept = mc.run_member("all", mem.masks[m], every, *mem.params(m), mem.q[m], dtype, f=f)[0]
        reset = mc.run_member("all", masks[k], every, *mem.params(m), half, dtype, f=f)[0]
        old_q = mc.run_member("all", masks[k], every, *mem.params(m), mem.q[m], dtype, f=f)[0]
        assert np.isfinite(reset).all()
        assert kept.tobytes() != reset.tobytes() and old_q.tobytes() != reset.tobytes(), m      # the mask matters, and so does the reset
        if qfirst <= m < qfirst + qcount:
            new = mc.run_member("all", masks[k], every, *mem.params(m), q[m - qfirst], dtype, f=f)[0]
            assert new.tobytes() != reset.tobytes() and new.tobytes() != old_q.tobytes(), m
