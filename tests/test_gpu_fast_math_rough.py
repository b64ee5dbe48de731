"""GPU: the contracted (option "fast_math") marching kernels — k_march3 at two, three and four steps per pass, their halo-line kernels, the chain
blocks and the general columns are code objects of their own — from a start state in which no two sites are alike (tests/_rough_start.py), on
lattices with seams, halo lines between windows and a ragged last window, on the stability net, across a mask change, on slabs and on the plan cut by
measured time.

v_rcp_f32 / v_rsq_f32 cannot be reproduced on the CPU, so (tests/_fast_math_cases.py; tests/test_fast_math_host.py holds that the references can tell
a misread):
  the bound     max |device - fp64 oracle| <= 4 d32 per plane (f, rho, ux, uy) after EVERY call, d32 = max |fp32 oracle - fp64 oracle| of that plane
                at that step count;
  the bits      collide_contracted is built from explicit builtins only, so every contracted form computes the same bits as every other: this is
                what sees a site that got the IEEE collision, or an error of one ulp.
Every engine asserts that the contracted passes it is about really ran (fast_math, no overlapping windows, no single step); every form of a test
runs before the verdict, which names the forms, steps and planes that differ.  Lines "RATIO case | form | plane | worst device / d32 over the
boundaries" are printed for profiles/fast_math_rough_ratios.txt."""
import numpy as np
import pytest

import _fast_math_cases as fm
import _rough_start as rs
from conftest import bits_equal

pytestmark = pytest.mark.gpu


def _forms(depths=(2, 3, 4)):
    """(name, options): depth 2, and depths 3 and 4 each with and without chain blocks."""
    return [(f"depth {d}" + ("" if c is None else f" chain {c}"), {"fuse_depth": d, **({} if c is None else {"chain": c})})
            for d in depths for c in ((1, 0) if d >= 3 else (None,))]


def _assert_contracted(e, name, opts, singles=True):
    assert e.get_option("fast_math") == 1.0 and e.get_option("fuse_active") == 1.0 and e.get_option("window_overlap") == 0.0, name
    assert e.get_option("passes") > 0 and e.get_option("chain_downgrades") == 0 and e.get_option("chain_units") % 4 == 0, name
    if singles:
        assert e.get_option("single_steps") == 0, (name, e.get_option("single_steps"))
    if "fuse_depth" in opts:
        assert e.get_option("fuse_depth") == opts["fuse_depth"], name
    if opts.get("chain") == 0:
        assert e.get_option("chain_units") == 0, name


def _engine(pkg, case, opts, tune=0):
    e = pkg.Engine(case.nx, case.ny, dtype="float32")
    e.set_option("fast_math", 1)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_option("fuse_steps", 2)
    if tune is not None:
        e.set_option("tune", tune)
    return e


def _planes(e):
    return (e.read_f(),) + tuple(e.read_macro())


def _march(pkg, case, calls, name, opts, tune=0, check=None):
    """One engine through the calls from the case's rough state: ([planes after every call], [clamp events after every call])."""
    with _engine(pkg, case, opts, tune) as e:
        e.set_mask(rs.mask_of(case.mask, case.nx, case.ny))
        e.write_f(rs.start_of(case))
        out, events = [], []
        for n in calls:
            e.step(n, case.tau, rs.U0)
            out.append(_planes(e))
            events.append(e.clamp_events())
        assert e.info().steps_done == sum(calls)
        _assert_contracted(e, (case.id, name), opts)
        if check:
            check(e)
        return out, events


class _Verdict:
    """Collects what is over the bound or differs in bits, and the worst ratio per (form, plane)."""

    def __init__(self, case, calls):
        self.tag, self.wrong, self.worst = fm.run_id(case, calls), [], {}

    def bound(self, form, planes, refs):
        for got, ref in zip(planes, refs):
            fm.assert_yardstick(ref)
            for name, q in zip(fm.NAMES, fm.ratios(got, ref)):
                if not q <= self.worst.get((form, name), 0.0):
                    self.worst[(form, name)] = q
            bad = fm.over(got, ref, fm.BOUND)
            if bad:
                self.wrong.append((form, "step", ref.steps, "over the bound", bad))

    def same_bits(self, form, planes, other_form, other, steps):
        for got, want, s in zip(planes, other, steps):
            differ = [n for n, a, b in zip(fm.NAMES, got, want) if not bits_equal(a, b)]
            if differ:
                self.wrong.append((form, "step", s, "bits differ from", other_form, differ,
                                   [int((rs._bits(a) != rs._bits(b)).sum()) for a, b in zip(got, want)]))

    def close(self):
        for (form, name), q in self.worst.items():
            print(f"RATIO {self.tag} | {form} | {name} | {q:.3f}")
        assert not self.wrong, (self.tag, self.wrong)


# A, B, C ---------------------------------------------------------------------------------------------------------------------------------------
RUNS = [(c, chunk, calls) for c, chunk in fm.SMALL + tuple((c, fm.NET_CHUNK) for c in fm.NET) for calls in (fm.EVEN, fm.ODD)]


@pytest.mark.parametrize("case,chunk,calls", RUNS, ids=[fm.run_id(r[0], r[2]) for r in RUNS])
def test_every_contracted_form(pkg, oracle_c, case, chunk, calls):
    """A: every form within the bound after every call.  B: on EVEN all five forms hold the bits of depth 2, on ODD (a two-step plan would take
    single steps, which collide in IEEE arithmetic) the depth-3 and depth-4 forms those of the first of them.  C (net cases): the oracle's clamp events after
    every call — the first run of the rsq branch and of the density clamp after the reciprocal."""
    refs = fm.references(oracle_c, case, calls)
    steps = [r.steps for r in refs]
    verdict, first = _Verdict(case, calls), None
    for name, opts in _forms((2, 3, 4) if calls == fm.EVEN else (3, 4)):
        def check(e):
            if opts.get("chain") == 1 and case.mask == "empty":
                chain, units = e.get_option("chain_units"), e.get_option("fuse_units")
                assert 0 < chain < units, (name, chain, units)                 # chain blocks and solo units
        planes, events = _march(pkg, case, calls, name, dict(opts, fuse_chunk=chunk), check=check)
        verdict.bound(name, planes, refs)
        if first is None:
            first = (name, planes)
        else:
            verdict.same_bits(name, planes, first[0], first[1], steps)
        if case.net and events != [r.events for r in refs]:
            verdict.wrong.append((name, "clamp events", events, [r.events for r in refs]))
    if case.net:
        assert refs[0].events[0] > 0 and refs[0].events[1] > 0
    verdict.close()


# D ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("case", fm.MASK_CHANGE, ids=[c.id for c in fm.MASK_CHANGE])
def test_mask_change_in_mid_run(pkg, oracle_c, case, depth):
    """From the empty mask to the body mask after 9 steps: within the bound at the change and at the end, and at the end the bits of an engine
    that never held the empty mask (started by write_f of the state at the change)."""
    refs = fm.references(oracle_c, case, fm.MASK_CHANGE_CALLS)
    (kind0, n0), (kind1, n1) = fm.schedule(case, fm.MASK_CHANGE_CALLS)
    opts, name = {"fuse_depth": depth}, f"depth {depth}"
    verdict = _Verdict(case, fm.MASK_CHANGE_CALLS)
    with _engine(pkg, case, opts) as e:
        e.set_mask(rs.mask_of(kind0, case.nx, case.ny))
        e.write_f(rs.start_of(case))
        e.step(n0, case.tau, rs.U0)
        _assert_contracted(e, name, opts)
        p0 = e.get_option("passes")
        at_change = _planes(e)
        e.set_mask(rs.mask_of(kind1, case.nx, case.ny))
        e.step(n1, case.tau, rs.U0)
        _assert_contracted(e, name, opts)
        assert e.get_option("passes") > p0 and e.info().steps_done == n0 + n1
        end = _planes(e)
    with _engine(pkg, case, opts) as e:
        e.set_mask(rs.mask_of(kind1, case.nx, case.ny))
        e.write_f(at_change[0])
        e.step(n1, case.tau, rs.U0)
        _assert_contracted(e, name + " fresh", opts)
        fresh = _planes(e)
    verdict.bound(name, [at_change, end], refs)
    verdict.bound(name + " fresh", [fresh], refs[1:])
    verdict.same_bits(name, [end], name + " fresh", [fresh], [refs[1].steps])
    verdict.close()


# E ---------------------------------------------------------------------------------------------------------------------------------------------
def test_slabs(pkg, oracle_c):
    """Three local slabs cut by the caller, refresh 1 and 2 with and without trimmed ghost passes, refresh 0 with them: the owned columns, side by
    side, within the bound after every call; refresh 1 and 2 hold the bits of a whole-lattice contracted engine stepped through the same calls
    (refresh 0 takes single steps, which collide in IEEE arithmetic)."""
    case, calls = fm.SLABS, fm.SLAB_CALLS
    refs = fm.references(oracle_c, case, calls)
    steps = [r.steps for r in refs]
    mask, f0 = rs.mask_of(case.mask, case.nx, case.ny), rs.start_of(case)
    n = len(rs.SLAB_EDGES) - 1
    verdict = _Verdict(case, calls)
    whole, _ = _march(pkg, case, calls, "whole lattice", {"fuse_depth": 4})
    verdict.bound("whole lattice", whole, refs)
    for refresh, trim in ((1, 1), (1, 0), (2, 1), (2, 0), (0, 1)):
        name = f"refresh {refresh} trim {trim}"
        es = [pkg.Engine(case.nx, case.ny, dtype="float32", rank=r, nranks=n, halo=rs.SLAB_HALO, edges=list(rs.SLAB_EDGES)) for r in range(n)]
        try:
            assert [e.x0 for e in es] == list(rs.SLAB_EDGES[:-1])
            pkg.Engine.link_local(es)
            for e in es:
                for k, v in (("fast_math", 1), ("fuse_steps", 2), ("tune", 0), ("refresh", refresh), ("trim_ghosts", trim)):
                    e.set_option(k, v)
                e.set_mask(mask)
                e.write_f(np.ascontiguousarray(f0[:, :, e.x0:e.x0 + e.width]))
            planes = []
            for k in calls:
                pkg.Engine.step_group(es, k, case.tau, rs.U0)
                parts = [_planes(e) for e in es]
                planes.append(tuple(np.concatenate(p, axis=-1) for p in zip(*parts)))
            for e in es:
                assert e.info().steps_done == case.steps
                _assert_contracted(e, name, {}, singles=bool(refresh))
                assert (e.get_option("trimmed_passes") > 0) == bool(trim), (name, e.get_option("trimmed_passes"))
                if refresh:
                    assert (e.get_option("boundary_exchanges") > 0) == (refresh == 1) and (e.get_option("fused_renewals") > 0) == (refresh == 2), name
        finally:
            for e in es:
                e.close()
        verdict.bound(name, planes, refs)
        if refresh:
            verdict.same_bits(name, planes, "whole lattice", whole, steps)
    verdict.close()


# F ---------------------------------------------------------------------------------------------------------------------------------------------
def test_plan_cut_by_measured_time(pkg, oracle_c):
    """Default fuse_chunk and tune on 1000 x 646: the units are timed and cut again, and the tuner's trial passes leave a contracted state as it was."""
    case, calls = fm.LARGE, fm.LARGE_CALLS
    refs = fm.references(oracle_c, case, calls)

    def check(e):
        assert e.get_option("tune") == 1.0 and e.get_option("tune_rounds") > 0
        print(case.id, {k: e.get_option(k) for k in ("fuse_depth", "fuse_units", "chain_units", "tune_rounds", "passes", "single_steps", "pass_depth")})
    planes, _ = _march(pkg, case, calls, "measured plan", {"fuse_depth": 4}, tune=None, check=check)
    verdict = _Verdict(case, calls)
    verdict.bound("measured plan", planes, refs)
    verdict.close()
