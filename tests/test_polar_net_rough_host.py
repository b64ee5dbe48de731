"""Every batch step kernel on the stability net from a rough start: what needs no GPU.  tests/test_gpu_polar_net_rough.py compares the
kernels with the references of tests/_net_rough_cases.py bit for bit; this file holds those references, alone, to the conditions that make
that comparison one of the clamp branches of every kernel: every population finite, the driven members on both kinds of bound at the early
checkpoints and the healthy one on none, every bound met in every tile class, no site with the bits of a neighbour or of its own past, each
storage and each collision a reference of its own, and the state after the first step depending on each of the three bounds to the last bit.
"""
import os

import numpy as np
import pytest

from conftest import ROOT
import lbm_numpy
import _half_reference as half
import _ibb_reference as ibb
import _net_cases as nc
import _net_rough_cases as nrc
import _restart_cases as rc
import _trt_cases as tc
import _trt_reference as trt

EVENTS_FILE = os.path.join(ROOT, "profiles", "polar_net_rough_events.txt")


def test_the_cases_are_the_ones_meant():
    assert len(nrc.ALL_CASES) == len(set(nrc.ALL_CASES)) == 64
    assert nrc.MARKS == (1, 3, 4, 7, 12, 19) and nrc.STEPS == rc.STEPS == 19
    assert {n % 2 for n in nrc.CALLS} == {0, 1}                                # both walk directions
    assert len(set(nrc.SEEDS)) == nrc.B == 3 and rc.TAU[nrc.HEALTHY] == 0.9
    for lattice in nrc.LATTICES:
        start = nrc.starts(lattice)
        assert np.isfinite(start).all()
        assert all(not np.array_equal(start[m], start[o]) for m in range(nrc.B) for o in range(m))
        for m in nrc.DRIVEN:                                                    # the noise itself lies beyond the bounds
            f = start[m].astype(np.float64)
            rho = f.sum(axis=0)
            speed = np.hypot(f[1] + f[5] + f[8] - f[3] - f[6] - f[7], f[2] + f[5] + f[6] - f[4] - f[7] - f[8]) / rho
            assert rho.min() < lbm_numpy.RHO_MIN and speed.max() > lbm_numpy.U_MAX, (lattice, m, rho.min(), speed.max())


@pytest.mark.parametrize("lattice,variant,stored", nrc.ALL_CASES, ids=nrc.IDS)
def test_the_reference_is_finite_on_the_net_and_sensitive(lattice, variant, stored):
    nx, ny, dtype = nrc.LATTICES[lattice]
    masks, q, start, runs = nrc.reference(lattice, variant, stored)
    assert (q is not None) is ("ibb" in variant)
    if stored:                                                                  # the start went through Store first
        assert all(start[m].dtype == np.float16 and start[m].tobytes() == half.store(nrc.starts(lattice)[m]).tobytes() for m in range(nrc.B))
    tj = 64 * (16 // np.dtype(dtype).itemsize)
    present = ("all",) if stored else (("fast",) if ny >= tj else ()) + ("general", "link")
    for m, run in enumerate(runs):
        assert len(run.states) == len(run.events) == len(run.insensitive) == len(nrc.MARKS) and len(run.per_step) == nrc.STEPS
        assert all(s.dtype == (np.float16 if stored else np.dtype(dtype)) and s.shape == (9, ny, nx) for s, _ in run.states)
        # a condition, not a measurement: NaN payloads are not comparable between NumPy and the device
        assert run.finite and run.max_abs < 10.0, (lattice, variant, m, run.max_abs)
        print(f"{nrc.case_id(lattice, variant, stored)} member {m}: max |f| {run.max_abs:.3g}; clamp_events at steps {nrc.MARKS}: {run.events}")
        assert run.insensitive == [(0, 0)] * len(nrc.MARKS), (lattice, variant, m, run.insensitive)
        classes = nrc.classes_of(lattice, stored)[m]
        assert set(classes) == ({"all"} if stored else {"fast", "general", "link"})
        assert all(bool(cells.any()) is (cls in present) for cls, cells in classes.items())
        if m == nrc.HEALTHY:
            assert run.events == [(0, 0)] * len(nrc.MARKS), (lattice, variant, m, run.events)
            assert all(run.met(kind, cls) == 0 for kind in nrc.KINDS for cls in classes)
            continue
        assert all(min(run.events[k]) > 0 for k in (0, 1)), (lattice, variant, m, run.events)
        assert run.events[2][1] > 0, (lattice, variant, m, run.events)
        if m == 0:
            met = {kind: {cls: run.met(kind, cls) for cls in present} for kind in nrc.KINDS}
            print(f"    (step, cell) pairs at a bound over the run: {met}")
            assert all(met[kind][cls] > 0 for kind in nrc.KINDS for cls in present), (lattice, variant, met)


@pytest.mark.parametrize("lattice,variant,stored", nrc.HALF_CASES, ids=[nrc.case_id(*c) for c in nrc.HALF_CASES])
def test_a_half_case_has_a_reference_of_its_own(lattice, variant, stored):
    """Store of the native reference is not the half reference: every step of the half one rounds to binary16."""
    runs, native = nrc.reference(lattice, variant, True)[3], nrc.reference(lattice, variant, False)[3]
    for m in range(nrc.B):
        for k in range(len(nrc.MARKS)):
            assert runs[m].states[k][0].tobytes() != half.store(native[m].states[k][0]).tobytes(), (lattice, variant, m, k)


@pytest.mark.parametrize("lattice,variant,stored", [c for c in nrc.ALL_CASES if nrc.is_trt(c[1])],
                         ids=[nrc.case_id(*c) for c in nrc.ALL_CASES if nrc.is_trt(c[1])])
def test_a_trt_case_differs_from_the_single_relaxation_time_one(lattice, variant, stored):
    runs, other = nrc.reference(lattice, variant, stored)[3], nrc.reference(lattice, tc.rc_variant(variant), stored)[3]
    for m in range(nrc.B):
        for k in range(len(nrc.MARKS)):
            assert runs[m].states[k][0].tobytes() != other[m].states[k][0].tobytes(), (lattice, variant, m, k)


# ---- the net itself ------------------------------------------------------------------------------
# (constant, the kind of event it sets, the direction of the neighbouring value: each bound moves inwards)
BOUNDS = (("U_MAX", "u", 0.0), ("RHO_MIN", "rho_min", 1.0), ("RHO_MAX", "rho_max", 1.0))


@pytest.mark.parametrize("bound,kind,towards", BOUNDS, ids=[b[0] for b in BOUNDS])
@pytest.mark.parametrize("variant", ["bgk", "les", "trt", "trt+les"])
@pytest.mark.parametrize("lattice", list(nrc.LATTICES))
def test_the_first_step_depends_on_each_bound_to_the_last_bit(monkeypatch, lattice, variant, bound, kind, towards):
    """One variant per collision.  With one bound moved by one ulp of the lattice's dtype, the state after the first step changes in
    bits in cells that sit at that bound, and in no cell that sits at none: a kernel whose copy of the clamp held another constant, or
    applied it elsewhere, would not have the reference's bits."""
    nx, ny, dtype = nrc.LATTICES[lattice]
    T = np.dtype(dtype).type
    masks, q, start, runs = nrc.reference(lattice, variant)                    # (computed with the constants as they are)
    events = {m: nc.event_cells(runs[m].states[0][1]) for m in nrc.DRIVEN}      # (likewise)
    today = getattr(lbm_numpy, bound)
    moved = float(np.nextafter(T(today), T(towards)))
    assert T(moved) != T(today)
    for module in (lbm_numpy, ibb, trt):                                        # the three modules that bind the constants by name
        assert getattr(module, bound) == today
        monkeypatch.setattr(module, bound, moved)
    for m in nrc.DRIVEN:
        want, ev = runs[m].states[0][0], events[m]
        got = nrc.stepper(variant, m, masks[m], None, dtype)(start[m])[0]
        differs = (got.view(np.uint8) != want.view(np.uint8)).reshape(9, ny, nx, -1).any(axis=(0, 3))
        at = ev[kind] & nc.interior_fluid(masks[m])
        elsewhere = ~(ev["u"] | ev["rho_max"] | ev["rho_min"])
        print(f"{lattice} {variant} member {m}, {bound} -> {moved!r}: {int((differs & at).sum())} of {int(at.sum())} cells at the bound change")
        assert (differs & at).any(), (lattice, variant, m, bound)
        assert not (differs & elsewhere).any(), (lattice, variant, m, bound)   # (and the step is local: no cell off the net changes)


def test_the_committed_table_of_events_is_the_references():
    """profiles/polar_net_rough_events.txt is _net_rough_cases.table(), as printed."""
    with open(EVENTS_FILE) as fh:
        assert fh.read() == nrc.table()
