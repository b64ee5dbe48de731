"""Batched sweeps at the stability net: what needs no GPU.  tests/test_gpu_polar_net.py compares the step kernels with the references
of tests/_net_cases.py bit for bit; this file holds those references to the conditions that make the comparison one of the clamp
branches: on the reference alone, every driven member has met every bound of the net in every tile class of its lattice by the
checkpoint that is meant to meet it, with every population finite.
"""
import numpy as np
import pytest

import lbm_numpy
import _les_reference as les
import _net_cases as nc

PAIRS = [(name, config) for name in nc.CASES for config in nc.CONFIGS]
IDS = [f"{name}-{config}" for name, config in PAIRS]


@pytest.mark.parametrize("name", list(nc.CASES))
def test_lattices_hold_the_tile_classes_they_were_chosen_for(name):
    nx, ny, dtype = nc.CASES[name]
    masks, q = nc.inputs(name)
    tj = 64 * (16 // np.dtype(dtype).itemsize)
    for m in range(len(nc.MEMBERS)):
        fast = nc.fast_cells(masks[m], dtype)
        classes = nc.cell_classes(masks[m], dtype)
        assert classes["general"].sum() > 1000 and classes["link"].sum() > 200
        if ny < tj:
            assert not fast.any()                                           # ragged tiles only
            continue
        assert ny // tj == 1 and ny % tj != 0                               # one full tile and a ragged one per column
        assert not fast[tj:].any() and classes["general"][tj:].sum() > (ny - tj - 2) * (nx - 2) * 0.8
        cols = np.flatnonzero(fast[0])
        assert cols.size >= 4 and cols[0] == 1 and cols[-1] == nx - 2       # FAST columns either side of the body
        assert fast[:tj, cols].all() and classes["fast"].sum() > 800
        body = np.flatnonzero(masks[m][:tj].any(axis=0))
        assert not fast[:, body[0] - 1:body[-1] + 2].any()                  # the body's columns and their neighbours are GENERAL


@pytest.mark.parametrize("name", list(nc.CASES))
def test_wall_distances_and_narrow_gaps(name):
    from _ibb_reference import fallback_links
    from _mex_reference import link_masks
    masks, q = nc.inputs(name)
    for m in range(len(nc.MEMBERS)):
        own = np.stack(link_masks(masks[m])[1:])
        counts = [int((own & sel).sum()) for sel in (q[m] < 0.5, q[m] > 0.5, q[m] == 0.5, q[m] == 1, q[m] == q.dtype.type(2.0 ** -12))]
        fallback = fallback_links(masks[m], q[m])
        print(f"{name} member {m}: {int(own.sum())} links, q < 0.5 at {counts[0]}, > 0.5 at {counts[1]}, = 0.5 at {counts[2]}, = 1 at {counts[3]}, "
              f"= 2^-12 at {counts[4]}; {fallback} short links with a wall behind")
        assert min(counts) > 0 and fallback > 0


@pytest.mark.parametrize("name,config", PAIRS, ids=IDS)
def test_the_reference_meets_every_bound_in_every_tile_class(name, config):
    nx, ny, dtype = nc.CASES[name]
    masks, _ = nc.inputs(name)
    marks = nc.CHECKPOINTS[name]
    runs = nc.reference(name, config)
    assert len(marks) == len(nc.KINDS) and list(marks) == sorted(set(marks))
    for m, run in enumerate(runs):
        classes = nc.cell_classes(masks[m], dtype)
        present = [cls for cls in ("fast", "general") if classes[cls].any()] + (["link"] if config != "les" else [])
        assert len(run.states) == len(marks)
        # a condition, not a measurement: NaN payloads are not comparable between NumPy and the device
        assert run.finite and run.max_abs < 10.0, (name, config, m, run.max_abs)
        at_marks = [lbm_numpy.clamp_events(*macro, masks[m]) for _, macro in run.states]
        print(f"{name} {config} member {m}: max |f| {run.max_abs:.3g}; clamp_events at steps {marks}: {at_marks}")
        if m == nc.HEALTHY:
            assert all(v is None for kind in nc.KINDS for v in run.first[kind].values())
            assert at_marks == [(0, 0)] * len(marks)
            continue
        for k, kind in enumerate(nc.KINDS):
            print(f"    {kind}: first met at step {run.first[kind]}, (step, cell) pairs by step {marks[k]}: {run.counted[k][kind]}")
            for cls in present:
                assert run.first[kind][cls] is not None and run.first[kind][cls] <= marks[k], (name, config, m, kind, cls, run.first[kind][cls])
                assert run.counted[k][kind][cls] > 0
        assert all(e != (0, 0) for e in at_marks) and min(at_marks[-1]) > 0     # wtp_clamp_events has something to report
        cs = 0.0 if config == "ibb-bgk" else nc.MEMBERS[m][2]
        if cs > 0:                                                             # the model acts at every cell that sits at a bound
            assert run.at_bound > 1000 and run.acted == run.at_bound, (name, config, m, run.acted, run.at_bound)
        else:
            assert run.at_bound == 0


@pytest.mark.parametrize("name", list(nc.CASES))
def test_references_agree_with_the_bgk_oracle_at_the_net(name):
    """From a state on the net (the cs = 0 member at its last checkpoint): _les_reference with c = 0 and _ibb_reference with every
    distance at 0.5, with either collision at c = 0, give lbm_numpy.step's populations and moments, whose clamp is held to the C
    oracle and the page's shader."""
    import _ibb_reference as ibb
    nx, ny, dtype = nc.CASES[name]
    masks, _ = nc.inputs(name)
    tau, u0, _ = nc.MEMBERS[1]
    f, macro = nc.reference(name, "les")[1].states[2]
    ev = nc.event_cells(lbm_numpy.step(f, masks[1], tau, u0)[1])
    fluid = nc.interior_fluid(masks[1])
    assert (ev["u"] & fluid).any() and ((ev["rho_max"] | ev["rho_min"]) & fluid).any()
    want_f, want_macro = lbm_numpy.step(f, masks[1], tau, u0)
    zero, half = les.les_constant(0.0, dtype), np.full((8, ny, nx), 0.5, dtype)
    got = [les.step(f, masks[1], tau, u0, zero)[:2], ibb.step(f, masks[1], tau, u0, half, None), ibb.step(f, masks[1], tau, u0, half, zero)]
    for k, (gf, gm) in enumerate(got):
        assert np.array_equal(gf, want_f), k
        assert all(np.array_equal(a, b) for a, b in zip(gm, want_macro)), k
