"""GPU: every batch step kernel on the stability net from a rough start: the density clamp (0.5 / 2.0) and the velocity clamp (0.35) in
collide, collide_les and collide_trt, in the straight-line path of TILE_FAST tiles and in site_general, with half-way and interpolated
walls, the inclined free stream and half storage (the instantiations of k_step_batch and
k_step_half_batch), against the NumPy references of tests/_net_rough_cases.py.

There is no tolerance on the state: the kernels and the references round every operation once, in the same order, so populations (or
stored halves) and macroscopic fields are the same bits at every checkpoint, clamped cells included, and the event counts are equal.
That the references are finite, sit on every bound in every tile class and depend on each bound to the last bit is asserted in
tests/test_polar_net_rough_host.py.  The momentum exchange of the state after the first step, when thousands of cells are clamped and
the populations are O(1) and far from equilibrium (k_mex_batch, k_mex_half_batch), is held to the derived summation bounds of
_mex_reference / _ibb_reference.
"""
import numpy as np
import pytest

from conftest import bits_equal
import _half_reference as half
import _ibb_reference as ibb
import _mex_reference as mex
import _net_rough_cases as nrc
import _restart_cases as rc

pytestmark = pytest.mark.gpu


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rows_differ(got, want):
    g, w = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    return int((g != w).reshape(got.shape[0], got.shape[-2], -1).any(axis=(0, 2)).sum())


@pytest.mark.parametrize("lattice,variant,stored", nrc.ALL_CASES, ids=nrc.IDS)
def test_state_on_the_net_from_a_rough_start_is_the_references_bits(pkg, lattice, variant, stored):
    nx, ny, dtype = nrc.LATTICES[lattice]
    masks, q, start, runs = nrc.reference(lattice, variant, stored)           # continued from its own checkpoints, never from the device's
    rough = nrc.starts(lattice)
    B = nrc.B
    xr, yr = [0.3641 * nx + 1.7 * m for m in range(B)], [0.5 * ny - 0.85 * m - 3.3 for m in range(B)]
    assert all(r.finite and len(r.states) == len(nrc.MARKS) for r in runs)    # no NaN or infinity is compared, or written
    assert np.isfinite(rough).all()
    with pkg.PolarEngine(nx, ny, B, dtype=dtype, storage="half" if stored else "native") as b:
        nrc.configure(b, variant, masks, q)
        assert b.trt_enabled is nrc.is_trt(variant)
        assert b.les_enabled is ("les" in variant) and b.interpolated_walls is ("ibb" in variant) and b.wind_enabled is ("wind" in variant)
        b.enable_momentum_exchange(xr, yr)
        for m in range(B):
            b.write_f(m, rough[m])                                            # in a half batch through Store, on the device
        for m in range(B):
            if stored:
                assert _same(b.read_stored(m), start[m].view(np.uint16)), (lattice, variant, m, "start")
            else:
                assert _same(b.read_f(m), start[m]), (lattice, variant, m, "start")
        forces = None
        for k, n in enumerate(nrc.CALLS):
            b.step(n, rc.TAU, rc.U0)
            mark = nrc.MARKS[k]
            assert b.step_count == mark
            rho_ev, u_ev = b.clamp_events()
            for m in range(B):
                want, want_macro = runs[m].states[k]
                if stored:
                    got = b.read_stored(m)
                    assert _same(got, want.view(np.uint16)), (lattice, variant, "member", m, "step", mark, _rows_differ(got, want), "rows differ")
                else:
                    got = b.read_f(m)
                    assert bits_equal(got, want), (lattice, variant, "member", m, "step", mark, _rows_differ(got, want), "rows differ")
                for g, w, what in zip(b.read_macro(m), want_macro, ("rho", "ux", "uy")):
                    assert bits_equal(g, w), (lattice, variant, "member", m, "step", mark, what, _rows_differ(g[None], w[None]), "rows differ")
                assert (int(rho_ev[m]), int(u_ev[m])) == runs[m].events[k], (lattice, variant, m, mark)
            if k == 0:                                                          # the state is now fully on the net
                forces = b.momentum_exchange()
                loaded = [b.read_f(m) for m in range(B)]
    fx, fy, mz, links = forces
    worst = [0.0, 0.0, 0.0]
    for m in range(B):
        f = runs[m].states[0][0]                                                # the device's bits, as asserted above
        if stored:
            f = half.load(f)
            assert _same(loaded[m], f), (lattice, variant, m)                   # read_f is Load of the halves
        ref = ibb.mex_reference(f, masks[m], q[m], xr[m], yr[m]) if "ibb" in variant else mex.mex_reference(f, masks[m], xr[m], yr[m])
        assert int(links[m]) == ref.links > 200, (lattice, variant, m, links[m], ref.links)
        for j, (got, want, bound) in enumerate(((fx[m], ref.fx, ref.fx_bound), (fy[m], ref.fy, ref.fy_bound), (mz[m], ref.mz, ref.mz_bound))):
            err = abs(float(got) - want)
            worst[j] = max(worst[j], err / bound)
            assert err <= bound, (lattice, variant, m, "fx fy mz".split()[j], float(got), want, bound)
        if m in nrc.DRIVEN:
            assert min(runs[m].events[0]) > 0 and float(np.abs(f).max()) > 1.0   # (populations of a clamped state, not near equilibrium)
        else:
            assert runs[m].events == [(0, 0)] * len(nrc.MARKS)                  # the driven members do not leak into the healthy one
    print(f"{nrc.case_id(lattice, variant, stored)}: steps {nrc.MARKS}, bit-identical; momentum exchange at step {nrc.MARKS[0]}: worst |x - ref| / bound = "
          f"{worst[0]:.3g} (fx), {worst[1]:.3g} (fy), {worst[2]:.3g} (mz)")
