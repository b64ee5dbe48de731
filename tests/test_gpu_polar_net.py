"""GPU: the step kernels of batched sweeps at the stability net: the density clamp (0.5 / 2.0) and the velocity clamp (0.35) under the
Smagorinsky collision (k_step_batch with COLLIDE_LES) and under interpolated walls with either collision (WALL_INTERP), in the straight-line
path of TILE_FAST tiles and in site_general, against the NumPy references of tests/_net_cases.py.

There is no tolerance on the state: the kernels and the references round every operation once, in the same order, so populations
and macroscopic fields are the same bits at every checkpoint, clamped cells included.  That the references reach every bound in
every tile class by these checkpoints, with every population finite, is asserted in tests/test_polar_net_host.py.  The momentum
exchange of the clamped state, whose populations are O(1) and far from equilibrium, is held to the derived summation bounds of
_mex_reference / _ibb_reference.
"""
import numpy as np
import pytest

from conftest import bits_equal
import lbm_numpy
import _ibb_reference as ibb
import _mex_reference as mex
import _net_cases as nc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("config", nc.CONFIGS)
@pytest.mark.parametrize("name", list(nc.CASES))
def test_state_at_the_net_is_the_references_bits(pkg, name, config):
    nx, ny, dtype = nc.CASES[name]
    masks, q = nc.inputs(name)
    marks = nc.CHECKPOINTS[name]
    runs = nc.reference(name, config)                                       # continued from its own checkpoints, never from the device's
    B = len(nc.MEMBERS)
    tau, u0, cs = ([m[k] for m in nc.MEMBERS] for k in range(3))
    xr, yr = [0.3641 * nx + 1.7 * m for m in range(B)], [0.5 * ny - 0.85 * m - 3.3 for m in range(B)]
    assert all(r.finite and len(r.states) == len(marks) for r in runs)
    with pkg.PolarEngine(nx, ny, B, dtype=dtype) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        if config != "les":
            b.enable_interpolated_walls()
            b.set_wall_distances(q)
        if config != "ibb-bgk":
            b.enable_les(cs)
        b.enable_momentum_exchange(xr, yr)
        done = 0
        for k, mark in enumerate(marks):
            b.step(mark - done, tau, u0)
            done = mark
            rho_ev, u_ev = b.clamp_events()
            for m in range(B):
                want_f, want_macro = runs[m].states[k]
                f, macro = b.read_f(m), b.read_macro(m)
                bad = int((f.view(np.uint8) != want_f.view(np.uint8)).reshape(9, ny, -1).any(axis=(0, 2)).sum())
                assert bits_equal(f, want_f), (name, config, "member", m, "step", mark, bad, "rows differ")
                for got, want, what in zip(macro, want_macro, ("rho", "ux", "uy")):
                    bad = int((got.view(np.uint8) != want.view(np.uint8)).reshape(ny, -1).any(axis=1).sum())
                    assert bits_equal(got, want), (name, config, "member", m, "step", mark, what, bad, "rows differ")
                want_ev = lbm_numpy.clamp_events(*want_macro, masks[m])
                assert (int(rho_ev[m]), int(u_ev[m])) == want_ev, (name, config, m, mark)
                if m == nc.HEALTHY:
                    assert want_ev == (0, 0)                                # the driven members do not leak into it
                else:
                    assert want_ev != (0, 0) and (k + 1 < len(marks) or min(want_ev) > 0), (name, config, m, mark, want_ev)
        fx, fy, mz, links = b.momentum_exchange()
    worst = [0.0, 0.0, 0.0]
    for m in range(B):
        f = runs[m].states[-1][0]                                           # the device's bits, as asserted above
        ref = mex.mex_reference(f, masks[m], xr[m], yr[m]) if config == "les" else ibb.mex_reference(f, masks[m], q[m], xr[m], yr[m])
        assert int(links[m]) == ref.links > 200, (name, config, m, links[m], ref.links)
        for k, (got, want, bound) in enumerate(((fx[m], ref.fx, ref.fx_bound), (fy[m], ref.fy, ref.fy_bound), (mz[m], ref.mz, ref.mz_bound))):
            err = abs(float(got) - want)
            worst[k] = max(worst[k], err / bound)
            assert err <= bound, (name, config, m, "fx fy mz".split()[k], float(got), want, bound)
        if m != nc.HEALTHY:
            assert float(np.abs(f).max()) > 1.0                             # (populations of a clamped state, not near equilibrium)
    print(f"{name} {config}: steps {marks}, bit-identical; momentum exchange at step {marks[-1]}: worst |x - ref| / bound = "
          f"{worst[0]:.3g} (fx), {worst[1]:.3g} (fy), {worst[2]:.3g} (mz)")
