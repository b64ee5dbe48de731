"""Sample reductions of batched sweeps past 1024 columns: what needs no GPU.  tests/test_gpu_polar_wide.py compares the kernels with
the references on the batch's own state; this file checks, on the NumPy references' state after the same steps, that the members of
tests/_wide_cases.py make that comparison one of the second trip of the final sums: member 0's partials reach past index 1023 in
all three kernels and the terms added there are signal, 1e3 times the comparison's bound, in every sum.
"""
import functools

import numpy as np
import pytest

import lbm_numpy
import _ibb_reference as ibb
import _mex_reference as mex
import _net_cases as nc
import _wide_cases as wc
from _loads_reference import loads_reference


@functools.lru_cache(maxsize=None)
def _state(dtype, walls, steps):
    """Member 0 after `steps` steps from equilibrium: (f, rho, q)."""
    mask = wc.masks()[0]
    tau, u0 = wc.MEMBERS[0]
    if walls == "halfway":
        f = None if steps == wc.EVERY else _state(dtype, walls, steps - wc.EVERY)[0]
        f, macro = lbm_numpy.run(mask, wc.EVERY, tau, u0, np.dtype(dtype), f=f)
        return f, macro[0], None
    q = nc.random_q(wc.NX, wc.NY, dtype, np.random.default_rng(7))
    f = None if steps == wc.EVERY else _state(dtype, walls, steps - wc.EVERY)[0]
    f, macro = ibb.run(mask, wc.EVERY, tau, u0, q, None, np.dtype(dtype), f=f)
    return f, macro[0], q


def test_members_have_the_windows_they_were_chosen_for():
    masks = wc.masks()
    widths = [wc.window(m) for m in masks]
    assert widths[0] == (19, 1062) and widths[0][1] > wc.NT and widths[1] == (399, 22) and widths[2][1] == 0
    assert wc.window(wc.short_mask()) == (699, 22)
    assert wc.NX > wc.NT and wc.NX % wc.NT != 0                            # k_loads_batch: a full trip and a partial one
    assert masks[0][:, wc.NT:].any() and not masks[1][:, wc.NT:].any()
    upper = masks[0][14:, :].sum(axis=0)
    assert not upper[:1050].any() and upper[1050:1080].all()               # the step lies past column 1024 and past window index 1024
    assert 1050 - widths[0][0] >= wc.NT
    assert [mex.count_links(m) for m in masks] == [6410, 164, 0] and mex.count_links(wc.short_mask()) == 152
    assert (wc.loads_columns(masks[0]) >= wc.NT).sum() > 100 and (wc.mex_columns(masks[0]) - widths[0][0] >= wc.NT).sum() > 100


@pytest.mark.parametrize("call", range(1, wc.CALLS + 1))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("walls", ["halfway", "interpolated"])
def test_the_second_trip_carries_signal(dtype, walls, call):
    mask = wc.masks()[0]
    xr, yr = wc.refs()
    f, rho, q = _state(dtype, walls, wc.EVERY * call)
    assert np.isfinite(f).all()
    lo = loads_reference(rho, mask, xr[0], yr[0])
    late = wc.second_trip_loads(lo, mask)
    print(f"{dtype} {walls} step {wc.EVERY * call}: loads Mz {lo.mz:.6g}, second trip {late:.6g}, bound {lo.mz_bound:.3g}")
    assert abs(late) > 1e3 * lo.mz_bound and abs(lo.mz - late) > 1e3 * lo.mz_bound      # (and so does the first)
    mx = mex.mex_reference(f, mask, xr[0], yr[0]) if q is None else ibb.mex_reference(f, mask, q, xr[0], yr[0])
    sums = wc.second_trip_mex(mx, mask)
    for what, part, whole, bound in zip(("fx", "fy", "mz"), sums, (mx.fx, mx.fy, mx.mz), (mx.fx_bound, mx.fy_bound, mx.mz_bound)):
        print(f"{dtype} {walls} step {wc.EVERY * call}: momentum exchange {what} {whole:.6g}, second trip {part:.6g}, bound {bound:.3g}")
        assert abs(part) > 1e3 * bound and abs(whole - part) > 1e3 * bound, what
