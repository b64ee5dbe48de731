"""GPU: the final sums of the sample reductions of batched sweeps (k_loads_batch, k_mex_batch, k_mex_ibb_batch, k_mex_half_batch) when a member holds more
than NT = 1024 column partials, so that the loop through LDS takes a second, partial trip: the carry of the running sums across
trips, the count of the last trip, the re-use of the LDS array.  1100 x 24, the members of tests/_wide_cases.py: a plate whose
window is 1062 columns wide, a block whose window is 22 columns wide in a grid sized by the plate, a member without a body.

The references are those of the narrow tests, evaluated on the batch's own state (read_f / read_macro after every sampled call), and
so are the tolerances, which are derived, not measured: Loads.mz_bound, Mex.fx_bound / fy_bound / mz_bound, MexIbb's with interpolated
walls.  The surface sums add the same doubles in the same order on both sides: same bits.

The three momentum-exchange kernels share one source text of that loop and are three code objects: each is taken past 1024 partials,
the half batch's as tests/test_gpu_polar_half.py compares its samples (_mex_reference on the batch's own read_f, which is Load of the
stored halves).
"""
import functools

import numpy as np
import pytest

from conftest import bits_equal
import _ibb_reference as ibb
import _mex_reference as mex
import _net_cases as nc
import _wide_cases as wc
from _loads_reference import loads_reference, surface_rows, surface_sums

pytestmark = pytest.mark.gpu

ROW_KEYS = ("fx", "fy", "mz", "fx_mex", "fy_mex", "mz_mex")


@functools.lru_cache(maxsize=None)
def _q(dtype):
    q = np.stack([nc.random_q(wc.NX, wc.NY, dtype, np.random.default_rng(7 + m)) for m in range(len(wc.MEMBERS))])
    q.setflags(write=False)
    return q


def _sequence(dtype, walls, swap, read=True, storage="native"):
    """CALLS sampled calls of EVERY steps from equilibrium; then, with `swap`, member 0's plate is replaced by a short block
    (set_masks keeps the flow); then one more sampled call.  After every call: the history so far is left to the end, the on-demand
    moment and momentum exchange and, with `read`, read_f and read_macro of every member."""
    import airfoil_cfd_tool_amd as pkg
    masks = wc.masks()
    B = len(wc.MEMBERS)
    tau, u0 = [m[0] for m in wc.MEMBERS], [m[1] for m in wc.MEMBERS]
    xr, yr = wc.refs()
    out = {"f": [], "macro": [], "moment": [], "mex": [], "masks": [masks] * wc.CALLS}
    with pkg.PolarEngine(wc.NX, wc.NY, B, dtype=dtype, history_cap=wc.CALLS + 1, storage=storage) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        if walls == "interpolated":
            b.enable_interpolated_walls()
            b.set_wall_distances(_q(dtype))
        b.enable_loads(xr, yr)
        b.enable_momentum_exchange(xr, yr)
        for call in range(wc.CALLS + 1):
            if call == wc.CALLS:
                out["surface"] = [b.surface(m) for m in range(B)]
                if swap:
                    b.set_masks(wc.short_mask(), first=0)
                    if walls == "interpolated":
                        b.set_wall_distances(_q(dtype)[0], first=0)         # (set_masks reset them to 0.5)
                    masks = masks.copy()
                    masks[0] = wc.short_mask()
                out["masks"].append(masks)
            b.step(wc.EVERY, tau, u0, sample_every=wc.EVERY)
            out["moment"].append(b.moment())
            out["mex"].append(b.momentum_exchange())
            if read:
                out["f"].append([b.read_f(m) for m in range(B)])
                out["macro"].append([b.read_macro(m) for m in range(B)])
        out["h"] = b.history()
    return out


@functools.lru_cache(maxsize=None)
def _swapped(dtype, walls):
    return _sequence(dtype, walls, True)


def _ratio(err, bound):
    return err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))


def _check_sums(run, dtype, walls):
    h = run["h"]
    B, rows = len(wc.MEMBERS), wc.CALLS + 1
    xr, yr = wc.refs()
    q = _q(dtype) if walls == "interpolated" else None
    assert list(h["step"]) == [wc.EVERY * (r + 1) for r in range(rows)]
    worst = dict.fromkeys(("mz", "fx_mex", "fy_mex", "mz_mex"), 0.0)
    for r in range(rows):
        masks = run["masks"][r]
        for m in range(B):
            f, rho = run["f"][r][m], run["macro"][r][m][0]
            lo = loads_reference(rho, masks[m], xr[m], yr[m])
            mx = mex.mex_reference(f, masks[m], xr[m], yr[m]) if q is None else ibb.mex_reference(f, masks[m], q[m], xr[m], yr[m])
            assert int(h["surf"][r, m]) == lo.n and int(h["links"][r, m]) == mx.links == int(run["mex"][r][3][m]), (r, m)
            assert (lo.n > 0 and mx.links > 0) == bool(masks[m].any())
            checks = (("mz", h["mz"][r, m], run["moment"][r][m], lo.mz, lo.mz_bound),
                      ("fx_mex", h["fx_mex"][r, m], run["mex"][r][0][m], mx.fx, mx.fx_bound),
                      ("fy_mex", h["fy_mex"][r, m], run["mex"][r][1][m], mx.fy, mx.fy_bound),
                      ("mz_mex", h["mz_mex"][r, m], run["mex"][r][2][m], mx.mz, mx.mz_bound))
            for what, row, call, want, bound in checks:
                assert row.tobytes() == call.tobytes(), (r, m, what)            # a history row is the on-demand call on that state
                err = abs(float(row) - want)
                worst[what] = max(worst[what], _ratio(err, bound))
                assert err <= bound, (dtype, walls, r, m, what, float(row), want, bound)
            if m == 0 and r < wc.CALLS:
                # not vacuous, on the reference: what the second trip adds is signal in every sum, and so is what the first adds
                late = (wc.second_trip_loads(lo, masks[0]),) + wc.second_trip_mex(mx, masks[0])
                for (what, _, _, want, bound), part in zip(checks, late):
                    assert abs(part) > 1e3 * bound and abs(want - part) > 1e3 * bound, (r, what, part, want, bound)
            if m == 0 and r == wc.CALLS:
                # the short body's window: partials past its width, left by the plate, are not read
                assert mx.links == 152 and wc.window(masks[0])[1] == 22 and abs(mx.fx) > 1e3 * mx.fx_bound and abs(lo.mz) > 1e3 * lo.mz_bound
    print(f"{dtype} {walls}: worst |x - ref| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f" over {rows} rows x {B} members")
    # the surface sums of the first CALLS samples (set_masks cleared member 0's afterwards): bits, on 1060 columns
    first = wc.masks()
    for m in range(B):
        s = run["surface"][m]
        ju, jl = surface_rows(first[m])
        su, sl, nu, nl = surface_sums([run["macro"][r][m][0] for r in range(wc.CALLS)], first[m])
        assert np.array_equal(s["j_upper"], ju) and np.array_equal(s["j_lower"], jl)
        assert np.array_equal(s["n_upper"], nu) and np.array_equal(s["n_lower"], nl)
        assert bits_equal(s["rho_upper"], su) and bits_equal(s["rho_lower"], sl)
        assert int((nu > 0).sum()) == int((nl > 0).sum()) == (1060, 20, 0)[m]
    assert (run["surface"][0]["n_upper"][wc.NT:1080] == wc.CALLS).all()


@pytest.mark.parametrize("walls", ["halfway", "interpolated"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_sums_past_1024_partials_match_the_references(dtype, walls):
    _check_sums(_swapped(dtype, walls), dtype, walls)


def test_half_storage_sums_past_1024_partials_match_the_references():
    """k_mex_half_batch's own second trip: the same lattice, masks, swap and checks on a half batch, whose read_f is Load of the stored
    halves, so that _mex_reference stands on the state the kernel summed."""
    run = _sequence("float32", "halfway", True, storage="half")
    assert run["f"][0][0].dtype == np.float32
    _check_sums(run, "float32", "halfway")
    native = _swapped("float32", "halfway")
    assert not bits_equal(run["h"]["fx_mex"], native["h"]["fx_mex"])               # (the half model's state, not the fp32 one's)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_short_member_is_untouched_and_runs_repeat(dtype):
    run = _swapped(dtype, "halfway")
    again = _sequence(dtype, "halfway", True, read=False)
    plain = _sequence(dtype, "halfway", False, read=False)
    for k in ROW_KEYS:
        assert bits_equal(again["h"][k], run["h"][k]), k                    # the same sequence twice: the same bits
        assert bits_equal(plain["h"][k][:, 1:], run["h"][k][:, 1:]), k      # members 1 and 2 never saw member 0's mask change
        assert bits_equal(plain["h"][k][:wc.CALLS], run["h"][k][:wc.CALLS]), k
        assert plain["h"][k][wc.CALLS, 0] != run["h"][k][wc.CALLS, 0], k    # (while member 0 did)
    for k in ("surf", "rev", "links"):
        assert np.array_equal(again["h"][k], run["h"][k]) and np.array_equal(plain["h"][k][:, 1:], run["h"][k][:, 1:]), k
    for a, c in zip(again["mex"][-1], run["mex"][-1]):
        assert a.tobytes() == c.tobytes()
    assert int(plain["h"]["links"][-1, 0]) == 6410 and int(run["h"]["links"][-1, 0]) == 152

