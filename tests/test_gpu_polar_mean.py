"""GPU: mean fields of batched sweeps (k_mean_batch) against the NumPy loop of tests/_mean_reference.py over the batch's own
wtp_read_macro at the sampled steps.

There is no tolerance: both sides add the same doubles in the same order with one rounding per operation, so the seven sums and
the count are the same bits.  Only the run_polar test compares means formed two ways, within _mean_reference.mean_bound.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

from conftest import bits_equal
from _mean_reference import SUMS, accumulate, mean_bound, mean_flow_reference
from test_gpu_polar_loads import MEMBERS

pytestmark = pytest.mark.gpu

WT_ERR_ARG, WT_ERR_STATE = -1, -5
EVERY = 12
FP64_MEMBERS = [("naca4412", 14.0, 0.56, 0.08), ("naca0012", 4.0, 0.58, 0.06), ("clark_y", -6.0, 0.9, 0.03)]


def _masks(pkg, nx, ny, members):
    return np.stack([pkg.geometry.build_geometry(nx, ny, a, None, s).mask for s, a, _, _ in members])


def _block_masks(nx, ny, n):
    """One solid rectangle per member, at another place in each: any lattice takes it."""
    masks = np.zeros((n, ny, nx), np.uint8)
    for m in range(n):
        j0, i0 = ny // 2 - 20 + 37 * m, nx // 3 + 3 * m
        masks[m, j0:j0 + 31, i0:i0 + 7] = 1
    return masks


def _sampled_run(pkg, nx, ny, masks, members, dtype, calls, mean=True, others=False, read=True):
    """`calls` calls of EVERY steps, each ending in a sample; read: wtp_read_macro of every member after each call, the
    reference's input.  others: the surface loads and the momentum exchange are on as well."""
    tau, u0 = [m[2] for m in members], [m[3] for m in members]
    B = len(members)
    out = {"masks": masks, "samples": [[] for _ in range(B)]}
    with pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=calls) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        if others:
            b.enable_loads(0.36 * nx, 0.5 * ny - 0.85)
            b.enable_momentum_exchange(0.37 * nx, 0.5 * ny + 1.3)
        if mean:
            b.enable_mean_fields()
        for _ in range(calls):
            b.step(EVERY, tau, u0, sample_every=EVERY)
            if read:
                for m in range(B):
                    out["samples"][m].append(b.read_macro(m))
        if mean:
            out["sums"] = [b.mean_sums(m) for m in range(B)]
        out["h"] = b.history()
        out["forces"] = b.forces()
        if others:
            out["surface"] = [b.surface(m) for m in range(B)]
        out["f"] = [b.read_f(m) for m in range(B)]
        out["macro"] = [b.read_macro(m) for m in range(B)]
        out["clamp"] = b.clamp_events()
    return out


def _assert_bit_identical(run, calls):
    for m, got in enumerate(run["sums"]):
        ref = accumulate(run["samples"][m])
        assert got["n"] == ref["n"] == calls, (m, got["n"])
        for k in SUMS:
            assert got[k].dtype == np.float64 and got[k].shape == run["masks"][m].shape
            diff = int((got[k].view(np.uint64) != ref[k].view(np.uint64)).sum())
            assert bits_equal(got[k], ref[k]), (m, k, diff, "entries differ")
        assert ref["rho"].min() > 0.5 * calls and np.isfinite(ref["ux2"]).all()
    print(f"mean sums: {len(run['sums'])} members x 7 planes of {run['masks'][0].shape}, {calls} samples, bit-identical")


@pytest.fixture(scope="module")
def run_320(pkg):
    return _sampled_run(pkg, 320, 160, _masks(pkg, 320, 160, MEMBERS), MEMBERS, "float32", 20)


def test_sums_are_bit_identical(run_320):
    _assert_bit_identical(run_320, 20)


def test_the_comparison_is_not_vacuous(run_320):
    """On the reference itself: the flow fluctuates at every fluid cell whose values a step computes, and the members differ.
    The far-field cells (inlet column, top and bottom rows) are fluid too, but the boundary condition pins their emitted values
    to (1, U0, 0) at every step, and the two corner cells of the outlet column copy such a cell: there the central moment is
    exactly 0, which is asserted instead."""
    u0 = [m[3] for m in MEMBERS]
    for m in (0, 1, 4):
        ref = mean_flow_reference(run_320["samples"][m], u0[m])
        fluid = run_320["masks"][m] == 0
        far = np.zeros_like(fluid)
        far[:, 0] = far[0, :] = far[-1, :] = True                      # (the outlet column copies its neighbour: computed, but for its corners)
        evolved = fluid & ~far
        print(f"member {m}: uu over {int(evolved.sum())} computed fluid cells: {int((ref['uu'][evolved] == 0).sum())} at 0, min {ref['uu'][evolved].min():.3g}, max {ref['uu'][evolved].max():.3g}; "
              f"{int((ref['uu'][far & fluid] == 0).sum())} of {int((far & fluid).sum())} far-field cells at 0")
        assert (ref["uu"][evolved] > 0).all()
        assert (ref["uu"][far & fluid] == 0).all() and (ref["ux"][:, :-1][(far & fluid)[:, :-1]] == np.float32(u0[m])).all()
        assert (ref["uu"][~fluid] == 0).all() and (ref["rho"][~fluid] == 1).all()       # solid cells emit (1, 0, 0)
    a, b = run_320["sums"][0], run_320["sums"][1]
    for k in SUMS:
        assert (a[k] != b[k]).mean() > 0.9, k


def test_ragged_lattice(pkg):
    """301x150 fp32: NX no multiple of 4, NY no multiple of 64; 75 two-row runs per column, so a wave spans columns."""
    members = MEMBERS[:2]
    run = _sampled_run(pkg, 301, 150, _masks(pkg, 301, 150, members), members, "float32", 6)
    _assert_bit_identical(run, 6)


def test_fp64_batch(pkg):
    """96x48 fp64: NY below one 64-row chunk; the products round once on both sides."""
    run = _sampled_run(pkg, 96, 48, _masks(pkg, 96, 48, FP64_MEMBERS), FP64_MEMBERS, "float64", 8)
    _assert_bit_identical(run, 8)
    x = run["samples"][0][-1][1].astype(np.float64)
    assert (x.astype(np.longdouble) * x.astype(np.longdouble) != x * x).any()       # (fp64 values whose squares do round)


@pytest.mark.parametrize("nx,ny", [(40, 300), (37, 299)])
def test_tall_lattice(pkg, nx, ny):
    """40x300 fp32: pitch 512, more than one 256-row block in a column, 212 pad rows that are never moved.  37x299: an odd NY, whose
    last run of a column owns one row."""
    members = [("block", 0.0, 0.6, 0.05), ("block", 0.0, 0.75, 0.08)]
    run = _sampled_run(pkg, nx, ny, _block_masks(nx, ny, 2), members, "float32", 5)
    _assert_bit_identical(run, 5)
    assert not bits_equal(run["sums"][0]["ux"], run["sums"][1]["ux"])


@pytest.fixture(scope="module")
def run_on(pkg, run_320):
    return _sampled_run(pkg, 320, 160, run_320["masks"], MEMBERS, "float32", 20, mean=True, others=True, read=False)


def test_two_runs_give_the_same_bits(run_320, run_on):
    """... and the sums do not depend on the other read-outs being on."""
    for m in range(len(MEMBERS)):
        assert run_on["sums"][m]["n"] == run_320["sums"][m]["n"] == 20
        for k in SUMS:
            assert bits_equal(run_on["sums"][m][k], run_320["sums"][m][k]), (m, k)


def test_the_sampling_changes_nothing_else(pkg, run_320, run_on):
    off = _sampled_run(pkg, 320, 160, run_320["masks"], MEMBERS, "float32", 20, mean=False, others=True, read=False)
    keys = ["step", "fx", "fy", "surf", "rev", "mz", "fx_mex", "fy_mex", "mz_mex", "links"]
    assert list(off["h"]) == keys and list(run_on["h"]) == keys
    for k in keys:
        assert run_on["h"][k].tobytes() == off["h"][k].tobytes(), k
    assert np.isfinite(off["h"]["mz"]).all() and np.isfinite(off["h"]["fx_mex"]).all() and (off["h"]["links"] > 0).all()
    for a, b in zip(run_on["forces"], off["forces"]):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(run_on["clamp"], off["clamp"]):
        assert np.array_equal(a, b)
    for m in range(len(MEMBERS)):
        for k, v in run_on["surface"][m].items():
            assert v.tobytes() == off["surface"][m][k].tobytes(), (m, k)
        assert bits_equal(run_on["f"][m], off["f"][m])
        assert all(bits_equal(a, b) for a, b in zip(run_on["macro"][m], off["macro"][m]))
    # and a batch with the mean fields alone has the forces and the state of one with everything on
    for k in ("fx", "fy"):
        assert bits_equal(run_320["h"][k], off["h"][k]), k
    for m in range(len(MEMBERS)):
        assert bits_equal(run_320["f"][m], off["f"][m])


def test_life_cycle(pkg):
    nx, ny = 160, 80
    members = MEMBERS[:3]
    tau, u0 = [m[2] for m in members], [m[3] for m in members]
    masks = _masks(pkg, nx, ny, members)

    def counts(b):
        return [b.mean_sums(m)["n"] for m in range(3)]

    def is_zero(s):
        return s["n"] == 0 and not any(s[k].any() for k in SUMS)

    def same(s, t):
        return s["n"] == t["n"] and all(bits_equal(s[k], t[k]) for k in SUMS)

    with pkg.PolarEngine(nx, ny, 3, history_cap=16) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        assert not b.mean_enabled
        with pytest.raises(pkg.WTError) as ei:
            b.mean_sums(0)
        assert ei.value.code == WT_ERR_STATE and "wtp_enable_mean" in str(ei.value)
        b.step(EVERY, tau, u0, sample_every=EVERY)                      # a sample before the read-out is on: not in the sums
        b.enable_mean_fields()
        assert b.mean_enabled and all(is_zero(b.mean_sums(m)) for m in range(3))
        for member in (-1, 3):
            with pytest.raises(pkg.WTError) as ei:
                b.mean_sums(member)
            assert ei.value.code == WT_ERR_ARG
        b.step(3 * EVERY, tau, u0, sample_every=EVERY)
        assert counts(b) == [3, 3, 3] and len(b.history()["step"]) == 4
        b.step(5, tau, u0)                                              # sample_every = 0: no sample, nothing added
        b.step(7, tau, u0, sample_every=0)
        before = [b.mean_sums(m) for m in range(3)]
        assert [s["n"] for s in before] == [3, 3, 3] and before[0]["rho"].min() > 2.5
        # the on-demand calls add nothing
        b.enable_loads(0.36 * nx, 0.5 * ny)
        b.enable_momentum_exchange(0.36 * nx, 0.5 * ny)
        b.forces(), b.moment(), b.momentum_exchange()
        assert all(same(b.mean_sums(m), before[m]) for m in range(3))
        # any output may be NULL
        n = np.zeros(1, np.int64)
        uy2 = np.empty((ny, nx))
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
        assert b._lib.wtp_mean_sums(b._b, 2, n.ctypes.data_as(ip), None, None, None, None, None, uy2.ctypes.data_as(dp), None) == 0
        assert n[0] == 3 and bits_equal(uy2, before[2]["uy2"])
        assert b._lib.wtp_mean_sums(b._b, 2, None, None, None, None, None, None, None, None) == 0
        # a new mask restarts the touched member only
        b.set_masks(pkg.geometry.build_geometry(nx, ny, 9.0, None, "naca0012").mask, first=1)
        assert is_zero(b.mean_sums(1)) and same(b.mean_sums(0), before[0]) and same(b.mean_sums(2), before[2])
        b.step(EVERY, tau, u0, sample_every=EVERY)
        assert counts(b) == [4, 1, 4]
        b.clear_history()
        assert all(is_zero(b.mean_sums(m)) for m in range(3))
        b.step(2 * EVERY, tau, u0, sample_every=EVERY)
        assert counts(b) == [2, 2, 2]
        b.enable_mean_fields()                                          # again: zeroed
        assert all(is_zero(b.mean_sums(m)) for m in range(3))
        b.step(EVERY, tau, u0, sample_every=EVERY)
        assert counts(b) == [1, 1, 1]
        rho, ux, uy = (a.astype(np.float64) for a in b.read_macro(1))
        one = b.mean_sums(1)
        assert bits_equal(one["rho"], rho) and bits_equal(one["uxuy"], ux * uy) and bits_equal(one["uy2"], uy * uy)
        b.init_equilibrium(u0)
        assert all(is_zero(b.mean_sums(m)) for m in range(3)) and b.mean_enabled
        b.step(EVERY, tau, u0, sample_every=EVERY)
        assert counts(b) == [1, 1, 1]


def test_run_polar_attaches_the_mean_flow(pkg):
    from airfoil_cfd_tool_amd.polar import mean_flow, quarter_chord
    from airfoil_cfd_tool_amd.windtunnel import TAU_DEFAULT, U0_DEFAULT
    alphas = [0, 8]
    kw = dict(nx=160, ny=80, warmup_steps=120, samples=8)
    res = pkg.run_polar(alphas, mean_fields=True, **kw)
    off = pkg.run_polar(alphas, mean_fields=False, **kw)
    nx, ny, tau, u0 = 160, 80, TAU_DEFAULT, U0_DEFAULT
    assert (res.tau, res.u0, res.sample_every) == (tau, u0, EVERY)
    # the same sweep by hand: run_polar's masks and inputs, eight calls that each end in a sample
    masks = np.stack([pkg.geometry.build_geometry(nx, ny, float(a), [], "naca2412").mask for a in alphas])
    samples = [[], []]
    with pkg.PolarEngine(nx, ny, 2, history_cap=8) as b:
        b.set_masks(masks)
        b.init_equilibrium(u0)
        b.enable_loads(*quarter_chord(nx, ny))
        b.step(120, tau, u0)
        for _ in range(8):
            b.step(EVERY, tau, u0, sample_every=EVERY)
            for m in range(2):
                samples[m].append(b.read_macro(m))
    for m, p in enumerate(res.points):
        assert p.mean["n"] == 8
        for k in ("rho", "ux", "uy", "uu", "vv", "uv", "rho_var", "cp_mean", "cp_rms", "speed", "tke"):
            assert p.mean[k].shape == (80, 160) and np.isfinite(p.mean[k]).all(), k
        ux = np.stack([s[1].astype(np.float64) for s in samples[m]])
        err = float(np.abs(p.mean["ux"] - ux.mean(axis=0)).max())
        bound = mean_bound(8, float(np.abs(ux).max()))
        print(f"alpha {p.alpha}: max |mean ux - mean of 8 read_macro| = {err:.3g}, bound {bound:.3g}; max tke {p.mean['tke'].max():.3g}")
        assert err <= bound
        want = mean_flow(accumulate(samples[m]), u0)
        assert all(bits_equal(p.mean[k], want[k]) for k in want if k != "n")
        assert p.mean["tke"].max() > 0 and (p.mean["speed"][masks[m] != 0] == 0).all()
    for p, q in zip(res.points, off.points):
        assert q.mean is None
        for f in dataclasses.fields(p):
            a, c = getattr(p, f.name), getattr(q, f.name)
            if isinstance(a, dict):
                assert list(a) == list(c) and all(a[k].tobytes() == c[k].tobytes() for k in a), f.name
            else:
                assert a == c, f.name
        assert p.cl_total_mean is None and q.cl_total_mean is None
    assert pkg.polar_rows(res) == pkg.polar_rows(off)
