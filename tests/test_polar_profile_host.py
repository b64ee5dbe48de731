"""The prescribed far-field profile of batched sweeps (wtp_enable_far_profile, wtp_set_far_profile, PolarEngine.enable_far_profile /
set_far_profile, far_profile, vortex_update, run_polar(far_field=)): what needs no GPU.  The C-ABI's declaration, export and binding,
the NumPy reference itself (tests/_profile_reference.py) and the cases the GPU tests compare against (tests/_profile_cases.py), the two
pure functions of the far-field correction on hand values, and run_polar's argument checks.

The misreads.  Four wrong readings of the tables (top for bottom, an entry shifted by one, ux and uy swapped, rho forced to 1) change
bits at far-field cells on every lattice with the vortex tables, in every member whose strength is not zero, and with the random tables
in every member.  The fifth, the corner of column 0 taken from `bottom` / `top` instead of `left`, cannot be told with tables from
far_profile, whichever strengths they have: left[.][0] and bottom[.][0] are the same function of the same cell centre (0.5, 0.5), the
same bits.  It is told on every lattice with the random tables, which is why the GPU tests run those on every lattice too.
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, bits_equal
import lbm_numpy
import _profile_cases as pc
import _profile_reference as prof
import _wind_reference as wind

WT_ERR_ARG = -1


# ---- 1. the C-ABI without a GPU ----------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(pkg):
    from airfoil_cfd_tool_amd.polar import EXPORTS, POLAR_LIB_PATH
    with open(os.path.join(ROOT, "include", "wt_polar.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+wtp_enable_far_profile\s*\(\s*wtp_batch\s*\*\s*b\s*,\s*int\s+on\s*\)", header)
    assert re.search(r"\bint\s+wtp_set_far_profile\s*\(\s*wtp_batch\s*\*\s*b\s*,\s*int\s+first\s*,\s*int\s+count\s*,\s*const\s+void\s*\*\s*left\s*,"
                     r"\s*const\s+void\s*\*\s*bottom\s*,\s*const\s+void\s*\*\s*top\s*\)", header)
    out = subprocess.run(["nm", "-D", "--defined-only", POLAR_LIB_PATH], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {s for s in syms if s.startswith("wtp_")} == set(EXPORTS) and len(set(EXPORTS)) == len(EXPORTS)
    assert set(re.findall(r"\b(wtp_\w+)\s*\(", header)) == set(EXPORTS)          # every prototype of the header, and nothing else
    lib = pkg.polar.load_polar_library()
    assert lib.wtp_enable_far_profile.restype is ctypes.c_int and lib.wtp_enable_far_profile.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert lib.wtp_set_far_profile.restype is ctypes.c_int
    assert lib.wtp_set_far_profile.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    version = lib.wtp_version()
    for phrase in (b"prescribed far-field profile", b"two-relaxation-time collision", b"inclined free stream", b"interpolated bounce-back"):
        assert phrase in version, phrase
    assert lib.wtp_enable_far_profile(None, 1) == WT_ERR_ARG and b"null batch" in lib.wtp_last_error()
    t = np.ones((1, 3, 8), np.float32)
    p = t.ctypes.data_as(ctypes.c_void_p)
    assert lib.wtp_set_far_profile(None, 0, 1, p, p, p) == WT_ERR_ARG and b"null batch" in lib.wtp_last_error()
    assert callable(pkg.PolarEngine.enable_far_profile) and callable(pkg.PolarEngine.set_far_profile)
    assert isinstance(pkg.PolarEngine.far_profile_enabled, property)
    doc = " ".join(" ".join(re.sub(r"^\s*/?\*+/?", "", line) for line in text.splitlines()).split())
    for needle in ("takes left[.][j] if i == 0, else bottom[.][i] if j == 0, else top[.][i]", "corners of column 0 therefore belong to `left`",
                   "entries 0 and NX-1 of `bottom` and `top` are never read", "gives the bits of a batch with wtp_enable_wind",
                   "On a half batch both calls return WT_ERR_STATE", "as long as any member has never been given a profile"):
        assert needle in doc, needle


# ---- 2. the reference --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["96x48-f32", "24x140-f64"])
def test_a_uniform_profile_is_the_wind_reference(name):
    nx, ny, dtype, B = pc.lattice(name)
    tau, u0, v0, _ = pc.params(name)
    masks, _, ref = pc.reference(name, "uniform")
    assert 0.0 in v0 and any(v != 0 for v in v0)
    for m in range(B):
        want = wind.run(masks[m], pc.STEPS, tau[m], u0[m], v0[m], dtype=dtype)
        assert bits_equal(ref[m][0], want[0]) and all(bits_equal(a, b) for a, b in zip(ref[m][1], want[1])), (name, m)
        if v0[m] == 0:                                                     # ... and with v0 = 0 the plain oracle
            assert bits_equal(ref[m][0], lbm_numpy.run(masks[m], pc.STEPS, tau[m], u0[m], dtype)[0])
    # a zero-strength vortex profile is the uniform one, entry for entry
    zero = pc.vortex_tables(name, 0.0)
    for m in range(B):
        for a, b in zip(zero[m], pc.tables_of(name, "uniform")[m]):
            assert bits_equal(a, b), (name, m)


@pytest.mark.parametrize("kind", ["vortex", "random"])
@pytest.mark.parametrize("name", list(pc.CASES))
def test_the_reference_tells_a_misread_table(name, kind):
    nx, ny, dtype, B = pc.lattice(name)
    masks, _, ref = pc.reference(name, kind, steps=1)
    told = {}
    for what in prof.MISREADS:
        wrong = pc.reference(name, kind, steps=1, read=what)[2]
        told[what] = []
        for m in range(B):
            far = wind.far_field(masks[m])
            diff = (ref[m][0] != wrong[m][0]).any(axis=0) | np.any([a != b for a, b in zip(ref[m][1], wrong[m][1])], axis=0)
            assert not diff[~far].any(), (name, kind, what, m)              # one step: nothing but far-field cells can differ
            told[what].append(int(diff[far].sum()))
    print(name, kind, told)
    live = range(B) if kind == "random" else [m for m in range(B) if pc.VORTEX[name][m] != (0.0, 0.0)]
    assert len(live) >= 2
    for what, counts in told.items():
        if kind == "vortex" and what == "corner from bottom and top":
            assert counts == [0] * B, counts                               # the same function of the same cell centre (module docstring)
            continue
        for m in live:
            assert counts[m] > 0, (name, kind, what, m, counts)
    if kind == "random":
        assert all(c == 2 for c in told["corner from bottom and top"])     # exactly the two corners


@pytest.mark.parametrize("name,variant", [(n, "") for n in pc.CASES] + [(n, v) for n in pc.COMBINED for v in pc.VARIANTS])
def test_the_cases_keep_the_reference_off_the_stability_net(name, variant):
    for kind in ("vortex", "random"):
        masks, _, ref = pc.reference(name, kind, variant)
        for m, (f, (rho, ux, uy)) in enumerate(ref):
            assert np.isfinite(f).all()
            assert lbm_numpy.clamp_events(rho, ux, uy, masks[m]) == (0, 0), (name, kind, variant, m)
    both = [np.sign(s) for s, _ in pc.VORTEX[name]]
    assert both[0] == 0 and sorted(both[1:]) == [-1, 1]                    # one member with both zero, both signs of strength


def test_every_table_of_the_cases_is_inside_the_limits():
    for name in pc.CASES:
        for kind in ("vortex", "random", "uniform"):
            for left, bottom, top in pc.tables_of(name, kind):
                for t in (left, bottom, top):
                    t = t.astype(np.float64)
                    assert np.isfinite(t).all() and (t[0] >= 0.5).all() and (t[0] <= 2).all() and (t[1] ** 2 + t[2] ** 2 <= 0.35 ** 2).all()
        for tabs in pc.random_tables(name):
            v = np.concatenate([t.ravel() for t in tabs])
            assert np.unique(v).size == v.size                             # no two entries alike


# ---- 3. far_profile and vortex_update ----------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_far_profile_on_hand_values(pkg, dtype):
    nx, ny, u0, v0, s, q, xc, yc = 12, 8, 0.1, 0.02, 0.3, 0.05, 4.25, 3.5
    left, bottom, top = pkg.far_profile(nx, ny, u0, v0, s, q, xc, yc, dtype)
    assert left.shape == (3, ny) and bottom.shape == top.shape == (3, nx) and left.dtype == bottom.dtype == top.dtype == np.dtype(dtype)

    def hand(i, j):
        dx, dy = i + 0.5 - xc, j + 0.5 - yc
        r2 = dx * dx + dy * dy
        ux = u0 + s * dy / r2 + q * dx / r2
        uy = v0 - s * dx / r2 + q * dy / r2
        return [1 + 1.5 * ((u0 * u0 + v0 * v0) - (ux * ux + uy * uy)), ux, uy]

    T = np.dtype(dtype).type
    for tab, cells in ((left, [(0, 0), (0, 3), (0, ny - 1)]), (bottom, [(0, 0), (5, 0), (nx - 1, 0)]), (top, [(0, ny - 1), (7, ny - 1)])):
        for i, j in cells:
            got = tab[:, j] if tab is left else tab[:, i]
            assert [T(v) for v in hand(i, j)] == list(got), (i, j)
    # above the vortex the flow is faster and the density lower, below it the other way round; behind the source the flow is faster
    above, below = top[:, 4], bottom[:, 4]
    assert above[1] > u0 > below[1] and above[0] < 1 < below[0]
    # the values by hand, once: cell (0, 0), dx = -3.75, dy = -3, r2 = 23.0625
    ux = 0.1 + 0.3 * -3.0 / 23.0625 + 0.05 * -3.75 / 23.0625
    uy = 0.02 - 0.3 * -3.75 / 23.0625 + 0.05 * -3.0 / 23.0625
    assert left[1, 0] == T(ux) and left[2, 0] == T(uy) and abs(ux - 0.05284553) < 1e-8 and abs(uy - 0.06227642) < 1e-8
    # no vortex and no source: the uniform tables exactly
    for tab in pkg.far_profile(nx, ny, u0, v0, 0.0, 0.0, xc, yc, dtype):
        assert (tab[0] == T(1.0)).all() and (tab[1] == T(u0)).all() and (tab[2] == T(v0)).all()


def test_vortex_update_on_hand_values(pkg):
    from airfoil_cfd_tool_amd.polar import VORTEX_SPEED_MAX, vortex_bound, vortex_update, wind_axes
    two_pi = 2 * math.pi
    # body frame (alpha = 0): lift is fy, drag is fx
    s, q, clipped = vortex_update([0.0], [0.0], [0.02], [0.1], [0.0], 0.1, 0.3, 20.0)
    assert s[0] == 0.0 + 0.3 * (0.1 / (two_pi * 0.1) - 0.0) and q[0] == 0.3 * (0.02 / (two_pi * 0.1)) and not clipped[0]
    assert abs(s[0] - 0.0477464829) < 1e-9 and abs(q[0] - 0.0095492966) < 1e-9
    # from a previous value, full relaxation: the target itself
    s, q, _ = vortex_update([0.4], [0.1], [0.02], [0.1], [0.0], 0.1, 1.0, 20.0)
    assert s[0] == 0.4 + 1.0 * (0.1 / (two_pi * 0.1) - 0.4) and abs(s[0] - 0.1 / (two_pi * 0.1)) < 1e-15
    # wind frame: the forces are turned first
    d, l = wind_axes([0.02], [0.1], [6.0])
    s, q, _ = vortex_update([0.0], [0.0], [0.02], [0.1], [6.0], 0.1, 0.3, 20.0)
    assert s[0] == 0.3 * (l[0] / (two_pi * 0.1)) and q[0] == 0.3 * (d[0] / (two_pi * 0.1)) and l[0] < 0.1 and d[0] > 0.02
    # without the source the drag is not used
    s2, q2, _ = vortex_update([0.0], [0.0], [0.02], [0.1], [6.0], 0.1, 0.3, 20.0, with_source=False)
    assert s2[0] == s[0] and q2[0] == 0.0
    # the clip: a lift of 3 asks for 4.77 at full relaxation; with the source at distance 20 that induces 0.242, so both are scaled to induce 0.1
    s, q, clipped = vortex_update([0.0, 0.0], [0.0, 0.0], [0.5, 0.02], [3.0, 0.1], [0.0, 0.0], 0.1, 1.0, 20.0)
    assert list(clipped) == [True, False]
    assert abs(math.hypot(s[0], q[0]) / 20.0 - VORTEX_SPEED_MAX) < 1e-15 and abs(q[0] / s[0] - 0.5 / 3.0) < 1e-15
    assert abs(s[0] - 2.0 * 3.0 / math.hypot(3.0, 0.5)) < 1e-12
    # negative lift clips to the negative bound
    s, _, clipped = vortex_update([0.0], [0.0], [0.0], [-3.0], [0.0], 0.1, 1.0, 20.0, with_source=False)
    assert clipped[0] and abs(s[0] + 2.0) < 1e-12
    # the bound is the distance to the nearest far-field cell centre, and keeps a profile inside set_far_profile's limits at u0 = 0.25
    nx, ny = 320, 160
    xc, yc = pkg.polar.quarter_chord(nx, ny)
    bound = vortex_bound(nx, ny, xc, yc)
    assert bound == min(xc - 0.5, yc - 0.5, ny - 0.5 - yc) == 79.5
    for sign in (1.0, -1.0):
        for tab in pkg.far_profile(nx, ny, 0.25, 0.0, sign * 0.1 * bound, 0.0, xc, yc, "float32"):
            t = tab.astype(np.float64)
            assert (t[1] ** 2 + t[2] ** 2 <= 0.35 ** 2).all() and (t[0] >= 0.5).all() and (t[0] <= 2.0).all()


# ---- 4. run_polar ------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(far_field="doublet"), dict(far_field=None), dict(far_field="vortex", vortex_every=0),
                                 dict(far_field="vortex", vortex_every=-5), dict(far_field="vortex+source", vortex_relax=0.0),
                                 dict(far_field="vortex", vortex_relax=1.5), dict(far_field="vortex", vortex_relax=float("nan")),
                                 dict(far_field="vortex", storage="half"), dict(far_field="vortex+source", storage="half")],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_run_polar_refuses_bad_arguments_before_an_engine_exists(pkg, monkeypatch, bad):
    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(pkg.polar, "PolarEngine", no_engine)
    with pytest.raises(ValueError):
        pkg.run_polar([2.0], nx=96, ny=48, samples=2, **bad)


def test_run_polar_signature_and_results(pkg):
    import dataclasses
    import inspect
    sig = inspect.signature(pkg.run_polar)
    assert sig.parameters["far_field"].default == "uniform" and sig.parameters["vortex_every"].default == 96
    assert sig.parameters["vortex_relax"].default == 0.3 and sig.parameters["vortex_after"].default is None
    assert pkg.polar.FAR_FIELDS == ("uniform", "vortex", "vortex+source")
    r = pkg.polar.PolarResult(points=[], nx=8, ny=8, tau=0.6, u0=0.1, warmup_steps=0, sample_every=1)
    assert r.far_field == "uniform" and r.vortex_history is None
    names = [f.name for f in dataclasses.fields(pkg.polar.PolarPoint)]
    assert "vortex_strength" not in names                                  # attributes that run_polar sets, no fields
    p = pkg.polar.polar_point(2.0, [1], [0.1], [0.2], [4], [0], 0.1, 96)
    assert p.vortex_strength is None and p.vortex_source is None
    doc = " ".join(pkg.run_polar.__doc__.split())
    assert "removes a part of the tunnel effect, not all of it, and a taller lattice (`ny`) removes more" in doc
