"""The device-side far-field vortex of batched sweeps (wtp_enable_far_vortex and its read-backs, PolarEngine.enable_far_vortex,
vortex_update(norm=), run_polar(vortex_on=)): what needs no GPU.  The two norms of vortex_update on hand values, the C-ABI's
declaration, export and binding, run_polar's argument check, and that the cases the GPU tests run (tests/_vortex_cases.py) stay
unclipped in the NumPy reference of the whole loop, without which device and host loop need not agree.
"""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _vortex_cases as vc

WT_ERR_ARG = -1


# ---- 1. vortex_update's norms ------------------------------------------------------------------
def test_vortex_update_norms_on_hand_values(pkg):
    from airfoil_cfd_tool_amd.polar import VORTEX_NORMS, VORTEX_SPEED_MAX, vortex_update
    assert VORTEX_NORMS == ("hypot", "sqrt") and inspect.signature(vortex_update).parameters["norm"].default == "hypot"
    # unclipped: both norms, and the call without the keyword, give the same bits
    old_s, old_q = [0.0, 0.4, -0.3], [0.0, 0.1, 0.02]
    fx, fy, alpha = [0.02, 0.03, -0.01], [0.1, -0.2, 0.15], [0.0, 6.0, -4.0]
    plain = vortex_update(old_s, old_q, fx, fy, alpha, 0.1, 0.3, 20.0)
    for norm in VORTEX_NORMS:
        got = vortex_update(old_s, old_q, fx, fy, alpha, 0.1, 0.3, 20.0, norm=norm)
        assert not got[2].any()
        for a, b in zip(got, plain):
            assert a.tobytes() == b.tobytes(), norm
    # ... which are the rule written out, one rounding per operation
    c, s = np.cos(np.radians(6.0)), np.sin(np.radians(6.0))
    drag, lift = 0.03 * c + -0.2 * s, -0.03 * s + -0.2 * c
    den = 2 * math.pi * 0.1
    assert plain[0][1] == 0.4 + 0.3 * (lift / den - 0.4) and plain[1][1] == 0.1 + 0.3 * (drag / den - 0.1)
    # clipped, norm="sqrt": a lift of 3 and a drag of 0.5 at full relaxation ask for (4.77, 0.80), which induce 0.242 at distance 20
    got = vortex_update([0.0], [0.0], [0.5], [3.0], [0.0], 0.1, 1.0, 20.0, norm="sqrt")
    ns, nq = 0.0 + 1.0 * (3.0 / den - 0.0), 0.0 + 1.0 * (0.5 / den - 0.0)
    speed = math.sqrt(ns * ns + nq * nq) / 20.0
    scale = VORTEX_SPEED_MAX / speed
    assert got[2][0] and speed > 0.24 and got[0][0] == ns * scale and got[1][0] == nq * scale
    assert abs(math.sqrt(got[0][0] ** 2 + got[1][0] ** 2) / 20.0 - VORTEX_SPEED_MAX) < 1e-15
    hyp = vortex_update([0.0], [0.0], [0.5], [3.0], [0.0], 0.1, 1.0, 20.0)          # the default clips too, to within the scale's last bit
    assert hyp[2][0] and abs(hyp[0][0] - got[0][0]) <= 2 * np.spacing(got[0][0])
    with pytest.raises(ValueError):
        vortex_update([0.0], [0.0], [0.5], [3.0], [0.0], 0.1, 1.0, 20.0, norm="l1")


# ---- 2. the C-ABI without a GPU ----------------------------------------------------------------
NEW = {
    "wtp_read_far_profile": r"wtp_batch \* b , int first , int count , void \* left , void \* bottom , void \* top",
    "wtp_enable_far_vortex": r"wtp_batch \* b , int every , int64_t after , double relax , double u_ref , int with_source , double xc , double yc , "
                             r"const double \* u_far , const double \* v_far , const double \* cos_a , const double \* sin_a , int log_cap",
    "wtp_set_far_vortex": r"wtp_batch \* b , const double \* strength , const double \* source",
    "wtp_far_vortex": r"wtp_batch \* b , double \* strength , double \* source",
    "wtp_far_vortex_update": r"wtp_batch \* b",
    "wtp_far_vortex_log": r"wtp_batch \* b , int first , int count , int64_t \* step , double \* fx , double \* fy , double \* strength , "
                          r"double \* source , int32_t \* clipped",
}


def test_entry_points_are_declared_exported_and_bound(pkg):
    from airfoil_cfd_tool_amd.polar import EXPORTS, POLAR_LIB_PATH
    with open(os.path.join(ROOT, "include", "wt_polar.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    spaced = " ".join(re.sub(r"([(),*])", r" \1 ", header).split())          # every token apart, one blank between
    for name, args in NEW.items():
        assert re.search(r"\bint " + name + r" \( " + args + r" \)", spaced), name
        assert name in EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", POLAR_LIB_PATH], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {s for s in syms if s.startswith("wtp_")} == set(EXPORTS) and len(set(EXPORTS)) == len(EXPORTS)
    assert set(re.findall(r"\b(wtp_\w+)\s*\(", header)) == set(EXPORTS)
    with open(os.path.join(ROOT, "airfoil-cfd-tool_amd", "csrc", "libwtpolar.map")) as fh:
        assert "global: wtp_*;" in fh.read()
    lib = pkg.polar.load_polar_library()
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    want = {"wtp_read_far_profile": [vp, ci, ci, vp, vp, vp],
            "wtp_enable_far_vortex": [vp, ci, ctypes.c_int64, cd, cd, ci, cd, cd, dp, dp, dp, dp, ci],
            "wtp_set_far_vortex": [vp, dp, dp], "wtp_far_vortex": [vp, dp, dp], "wtp_far_vortex_update": [vp],
            "wtp_far_vortex_log": [vp, ci, ci, ip, dp, dp, dp, dp, ctypes.POINTER(ctypes.c_int32)]}
    for name, argtypes in want.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes == argtypes, name
    version = lib.wtp_version()
    for phrase in (b"device-side far-field vortex", b"prescribed far-field profile", b"two-relaxation-time collision", b"state upload and restart"):
        assert phrase in version, phrase
    # a null batch is an argument error in every one of them
    one = np.ones(4)
    p = one.ctypes.data_as(dp)
    tab = np.ones((1, 3, 8), np.float32).ctypes.data_as(vp)
    calls = [lambda: lib.wtp_read_far_profile(None, 0, 1, tab, tab, tab),
             lambda: lib.wtp_enable_far_vortex(None, 8, 16, 0.3, 0.1, 1, 10.0, 10.0, p, p, p, p, 4),
             lambda: lib.wtp_enable_far_vortex(None, 0, 0, 0.0, 0.0, 0, 0.0, 0.0, None, None, None, None, 0),
             lambda: lib.wtp_set_far_vortex(None, p, p), lambda: lib.wtp_far_vortex(None, p, p), lambda: lib.wtp_far_vortex_update(None),
             lambda: lib.wtp_far_vortex_log(None, 0, 0, None, None, None, None, None, None)]
    for k, call in enumerate(calls):
        assert call() == WT_ERR_ARG and b"null batch" in lib.wtp_last_error(), k
    for name in ("enable_far_vortex", "set_far_vortex", "far_vortex", "far_vortex_update", "far_vortex_log", "read_far_profile"):
        assert callable(getattr(pkg.PolarEngine, name)), name
    assert isinstance(pkg.PolarEngine.far_vortex_enabled, property)
    doc = " ".join(" ".join(re.sub(r"^\s*/?\*+/?", "", line) for line in text.splitlines()).split())
    for needle in ("speed = sqrt(ns*ns + nq*nq)/bound", "clipped = speed > 0.1; scale = clipped ? 0.1/speed : 1.0",
                   "Call boundaries do not matter: 5 + 7 steps schedule as 12 do", "wtp_set_step_count leaves `since` alone",
                   "While it is on, wtp_set_far_profile returns WT_ERR_STATE", "unless an update clips"):
        assert needle in doc, needle


# ---- 3. run_polar ------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["gpu", None, "Device"])
def test_run_polar_refuses_an_unknown_vortex_on_before_an_engine_exists(pkg, monkeypatch, bad):
    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(pkg.polar, "PolarEngine", no_engine)
    for far_field in ("vortex", "uniform"):
        with pytest.raises(ValueError, match="vortex_on"):
            pkg.run_polar([2.0], nx=96, ny=48, samples=2, far_field=far_field, vortex_on=bad)


def test_run_polar_signature(pkg):
    sig = inspect.signature(pkg.run_polar)
    assert sig.parameters["vortex_on"].default == "host" and pkg.polar.VORTEX_ON == ("host", "device")
    doc = " ".join(pkg.run_polar.__doc__.split())
    assert "Device and host mode are the same run, bit for bit, unless an update clips" in doc


# ---- 4. the cases stay unclipped in the reference ----------------------------------------------
@pytest.mark.parametrize("name", vc.LATTICES)
def test_the_cases_stay_far_from_the_clip_in_the_reference(pkg, name):
    from airfoil_cfd_tool_amd.polar import VORTEX_SPEED_MAX, vortex_update
    log = vc.reference_loop(name)
    assert [row[0] for row in log] == vc.UPDATE_STEPS == [16, 24, 32, 40, 48, 56]
    speeds = np.array([row[6] for row in log])
    print(name, speeds.max(axis=0))
    assert not any(row[5].any() for row in log) and speeds.max() < 0.5 * VORTEX_SPEED_MAX
    assert all(np.abs(log[-1][3]) + np.abs(log[-1][4]) > 0)                  # every member's vortex or source acts
    s = vc.settings(name)
    assert s["bound"] >= 1 and (s["u_far"] ** 2 + s["v_far"] ** 2 <= 0.25 ** 2).all()
    # the clipped case of the single update: with u_ref = 0.002 and full relaxation the first forces clip every member
    B = len(s["alpha"])
    _, _, clipped = vortex_update(np.zeros(B), np.zeros(B), log[0][1], log[0][2], s["alpha"], vc.U_REF_CLIP, vc.RELAX_CLIP, s["bound"], norm="sqrt")
    assert clipped.all()
