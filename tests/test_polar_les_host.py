"""The Smagorinsky subgrid viscosity of batched sweeps (wtp_enable_les, polar.py): what needs no GPU."""
import ctypes
import dataclasses
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _les_reference as les
import _polar_isa

WT_ERR_ARG = -1


# ---- the C-ABI without a GPU -------------------------------------------------------------------
def test_new_entry_point_is_declared_exported_and_bound(pkg):
    from airfoil_cfd_tool_amd.polar import EXPORTS, POLAR_LIB_PATH
    with open(os.path.join(ROOT, "include", "wt_polar.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", POLAR_LIB_PATH], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = pkg.polar.load_polar_library()
    name = "wtp_enable_les"
    assert re.search(r"\bint\s+%s\s*\(\s*wtp_batch\s*\*\s*b\s*,\s*const\s+double\s*\*\s*cs\s*\)" % name, header)
    assert name in syms and name in EXPORTS
    assert len(lib.wtp_enable_les.argtypes) == 2 and lib.wtp_enable_les.argtypes[1] is ctypes.POINTER(ctypes.c_double)
    # the header carries the definition and says that an LES member has no single-handle twin
    doc = " ".join(" ".join(re.sub(r"^\s*/?\*+/?", "", line) for line in text.splitlines()).split())       # (comment leaders dropped)
    for needle in ("te = 0.5 * (tau + sqrt(tau*tau + (c*q)/rho))", "fo[k] = fin[k] - n[k] / te", "18.0 * sqrt(2.0) * cs * cs",
                   "no libwindtunnel twin"):
        assert needle in doc, needle
    assert b"Smagorinsky" in lib.wtp_version()


def test_null_batch_is_an_argument_error(pkg):
    lib = pkg.polar.load_polar_library()
    cs = (ctypes.c_double * 4)(0.1, 0.1, 0.1, 0.1)
    assert lib.wtp_enable_les(None, cs) == WT_ERR_ARG
    assert b"null batch" in lib.wtp_last_error()
    assert lib.wtp_enable_les(None, None) == WT_ERR_ARG


# ---- run_polar, PolarEngine, PolarResult -------------------------------------------------------
@pytest.mark.parametrize("bad", [-0.01, float("nan"), float("inf"), -float("inf")])
def test_run_polar_validates_les_before_creating_the_engine(pkg, monkeypatch, bad):
    def no_engine(*a, **k):
        raise AssertionError("the engine was created")
    monkeypatch.setattr(pkg.polar, "PolarEngine", no_engine)
    with pytest.raises(ValueError, match="les"):
        pkg.run_polar([4.0], nx=96, ny=48, les=bad)


def test_run_polar_engine_and_result_expose_the_switch(pkg):
    from airfoil_cfd_tool_amd.polar import PolarResult
    sig = inspect.signature(pkg.run_polar)
    assert sig.parameters["les"].default is None and sig.parameters["les"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig.parameters)[-1] == "les"
    assert callable(pkg.PolarEngine.enable_les)
    names = [f.name for f in dataclasses.fields(PolarResult)]
    assert names[-1] == "les" and names[:-1] == ["points", "nx", "ny", "tau", "u0", "warmup_steps", "sample_every"]
    r = PolarResult(points=[], nx=320, ny=160, tau=0.58, u0=0.06, warmup_steps=0, sample_every=12)
    assert r.les is None
    assert PolarResult([], 320, 160, 0.58, 0.06, 0, 12, 0.1).les == 0.1


# ---- the reference -----------------------------------------------------------------------------
def test_les_constant_is_the_headers_product():
    c32, c64 = les.les_constant(0.1, np.float32), les.les_constant(0.17, np.float64)
    assert type(c32) is np.float32 and type(c64) is np.float64
    assert c64 == 18.0 * math.sqrt(2.0) * 0.17 * 0.17 and c32 == np.float32(18.0 * math.sqrt(2.0) * 0.1 * 0.1)
    assert les.les_constant(0.0, np.float32) == 0 and abs(float(c32) - 0.2545584) < 1e-6


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_with_c_zero_is_the_bgk_oracle(pkg, oracle_np, dtype):
    """te = 0.5 (tau + sqrt(RN(tau tau))) = tau exactly, so every byte is oracle.lbm_numpy.step's: 100 steps at 96x48, with a tau
    near 0.5 (whose square rounds) as well as the page's."""
    nx, ny, u0 = 96, 48, 0.06
    mask = pkg.geometry.build_geometry(nx, ny, 6.0, None, "naca2412").mask
    for tau in (0.5008, 0.58):
        f, _ = oracle_np.equilibrium_init(nx, ny, u0, dtype)
        g = f.copy()
        for _ in range(100):
            f, mf = oracle_np.step(f, mask, tau, u0)
            g, mg, te = les.step(g, mask, tau, u0, 0.0)
            assert (te == dtype(tau)).all() and te.dtype == dtype
        assert f.tobytes() == g.tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(mf, mg))
        assert np.ptp(f[1]) > 1e-3                                       # (a flow, not the initial state)


def test_reference_with_the_model_differs_from_bgk_in_interior_fluid_cells_only(pkg, oracle_np):
    nx, ny, u0, tau = 96, 48, 0.06, 0.5008
    mask = pkg.geometry.build_geometry(nx, ny, 6.0, None, "naca2412").mask
    f, _ = oracle_np.equilibrium_init(nx, ny, u0, np.float32)
    for _ in range(40):
        f, _ = oracle_np.step(f, mask, tau, u0)
    a, ma = oracle_np.step(f, mask, tau, u0)
    b, mb, te = les.step(f, mask, tau, u0, les.les_constant(0.17, np.float32))
    interior = np.zeros(mask.shape, bool)
    interior[1:-1, 1:-1] = True
    touched = interior & (mask == 0)
    assert (te[~touched] == np.float32(tau)).all() and (te[touched] >= np.float32(tau)).all()
    assert (te[touched] != np.float32(tau)).mean() > 0.5
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ma, mb))       # the stored moments are pre-collision: the same
    diff = (a != b).any(axis=0)
    assert not diff[~touched].any() and diff[touched].mean() > 0.5


def test_the_model_keeps_re_20000_off_the_stability_net_on_the_reference(pkg, oracle_np):
    """160x80 fp32, NACA 0012 at 10 deg, U0 0.06, Re 20 000 (tau 0.500783), 1500 steps, clamp events every 50th step: plain BGK
    reports events from step 800 on, the model with Cs = 0.1 none.  This is what the GPU test of the same run stands on."""
    from airfoil_cfd_tool_amd.windtunnel import tau_from_reynolds
    nx, ny, u0 = 160, 80, 0.06
    tau = tau_from_reynolds(20000.0, u0, nx)
    assert tau == 0.5 + 3 * 0.06 * (160 / 1.84) / 20000 and abs(tau - 0.500783) < 1e-6
    mask = pkg.geometry.build_geometry(nx, ny, 10.0, None, "naca0012").mask
    c = les.les_constant(0.1, np.float32)
    f, _ = oracle_np.equilibrium_init(nx, ny, u0, np.float32)
    g = f.copy()
    first, worst, te_max = None, (0, 0), 0.0
    for s in range(1, 1501):
        if first is None or s <= 1000:                                   # (BGK is followed to step 1000: past its first events)
            f, mf = oracle_np.step(f, mask, tau, u0)
        g, mg, te = les.step(g, mask, tau, u0, c)
        if s % 50 == 0:
            if s <= 1000:
                ev = oracle_np.clamp_events(*mf, mask)
                worst = (max(worst[0], ev[0]), max(worst[1], ev[1]))
                if ev != (0, 0) and first is None:
                    first = s
            assert oracle_np.clamp_events(*mg, mask) == (0, 0), s
            te_max = max(te_max, float(te.max()))
            assert np.isfinite(g).all()
    print(f"BGK: first clamp events at step {first}, worst (rho, u) to step 1000 {worst}; Cs 0.1: none, max te at the checks {te_max:.6f}")
    assert first == 800 and worst[1] > 0
    assert 0.5008 < te_max < 0.52


# ---- the kernel's code object ------------------------------------------------------------------
@pytest.fixture(scope="module")
def polar_isa():
    return _polar_isa.polar_isa()


def test_les_step_has_four_instantiations_and_no_scratch(polar_isa):
    """fp32 and fp64, emitting and not; no spill: the per-site relaxation time costs registers, not scratch."""
    chk, files = polar_isa
    family = lambda v: v[0] == "native" and v[3:] == (_polar_isa.LES, _polar_isa.HALFWAY, _polar_isa.AXIAL)      # noqa: E731
    seen = {name: r for name, (_, r) in _polar_isa.step_kernels(chk, files, family).items()}
    for name, r in seen.items():
        assert r.get("private_seg_size", 0) == 0, (name, r)
    print({k: v.get("num_vgpr") for k, v in seen.items()})
    assert len(seen) == 4, sorted(seen)
