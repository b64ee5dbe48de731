"""The two-relaxation-time collision of batched sweeps (wtp_enable_trt, PolarEngine.enable_trt, run_polar(collision="trt")): what needs
no GPU.  The C-ABI's declaration, export and binding, run_polar's argument checks, and the NumPy reference itself (tests/_trt_reference.py):
its relation to BGK and to the Smagorinsky model, the sensitivity of the cases the GPU tests compare against (tests/_trt_cases.py), and
the wall position in a channel, which is what the collision is for.
"""
import ctypes
import dataclasses
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import lbm_numpy
import _les_reference as les
import _restart_cases as rc
import _trt_cases as tc
import _trt_reference as trt
from _rough_start import assert_sensitive, body_mask, rough_state

WT_ERR_ARG = -1


# ---- 1. the C-ABI without a GPU ----------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound(pkg):
    from airfoil_cfd_tool_amd.polar import EXPORTS, POLAR_LIB_PATH
    with open(os.path.join(ROOT, "include", "wt_polar.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+wtp_enable_trt\s*\(\s*wtp_batch\s*\*\s*b\s*,\s*const\s+double\s*\*\s*magic\s*\)", header)
    out = subprocess.run(["nm", "-D", "--defined-only", POLAR_LIB_PATH], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "wtp_enable_trt" in syms and "wtp_enable_trt" in EXPORTS
    lib = pkg.polar.load_polar_library()
    assert lib.wtp_enable_trt.restype is ctypes.c_int and len(lib.wtp_enable_trt.argtypes) == 2
    assert lib.wtp_enable_trt.argtypes[1] is ctypes.POINTER(ctypes.c_double)
    version = lib.wtp_version()
    assert b"two-relaxation-time collision" in version
    for phrase in (b"Smagorinsky subgrid viscosity", b"interpolated bounce-back", b"inclined free stream", b"half-precision population storage",
                   b"state upload and restart", b"momentum exchange", b"mean fields", b"surface loads"):
        assert phrase in version, phrase                                       # every earlier phrase is kept
    magic = np.array([0.1875])
    assert lib.wtp_enable_trt(None, magic.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == WT_ERR_ARG
    assert b"null batch" in lib.wtp_last_error()
    assert lib.wtp_enable_trt(None, None) == WT_ERR_ARG
    assert callable(pkg.PolarEngine.enable_trt) and isinstance(pkg.PolarEngine.trt_enabled, property)
    doc = " ".join(" ".join(re.sub(r"^\s*/?\*+/?", "", line) for line in text.splitlines()).split())
    for needle in ("tm = 0.5 + lam / (tp - 0.5)", "fo[k] = (fin[k] - ds) - da", "fo[o] = (fin[o] - ds) + da", "Mass and momentum are conserved",
                   "not bit for bit", "A TRT member has no libwindtunnel twin", "is not greater than 0.5"):
        assert needle in doc, needle


# ---- 2. run_polar ------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(collision="mrt"), dict(collision=None), dict(collision="trt", magic=0.0), dict(collision="trt", magic=-0.25),
                                 dict(collision="trt", magic=1.5), dict(collision="trt", magic=float("nan")), dict(collision="trt", tau=0.5),
                                 dict(collision="trt", tau=0.4), dict(collision="trt", tau=0.5 + 1e-9)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_run_polar_rejects_bad_arguments_before_creating_the_engine(pkg, monkeypatch, bad):
    def no_engine(*a, **k):
        raise AssertionError("the engine was created")
    monkeypatch.setattr(pkg.polar, "PolarEngine", no_engine)
    with pytest.raises(ValueError, match="collision|magic|tau"):              # (0.5 + 1e-9 is 0.5 in float32)
        pkg.run_polar([2.0, 4.0], nx=96, ny=48, samples=4, **bad)
    with pytest.raises(AssertionError, match="the engine was created"):        # (good arguments get as far as the engine)
        pkg.run_polar([2.0, 4.0], nx=96, ny=48, samples=4, collision="trt", magic=1.0, tau=0.501)
    with pytest.raises(AssertionError, match="the engine was created"):        # (bgk accepts what it always accepted)
        pkg.run_polar([2.0, 4.0], nx=96, ny=48, samples=4, tau=0.5)


def test_run_polar_and_result_expose_the_collision(pkg):
    from airfoil_cfd_tool_amd.polar import PolarResult
    sig = inspect.signature(pkg.run_polar)
    assert sig.parameters["collision"].default == "bgk" and sig.parameters["magic"].default == 3 / 16
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("collision", "magic"))
    assert [f.name for f in dataclasses.fields(PolarResult)] == ["points", "nx", "ny", "tau", "u0", "warmup_steps", "sample_every", "les"]
    base = dict(points=[], nx=96, ny=48, tau=0.58, u0=0.06, warmup_steps=0, sample_every=12)
    r = PolarResult(**base)
    assert r.collision == "bgk" and r.magic is None
    t = PolarResult(**base, collision="trt", magic=0.25)
    assert (t.collision, t.magic) == ("trt", 0.25) and t == r                  # init-only: == and repr stay as they were


# ---- 3. tm == tp: BGK as a number, not as bits --------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_at_tm_equal_tp_the_reference_is_bgk_within_one_eps(dtype):
    nx, ny, tau, lam, u0 = 96, 48, 0.75, 0.0625, 0.06
    T = np.dtype(dtype).type
    assert T(0.5) + T(lam) / (T(tau) - T(0.5)) == T(tau)                        # tm == tp exactly
    mask = body_mask(nx, ny, 71)
    f = rough_state(nx, ny, u0, np.dtype(dtype), 72)
    got, macro = trt.step(f, mask, tau, u0, lam)
    want, want_macro = lbm_numpy.step(f, mask, tau, u0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(macro, want_macro))
    diff = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    eps = float(np.finfo(dtype).eps)
    print(f"{dtype}: largest |trt - bgk| after one step {diff / eps:.4g} eps")
    assert diff <= eps
    assert (got.view(np.uint8) != want.view(np.uint8)).any()                    # the split rounds differently
    cells = tc.interior_fluid(mask)
    assert all(got[k][~cells].tobytes() == want[k][~cells].tobytes() for k in range(9))      # nothing but interior fluid cells collides


# ---- 4. Smagorinsky at c = 0 is the plain form --------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_reference_with_c_zero_is_the_reference_without_the_model(dtype):
    nx, ny, u0 = 96, 48, 0.06
    mask = body_mask(nx, ny, 73)
    f0 = rough_state(nx, ny, u0, np.dtype(dtype), 74)
    for tau, lam in ((0.56, 3 / 16), (0.9, 0.25), (0.5008, 1 / 12)):
        a, b = f0, f0
        for _ in range(5):
            a, ma = trt.step(a, mask, tau, u0, lam, les.les_constant(0.0, dtype))
            b, mb = trt.step(b, mask, tau, u0, lam)
        assert a.tobytes() == b.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(ma, mb))
        c, _ = trt.step(f0, mask, tau, u0, lam, les.les_constant(0.17, dtype))
        d, _ = trt.step(f0, mask, tau, u0, lam)
        assert c.tobytes() != d.tobytes()                                       # (while a positive constant acts)


# ---- 5. the cases of the GPU tests --------------------------------------------------------------
@pytest.mark.parametrize("lattice,variant,stored", [pytest.param(lat, v, False, id=f"{lat}-{v}-native") for lat, v in tc.NATIVE_CASES]
                         + [pytest.param(lat, v, True, id=f"{lat}-{v}-half") for lat, v in tc.HALF_CASES])
def test_rough_start_case_is_sensitive_and_tells_the_collision_apart(lattice, variant, stored):
    nx, ny, dtype = rc.LATTICES[lattice]
    masks, q, start, ref = tc.reference(lattice, variant, stored)
    alts = tc.alternatives(lattice, variant, stored)
    assert len(set(tc.MAGIC)) == rc.B and all(tc.MAGIC[m] != tc.OTHER_MAGIC[m] for m in range(rc.B))
    least = 1.0
    for m, (s, macro, prev) in enumerate(ref):
        assert s.dtype == (np.float16 if stored else np.dtype(dtype)) and s.shape == (9, ny, nx)
        a, b = (s.astype(np.float32), prev.astype(np.float32)) if stored else (s, prev)      # (exact and one-to-one)
        assert_sensitive(a, b, masks[m])
        assert all(np.isfinite(p).all() for p in macro)
        assert lbm_numpy.clamp_events(*macro, masks[m]) == (0, 0), (lattice, variant, m)
        cells = tc.interior_fluid(masks[m])
        shares = {name: float((s != other).any(axis=0)[cells].mean()) for name, other in alts[m].items()}
        least = min(least, *shares.values())
        assert all(v > 0.9 for v in shares.values()), (lattice, variant, m, shares)
    print(f"{lattice} {variant} {'half' if stored else 'native'}: the smallest share of interior fluid cells that differ from an alternative is {least:.3f}")


@pytest.mark.parametrize("name", list(tc.EQ_CASES))
def test_equilibrium_case_is_finite_off_the_net_and_not_bgk(name):
    """From equilibrium no reference can meet assert_sensitive: outside the sound front of the body (60 / sqrt(3) rows either side) every
    site still holds its neighbours' bits, and there the collision has nothing to act on.  So these cases are held to what they can show
    (finite, off the net, the collision acting wherever a disturbance has arrived: a quarter of the cells, as test_gpu_polar_les.py asks of
    the same lattices), and the misplaced-read sensitivity is the rough-start family's."""
    nx, ny, dtype, members = tc.EQ_CASES[name]
    masks, ref = tc.eq_reference(name)
    taus, magics = [m[2] for m in members], [m[4] for m in members]
    assert min(abs(t - 0.5) for t in taus) < 1e-3 and sorted(magics) == sorted(tc.MAGIC)
    assert len({(m[2], m[3], m[4]) for m in members}) == 3
    for m, (f, macro, bgk) in enumerate(ref):
        assert np.isfinite(f).all() and all(np.isfinite(p).all() for p in macro)
        assert lbm_numpy.clamp_events(*macro, masks[m]) == (0, 0), (name, m)
        differs = float((f != bgk).any(axis=0)[tc.interior_fluid(masks[m])].mean())
        print(f"{name} member {m}: populations differ from BGK's at {differs:.3f} of the interior fluid cells")
        assert differs > 0.25, (name, m, differs)


# ---- the kernels' code objects -------------------------------------------------------------------
def test_trt_step_kernels_are_built_and_have_no_scratch():
    """k_step_batch with the two-relaxation-time collisions and the inclined far field: fp32 and fp64, emitting and not, without and with the
    Smagorinsky model, half-way, interpolated and moving walls (24); k_step_half_batch with them: emitting and not, without and with the model (4).
    No spill; fp32 within 5 waves' 96 VGPRs, fp64 within 4 waves' 128."""
    import _polar_isa
    chk, files = _polar_isa.polar_isa()
    family = lambda v: v[3] in (_polar_isa.TRT, _polar_isa.TRT_LES) and v[5] == _polar_isa.INCLINED      # noqa: E731
    seen = _polar_isa.step_kernels(chk, files, family)
    for name, (_, r) in seen.items():
        assert r.get("private_seg_size", 0) == 0, (name, r)
    print({k: r.get("num_vgpr") for k, (_, r) in seen.items()})
    tiled = {k: (v, r) for k, (v, r) in seen.items() if v[0] == "native"}
    assert len(tiled) == 24 and sum(v[0] == "half" for v, _ in seen.values()) == 4, sorted(seen)
    for name, (v, r) in tiled.items():
        assert r["num_vgpr"] <= (96 if v[1] == "f" else 128), (name, r)


# ---- 6. the wall position ----------------------------------------------------------------------
def test_channel_walls_sit_half_way_under_trt_and_not_under_bgk():
    """64x14 fp64, rows 0 and NY-1 solid, tau = 2.0, U0 = 0.04, 7264 steps from equilibrium; the parabola fitted to ux over rows 1 .. NY-2
    of column 48.  Theory: BGK at tau = 2 has Lambda = 2.25 and walls 0.225 cells outside the half-way ones (measured 0.32: the rest is
    the developing flow); TRT at Lambda = 3/16 has them half-way (measured 0.035)."""
    C = trt.CHANNEL
    mask = trt.channel_mask()
    _, bgk = lbm_numpy.run(mask, C["steps"], C["tau"], C["u0"], np.float64)
    _, two = trt.run(mask, C["steps"], C["tau"], C["u0"], 3.0 / 16.0, dtype=np.float64)
    off_bgk = trt.wall_offsets(bgk[1][:, C["column"]])
    off_trt = trt.wall_offsets(two[1][:, C["column"]])
    print(f"wall offsets (cells outside y = 1, y = NY - 1): BGK {off_bgk[0]:.4f} {off_bgk[1]:.4f}, TRT 3/16 {off_trt[0]:.4f} {off_trt[1]:.4f}")
    assert all(v > 0.15 for v in off_bgk)
    assert all(abs(v) < 0.1 for v in off_trt)
