"""Half-precision population storage of batched sweeps (wtp_create_stored, polar.py): what needs no GPU."""
import ctypes
import dataclasses
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _half_reference as half
import _les_reference as les
import _polar_isa

WT_ERR_ARG = -1
WT_F32, WT_F64 = 0, 1


# ---- 1. the weights ----------------------------------------------------------------------------
def test_weights_are_feqs(oracle_np):
    w = half.W.reshape(9)
    assert w.dtype == np.float32
    assert w.tobytes() == np.array(oracle_np.weights(np.float32), np.float32).tobytes()
    # ... and np.float32 of the double weights: one fp32 division rounds where the double quotient rounds
    assert w.tobytes() == np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, np.float64).astype(np.float32).tobytes()
    one = np.ones((2, 3), np.float32)
    zero = np.zeros((2, 3), np.float32)
    for k in range(9):                                                   # feq at rest is the weight itself
        assert (oracle_np.feq(k, one, zero, zero, np.float32) == w[k]).all()


# ---- 2. Store(Load(h)) == h --------------------------------------------------------------------
def test_store_of_load_is_the_identity_on_every_finite_half_but_minus_zero():
    """Exhaustive: all 65 536 patterns against each of the three weights.  Every finite pattern comes back but one: 0x8000, minus
    zero, whose Load is w_k itself and whose Store is then +0.  (A Store yields -0 where f - w_k is negative and below 2^-25 in
    magnitude; a solid or outlet cell that copies such a value writes +0.  The kernel and the reference do the same.)"""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    h = bits.view(np.float16)
    finite = np.isfinite(h)
    assert int(finite.sum()) == 65536 - 2 * 1024
    for k in (0, 1, 5):
        planes = np.zeros((9, 65536), np.float16)
        planes[k] = h
        with np.errstate(invalid="ignore"):
            back = half.store(half.load(planes))[k].view(np.uint16)
        bad = bits[finite & (back != bits)]
        assert [hex(b) for b in bad] == ["0x8000"], (k, [hex(b) for b in bad[:20]], bad.size)
        assert back[0x8000] == 0
    sub = bits[(bits & 0x7C00) == 0]                                      # subnormal halves (and the zeros) load exactly
    for k in (0, 1, 5):
        w = np.float64(half.W[k, 0, 0])
        planes = np.zeros((9, sub.size), np.float16)
        planes[k] = sub.view(np.float16)
        assert (half.load(planes)[k].astype(np.float64) == sub.view(np.float16).astype(np.float64) + w).all()


# ---- 3. the wrapper composes -------------------------------------------------------------------
def test_wrapped_reference_with_v0_zero_and_c_zero_is_the_wrapped_plain_one(pkg, oracle_np):
    nx, ny, tau, u0 = 96, 48, 0.52, 0.08
    mask = pkg.geometry.build_geometry(nx, ny, 6.0, None, "naca2412").mask
    plain = half.run(mask, 40, tau, u0)
    c0 = les.les_constant(0.0, np.float32)
    for base, extra in ((les.step, (c0,)), (half.windy(oracle_np.step), (0.0,)), (half.windy(les.step), (0.0, c0))):
        out = half.run(mask, 40, tau, u0, *extra, base_step=base)
        assert out[0].dtype == np.float16 and out[0].tobytes() == plain[0].tobytes()
        assert all(a.dtype == np.float32 and a.tobytes() == b.tobytes() for a, b in zip(out[1], plain[1]))
    assert np.ptp(half.load(plain[0])[1]) > 1e-3                          # (a flow, not the start state)
    # and the models act under the wrapper
    assert half.run(mask, 40, tau, u0, les.les_constant(0.17, np.float32), base_step=les.step)[0].tobytes() != plain[0].tobytes()
    assert half.run(mask, 40, tau, u0, 0.02, base_step=half.windy(oracle_np.step), v0=0.02)[0].tobytes() != plain[0].tobytes()
    # the start state: Store of the fp32 start values, macroscopic planes untouched
    h0, macro = half.half_init(nx, ny, u0)
    f0, m0 = oracle_np.equilibrium_init(nx, ny, u0, np.float32)
    assert h0.tobytes() == half.store(f0).tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(macro, m0))


# ---- 4. run_polar, PolarEngine, PolarResult ----------------------------------------------------
def _no_engine(pkg, monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("the engine was created")
    monkeypatch.setattr(pkg.polar, "PolarEngine", no_engine)

    def no_library(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(pkg.polar, "load_polar_library", no_library)


@pytest.mark.parametrize("bad", ["fp16", "", None, 1, "Half"])
def test_run_polar_validates_storage_before_loading_the_library(pkg, monkeypatch, bad):
    engine = pkg.PolarEngine
    _no_engine(pkg, monkeypatch)
    with pytest.raises(ValueError, match="storage"):
        pkg.run_polar([4.0], nx=96, ny=48, storage=bad)
    with pytest.raises(ValueError, match="storage"):
        engine(96, 48, 2, storage=bad)


def test_run_polar_rejects_half_with_float64_or_interpolated_walls(pkg, monkeypatch):
    engine = pkg.PolarEngine
    _no_engine(pkg, monkeypatch)
    with pytest.raises(ValueError, match="float32"):
        pkg.run_polar([4.0], nx=96, ny=48, storage="half", dtype="float64")
    with pytest.raises(ValueError, match="interpolated"):
        pkg.run_polar([4.0], nx=96, ny=48, storage="half", walls="interpolated")
    with pytest.raises(ValueError, match="float32"):
        engine(96, 48, 2, dtype="float64", storage="half")
    with pytest.raises(ValueError, match="storage"):
        engine(96, 48, 2, storage="bf16")
    for ok in (dict(storage="native", dtype="float64"), dict(storage="native", walls="interpolated"), dict(storage="half"), dict()):
        with pytest.raises(AssertionError, match="engine was created"):   # (these pass the checks)
            pkg.run_polar([4.0], nx=96, ny=48, **ok)


def test_run_polar_engine_and_result_expose_the_switch(pkg):
    from airfoil_cfd_tool_amd.polar import EXPORTS, STORAGES, PolarResult
    assert STORAGES == ("native", "half")
    assert "wtp_create_stored" in EXPORTS and "wtp_read_stored" in EXPORTS
    sig = inspect.signature(pkg.run_polar)
    assert sig.parameters["storage"].default == "native" and sig.parameters["storage"].kind is inspect.Parameter.KEYWORD_ONLY
    esig = inspect.signature(pkg.PolarEngine)
    assert esig.parameters["storage"].default == "native" and list(esig.parameters)[-1] == "storage"
    assert callable(pkg.PolarEngine.read_stored)
    assert "storage" not in [f.name for f in dataclasses.fields(PolarResult)]    # (the fields callers enumerate are unchanged)
    r = PolarResult(points=[], nx=320, ny=160, tau=0.58, u0=0.06, warmup_steps=0, sample_every=12)
    assert r.storage == "native" and r.walls == "staircase" and r.frame == "body"
    r = PolarResult(points=[], nx=320, ny=160, tau=0.58, u0=0.06, warmup_steps=0, sample_every=12, storage="half")
    assert r.storage == "half"
    assert PolarResult([], 320, 160, 0.58, 0.06, 0, 12, None, "staircase", "wind", "half").storage == "half"      # (after frame)


# ---- the C-ABI without a GPU -------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound(pkg):
    from airfoil_cfd_tool_amd.polar import POLAR_LIB_PATH
    with open(os.path.join(ROOT, "include", "wt_polar.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", POLAR_LIB_PATH], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = pkg.polar.load_polar_library()
    assert re.search(r"\bint\s+wtp_create_stored\s*\(\s*int\s+nx\s*,\s*int\s+ny\s*,\s*int\s+dtype\s*,\s*int\s+storage\s*,\s*int\s+members\s*,"
                     r"\s*int\s+history_cap\s*,\s*int\s+device\s*,\s*wtp_batch\s*\*\*\s*out\s*\)", header)
    assert re.search(r"\bint\s+wtp_read_stored\s*\(\s*wtp_batch\s*\*\s*b\s*,\s*int\s+member\s*,\s*uint16_t\s*\*\s*h\s*\)", header)
    assert re.search(r"#define\s+WTP_STORE_NATIVE\s+0\b", header) and re.search(r"#define\s+WTP_STORE_HALF\s+1\b", header)
    assert pkg.polar.WTP_STORE_NATIVE == 0 and pkg.polar.WTP_STORE_HALF == 1
    assert {"wtp_create_stored", "wtp_read_stored"} <= syms
    assert lib.wtp_create_stored.argtypes == [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_void_p)]
    assert lib.wtp_read_stored.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert b"half-precision population storage" in lib.wtp_version()

    # the header, the kernel's comment and the reference carry one definition
    def words(path):
        with open(path) as fh:
            return " ".join(" ".join(re.sub(r"^\s*(/?\*+/?|//)", "", line) for line in fh.read().splitlines()).split())
    ref = words(os.path.join(ROOT, "tests", "_half_reference.py"))
    definition = ref[ref.index("Weights. w_k are"):ref.index("the macroscopic planes are unchanged.") + len("the macroscopic planes are unchanged.")]
    for needle in ("4.0f/9.0f for k = 0, 1.0f/9.0f for k = 1..4, 1.0f/36.0f for k = 5..8", "Store. h = RN16(f - w_k)", "round-to-nearest-even",
                   "Subnormal halves are kept; nothing is flushed and nothing is scaled.", "Load. f = (float)h + w_k",
                   "solid (the swap), outlet (the copy), far field (the equilibrium), interior", "Start. wtp_init_equilibrium stores Store(v_k)"):
        assert needle in definition, needle
    for path in (os.path.join(ROOT, "include", "wt_polar.h"), os.path.join(ROOT, "airfoil-cfd-tool_amd", "csrc", "polar.hip")):
        assert definition in words(path), path
    head = words(os.path.join(ROOT, "include", "wt_polar.h")).split("Half-precision population storage")[1]
    assert "Out of scope" in head and "wtp_enable_ibb and wtp_set_wall_q on a half batch return WT_ERR_STATE" in head


@pytest.mark.parametrize("dtype,storage,needle", [(WT_F64, 1, b"WT_F32"), (WT_F32, 2, b"storage"), (WT_F32, -1, b"storage"), (WT_F64, 7, b"storage")])
def test_create_stored_argument_errors_without_a_gpu(pkg, dtype, storage, needle):
    lib = pkg.polar.load_polar_library()
    b = ctypes.c_void_p()
    assert lib.wtp_create_stored(64, 64, dtype, storage, 4, 8, 0, ctypes.byref(b)) == WT_ERR_ARG
    assert needle in lib.wtp_last_error()
    assert not b
    assert lib.wtp_create_stored(2, 64, WT_F32, 1, 4, 8, 0, ctypes.byref(b)) == WT_ERR_ARG and b"3x3" in lib.wtp_last_error()
    assert lib.wtp_read_stored(None, 0, None) == WT_ERR_ARG and b"null batch" in lib.wtp_last_error()


# ---- 5. closeness ------------------------------------------------------------------------------
def test_half_storage_stays_close_to_fp32_storage_and_differs_in_every_interior_fluid_cell(pkg, oracle_np):
    """96x48, NACA 2412 at 6 degrees, tau 0.52, U0 0.08, 60 steps of the wrapped oracle against the fp32 oracle (lbm_numpy.run).
    Measured on the CPU when the feature was written: max |f_half - f_fp32| = 7.664e-5 over all populations and cells, every interior
    fluid cell differs, the largest stored |h| is 0.0385.  The bound is four times the measured value, 3.07e-4, the margin for other
    members (the GPU tests' members reach 1.39e-4)."""
    nx, ny, tau, u0, steps = 96, 48, 0.52, 0.08, 60
    mask = pkg.geometry.build_geometry(nx, ny, 6.0, None, "naca2412").mask
    f32 = oracle_np.run(mask, steps, tau, u0, np.float32)[0]
    h, macro = half.run(mask, steps, tau, u0)
    f = half.load(h)
    inner = np.zeros((ny, nx), bool)
    inner[1:ny - 1, 1:nx - 1] = True
    inner &= mask == 0
    worst = float(np.abs(f.astype(np.float64) - f32.astype(np.float64)).max())
    stored = float(np.abs(h.astype(np.float32)).max())
    a = np.abs(h.astype(np.float32))
    print(f"max |f_half - f_fp32| = {worst:.4g}, max |h| = {stored:.4g}, subnormal halves {int(((a > 0) & (a < 2.0 ** -14)).sum())}")
    assert (f != f32).any(axis=0)[inner].all()
    assert worst <= 4 * 7.664e-5
    assert stored < 0.05 and np.isfinite(h).all()
    assert all(m.dtype == np.float32 for m in macro)


# ---- the kernels' code object ------------------------------------------------------------------
@pytest.fixture(scope="module")
def polar_isa():
    return _polar_isa.polar_isa()


def test_half_kernels_have_their_instantiations_and_no_scratch(polar_isa):
    """k_step_half_batch: emitting and not, BGK and Smagorinsky, axial and inclined.  No spill."""
    chk, files = polar_isa
    family = lambda v: v[0] == "half" and v[3] in (_polar_isa.BGK, _polar_isa.LES)      # noqa: E731
    step = _polar_isa.step_kernels(chk, files, family)
    seen = {}
    for f in files:
        for name, r in chk.resources(f).items():
            if name in step or _polar_isa.mex_variant(name) == ("half", "Halfway") or "k_fill_half" in name:
                seen[name] = r
                assert r.get("private_seg_size", 0) == 0, (name, r)
    print({k: v.get("num_vgpr") for k, v in seen.items()})
    assert sum(n in step for n in seen) == 8, sorted(seen)
    assert sum(_polar_isa.mex_variant(n) == ("half", "Halfway") for n in seen) == 1 and sum("k_fill_half" in n for n in seen) == 1, sorted(seen)
