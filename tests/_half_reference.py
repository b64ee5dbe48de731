"""Half-precision population storage of batched sweeps (include/wt_polar.h, wtp_create_stored with WTP_STORE_HALF) in NumPy: test
infrastructure only.

The model is a wrapper around any base step of the fp32 reference: oracle.lbm_numpy.step, _les_reference.step, or
_wind_reference.wind_step around either.  The header's definition:

  Weights.  w_k are the fp32 weights as feq_all forms them: 4.0f/9.0f for k = 0, 1.0f/9.0f for k = 1..4, 1.0f/36.0f for
  k = 5..8, each one fp32 division.
  Store.  h = RN16(f - w_k): one fp32 subtraction, then one conversion to IEEE binary16, round-to-nearest-even.  Subnormal
  halves are kept; nothing is flushed and nothing is scaled.
  Load.  f = (float)h + w_k: an exact conversion and one fp32 addition.
  Step.  Every population a step reads goes through Load and every population it writes goes through Store, in every branch:
  solid (the swap), outlet (the copy), far field (the equilibrium), interior.  Everything between is the fp32 step, operation
  for operation: gather, half-way bounce-back, moments, the net, the collision.  The macroscopic planes stay fp32 and hold what
  the fp32 arithmetic produced.
  Start.  wtp_init_equilibrium stores Store(v_k) of the fp32 start values it forms without the mode, including the
  inclined-stream start; the macroscopic planes are unchanged.

NumPy's float32 -> float16 conversion rounds to nearest even and keeps subnormals; float16 -> float32 is exact.
"""
import numpy as np

import lbm_numpy
import _wind_reference as wind

F32 = np.float32
# the weights, one fp32 division each; [9][1][1] so that they broadcast over [9][NY][NX]
W = np.array([F32(4.0) / F32(9.0)] + [F32(1.0) / F32(9.0)] * 4 + [F32(1.0) / F32(36.0)] * 4, dtype=F32).reshape(9, 1, 1)


def load(h):
    """[9][...] float16 (or its uint16 bit patterns) -> the fp32 populations."""
    h = np.asarray(h)
    if h.dtype == np.uint16:
        h = h.view(np.float16)
    assert h.dtype == np.float16
    w = W.reshape((9,) + (1,) * (h.ndim - 1))
    out = h.astype(F32) + w
    assert out.dtype == F32
    return out


def store(f):
    """[9][...] float32 -> the stored float16 deviations."""
    f = np.asarray(f)
    assert f.dtype == F32
    w = W.reshape((9,) + (1,) * (f.ndim - 1))
    d = f - w
    assert d.dtype == F32
    with np.errstate(over="ignore"):
        return d.astype(np.float16)


def half_step(base_step, h, solid, tau, u0, *extra):
    """One step of `base_step(f, solid, tau, u0, *extra)` on stored halves.  Returns (h_out, (rho, ux, uy)) and whatever the base
    step returns after them."""
    out = base_step(load(h), solid, tau, u0, *extra)
    return (store(out[0]), out[1], *out[2:])


def half_init(nx, ny, u0, v0=0.0):
    """The start state: (h [9][NY][NX] float16, (rho, ux, uy) float32).  With v0 = 0 the fp32 values are equilibrium_init's."""
    f, macro = wind.wind_init(nx, ny, u0, v0, F32)
    if v0 == 0:
        assert f.tobytes() == lbm_numpy.equilibrium_init(nx, ny, u0, F32)[0].tobytes()
    return store(f), macro


def windy(base_step):
    """`base_step` under the inclined free stream: a base step that takes v0 after u0."""
    def step(f, solid, tau, u0, v0, *extra):
        return wind.wind_step(base_step, f, solid, tau, u0, v0, *extra)
    return step


def run(solid, steps, tau, u0, *extra, base_step=lbm_numpy.step, v0=0.0, h=None):
    """`steps` wrapped steps from `h` (default: half_init(u0, v0); v0 only sets the start state, a wind base step takes its own v0
    through `extra`).  Returns what the last step returned, (h, (rho, ux, uy), ...)."""
    ny, nx = solid.shape
    out = None
    if h is None:
        h, macro = half_init(nx, ny, u0, v0)
        out = (h, macro)
    for _ in range(steps):
        out = half_step(base_step, h, solid, tau, u0, *extra)
        h = out[0]
    return out
