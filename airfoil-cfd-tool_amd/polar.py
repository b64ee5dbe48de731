"""Angle-of-attack sweeps on the LBM wind tunnel: many small tunnels in one launch.

The reference's analysis page sweeps the angle of attack (``pages/Airfoil_Analysis.py:758-787``, range -20..20 deg)
with one XFOIL request per angle (``:930-966``) and tabulates CL, CD, L/D and Cm per angle.  Here the angles of a
sweep are the members of one batch of ``libwtpolar.so`` (include/wt_polar.h): every member is a whole wind tunnel,
bit-identical to a :class:`~airfoil_cfd_tool_amd.WindTunnel` with the same inputs, and all of them advance by one
kernel launch per step.  Lift, drag and separation are sampled on the device into a history that is read once; with
surface loads enabled (``PolarEngine.enable_loads``, ``run_polar(loads=True)``) so are the pitching moment and the
chordwise surface pressure; with the momentum exchange enabled (``PolarEngine.enable_momentum_exchange``,
``run_polar(total_forces=True)``) a second force read-out that holds pressure and friction together; with the mean fields
enabled (``PolarEngine.enable_mean_fields``, ``run_polar(mean_fields=True)``) the time-mean flow field of every angle and the
fluctuation about it (:func:`mean_flow`: Reynolds stresses, pressure r.m.s.), from seven running sums kept on the device.
At airfoil Reynolds numbers, where tau falls to within 1e-3 of 0.5, the Smagorinsky subgrid viscosity
(``PolarEngine.enable_les``, ``run_polar(les=0.1)``) keeps the members off the stability net.  With interpolated bounce-back
(``PolarEngine.enable_interpolated_walls``, ``run_polar(walls="interpolated")``) the wall of every member is the panel polygon
itself, through a wall distance per link (``geometry.wall_distances``), and not the staircase of its raster mask.  With an
inclined free stream (``PolarEngine.enable_wind``, ``run_polar(frame="wind")``) every member holds the same body at 0 degrees
and the angle of attack turns its free stream, so the polar carries no raster jump from angle to angle.  With half-precision
population storage (``PolarEngine(storage="half")``, ``run_polar(storage="half")``) a float32 batch keeps every population as the
binary16 deviation from its lattice weight and computes in fp32: half the bytes per step and per batch, at a small bias of CL and CD.
A sweep can be continued without a second warm-up: ``PolarEngine.state`` / ``restore`` (``write_f``, ``write_stored``,
``set_step_count``) and ``run_polar(keep_state=True)`` followed by ``run_polar(start=result.state)``.
With the two-relaxation-time collision (``PolarEngine.enable_trt``, ``run_polar(collision="trt")``) the effective position of a
half-way wall is set by a magic number and not by tau, so a body keeps its thickness when the Reynolds number of a sweep changes.
With a prescribed far-field profile (``PolarEngine.enable_far_profile`` / ``set_far_profile``) every far-field cell holds the
equilibrium of its own (rho, ux, uy); ``run_polar(far_field="vortex")`` uses it for the textbook far-field correction of airfoil
computations, the free stream plus a point vortex that follows the lift (:func:`far_profile`, :func:`vortex_update`);
``run_polar(vortex_on="device")`` leaves those updates to the device (``PolarEngine.enable_far_vortex``), in stream order and without a wait.
With probe points (``PolarEngine.enable_probes`` / ``set_probes``) the device samples (rho, ux, uy) at caller-given points of every member
and keeps their running sums; ``run_polar(boundary_layer=True)`` puts rakes along the wall normals (``geometry.surface_stations``,
:func:`boundary_layer_points`) and attaches the boundary-layer read-out of every angle (:func:`boundary_layer`: x/c, Ue, delta*, theta, Cf,
H per surface and where the skin friction changes sign).
With a wall velocity (``PolarEngine.enable_wall_velocity`` / ``set_wall_velocity``, on top of interpolated bounce-back) the walls of a
member move or transpire: a velocity per wall link (``geometry.rigid_wall_velocity``, ``geometry.slot_wall_velocity``) enters the
reflected population as Ladd's moving-wall term; ``run_polar(walls="interpolated", slot={...})`` blows or sucks through a slot.

* :class:`PolarEngine` — ctypes binding of libwtpolar.so (loaded lazily, after torch, like ``_capi.load_library``).
* :func:`run_polar` — masks from ``geometry.build_geometry`` per angle, warm-up, sampled run, statistics per angle.
* :func:`sweep_alphas` / :func:`polar_rows` — the page's list of angles and its sweep-table rows.
"""
from __future__ import annotations

import ctypes
import math
import os
from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_int64, c_void_p
from dataclasses import InitVar, dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import geometry as geo
from ._capi import WT_F32, WT_F64, WT_OK, WTError, _np_dtype
from .windtunnel import TAU_DEFAULT, U0_DEFAULT, chord_cells, stall_label, tau_from_reynolds

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
POLAR_LIB_PATH = os.path.join(_PKG_DIR, "lib", "libwtpolar.so")

EXPORTS = (
    "wtp_create", "wtp_destroy", "wtp_last_error", "wtp_version", "wtp_set_masks", "wtp_init_equilibrium", "wtp_step",
    "wtp_history", "wtp_clear_history", "wtp_forces", "wtp_clamp_events", "wtp_read_f", "wtp_read_macro", "wtp_sync",
    "wtp_enable_loads", "wtp_history_moment", "wtp_moment", "wtp_surface",
    "wtp_enable_mex", "wtp_history_mex", "wtp_mex",
    "wtp_enable_mean", "wtp_mean_sums",
    "wtp_enable_les",
    "wtp_enable_ibb", "wtp_set_wall_q",
    "wtp_enable_wind",
    "wtp_create_stored", "wtp_read_stored",
    "wtp_write_f", "wtp_write_stored", "wtp_step_count", "wtp_set_step_count",
    "wtp_enable_trt",
    "wtp_enable_far_profile", "wtp_set_far_profile", "wtp_read_far_profile",
    "wtp_enable_far_vortex", "wtp_set_far_vortex", "wtp_far_vortex", "wtp_far_vortex_update", "wtp_far_vortex_log",
    "wtp_enable_probes", "wtp_set_probes", "wtp_probe_sums", "wtp_probe_sample",
    "wtp_enable_wall_velocity", "wtp_set_wall_velocity",
)

WTP_STORE_NATIVE, WTP_STORE_HALF = 0, 1
WALLS = ("staircase", "interpolated")                              # run_polar's wall rules
STORAGES = ("native", "half")                                      # how a batch stores its populations: in its dtype, or as binary16 deviations from the weights
COLLISIONS = ("bgk", "trt")                                        # run_polar's collisions: single relaxation time, or two with a magic number
MAGIC_DEFAULT = 3 / 16                                             # the magic number at which a half-way wall of a Poiseuille flow sits half-way at every tau
FAR_FIELDS = ("uniform", "vortex", "vortex+source")                 # run_polar's far fields: the free stream alone, plus a point vortex from the lift, plus a source from the drag
VORTEX_SPEED_MAX = 0.1                                             # the largest speed the vortex and the source together may induce at the nearest far-field cell centre
VORTEX_ON = ("host", "device")                                     # who updates the vortex of run_polar: the host between chunks of steps, or the device in stream order
VORTEX_NORMS = ("hypot", "sqrt")                                   # vortex_update's norm of (strength, source): np.hypot, or sqrt(s*s + q*q) as the device forms it
FRAMES = ("body", "wind")                                          # run_polar's ways to set the angle: turn the body, or the free stream
WIND_ALPHA_MAX = 30.0                                              # degrees: the largest |angle| of a frame="wind" sweep
MEAN_SUMS = ("rho", "ux", "uy", "rho2", "ux2", "uy2", "uxuy")      # wtp_mean_sums' planes, in its order
WTP_MAX_PROBES = 1 << 20                                           # the most probe points a member holds (wt_polar.h)
BL_HEIGHT_DEFAULT, BL_SPACING_DEFAULT = 0.15, 0.5                  # run_polar's boundary-layer rake: its height in chords and the spacing of its points in cells
BL_EDGE = 0.99                                                     # the share of the rake's largest tangential speed that marks the boundary layer's edge

_lib = None


def load_polar_library(path: str = POLAR_LIB_PATH, optional: Sequence[str] = ()) -> ctypes.CDLL:
    """Load libwtpolar.so, importing torch first when it is importable (one HIP runtime per process, as _capi.load_library).
    `optional`: entry points that an older build given as `path` may lack (tools/polar_bench.py --lib, to time a parent commit's
    library); every other one of EXPORTS is required, and so are these in the package's own library."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build it with `make lib`. There is no CPU fallback for the batched kernels.")
    try:
        import torch  # noqa: F401  (side effect: loads torch's libamdhip64 first)
    except Exception:  # pragma: no cover
        pass
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    B = c_void_p
    dp, ip = POINTER(c_double), POINTER(c_int64)
    sig = {
        "wtp_create": ([c_int, c_int, c_int, c_int, c_int, c_int, POINTER(B)], c_int),
        "wtp_destroy": ([B], c_int),
        "wtp_last_error": ([], c_char_p),
        "wtp_version": ([], c_char_p),
        "wtp_set_masks": ([B, c_int, c_int, c_void_p], c_int),
        "wtp_init_equilibrium": ([B, dp], c_int),
        "wtp_step": ([B, c_int, dp, dp, c_int], c_int),
        "wtp_history": ([B, c_int, c_int, ip, dp, dp, ip, ip], c_int),
        "wtp_clear_history": ([B], c_int),
        "wtp_forces": ([B, dp, dp, ip, ip], c_int),
        "wtp_clamp_events": ([B, ip, ip], c_int),
        "wtp_read_f": ([B, c_int, c_void_p], c_int),
        "wtp_read_macro": ([B, c_int, c_void_p, c_void_p, c_void_p], c_int),
        "wtp_sync": ([B], c_int),
        "wtp_enable_loads": ([B, dp, dp], c_int),
        "wtp_history_moment": ([B, c_int, c_int, dp], c_int),
        "wtp_moment": ([B, dp], c_int),
        "wtp_surface": ([B, c_int, dp, dp, ip, ip, POINTER(c_int32), POINTER(c_int32)], c_int),
        "wtp_enable_mex": ([B, dp, dp], c_int),
        "wtp_history_mex": ([B, c_int, c_int, dp, dp, dp, ip], c_int),
        "wtp_mex": ([B, dp, dp, dp, ip], c_int),
        "wtp_enable_mean": ([B], c_int),
        "wtp_mean_sums": ([B, c_int, ip, dp, dp, dp, dp, dp, dp, dp], c_int),
        "wtp_enable_les": ([B, dp], c_int),
        "wtp_enable_ibb": ([B, c_int], c_int),
        "wtp_set_wall_q": ([B, c_int, c_int, c_void_p], c_int),
        "wtp_enable_wind": ([B, dp], c_int),
        "wtp_create_stored": ([c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(B)], c_int),
        "wtp_read_stored": ([B, c_int, c_void_p], c_int),
        "wtp_write_f": ([B, c_int, c_void_p], c_int),
        "wtp_write_stored": ([B, c_int, c_void_p], c_int),
        "wtp_step_count": ([B, ip], c_int),
        "wtp_set_step_count": ([B, c_int64], c_int),
        "wtp_enable_trt": ([B, dp], c_int),
        "wtp_enable_far_profile": ([B, c_int], c_int),
        "wtp_set_far_profile": ([B, c_int, c_int, c_void_p, c_void_p, c_void_p], c_int),
        "wtp_read_far_profile": ([B, c_int, c_int, c_void_p, c_void_p, c_void_p], c_int),
        "wtp_enable_far_vortex": ([B, c_int, c_int64, c_double, c_double, c_int, c_double, c_double, dp, dp, dp, dp, c_int], c_int),
        "wtp_set_far_vortex": ([B, dp, dp], c_int),
        "wtp_far_vortex": ([B, dp, dp], c_int),
        "wtp_far_vortex_update": ([B], c_int),
        "wtp_far_vortex_log": ([B, c_int, c_int, ip, dp, dp, dp, dp, POINTER(c_int32)], c_int),
        "wtp_enable_probes": ([B, c_int], c_int),
        "wtp_set_probes": ([B, c_int, c_int, dp, dp], c_int),
        "wtp_probe_sums": ([B, c_int, ip, dp, dp, dp], c_int),
        "wtp_probe_sample": ([B, c_int, dp, dp, dp], c_int),
        "wtp_enable_wall_velocity": ([B, c_int], c_int),
        "wtp_set_wall_velocity": ([B, c_int, c_int, c_void_p], c_int),
    }
    for name, (argtypes, restype) in sig.items():
        if name in optional and path != POLAR_LIB_PATH and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = lib
    return lib


def _check(rc: int) -> int:
    if rc < WT_OK:
        raise WTError(rc, load_polar_library().wtp_last_error().decode("utf-8", "replace"))
    return rc


def _check_storage(storage, dtype, walls: str = "staircase") -> None:
    """ValueError for a storage outside STORAGES, and for "half" with a dtype other than float32 or with interpolated walls."""
    if not isinstance(storage, str) or storage not in STORAGES:
        raise ValueError(f"storage must be one of {STORAGES}, got {storage!r}")
    if storage == "half":
        if _np_dtype(dtype) != np.float32:
            raise ValueError('storage="half" stores float32 batches only')
        if walls == "interpolated":
            raise ValueError('storage="half" does not combine with walls="interpolated"')


def _check_state(state, nx: int, ny: int, dtype, storage: str, members: int) -> None:
    """ValueError where a PolarEngine.state() does not fit a batch of `members` nx x ny tunnels of `dtype` and `storage`."""
    try:
        got = (int(state["nx"]), int(state["ny"]), np.dtype(state["dtype"]), state["storage"], int(state["members"]))
        int(state["steps"]), state["f"]
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError(f"not a PolarEngine.state(): {e!r}") from None
    want = (int(nx), int(ny), _np_dtype(dtype), storage, int(members))
    for name, g, w in zip(("nx", "ny", "dtype", "storage", "members"), got, want):
        if g != w:
            raise ValueError(f"the state's {name} is {g!s}, the batch's is {w!s}")
    stored = np.uint16 if storage == "half" else want[2]
    f = np.asarray(state["f"])
    if f.shape != (want[4], 9, want[1], want[0]) or f.dtype != np.dtype(stored):
        raise ValueError(f"the state's f must be [B][9][NY][NX] = {(want[4], 9, want[1], want[0])} of {np.dtype(stored).name}, "
                         f"got {f.shape} of {f.dtype.name}")


def _f64(a, n: int) -> np.ndarray:
    """One value or [n] values -> a contiguous float64 [n]."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)))


def _dp(a: np.ndarray):
    return a.ctypes.data_as(POINTER(c_double))


def _ip(a: np.ndarray):
    return a.ctypes.data_as(POINTER(c_int64))


class PolarEngine:
    """One libwtpolar batch: `members` whole tunnels of nx x ny, each with its own mask, tau and U0."""

    def __init__(self, nx: int, ny: int, members: int, dtype="float32", history_cap: int = 0, device: int = 0, storage: str = "native"):
        """storage: "native" keeps the populations in `dtype`; "half" (float32 only) keeps each as the binary16 deviation from its
        lattice weight, with fp32 arithmetic (wt_polar.h "Half-precision population storage"): half the bytes per step and per batch."""
        _check_storage(storage, dtype)
        self._lib = load_polar_library()
        self.dtype = _np_dtype(dtype)
        self.storage = storage
        self.nx, self.ny, self.members, self.history_cap = int(nx), int(ny), int(members), int(history_cap)
        self._b = c_void_p()
        self.loads_enabled = False
        self.mex_enabled = False
        self.mean_enabled = False
        self.les_enabled = False
        self.interpolated_walls = False
        self.wall_velocity_enabled = False
        self._wind = False
        self._trt = False
        self._far_profile = False
        self._far_vortex = False
        self._far_given = np.zeros(self.members, bool)      # which members have tables (set_far_profile, enable_far_vortex)
        self._probes = 0                                    # probe points per member (0: the read-out is off)
        code = WT_F32 if self.dtype == np.float32 else WT_F64
        if storage == "half":
            _check(self._lib.wtp_create_stored(self.nx, self.ny, code, WTP_STORE_HALF, self.members, self.history_cap, int(device),
                                               ctypes.byref(self._b)))
        else:
            _check(self._lib.wtp_create(self.nx, self.ny, code, self.members, self.history_cap, int(device), ctypes.byref(self._b)))

    def close(self) -> None:
        if getattr(self, "_b", None) is not None and self._b:
            self._lib.wtp_destroy(self._b)
            self._b = c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_masks(self, masks, first: int = 0) -> None:
        """masks [count][NY][NX] (or one [NY][NX]) for members first .. first+count-1; flow kept."""
        m = np.ascontiguousarray(masks, dtype=np.uint8)
        if m.ndim == 2:
            m = m[None]
        if m.shape[1:] != (self.ny, self.nx):
            raise ValueError(f"masks must have shape [count][NY][NX] = [count]{(self.ny, self.nx)}, got {m.shape}")
        _check(self._lib.wtp_set_masks(self._b, int(first), int(m.shape[0]), m.ctypes.data_as(c_void_p)))

    def init_equilibrium(self, u0) -> None:
        """u0: one value or [B]."""
        v = _f64(u0, self.members)
        _check(self._lib.wtp_init_equilibrium(self._b, _dp(v)))

    def step(self, nsteps: int, tau, u0, sample_every: int = 0) -> None:
        """Enqueue nsteps steps of every member; tau, u0: one value or [B]."""
        t, u = _f64(tau, self.members), _f64(u0, self.members)
        _check(self._lib.wtp_step(self._b, int(nsteps), _dp(t), _dp(u), int(sample_every)))

    def history(self) -> Dict[str, np.ndarray]:
        """Every row held: step [R], fx / fy [R][B] float64, surf / rev [R][B] int64; with loads enabled also mz [R][B] float64;
        with the momentum exchange enabled also fx_mex / fy_mex / mz_mex [R][B] float64 and links [R][B] int64."""
        rows = _check(self._lib.wtp_history(self._b, 0, 0, None, None, None, None, None))
        B = self.members
        out = {"step": np.empty(rows, np.int64), "fx": np.empty((rows, B)), "fy": np.empty((rows, B)),
               "surf": np.empty((rows, B), np.int64), "rev": np.empty((rows, B), np.int64)}
        _check(self._lib.wtp_history(self._b, 0, rows, _ip(out["step"]), _dp(out["fx"]), _dp(out["fy"]), _ip(out["surf"]),
                                     _ip(out["rev"])))
        if self.loads_enabled:
            out["mz"] = np.empty((rows, B))
            _check(self._lib.wtp_history_moment(self._b, 0, rows, _dp(out["mz"])))
        if self.mex_enabled:
            out.update({"fx_mex": np.empty((rows, B)), "fy_mex": np.empty((rows, B)), "mz_mex": np.empty((rows, B)),
                        "links": np.empty((rows, B), np.int64)})
            _check(self._lib.wtp_history_mex(self._b, 0, rows, _dp(out["fx_mex"]), _dp(out["fy_mex"]), _dp(out["mz_mex"]),
                                             _ip(out["links"])))
        return out

    def clear_history(self) -> None:
        _check(self._lib.wtp_clear_history(self._b))

    def forces(self):
        """(fx, fy, surf, rev), [B] each, of the last emitted state (wt_forces per member)."""
        B = self.members
        fx, fy, surf, rev = np.empty(B), np.empty(B), np.empty(B, np.int64), np.empty(B, np.int64)
        _check(self._lib.wtp_forces(self._b, _dp(fx), _dp(fy), _ip(surf), _ip(rev)))
        return fx, fy, surf, rev

    def enable_loads(self, xref, yref) -> None:
        """Sample the pitching moment about (xref, yref) (one value or [B], lattice units) and the surface density sums from the
        next sample on (wt_polar.h).  Calling it again replaces the points and clears the sums."""
        x, y = _f64(xref, self.members), _f64(yref, self.members)
        _check(self._lib.wtp_enable_loads(self._b, _dp(x), _dp(y)))
        self.loads_enabled = True

    def moment(self) -> np.ndarray:
        """Mz [B] of the last emitted state, counter-clockwise positive, lattice units; adds nothing to the surface sums."""
        mz = np.empty(self.members)
        _check(self._lib.wtp_moment(self._b, _dp(mz)))
        return mz

    def surface(self, member: int) -> Dict[str, np.ndarray]:
        """One member's surface sums per column: rho_upper / rho_lower (sums of rho over the samples), n_upper / n_lower (samples
        added), j_upper / j_lower (row of the sampled fluid cell, -1 where the column has none)."""
        nx = self.nx
        out = {"rho_upper": np.empty(nx), "rho_lower": np.empty(nx), "n_upper": np.empty(nx, np.int64), "n_lower": np.empty(nx, np.int64),
               "j_upper": np.empty(nx, np.int32), "j_lower": np.empty(nx, np.int32)}
        _check(self._lib.wtp_surface(self._b, int(member), _dp(out["rho_upper"]), _dp(out["rho_lower"]), _ip(out["n_upper"]),
                                     _ip(out["n_lower"]), out["j_upper"].ctypes.data_as(POINTER(c_int32)),
                                     out["j_lower"].ctypes.data_as(POINTER(c_int32))))
        return out

    def enable_momentum_exchange(self, xref, yref) -> None:
        """Sample the momentum-exchange force (pressure and friction together), its moment about (xref, yref) (one value or [B],
        lattice units) and the number of links from the next sample on (wt_polar.h).  Calling it again replaces the points.
        Independent of enable_loads."""
        x, y = _f64(xref, self.members), _f64(yref, self.members)
        _check(self._lib.wtp_enable_mex(self._b, _dp(x), _dp(y)))
        self.mex_enabled = True

    def momentum_exchange(self):
        """(fx, fy, mz, links), [B] each, of the current lattice: the momentum-exchange twin of forces() / moment()."""
        B = self.members
        fx, fy, mz, links = np.empty(B), np.empty(B), np.empty(B), np.empty(B, np.int64)
        _check(self._lib.wtp_mex(self._b, _dp(fx), _dp(fy), _dp(mz), _ip(links)))
        return fx, fy, mz, links

    def enable_mean_fields(self) -> None:
        """Add rho, ux, uy of every cell and their products to seven running sums per member from the next sample on
        (wt_polar.h).  Calling it again zeroes the sums and the counts.  Independent of enable_loads and
        enable_momentum_exchange."""
        _check(self._lib.wtp_enable_mean(self._b))
        self.mean_enabled = True

    def mean_sums(self, member: int) -> Dict[str, np.ndarray]:
        """One member's sample count `n` and its seven sums over the samples, [NY][NX] float64 each: rho, ux, uy, rho2, ux2,
        uy2, uxuy (see mean_flow)."""
        n = np.zeros(1, np.int64)
        out = {k: np.empty((self.ny, self.nx)) for k in MEAN_SUMS}
        _check(self._lib.wtp_mean_sums(self._b, int(member), _ip(n), *(_dp(out[k]) for k in MEAN_SUMS)))
        return {"n": int(n[0]), **out}

    def enable_les(self, cs) -> None:
        """Collide with a Smagorinsky eddy viscosity from the next step on (wt_polar.h): cs is the Smagorinsky constant, one value
        or [B], each in [0, 0.5]; a member with cs = 0 stays a BGK member, bit for bit.  None switches the model off again.  The
        flow state, the history and every running sum are kept; independent of the read-outs."""
        if cs is None:
            _check(self._lib.wtp_enable_les(self._b, None))
            self.les_enabled = False
            return
        v = _f64(cs, self.members)
        _check(self._lib.wtp_enable_les(self._b, _dp(v)))
        self.les_enabled = True

    def enable_interpolated_walls(self, on: bool = True) -> None:
        """Reflect at the walls by linear interpolated bounce-back from the next step on (wt_polar.h): every link uses its wall
        distance, 0.5 (half-way, the staircase) until set_wall_distances gives the true ones.  on=False switches back to the
        half-way kernels and keeps the distances.  The flow state, the history and every running sum are kept; combines with
        enable_les, independent of the read-outs."""
        _check(self._lib.wtp_enable_ibb(self._b, 1 if on else 0))
        self.interpolated_walls = bool(on)
        if not on:
            self.wall_velocity_enabled = False

    def set_wall_distances(self, q, first: int = 0) -> None:
        """q [count][8][NY][NX] (or one [8][NY][NX]) for members first .. first+count-1, each value in (0, 1], plane k - 1 for
        direction k (geometry.wall_distances); converted to the batch's dtype.  After set_masks, which resets the distances of
        the members it touches to 0.5."""
        a = np.ascontiguousarray(q, dtype=self.dtype)
        if a.ndim == 3:
            a = a[None]
        if a.ndim != 4 or a.shape[1:] != (8, self.ny, self.nx):
            raise ValueError(f"wall distances must have shape [count][8][NY][NX] = [count]{(8, self.ny, self.nx)}, got {a.shape}")
        _check(self._lib.wtp_set_wall_q(self._b, int(first), int(a.shape[0]), a.ctypes.data_as(c_void_p)))

    def enable_wall_velocity(self, on: bool = True) -> None:
        """Let the walls move or transpire from the next step on (wt_polar.h "Wall velocity"): every link carries Ladd's moving-wall term
        with its wall-normal velocity, +0 (a wall at rest) until set_wall_velocity gives others.  Needs enable_interpolated_walls;
        on=False switches back to the interpolating kernels and keeps the velocities, and so does enable_interpolated_walls(False).
        The flow state, the history, every running sum and every other setting are kept."""
        if not hasattr(self._lib, "wtp_enable_wall_velocity"):
            raise WTError(-1, "this libwtpolar.so has no wall velocity (wtp_enable_wall_velocity)")
        _check(self._lib.wtp_enable_wall_velocity(self._b, 1 if on else 0))
        self.wall_velocity_enabled = bool(on)

    def set_wall_velocity(self, un, first: int = 0) -> None:
        """un [count][8][NY][NX] (or one [8][NY][NX]) for members first .. first+count-1: e_k . u_w at the wall point of every link,
        plane k - 1 for direction k (geometry.rigid_wall_velocity, geometry.slot_wall_velocity), each finite with |un| <= 0.5;
        converted to the batch's dtype.  After set_masks, which resets the velocities of the members it touches to +0, and after
        set_wall_distances.  The values hold until they are replaced; steps already enqueued see the old ones."""
        a = np.ascontiguousarray(un, dtype=self.dtype)
        if a.ndim == 3:
            a = a[None]
        if a.ndim != 4 or a.shape[1:] != (8, self.ny, self.nx):
            raise ValueError(f"wall velocities must have shape [count][8][NY][NX] = [count]{(8, self.ny, self.nx)}, got {a.shape}")
        _check(self._lib.wtp_set_wall_velocity(self._b, int(first), int(a.shape[0]), a.ctypes.data_as(c_void_p)))

    def enable_wind(self, v0) -> None:
        """Incline the free stream (wt_polar.h): v0 is the cross-flow of the far field, one value or [B], each finite with
        |v0| <= 0.35; the far-field cells hold the equilibrium of (u0, v0) from the next step on, and the next init_equilibrium
        starts every member from it.  A member with v0 = 0 stays an axial member, bit for bit.  None switches the model off
        again.  The flow state, the history and every running sum are kept; combines with enable_les and
        enable_interpolated_walls, independent of the read-outs, which stay in lattice axes (wind_axes)."""
        if v0 is None:
            _check(self._lib.wtp_enable_wind(self._b, None))
            self._wind = False
            return
        v = _f64(v0, self.members)
        _check(self._lib.wtp_enable_wind(self._b, _dp(v)))
        self._wind = True

    @property
    def wind_enabled(self) -> bool:
        return self._wind

    def enable_trt(self, magic) -> None:
        """Collide with two relaxation times from the next step on (wt_polar.h "Two-relaxation-time collision"): magic is the
        magic number (tau+ - 1/2)(tau- - 1/2), one value or [B], each finite with 0 < magic <= 1; 3/16 puts a half-way wall
        half-way at every tau, 1/4 is the most stable.  None switches the model off again: the following steps are those of a batch
        that never enabled it.  While it is on, step raises WTError (WT_ERR_ARG) for a tau that is not above 0.5 in the batch's
        dtype.  The flow state, the history, every running sum and every other enable_* setting are kept; combines with enable_les,
        enable_interpolated_walls, enable_wind and storage="half", independent of the read-outs."""
        if magic is None:
            _check(self._lib.wtp_enable_trt(self._b, None))
            self._trt = False
            return
        v = _f64(magic, self.members)
        _check(self._lib.wtp_enable_trt(self._b, _dp(v)))
        self._trt = True

    @property
    def trt_enabled(self) -> bool:
        return self._trt

    def enable_far_profile(self, on: bool = True) -> None:
        """Hold every far-field cell at the equilibrium of its own (rho, ux, uy) from the next step on (wt_polar.h "Prescribed
        far-field profile"); set_far_profile gives the tables, and step raises WTError (WT_ERR_STATE) while a member has none.
        on=False switches back to the uniform far field and its bits and keeps the tables.  u0 of step and v0 of enable_wind are
        then not read by far-field cells; they still set the start state.  WTError (WT_ERR_STATE) on a storage="half" batch.  The
        flow state, the history, every running sum and every other enable_* setting are kept; combines with enable_les,
        enable_interpolated_walls, enable_trt and enable_wind, independent of the read-outs."""
        _check(self._lib.wtp_enable_far_profile(self._b, 1 if on else 0))
        self._far_profile = bool(on)
        if not on:
            self._far_vortex = False             # (the library switches the device-side vortex off with the profile)

    @property
    def far_profile_enabled(self) -> bool:
        return self._far_profile

    def set_far_profile(self, left, bottom, top, first: int = 0) -> None:
        """The tables of members first .. first+count-1: left [count][3][NY] for the cells (0, j), bottom and top [count][3][NX] for
        the cells (i, 0) and (i, NY-1) (or one member's [3][NY], [3][NX], [3][NX]), planes rho, ux, uy, converted to the batch's
        dtype.  The corners of column 0 are `left`'s; entries 0 and NX-1 of bottom and top are never read.  Every value finite, rho
        in [0.5, 2], ux^2 + uy^2 <= 0.35^2, else WTError (WT_ERR_ARG) and the batch is left as it was.  After enable_far_profile.
        Steps already enqueued see the old tables."""
        tabs = []
        for a, n, what in ((left, self.ny, "left"), (bottom, self.nx, "bottom"), (top, self.nx, "top")):
            a = np.ascontiguousarray(a, dtype=self.dtype)
            if a.ndim == 2:
                a = a[None]
            if a.ndim != 3 or a.shape[1:] != (3, n) or a.shape[0] != (tabs[0].shape[0] if tabs else a.shape[0]):
                raise ValueError(f"{what} must have shape [count][3][{n}], got {a.shape}")
            tabs.append(a)
        count = int(tabs[0].shape[0])
        _check(self._lib.wtp_set_far_profile(self._b, int(first), count, *(t.ctypes.data_as(c_void_p) for t in tabs)))
        self._far_given[first:first + count] = True

    def read_far_profile(self, first: int = 0, count: Optional[int] = None):
        """The read twin of set_far_profile: (left [count][3][NY], bottom [count][3][NX], top [count][3][NX]) of members first ..
        first+count-1 (default: to the last) as the device holds them, whether set_far_profile uploaded them or the device-side
        vortex wrote them.  WTError (WT_ERR_STATE) while the model was never enabled or a member has no profile."""
        count = self.members - int(first) if count is None else int(count)
        n = max(count, 0)
        tabs = (np.empty((n, 3, self.ny), self.dtype), np.empty((n, 3, self.nx), self.dtype), np.empty((n, 3, self.nx), self.dtype))
        _check(self._lib.wtp_read_far_profile(self._b, int(first), count, *(t.ctypes.data_as(c_void_p) for t in tabs)))
        return tabs

    def enable_far_vortex(self, every: int, after: int, relax: float, u_ref: float, with_source: bool, xc: float, yc: float, u_far, v_far,
                          alpha=0.0, log_cap: int = 0) -> None:
        """Keep the tables of the far-field profile up to date on the device (wt_polar.h "Device-side far-field vortex"): the free
        stream (u_far, v_far) plus a point vortex and, with `with_source`, a source at (xc, yc) whose strengths follow the pressure
        force, in stream order between two steps, with nothing synchronised.  The step that brings the count of steps since this call
        to a multiple of `every`, at an absolute step count of at least `after`, is followed by one update: forces() on the device,
        vortex_update(..., norm="sqrt") with `relax`, `u_ref` and the member's `alpha` (degrees; its cosine and sine are formed here as
        wind_axes forms them), far_profile of the new strengths into the tables, and one row of the log (far_vortex_log), which holds
        `log_cap` updates; a step whose updates would overflow it raises WTError (WT_ERR_STATE).  u_far, v_far, alpha: one value or
        [B].  After enable_far_profile; every member then has a profile, built from the current strengths (zero at the first call, kept
        afterwards).  every=0 switches the update off and keeps tables and strengths (the other arguments are not read).  While it is
        on, set_far_profile raises WTError (WT_ERR_STATE).  The same run updated by the host (forces, vortex_update, far_profile,
        set_far_profile) has the same bits unless an update clips."""
        B = self.members
        a = np.radians(_f64(alpha, B))
        u, v, c, s = _f64(u_far, B), _f64(v_far, B), np.ascontiguousarray(np.cos(a)), np.ascontiguousarray(np.sin(a))
        _check(self._lib.wtp_enable_far_vortex(self._b, int(every), int(after), float(relax), float(u_ref), 1 if with_source else 0, float(xc),
                                               float(yc), _dp(u), _dp(v), _dp(c), _dp(s), int(log_cap)))
        self._far_vortex = int(every) != 0
        if self._far_vortex:
            self._far_given[:] = True

    @property
    def far_vortex_enabled(self) -> bool:
        return self._far_vortex

    def set_far_vortex(self, strength, source) -> None:
        """Replace the strengths and the sources (one value or [B]) of the device-side vortex and rebuild every table on the device: the
        restart path.  WTError (WT_ERR_ARG) for a pair that induces more than VORTEX_SPEED_MAX at the bound or is not finite."""
        s, q = _f64(strength, self.members), _f64(source, self.members)
        _check(self._lib.wtp_set_far_vortex(self._b, _dp(s), _dp(q)))

    def far_vortex(self):
        """(strength, source), [B] float64 each: the current values of the device-side vortex."""
        s, q = np.empty(self.members), np.empty(self.members)
        _check(self._lib.wtp_far_vortex(self._b, _dp(s), _dp(q)))
        return s, q

    def far_vortex_update(self) -> None:
        """One update of the device-side vortex now, from the last emitted state, logged with the current step count."""
        _check(self._lib.wtp_far_vortex_update(self._b))

    def far_vortex_log(self) -> Dict[str, np.ndarray]:
        """Every update held: step [U] int64, fx, fy (the forces the update read, lattice axes), strength, source [U][B] float64 (the
        values after the update) and clipped [U][B] bool.  init_equilibrium and clear_history empty it."""
        rows = _check(self._lib.wtp_far_vortex_log(self._b, 0, 0, None, None, None, None, None, None))
        B = self.members
        out = {"step": np.empty(rows, np.int64), **{k: np.empty((rows, B)) for k in ("fx", "fy", "strength", "source")}}
        clipped = np.empty((rows, B), np.int32)
        _check(self._lib.wtp_far_vortex_log(self._b, 0, rows, _ip(out["step"]), *(_dp(out[k]) for k in ("fx", "fy", "strength", "source")),
                                            clipped.ctypes.data_as(POINTER(c_int32))))
        out["clipped"] = clipped != 0
        return out

    def enable_probes(self, npoints: int) -> None:
        """Sample (rho, ux, uy) at `npoints` points per member from the next sample on and keep the running sums (wt_polar.h "Probe
        points"); set_probes gives the points, and until then every point is inactive.  Calling it again starts over: every point
        inactive, the sums empty.  0 switches the read-out off and releases its buffers.  WTError (WT_ERR_ARG) for a count outside
        [0, WTP_MAX_PROBES], (WT_ERR_OOM) where the buffers do not fit; the batch then goes on as it was.  Works with every dtype
        and storage; independent of the other read-outs, and every other value keeps its bits."""
        _check(self._lib.wtp_enable_probes(self._b, int(npoints)))
        self._probes = int(npoints)

    @property
    def probes_enabled(self) -> bool:
        return self._probes > 0

    def set_probes(self, x, y, first: int = 0) -> None:
        """The points of members first .. first+count-1: x, y [count][P] (or one member's [P]) float64, lattice units, the centre of
        cell (i, j) at (i + 0.5, j + 0.5); valid inside [0.5, NX - 0.5] x [0.5, NY - 0.5].  A point whose x is NaN is inactive: never
        sampled, its sums stay 0.  Any other point outside the rectangle raises WTError (WT_ERR_ARG) and the batch is left as it
        was.  The sums and the counts of the members touched, and of no other, start again at zero.  After enable_probes."""
        xs, ys = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y))
        if xs.ndim == 1:
            xs, ys = xs[None], (ys[None] if ys.ndim == 1 else ys)
        if xs.ndim != 2 or xs.shape != ys.shape or xs.shape[1] != self._probes:
            raise ValueError(f"x and y must both have shape [count][P] = [count][{self._probes}], got {xs.shape} and {ys.shape}")
        _check(self._lib.wtp_set_probes(self._b, int(first), int(xs.shape[0]), _dp(xs), _dp(ys)))

    def probe_sums(self, member: int) -> Dict[str, object]:
        """One member's sample count `n` and the sums of rho, ux, uy over the samples at its points, [P] float64 each (0 at inactive
        points).  The time mean at a point is sum / n."""
        n = np.zeros(1, np.int64)
        out = {k: np.empty(self._probes) for k in ("rho", "ux", "uy")}
        _check(self._lib.wtp_probe_sums(self._b, int(member), _ip(n), *(_dp(out[k]) for k in ("rho", "ux", "uy"))))
        return {"n": int(n[0]), **out}

    def probe_sample(self, member: int) -> Dict[str, np.ndarray]:
        """rho, ux, uy of the last emitted state at one member's points, [P] float64 each, NaN at inactive points: the twin of
        forces().  Adds nothing to the sums.  WTError (WT_ERR_STATE) after write_f until a step has run."""
        out = {k: np.empty(self._probes) for k in ("rho", "ux", "uy")}
        _check(self._lib.wtp_probe_sample(self._b, int(member), *(_dp(out[k]) for k in ("rho", "ux", "uy"))))
        return out

    def clamp_events(self):
        """(density events, speed events), [B] each."""
        a, b = np.empty(self.members, np.int64), np.empty(self.members, np.int64)
        _check(self._lib.wtp_clamp_events(self._b, _ip(a), _ip(b)))
        return a, b

    def read_f(self, member: int) -> np.ndarray:
        f = np.empty((9, self.ny, self.nx), dtype=self.dtype)
        _check(self._lib.wtp_read_f(self._b, int(member), f.ctypes.data_as(c_void_p)))
        return f

    def read_stored(self, member: int) -> np.ndarray:
        """The raw binary16 bit patterns of one member's lattice in a storage="half" batch, [9][NY][NX] uint16 (view them as
        float16 for the stored deviations); read_f returns the loaded fp32 values.  WTError (WT_ERR_STATE) on a native batch."""
        h = np.empty((9, self.ny, self.nx), dtype=np.uint16)
        _check(self._lib.wtp_read_stored(self._b, int(member), h.ctypes.data_as(c_void_p)))
        return h

    def _planes(self, a, dtype, what: str) -> np.ndarray:
        """`a` as a contiguous [9][NY][NX] array of `dtype`; ValueError where its shape or dtype is another (nothing is converted)."""
        a = np.asarray(a)
        if a.shape != (9, self.ny, self.nx) or a.dtype != np.dtype(dtype):
            raise ValueError(f"{what} must be [9][NY][NX] = {(9, self.ny, self.nx)} of {np.dtype(dtype).name}, "
                             f"got {a.shape} of {a.dtype.name}")
        return np.ascontiguousarray(a)

    def write_f(self, member: int, f) -> None:
        """Replace one member's populations with f [9][NY][NX] of the batch's dtype: the inverse of read_f (wt_polar.h "State upload
        and restart").  A native batch stores the bits given; a storage="half" batch stores (f - w).astype(float16).  Afterwards
        read_macro, forces and moment raise WTError (WT_ERR_STATE) until a step has run, and the member's surface and mean sums are
        empty; the history, the step count and the other members are untouched.  After init_equilibrium only.  ValueError for
        another shape or dtype."""
        a = self._planes(f, self.dtype, "f")
        _check(self._lib.wtp_write_f(self._b, int(member), a.ctypes.data_as(c_void_p)))

    def write_stored(self, member: int, h) -> None:
        """The twin of read_stored in a storage="half" batch: h [9][NY][NX] uint16, raw binary16 bit patterns, stored as given.
        read_f then write_f does not restore the stored bits (a stored -0 comes back as +0); read_stored then write_stored does.
        WTError (WT_ERR_STATE) on a native batch; otherwise as write_f."""
        a = self._planes(h, np.uint16, "h")
        _check(self._lib.wtp_write_stored(self._b, int(member), a.ctypes.data_as(c_void_p)))

    @property
    def step_count(self) -> int:
        """Steps since init_equilibrium: a step samples when this count, after it, is a multiple of sample_every."""
        n = np.zeros(1, np.int64)
        _check(self._lib.wtp_step_count(self._b, _ip(n)))
        return int(n[0])

    def set_step_count(self, n: int) -> None:
        """Set the step count, so that the sampling cadence and the history's step column continue after a restart.  n >= 0, and not
        below the step of the last history row held (WTError).  Nothing else changes."""
        _check(self._lib.wtp_set_step_count(self._b, int(n)))

    def state(self) -> Dict[str, object]:
        """What a restart needs: nx, ny, dtype (its name), storage, members, steps (the step count) and f [B][9][NY][NX], the
        populations of every member: read_f's values on a native batch, read_stored's raw uint16 halves on a storage="half" batch.
        With a far-field profile on and given to every member, also far_profile: {"left", "bottom", "top"}, the tables in use, read
        back from the device (read_far_profile), which holds what set_far_profile gave it or what the device-side vortex wrote.
        Not in it: the history, the running sums (surface, mean fields), the masks, the wall distances and the enable_* settings."""
        read = self.read_stored if self.storage == "half" else self.read_f
        state = {"nx": self.nx, "ny": self.ny, "dtype": self.dtype.name, "storage": self.storage, "members": self.members,
                 "steps": self.step_count, "f": np.stack([read(m) for m in range(self.members)])}
        if self._far_profile and self._far_given.all():
            state["far_profile"] = dict(zip(("left", "bottom", "top"), self.read_far_profile()))
        return state

    def restore(self, state) -> None:
        """Write every member's populations from a state() and set its step count.  ValueError where the state's nx, ny, dtype,
        storage or members are not the engine's.  Call init_equilibrium first: it is what gives the pad columns and the lattice
        that is not written defined contents, and it clears the history, so that the restored count cannot fall below a row held.
        Masks, wall distances and enable_* settings are the caller's to set as they were; the running sums start empty and the
        macroscopic planes are valid again after the first step.  A state that carries far_profile tables switches the far-field
        profile on and puts them back (before enable_far_vortex: while the device owns the tables, set_far_profile is refused)."""
        _check_state(state, self.nx, self.ny, self.dtype, self.storage, self.members)
        write = self.write_stored if self.storage == "half" else self.write_f
        for m in range(self.members):
            write(m, state["f"][m])
        self.set_step_count(state["steps"])
        tables = state.get("far_profile")
        if tables is not None:                   # a state taken with a far-field profile on: the model on again, with the state's tables
            self.enable_far_profile()
            self.set_far_profile(tables["left"], tables["bottom"], tables["top"])

    def read_macro(self, member: int):
        rho, ux, uy = (np.empty((self.ny, self.nx), dtype=self.dtype) for _ in range(3))
        _check(self._lib.wtp_read_macro(self._b, int(member), rho.ctypes.data_as(c_void_p), ux.ctypes.data_as(c_void_p),
                                        uy.ctypes.data_as(c_void_p)))
        return rho, ux, uy

    def sync(self) -> None:
        _check(self._lib.wtp_sync(self._b))


# ---- statistics ------------------------------------------------------------------------------
@dataclass
class PolarPoint:
    """One angle of a sweep: time statistics of the sampled forces (WindTunnel.compute_forces' raw values)."""
    alpha: float
    cl_mean: float
    cl_std: float
    cd_mean: float
    cd_std: float
    sep_frac: float              # mean rev / surf
    separation: str              # stall_label(sep_frac)
    samples: int                 # samples with a body surface (surf > 0)
    finite: bool                 # every sample finite
    clamp_events: Tuple[int, int]
    # step, fx, fy, surf, rev of this angle; fx, fy (and fx_mex, fy_mex) are wind-axis forces in a run_polar(frame="wind") sweep
    history: Dict[str, np.ndarray] = field(repr=False, default_factory=dict)
    cm_mean: Optional[float] = None      # pitching-moment coefficient about the quarter chord, nose-up positive (None: not sampled)
    cm_std: Optional[float] = None
    surface: Optional[Dict[str, np.ndarray]] = field(repr=False, default=None)   # x_over_c, cp_upper, cp_lower per body column
    # Momentum-exchange ("total": pressure + friction) statistics, None when not sampled.  Init-only: they are accepted by the
    # constructor after the fields above and kept as attributes, while dataclasses.fields(), repr and == stay those of the
    # pressure read-out, which callers enumerate.
    cl_total_mean: InitVar[Optional[float]] = None
    cl_total_std: InitVar[Optional[float]] = None
    cd_total_mean: InitVar[Optional[float]] = None
    cd_total_std: InitVar[Optional[float]] = None
    cm_total_mean: InitVar[Optional[float]] = None
    cm_total_std: InitVar[Optional[float]] = None
    cd_friction_mean: InitVar[Optional[float]] = None      # cd_total_mean - cd_mean
    mean: InitVar[Optional[Dict[str, object]]] = None      # mean_flow() of this angle (None: not sampled); init-only like the totals
    # The last strengths of the far-field vortex and source of a run_polar(far_field="vortex" / "vortex+source") sweep (None: uniform far field).
    # Plain attributes that run_polar sets: no fields and no constructor arguments, so that the constructor ends with `mean` as it did.
    vortex_strength = None
    vortex_source = None
    # The boundary-layer read-out of a run_polar(boundary_layer=True) sweep, boundary_layer() of this angle (None: not sampled).  A plain attribute too.
    boundary_layer = None

    def __post_init__(self, cl_total_mean, cl_total_std, cd_total_mean, cd_total_std, cm_total_mean, cm_total_std, cd_friction_mean,
                      mean):
        self.cl_total_mean, self.cl_total_std = cl_total_mean, cl_total_std
        self.cd_total_mean, self.cd_total_std = cd_total_mean, cd_total_std
        self.cm_total_mean, self.cm_total_std = cm_total_mean, cm_total_std
        self.cd_friction_mean = cd_friction_mean
        self.mean = mean

    @property
    def converged(self) -> bool:
        return self.finite and self.samples > 0 and self.clamp_events == (0, 0)


@dataclass
class PolarResult:
    points: List[PolarPoint]
    nx: int
    ny: int
    tau: float
    u0: float
    warmup_steps: int
    sample_every: int
    les: Optional[float] = None          # the Smagorinsky constant of every member (None: plain BGK)
    # The wall rule of the sweep, "staircase" (half-way bounce-back on the raster mask) or "interpolated".  Init-only, as
    # PolarPoint's totals are: accepted by the constructor after the fields above and kept as an attribute.
    walls: InitVar[str] = "staircase"
    # How the angles were set: "body" (a rotated body per angle) or "wind" (one body at 0 degrees, the free stream turned).  Init-only too.
    frame: InitVar[str] = "body"
    # How the batch stored its populations: "native" (in its dtype) or "half" (binary16 deviations from the weights).  Init-only too.
    storage: InitVar[str] = "native"
    # PolarEngine.state() after the last sample of a run_polar(keep_state=True), to continue from (run_polar(start=)); else None.  Init-only too.
    state: InitVar[Optional[Dict[str, object]]] = None
    # The collision of the sweep, "bgk" or "trt", and the magic number of a "trt" sweep (None for "bgk").  Init-only too.
    collision: InitVar[str] = "bgk"
    magic: InitVar[Optional[float]] = None
    # The far field of the sweep, "uniform", "vortex" or "vortex+source", and for the latter two one entry per update of the strengths: step [U], fx, fy
    # (lattice axes), strength, source [U][B] float64 and clipped [U][B] bool (None for "uniform").  Init-only too.
    far_field: InitVar[str] = "uniform"
    vortex_history: InitVar[Optional[Dict[str, np.ndarray]]] = None
    # The blowing or suction slot of the sweep: {"surface", "x0", "x1", "vn", "links"}, links [B] the links that carry a velocity per angle
    # (None without a slot).  Init-only too.
    slot: InitVar[Optional[Dict[str, object]]] = None

    def __post_init__(self, walls, frame, storage, state, collision, magic, far_field="uniform", vortex_history=None, slot=None):
        self.slot = slot
        self.far_field = far_field
        self.vortex_history = vortex_history
        self.walls = walls
        self.frame = frame
        self.storage = storage
        self.state = state
        self.collision = collision
        self.magic = magic


def raw_coefficients(fx, fy, surf, rev, u0: float, nx: int):
    """WindTunnel.compute_forces' raw values per sample: CL = fy/q, CD = fx/q, separation rev/surf, q = U0^2/2 * chord_cells(nx);
    samples without a body surface (surf == 0) are dropped, as compute_forces returns None for them."""
    fx, fy = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    surf, rev = np.asarray(surf, np.int64), np.asarray(rev, np.int64)
    keep = surf != 0
    q = 0.5 * u0 * u0 * chord_cells(nx)
    return fy[keep] / q, fx[keep] / q, rev[keep] / surf[keep]


def moment_coefficient(mz, u0: float, nx: int):
    """Cm = -Mz / (U0^2/2 * chord_cells(nx)^2): Mz is counter-clockwise positive and the nose points in -x, so nose-up is clockwise."""
    c = chord_cells(nx)
    return -np.asarray(mz, np.float64) / (0.5 * u0 * u0 * (c * c))


def wind_axes(fx, fy, alpha):
    """Lattice-axis forces of a member whose free stream is inclined by `alpha` degrees, in wind axes: float64
    (drag-axis, lift-axis) = (fx cos a + fy sin a, -fx sin a + fy cos a), elementwise."""
    fx, fy = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    a = np.radians(np.asarray(alpha, np.float64))
    c, s = np.cos(a), np.sin(a)
    return fx * c + fy * s, -fx * s + fy * c


def quarter_chord(nx: int, ny: int) -> Tuple[float, float]:
    """The quarter-chord point (0.25, 0) in lattice units: the pivot of geometry.rotate, so the same point at every angle."""
    return (0.25 - geo.DX0) / (geo.DX1 - geo.DX0) * nx, ny / 2


def surface_cp(surface: Dict[str, np.ndarray], alpha: float, u0: float) -> Dict[str, np.ndarray]:
    """Cp(x/c) of one member from PolarEngine.surface: Cp = (mean rho - 1) / (1.5 U0^2), k_ranges' formula, NaN where a column
    has no sample on that side.  Columns that hold a body only.  x/c is the point of the chord line that the rotation about
    (0.25, 0) by `alpha` puts at the column centre's world x: 0.25 + (x - 0.25) / cos(alpha)."""
    nu, nl = surface["n_upper"], surface["n_lower"]
    nx = nu.size
    body = (surface["j_upper"] >= 0) | (surface["j_lower"] >= 0)
    xw = geo.DX0 + (np.arange(nx) + 0.5) / nx * (geo.DX1 - geo.DX0)
    with np.errstate(invalid="ignore", divide="ignore"):
        cpu = (surface["rho_upper"] / nu - 1.0) / (1.5 * u0 * u0)
        cpl = (surface["rho_lower"] / nl - 1.0) / (1.5 * u0 * u0)
    return {"x_over_c": (0.25 + (xw - 0.25) / math.cos(math.radians(alpha)))[body], "cp_upper": cpu[body], "cp_lower": cpl[body]}


def mean_flow(sums: Dict[str, np.ndarray], u0: float) -> Dict[str, object]:
    """The time-mean flow field and the fluctuation about it from PolarEngine.mean_sums (n samples, sums S over them), [NY][NX]
    float64 each, solid cells included as the device holds them:
    rho, ux, uy: the means S/n.  uu, vv, uv: the central second moments S2/n - mean * mean of (ux, ux), (uy, uy), (ux, uy), the
    Reynolds stresses per unit density; uu and vv are floored at 0 (the difference of two roundings can fall below it where the
    flow is steady).  rho_var: that of rho, floored likewise.  cp_mean = (mean rho - 1) / (1.5 U0^2), k_ranges' formula, as
    surface_cp; cp_rms = sqrt(rho_var) / (1.5 U0^2).  speed = |(mean ux, mean uy)|; tke = (uu + vv) / 2.  `n` is the count.
    Everything is NaN when n = 0."""
    n = int(sums["n"])
    if n == 0:
        nan = np.full(np.shape(sums["rho"]), np.nan)
        return {"n": 0, **{k: nan.copy() for k in ("rho", "ux", "uy", "uu", "vv", "uv", "rho_var", "cp_mean", "cp_rms", "speed", "tke")}}
    rho, ux, uy = (np.asarray(sums[k], np.float64) / n for k in ("rho", "ux", "uy"))
    uu = np.maximum(np.asarray(sums["ux2"], np.float64) / n - ux * ux, 0.0)
    vv = np.maximum(np.asarray(sums["uy2"], np.float64) / n - uy * uy, 0.0)
    uv = np.asarray(sums["uxuy"], np.float64) / n - ux * uy
    rho_var = np.maximum(np.asarray(sums["rho2"], np.float64) / n - rho * rho, 0.0)
    q = 1.5 * u0 * u0
    return {"n": n, "rho": rho, "ux": ux, "uy": uy, "uu": uu, "vv": vv, "uv": uv, "rho_var": rho_var, "cp_mean": (rho - 1.0) / q,
            "cp_rms": np.sqrt(rho_var) / q, "speed": np.hypot(ux, uy), "tke": 0.5 * (uu + vv)}


def polar_point(alpha: float, step, fx, fy, surf, rev, u0: float, nx: int, clamp_events=(0, 0), *, mz=None, surface=None,
                fx_mex=None, fy_mex=None, mz_mex=None, links=None) -> PolarPoint:
    """Statistics of one angle's force history; with `mz` (the sampled moments) also Cm over the samples that have a body surface.
    With `fx_mex`, `fy_mex`, `mz_mex` (the sampled momentum exchange; all three or none) also the total coefficients over the same
    samples, with the same normalisation: CL = fy/q, CD = fx/q, Cm = -mz/(q chord_cells(nx)); `links` only joins the history."""
    cl, cd, sep = raw_coefficients(fx, fy, surf, rev, u0, nx)
    finite = bool(np.all(np.isfinite(np.asarray(fx, np.float64))) and np.all(np.isfinite(np.asarray(fy, np.float64))))
    n = int(cl.size)

    def stats(v, scale=float):
        """(mean, std) of the samples v through `scale`; (nan, nan) when no sample has a body surface."""
        return (float(scale(v.mean())), float(abs(scale(v.std())))) if n else (float("nan"), float("nan"))

    def cm(mz_value):
        return moment_coefficient(mz_value, u0, nx)

    hist = {"step": np.asarray(step, np.int64), "fx": np.asarray(fx, np.float64), "fy": np.asarray(fy, np.float64),
            "surf": np.asarray(surf, np.int64), "rev": np.asarray(rev, np.int64)}
    sep_mean = float(sep.mean()) if n else 0.0
    cm_mean = cm_std = None
    if mz is not None:
        hist["mz"] = np.asarray(mz, np.float64)
        kept = hist["mz"][hist["surf"] != 0]
        cm_mean, cm_std = stats(kept, cm)
    (cl_mean, cl_std), (cd_mean, cd_std) = stats(cl), stats(cd)
    total = {}
    given = [v is not None for v in (fx_mex, fy_mex, mz_mex)]
    if any(given):
        if not all(given):
            raise ValueError("fx_mex, fy_mex and mz_mex come together")
        hist.update({"fx_mex": np.asarray(fx_mex, np.float64), "fy_mex": np.asarray(fy_mex, np.float64),
                     "mz_mex": np.asarray(mz_mex, np.float64)})
        if links is not None:
            hist["links"] = np.asarray(links, np.int64)
        keep = hist["surf"] != 0
        q = 0.5 * u0 * u0 * chord_cells(nx)
        finite = finite and bool(np.all(np.isfinite(hist["fx_mex"])) and np.all(np.isfinite(hist["fy_mex"])))
        for name, v in (("cl_total", hist["fy_mex"][keep] / q), ("cd_total", hist["fx_mex"][keep] / q)):
            total[name + "_mean"], total[name + "_std"] = stats(v)
        total["cm_total_mean"], total["cm_total_std"] = stats(hist["mz_mex"][keep], cm)      # (as cm_mean: the coefficient of the mean moment)
        total["cd_friction_mean"] = total["cd_total_mean"] - cd_mean
    return PolarPoint(alpha=float(alpha), cl_mean=cl_mean, cl_std=cl_std, cd_mean=cd_mean, cd_std=cd_std, sep_frac=sep_mean,
                      separation=stall_label(sep_mean), samples=n, finite=finite,
                      clamp_events=(int(clamp_events[0]), int(clamp_events[1])), history=hist, cm_mean=cm_mean, cm_std=cm_std,
                      surface=surface, **total)


# ---- probe points and the boundary layer -------------------------------------------------------
def probe_weights(x, y, nx: int, ny: int):
    """The weight rule of the probe points (wt_polar.h "Probe points") in NumPy, elementwise over x, y (lattice units, the centre of
    cell (i, j) at (i + 0.5, j + 0.5)): (i0, j0, w) with the base cell of each point, int64, and w [4][...] float64, the weights
    w00, w10, w01, w11 of the cells (i0, j0), (i0+1, j0), (i0, j0+1), (i0+1, j0+1).  In float64, one rounding per operation:
        gx = x - 0.5;  i0 = min(max(floor(gx), 0), NX - 2);  tx = gx - i0;  sx = 1.0 - tx        (and gy, j0, ty, sy from y)
        w00 = sx*sy;  w10 = tx*sy;  w01 = sx*ty;  w11 = tx*ty
    A point whose x is NaN is inactive: i0 = j0 = -1 and its weights are 0.  Any other point outside [0.5, NX - 0.5] x
    [0.5, NY - 0.5] (a NaN y included) raises ValueError, as wtp_set_probes refuses it."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.shape != y.shape:
        raise ValueError(f"x and y must have one shape, got {x.shape} and {y.shape}")
    off = np.isnan(x)
    with np.errstate(invalid="ignore"):
        ok = (x >= 0.5) & (x <= nx - 0.5) & (y >= 0.5) & (y <= ny - 0.5)
    if not (ok | off).all():
        k = np.argwhere(~(ok | off))[0]
        raise ValueError(f"point {tuple(int(v) for v in k)}, ({x[tuple(k)]!r}, {y[tuple(k)]!r}), lies outside [0.5, {nx - 0.5}] x [0.5, {ny - 0.5}] "
                         f"and is not inactive (x = NaN)")
    gx, gy = np.where(off, 0.0, x) - 0.5, np.where(off, 0.0, y) - 0.5
    i0 = np.minimum(np.maximum(np.floor(gx), 0.0), nx - 2.0)
    j0 = np.minimum(np.maximum(np.floor(gy), 0.0), ny - 2.0)
    tx, ty = gx - i0, gy - j0
    sx, sy = 1.0 - tx, 1.0 - ty
    w = np.where(off, 0.0, np.stack([sx * sy, tx * sy, sx * ty, tx * ty]))
    return np.where(off, -1, i0.astype(np.int64)), np.where(off, -1, j0.astype(np.int64)), w


def boundary_layer_points(stations: Dict[str, object], height: float, spacing: float):
    """The rake points of geometry.surface_stations: (x, y, heights) with x, y [S * H] float64, station-major and height-minor, the
    points station + h * n along the outward normal n for h = heights = spacing, 2 spacing, ... <= height (lattice units; H of them).
    The macroscopic planes are column-major, y fastest, so that with this order the gathers of neighbouring points fall into a few
    columns.  A point outside the valid rectangle [0.5, NX - 0.5] x [0.5, NY - 0.5] of the stations' lattice becomes NaN in x and y:
    inactive as a probe point, and its station's boundary layer is NaN.  height >= spacing > 0, else ValueError."""
    height, spacing = float(height), float(spacing)
    if not (spacing > 0.0 and height >= spacing and math.isfinite(height)):
        raise ValueError(f"a rake needs height >= spacing > 0, got height {height!r}, spacing {spacing!r}")
    heights = spacing * np.arange(1, int(math.floor(height / spacing + 1e-9)) + 1)
    nx, ny = stations["lattice"]
    x = np.asarray(stations["x"])[:, None] + heights[None, :] * np.asarray(stations["nrm_x"])[:, None]
    y = np.asarray(stations["y"])[:, None] + heights[None, :] * np.asarray(stations["nrm_y"])[:, None]
    with np.errstate(invalid="ignore"):
        ok = (x >= 0.5) & (x <= nx - 0.5) & (y >= 0.5) & (y <= ny - 0.5)
    return np.where(ok, x, np.nan).ravel(), np.where(ok, y, np.nan).ravel(), heights


def _sign_changes(xc, cf):
    """(x_sep, x_reattach) of one side's Cf along x/c, both ordered from the leading edge: the first place where Cf turns from >= 0 to
    < 0 and the next place where it turns back to >= 0, each linearly interpolated between the two stations; NaN where there is
    none.  Stations whose Cf is NaN are skipped."""
    keep = np.isfinite(cf) & np.isfinite(xc)
    xc, cf = xc[keep], cf[keep]

    def crossing(k):
        return float(xc[k - 1] + (xc[k] - xc[k - 1]) * (cf[k - 1] / (cf[k - 1] - cf[k])))

    sep = next((k for k in range(1, cf.size) if cf[k - 1] >= 0.0 and cf[k] < 0.0), None)
    if sep is None:
        return float("nan"), float("nan")
    back = next((k for k in range(sep + 1, cf.size) if cf[k] >= 0.0), None)
    return crossing(sep), (crossing(back) if back is not None else float("nan"))


def boundary_layer(stations: Dict[str, object], means: Dict[str, np.ndarray], heights, u0: float, tau: float) -> Dict[str, object]:
    """The boundary-layer read-out of one member from the time-mean velocity at its rake points: the columns of the reference's XFOIL
    dump (x, Ue, delta*, theta, Cf, H per surface) as this lattice gives them.  `stations`: geometry.surface_stations; `means`: "ux",
    "uy", the mean velocity at boundary_layer_points' points ([S * H] or [S][H]; PolarEngine.probe_sums over n); `heights`: that
    function's, in cells.  Definitions, per station, with u_t(h) = mean u . t the speed along the station's tangent at height h:
      Ue      = the u_t of largest magnitude over the rake's heights of one cell and more: the maximum of u_t wherever the outer flow
                runs from the leading edge to the trailing edge, and negative on the stretch between the leading edge and the stagnation
                point, where the layer runs towards the leading edge and the rake is read in its own direction.  The edge height h_e is
                the lowest of those heights with u_t/Ue >= 0.99.
      delta*  = integral from 0 to h_e of (1 - u_t/Ue) dh;  theta = integral from 0 to h_e of (u_t/Ue)(1 - u_t/Ue) dh;  H = delta*/theta.
                Both by the trapezoid rule over the wall, where u_t(0) = 0, and the rake heights from one cell to h_e.  The samples
                closer to the wall than one cell are left out: their stencils touch solid cells, whose stored velocity is 0 at the
                cell centre and not at the wall.  NaN where Ue = 0 or theta = 0 (a layer thinner than one cell: every ratio 0 or 1).
      Cf      = 2 nu (u_t(h_1)/h_1) / U0^2, with nu = (tau - 1/2)/3 and h_1 the first rake height >= 1 cell: a one-sided difference
                from the wall.  nu is the molecular viscosity: with a Smagorinsky model on (run_polar's `les`) the eddy viscosity is
                not in it.
    A station whose rake holds an inactive point (NaN) is NaN throughout.  What this is not: there is no transition detection, the
    wall is a staircase half a cell from the first fluid centre whatever the wall rule, and at a chord Reynolds number of a few
    hundred the layer is a tenth of a chord thick.
    Returns {"upper": side, "lower": side, "heights": heights}; a side holds, ordered from the leading edge by x/c: station (the
    indices into `stations`), x_over_c, ue (Ue/U0), dstar and theta (in chords), cf, H, and the scalars x_sep, the x/c at which Cf
    first turns negative going from the leading edge, linearly interpolated between the two stations, NaN if it never does, and
    x_reattach, the next change of sign behind it, NaN if none.  Cf that is negative from the first station on (the stretch between
    the leading edge and the stagnation point) is no separation."""
    heights = np.asarray(heights, np.float64)
    S, Hn = np.asarray(stations["x"]).size, heights.size
    ux, uy = (np.asarray(means[k], np.float64).reshape(S, Hn) for k in ("ux", "uy"))
    ut = ux * np.asarray(stations["tan_x"])[:, None] + uy * np.asarray(stations["tan_y"])[:, None]
    kept = np.nonzero(heights >= 1.0)[0]
    if kept.size == 0:
        raise ValueError("the rake holds no height of one cell or more")
    k1 = int(kept[0])
    nu = (float(tau) - 0.5) / 3.0
    chord = float(stations["chord_cells"])
    ue, dstar, theta = (np.full(S, np.nan) for _ in range(3))
    cf = 2.0 * nu * (ut[:, k1] / heights[k1]) / (u0 * u0)                   # (NaN where the rake's sample is)
    for s in range(S):
        u = ut[s]
        if not np.isfinite(u).all():
            cf[s] = np.nan
            continue
        top = float(u[kept][np.argmax(np.abs(u[kept]))])
        ue[s] = top / u0
        if top == 0.0:
            continue
        edge = next(k for k in kept if u[k] / top >= BL_EDGE)
        h = np.concatenate([[0.0], heights[k1:edge + 1]])
        r = np.concatenate([[0.0], u[k1:edge + 1]]) / top
        f1, f2 = 1.0 - r, r * (1.0 - r)
        dh = np.diff(h)
        dstar[s] = float(np.sum(0.5 * (f1[1:] + f1[:-1]) * dh)) / chord
        theta[s] = float(np.sum(0.5 * (f2[1:] + f2[:-1]) * dh)) / chord
    with np.errstate(invalid="ignore", divide="ignore"):
        shape = np.where(theta != 0.0, dstar / theta, np.nan)
    out: Dict[str, object] = {"heights": heights}
    upper, xc = np.asarray(stations["upper"], bool), np.asarray(stations["x_over_c"], np.float64)
    for name, side in (("upper", upper), ("lower", ~upper)):
        idx = np.nonzero(side)[0]
        idx = idx[np.argsort(xc[idx], kind="stable")]
        x_sep, x_re = _sign_changes(xc[idx], cf[idx])
        out[name] = {"station": idx, "x_over_c": xc[idx], "ue": ue[idx], "dstar": dstar[idx], "theta": theta[idx], "cf": cf[idx], "H": shape[idx],
                     "x_sep": x_sep, "x_reattach": x_re}
    return out


_boundary_layer_of = boundary_layer              # (run_polar has an argument of the function's name)


# ---- the far-field correction ------------------------------------------------------------------
def far_profile(nx: int, ny: int, u0: float, v0: float, strength: float, source: float, xc: float, yc: float, dtype="float32"):
    """The tables (left [3][NY], bottom [3][NX], top [3][NX]; planes rho, ux, uy) of PolarEngine.set_far_profile for the free stream
    (u0, v0) plus a point vortex and a point source at (xc, yc), lattice units.  All arithmetic in float64, each value rounded to
    `dtype` once.  For a cell centre (i + 0.5, j + 0.5):
        dx = i + 0.5 - xc, dy = j + 0.5 - yc, r2 = dx*dx + dy*dy
        ux = u0 + strength*dy/r2 + source*dx/r2
        uy = v0 - strength*dx/r2 + source*dy/r2
        rho = 1 + 1.5*((u0*u0 + v0*v0) - (ux*ux + uy*uy))          (Bernoulli with p = rho/3)
    `strength` is the clockwise circulation over 2 pi, positive for positive lift with the flow in +x; `source` is the volume flux
    over 2 pi.  With both zero every entry is (1, u0, v0) exactly."""
    u0, v0, strength, source, xc, yc = (float(v) for v in (u0, v0, strength, source, xc, yc))

    def table(i, j):
        dx, dy = i + 0.5 - xc, j + 0.5 - yc
        r2 = dx * dx + dy * dy
        ux = u0 + strength * dy / r2 + source * dx / r2
        uy = v0 - strength * dx / r2 + source * dy / r2
        rho = 1 + 1.5 * ((u0 * u0 + v0 * v0) - (ux * ux + uy * uy))
        return np.stack([rho, ux, uy]).astype(_np_dtype(dtype))

    i, j = np.arange(int(nx), dtype=np.float64), np.arange(int(ny), dtype=np.float64)
    return table(np.zeros_like(j), j), table(i, np.zeros_like(i)), table(i, np.full_like(i, ny - 1))


def vortex_bound(nx: int, ny: int, xc: float, yc: float) -> float:
    """The distance from (xc, yc) to the nearest far-field cell centre: min(xc - 0.5, yc - 0.5, NY - 0.5 - yc)."""
    return min(xc - 0.5, yc - 0.5, ny - 0.5 - yc)


def vortex_update(strength, source, fx, fy, alpha, u0: float, relax: float, bound: float, with_source: bool = True, norm: str = "hypot"):
    """The update rule of the far-field vortex and source, elementwise over the members; pure.  D, L = wind_axes(fx, fy, alpha), the
    drag and the lift in lattice units.  The targets are L/(2 pi u0) for the strength (Kutta-Joukowski with rho = 1) and D/(2 pi u0)
    for the source (0 when with_source is false); new = old + relax*(target - old).  Then both are scaled by one factor, where
    needed, so that the speed they induce together at the nearest far-field cell centre, hypot(strength, source)/bound, stays at
    most VORTEX_SPEED_MAX = 0.1: this keeps every profile inside set_far_profile's limits for u0 <= 0.25.
    `norm`: "hypot", the default, forms that speed with np.hypot; "sqrt" with sqrt(s*s + q*q), one rounding per operation, which is the
    rule of the device-side update (wt_polar.h "Device-side far-field vortex") as a NumPy function.  The two give the same bits whenever
    both find the update unclipped, because the scale is then exactly 1.
    Returns (strength, source, clipped): float64, float64, bool."""
    if norm not in VORTEX_NORMS:
        raise ValueError(f"norm must be one of {VORTEX_NORMS}, got {norm!r}")
    old_s, old_q = np.asarray(strength, np.float64), np.asarray(source, np.float64)
    drag, lift = wind_axes(fx, fy, alpha)
    tgt_s = lift / (2 * math.pi * u0)
    tgt_q = drag / (2 * math.pi * u0) if with_source else np.zeros_like(tgt_s)
    new_s = old_s + relax * (tgt_s - old_s)
    new_q = old_q + relax * (tgt_q - old_q)
    speed = (np.hypot(new_s, new_q) if norm == "hypot" else np.sqrt(new_s * new_s + new_q * new_q)) / bound
    clipped = speed > VORTEX_SPEED_MAX
    scale = np.where(clipped, VORTEX_SPEED_MAX / np.where(clipped, speed, 1.0), 1.0)
    return new_s * scale, new_q * scale, clipped


# ---- the sweep -------------------------------------------------------------------------------
def run_polar(alphas: Sequence[float], *, coords=None, shape: str = "naca2412", nx: int = 320, ny: int = 160, dtype="float32",
              u0: float = U0_DEFAULT, tau: Optional[float] = None, re: Optional[float] = None, warmup_steps: Optional[int] = None,
              samples: int = 256, sample_every: int = 12, device: int = 0, loads: bool = True,
              total_forces: bool = False, mean_fields: bool = False,
              boundary_layer: bool = False, bl_height: float = BL_HEIGHT_DEFAULT, bl_spacing: float = BL_SPACING_DEFAULT, start: Optional[Dict[str, object]] = None, keep_state: bool = False,
              collision: str = "bgk", magic: float = MAGIC_DEFAULT,
              far_field: str = "uniform", vortex_every: int = 96, vortex_relax: float = 0.3, vortex_after: Optional[int] = None,
              vortex_on: str = "host", slot: Optional[Dict[str, object]] = None, storage: str = "native", walls: str = "staircase", frame: str = "body", les: Optional[float] = None) -> PolarResult:
    """One batch member per angle: warm-up of `warmup_steps` (default two flow-throughs, 2*nx/u0 steps), then `samples` force
    samples every `sample_every` steps (12: the page's cadence, 4 steps per frame and forces every 3rd frame).  User `coords`
    win over `shape`, as in WindTunnel; tau from `re` when given (tau_from_reynolds), else `tau` or the page's 0.58.
    `loads`: also sample the pitching moment about the quarter chord and the surface pressure (PolarPoint.cm_mean / cm_std /
    surface); the forces and the flow are the same bits either way.
    `total_forces`: also sample the momentum exchange, the force of pressure and friction together and its moment about the
    quarter chord (PolarPoint.cl_total_mean ... cd_friction_mean; polar_rows(result, forces="total")).  Off by default: the
    sweep then runs, and costs, what it did without it; every other value is the same bits either way.
    `mean_fields`: also keep the running sums of rho, ux, uy and their products over the samples on the device and attach
    mean_flow() of each angle as PolarPoint.mean: the time-mean field, the Reynolds stresses, the pressure r.m.s.  The warm-up
    takes no sample, so nothing of it enters the mean.  Off by default, with the same guarantees as `total_forces`.
    `les`: the Smagorinsky constant (0.1 to 0.17 are the usual values; at most 0.5) of a subgrid eddy viscosity in every member's
    collision, from the first warm-up step on (PolarEngine.enable_les).  For sweeps at airfoil Reynolds numbers (`re` of 20 000
    and above), where plain BGK runs into the stability net and the angle fails.  None, the default, is plain BGK.
    `storage`: "native", the default, keeps the populations in `dtype`, with the bits they always had.  "half" (float32 only, not
    with walls="interpolated") keeps each as the binary16 deviation from its lattice weight and computes in fp32
    (PolarEngine(storage="half"), wt_polar.h "Half-precision population storage"): a step moves half the bytes and the batch takes
    half the memory.  It is no free lunch: on NACA 2412 at 320x160, 4 to 6 degrees, the mean CL comes out 0.006 to 0.007 higher
    (1.2 to 1.5 %) and CD 0.0006 to 0.0008 higher (0.5 to 0.6 %), many times their standard deviation over the samples (README,
    profiles/polar_half_sweep.txt).
    `walls`: "staircase", the default, reflects half-way to the next cell of the raster mask, with the bits it always had;
    "interpolated" reflects by linear interpolated bounce-back at the panel polygon of each angle, through the wall distances
    geometry.wall_distances computes from the Geometry the mask came from, from the first warm-up step on
    (PolarEngine.enable_interpolated_walls).  The momentum exchange (`total_forces`) then uses the interpolated link term.
    `frame`: "body", the default, rasterises a body rotated by each angle, with the bits it always had.  "wind" keeps one body at
    0 degrees in every member (one mask, and with walls="interpolated" one set of wall distances) and inclines the member's free
    stream instead: member m runs at (u0 cos a, u0 sin a), from the start state on (PolarEngine.enable_wind); tau and `re` are
    formed from the magnitude u0.  The sampled forces are turned into wind axes (wind_axes) before the statistics, so CL is
    across the free stream and CD along it, and PolarPoint.history then holds wind-axis fx, fy, fx_mex, fy_mex; the moment, its
    reference point and the surface pressure (x/c of the unrotated body) are unchanged.  Every |angle| must be at most 30
    degrees: the trailing edge sits 0.42 chords from the outlet and the half height is 0.46 chords, so up to there the wake
    leaves through the outlet.  The top and bottom rows stay equilibrium rows, now with inflow and outflow, and no blockage
    correction is made: the level of CL and CD differs from the body frame's (README).
    `keep_state`: PolarResult.state carries PolarEngine.state() taken after the last sample: the populations of every angle and
    the step count.  None otherwise.
    `start`: such a state, to continue from.  The engine is set up and initialised as always (masks, wall rule, free stream and
    collision are formed from the arguments of this call), then restored from `start` (PolarEngine.restore), then stepped.  The
    warm-up is then what the caller says, and its default is 0: the sweep that gave the state has paid it.  The step count goes
    on from the state's, so with the same `sample_every` the samples fall on the steps on which one longer run would have taken
    them, with the same bits.  The first sample follows at least one step, so the macroscopic planes belong to the restored
    populations again.  The running sums (surface pressure, mean fields) start empty: they cover this call's samples only, and
    so do the statistics of the points.  Continuing with other angles, another body or other settings than the state was
    taken with is the caller's decision: nothing checks it, and the flow then needs its own time to adjust.  A `start` whose
    nx, ny, dtype, storage or number of angles is not this call's raises ValueError before an engine is created.
    `collision`: "bgk", the default, is the single-relaxation-time collision, with the code path and the bits it always had.  "trt"
    is the two-relaxation-time collision with the magic number `magic` (default 3/16; finite, in (0, 1]) in every member, from the
    first warm-up step on (PolarEngine.enable_trt): the effective position of a staircase wall then no longer moves with tau, that
    is with `re`.  It needs a tau above 0.5 in `dtype` and combines with `les`, `walls`, `frame`, `storage` and `start`.  What it
    does to CL and CD was measured, not assumed: README, profiles/polar_trt_sweep.txt.  PolarResult.collision and .magic say what ran
    (magic is None for "bgk").  An unknown collision, a magic outside (0, 1] or "trt" with such a tau raises ValueError before an
    engine is created.
    `far_field`: "uniform", the default, holds every far-field cell (inlet column, top and bottom rows) at the free stream, with the
    code path and the bits it always had.  Those rows lie 0.46 chords from the body and act like the walls of a closed tunnel.
    "vortex" prescribes there the free stream plus the velocity of a point vortex at the quarter chord whose circulation follows
    the current lift (Kutta-Joukowski), the textbook far-field correction of airfoil computations; "vortex+source" adds a source
    that follows the current drag (PolarEngine.enable_far_profile, far_profile, vortex_update).  The warm-up and the sampling then run
    in chunks of `vortex_every` steps, counted from this call's first step; chunking does not move the samples, which fall on the
    multiples of `sample_every` of the step count.  After each chunk whose end lies at or beyond step `vortex_after` (default one
    chord transit, ceil(chord_cells(nx)/u0)) the pressure force of the state the chunk's last step emitted (PolarEngine.forces)
    moves the strengths by `vortex_relax` of the way to their targets and the new tables are uploaded.  The angle in the update is
    the member's in the wind frame and 0 in the body frame.  relax 0.3 every 100 steps from step 1000 is what was tried on the CPU
    definition and stayed stable; other values are untested.  It works with both frames, every collision, both wall rules and
    `start` / `keep_state`: the state carries the tables and the strengths, and a continued sweep goes on from them; when the first
    run's length is a multiple of `vortex_every`, the two runs together are one run of the combined length, bit for bit.  The
    correction removes a part of the tunnel effect, not all of it, and a taller lattice (`ny`) removes more, at its cost in work
    (README, profiles/polar_profile_sweep.txt).  PolarResult.far_field says what ran, PolarResult.vortex_history holds every update
    and PolarPoint.vortex_strength / .vortex_source the last values.  storage="half" with a far field other than "uniform", an
    unknown far_field, vortex_every < 1 or a vortex_relax outside (0, 1] raises ValueError before an engine is created.
    `vortex_on`: who updates the vortex.  "host", the default, is the loop above, with the code path and the bits it always had: every
    update reads the forces back, which waits for the stream, forms the tables in NumPy and uploads them, which waits again.
    "device" hands the updates to the library (PolarEngine.enable_far_vortex, wt_polar.h "Device-side far-field vortex"): the force
    read-out, the relaxation, the clip and the tables are enqueued between two steps, so that the warm-up and the sampling are two
    `step` calls as with the uniform far field, and a small `vortex_every` costs a few small launches per update and no wait.  The
    updates fall on the same steps, a last one after a short last chunk included, and PolarResult.vortex_history, the points'
    strengths and `state` are built from the device's log.  Device and host mode are the same run, bit for bit, unless an update clips
    (vortex_history["clipped"]): the device forms the norm of (strength, source) as sqrt(s*s + q*q) where the host uses np.hypot
    (vortex_update's `norm`), so a clipped update may differ in the last bit of its scale.  It is not read with the uniform far field.
    An unknown vortex_on raises ValueError before an engine is created.
    `boundary_layer`: also sample the flow along rakes normal to the wall, one rake per panel of the body (geometry.surface_stations,
    boundary_layer_points: 160 stations, points every `bl_spacing` cells up to `bl_height` chords from the wall), as probe points on the
    device (PolarEngine.enable_probes, wt_polar.h "Probe points"), and attach boundary_layer() of the time means as
    PolarPoint.boundary_layer: x/c, Ue, delta*, theta, Cf and H per surface, the columns of the reference's XFOIL boundary-layer dump, and
    x_sep / x_reattach, where the skin friction changes sign.  With frame="body" the rakes stand on each angle's rotated body, with
    frame="wind" one set serves every angle.  The probes are on before the warm-up, which takes no sample, and a continued sweep
    (`start`) starts with empty sums, like the other running sums.  Cf uses the molecular viscosity (tau - 1/2)/3, also with `les`.
    polar_rows then carries x_sep_upper and x_sep_lower.  Off by default: the sweep then launches the kernels, and returns the rows,
    results and bits, it always did; with it on every other value is the same bits.  bl_height and bl_spacing must be finite and
    positive, with the rake reaching at least one cell (bl_height * chord_cells(nx) >= max(bl_spacing, 1)) and at most WTP_MAX_PROBES
    points per angle, else ValueError before an engine is created.
    `slot`: blowing or suction through a slot of the surface, a dict with the keys "surface" ("upper" or "lower"), "x0" and "x1" (the
    slot's extent in x/c of the body's own axes, x0 <= x1) and "vn" (the normal velocity in units of `u0`; positive blows into the
    fluid).  Every wall link whose wall point lies nearest to a panel of the slot carries Ladd's moving-wall term with u_w = vn u0 times
    the panel's outward normal (geometry.slot_wall_velocity, PolarEngine.enable_wall_velocity, wt_polar.h "Wall velocity"), from the
    first warm-up step on.  It needs walls="interpolated" and is refused with storage="half"; it works in both frames: with
    frame="body" each angle's own panels are used, with frame="wind" one set serves every angle.  PolarResult.slot records what ran,
    and how many links of each angle carry a velocity.  The momentum exchange (`total_forces`) uses the moving-wall link term, without
    a Galilean-invariant correction.  None, the default, launches the kernels, and returns the bits, that the sweep always did.  A slot
    with other keys, an unknown surface, x0 > x1, a vn that is not finite or |vn| u0 sqrt(2) > 0.5 raises ValueError before an engine
    is created."""
    alphas = [float(a) for a in alphas]
    if not alphas:
        raise ValueError("no angles")
    if tau is not None and re is not None:
        raise ValueError("give tau or re, not both")
    if samples < 1 or sample_every < 1:
        raise ValueError("samples and sample_every must be >= 1")
    if les is not None:
        les = float(les)
        if not math.isfinite(les) or les < 0.0 or les > 0.5:
            raise ValueError(f"les must be a finite Smagorinsky constant in [0, 0.5], got {les!r}")
    if walls not in WALLS:
        raise ValueError(f"walls must be one of {WALLS}, got {walls!r}")
    if frame not in FRAMES:
        raise ValueError(f"frame must be one of {FRAMES}, got {frame!r}")
    _check_storage(storage, dtype, walls)
    if slot is not None:
        if storage == "half":
            raise ValueError('storage="half" does not combine with a slot')
        if walls != "interpolated":
            raise ValueError('a slot needs walls="interpolated"')
        if not isinstance(slot, dict) or set(slot) != {"surface", "x0", "x1", "vn"}:
            raise ValueError(f'slot must be a dict with the keys "surface", "x0", "x1" and "vn", got {slot!r}')
        if slot["surface"] not in ("upper", "lower"):
            raise ValueError(f'slot["surface"] must be "upper" or "lower", got {slot["surface"]!r}')
        slot = {"surface": slot["surface"], "x0": float(slot["x0"]), "x1": float(slot["x1"]), "vn": float(slot["vn"])}
        if not (math.isfinite(slot["x0"]) and math.isfinite(slot["x1"]) and slot["x0"] <= slot["x1"]):
            raise ValueError(f'slot needs finite x0 <= x1, got {slot["x0"]!r} and {slot["x1"]!r}')
        if not (math.isfinite(slot["vn"]) and abs(slot["vn"]) * abs(float(u0)) * math.sqrt(2.0) <= 0.5):
            raise ValueError(f'slot["vn"] must be finite with |vn| u0 sqrt(2) <= 0.5, got {slot["vn"]!r}')
    if not isinstance(collision, str) or collision not in COLLISIONS:
        raise ValueError(f"collision must be one of {COLLISIONS}, got {collision!r}")
    trt = collision == "trt"
    if trt:
        magic = float(magic)
        if not math.isfinite(magic) or not 0.0 < magic <= 1.0:
            raise ValueError(f"magic must be a finite magic number in (0, 1], got {magic!r}")
    if not isinstance(far_field, str) or far_field not in FAR_FIELDS:
        raise ValueError(f"far_field must be one of {FAR_FIELDS}, got {far_field!r}")
    if not isinstance(vortex_on, str) or vortex_on not in VORTEX_ON:
        raise ValueError(f"vortex_on must be one of {VORTEX_ON}, got {vortex_on!r}")
    vortex = far_field != "uniform"
    if vortex:
        if storage == "half":
            raise ValueError(f'storage="half" does not combine with far_field={far_field!r}')
        if int(vortex_every) != vortex_every or vortex_every < 1:
            raise ValueError(f"vortex_every must be a number of steps >= 1, got {vortex_every!r}")
        vortex_relax = float(vortex_relax)
        if not 0.0 < vortex_relax <= 1.0:                      # (false for a NaN)
            raise ValueError(f"vortex_relax must be in (0, 1], got {vortex_relax!r}")
    if boundary_layer:
        bl_height, bl_spacing = float(bl_height), float(bl_spacing)
        if not (math.isfinite(bl_height) and math.isfinite(bl_spacing) and bl_height > 0.0 and bl_spacing > 0.0):
            raise ValueError(f"bl_height and bl_spacing must be finite and positive, got {bl_height!r} and {bl_spacing!r}")
        rake_cells = bl_height * chord_cells(int(nx))
        if rake_cells < max(bl_spacing, 1.0):
            raise ValueError(f"the boundary-layer rake must reach at least one cell and one spacing: bl_height {bl_height!r} is {rake_cells:.3g} cells")
        if geo.NP * math.floor(rake_cells / bl_spacing + 1e-9) > WTP_MAX_PROBES:
            raise ValueError(f"the boundary-layer rakes would hold more than {WTP_MAX_PROBES} points per angle")
    wind = frame == "wind"
    if wind and any(not abs(a) <= WIND_ALPHA_MAX for a in alphas):
        raise ValueError(f'frame="wind" takes angles within +-{WIND_ALPHA_MAX:g} degrees, got {alphas!r}')
    nx, ny, u0 = int(nx), int(ny), float(u0)
    tau = float(tau) if tau is not None else (tau_from_reynolds(re, u0, nx) if re is not None else TAU_DEFAULT)
    if trt and not _np_dtype(dtype).type(tau) > 0.5:
        raise ValueError(f'collision="trt" needs tau above 0.5 in {_np_dtype(dtype).name}, got {tau!r}')
    if start is not None:
        _check_state(start, nx, ny, dtype, storage, len(alphas))
    if warmup_steps is None:
        warmup_steps = 0 if start is not None else int(math.ceil(2 * nx / u0))
    warmup_steps = int(warmup_steps)
    user = geo.round_coords(coords) if coords is not None and len(coords) else []
    if wind:                                                   # one body, at 0 degrees, in every member
        geoms = [geo.build_geometry(nx, ny, 0.0, user, shape)] * len(alphas)
        ux0 = np.array([u0 * math.cos(math.radians(a)) for a in alphas])
        vy0 = np.array([u0 * math.sin(math.radians(a)) for a in alphas])
    else:
        geoms = [geo.build_geometry(nx, ny, a, user, shape) for a in alphas]
        ux0 = u0
    masks = np.stack([g.mask for g in geoms])
    if boundary_layer:                                         # one set of stations and rake points per geometry (one in all with frame="wind")
        stations = [geo.surface_stations(g, nx, ny) for g in (geoms[:1] if wind else geoms)]
        rakes = [boundary_layer_points(s, bl_height * chord_cells(nx), bl_spacing) for s in stations]
        if wind:
            stations, rakes = stations * len(alphas), rakes * len(alphas)
    with PolarEngine(nx, ny, len(alphas), dtype=dtype, history_cap=samples, device=device, storage=storage) as eng:
        eng.set_masks(masks)
        if walls == "interpolated":
            eng.enable_interpolated_walls()
            q = geo.wall_distances(geoms[0].xp, geoms[0].yp, geoms[0].mask, nx, ny) if wind else None
            for m, g in enumerate(geoms):                      # (one member at a time: eight float64 planes each on the host)
                qm = q if wind else geo.wall_distances(g.xp, g.yp, g.mask, nx, ny)
                eng.set_wall_distances(qm, first=m)
                if slot is not None and (m == 0 or not wind):  # (one set of velocities serves every angle of the wind frame)
                    un = geo.slot_wall_velocity(g, g.mask, qm, nx, ny, slot["surface"], slot["x0"], slot["x1"], slot["vn"] * u0)
                if slot is not None:
                    if m == 0:
                        eng.enable_wall_velocity()
                        slot["links"] = []
                    eng.set_wall_velocity(un, first=m)
                    slot["links"].append(int(np.count_nonzero(un)))
        if wind:
            eng.enable_wind(vy0)
        eng.init_equilibrium(ux0)
        if loads:
            eng.enable_loads(*quarter_chord(nx, ny))
        if total_forces:
            eng.enable_momentum_exchange(*quarter_chord(nx, ny))
        if mean_fields:
            eng.enable_mean_fields()
        if boundary_layer:
            eng.enable_probes(rakes[0][0].size)
            eng.set_probes(np.stack([r[0] for r in rakes]), np.stack([r[1] for r in rakes]))
        if les is not None:
            eng.enable_les(les)
        if trt:
            eng.enable_trt(magic)
        if start is not None:
            eng.restore(start)
        if not vortex:
            if warmup_steps:
                eng.step(warmup_steps, tau, ux0)
            # the samples fall on the multiples of sample_every in (warm-up, warm-up + samples * sample_every]: exactly `samples` of them
            eng.step(samples * sample_every, tau, ux0, sample_every=sample_every)
        else:
            B = len(alphas)
            xc, yc = quarter_chord(nx, ny)
            bound = vortex_bound(nx, ny, xc, yc)
            after = int(math.ceil(chord_cells(nx) / u0)) if vortex_after is None else int(vortex_after)
            u_far, v_far = np.broadcast_to(np.asarray(ux0, np.float64), (B,)), (vy0 if wind else np.zeros(B))
            alpha_far = np.asarray(alphas if wind else [0.0] * B, np.float64)
            held = start.get("vortex") if start is not None else None
            strength = np.array(held["strength"], np.float64) if held else np.zeros(B)
            source = np.array(held["source"], np.float64) if held else np.zeros(B)
            total = warmup_steps + samples * sample_every
            eng.enable_far_profile()
            if vortex_on == "device":
                # the host loop below, enqueued: an update behind every vortex_every-th step of this call whose count lies at or beyond
                # `after`, and one behind a short last chunk; the log holds exactly those
                every, first = int(vortex_every), eng.step_count
                updates = sum(1 for k in range(1, total // every + 1) if first + k * every >= after)
                last = total % every != 0 and first + total >= after
                eng.enable_far_vortex(every, after, vortex_relax, u0, far_field == "vortex+source", xc, yc, u_far, v_far, alpha_far,
                                      log_cap=updates + int(last))
                if held:
                    eng.set_far_vortex(strength, source)
                if warmup_steps:
                    eng.step(warmup_steps, tau, ux0)
                eng.step(samples * sample_every, tau, ux0, sample_every=sample_every)
                if last:
                    eng.far_vortex_update()
                vortex_history = eng.far_vortex_log()
                strength, source = eng.far_vortex()
            else:
                vh = {k: [] for k in ("step", "fx", "fy", "strength", "source", "clipped")}

                def upload():
                    tabs = [far_profile(nx, ny, u_far[m], v_far[m], strength[m], source[m], xc, yc, eng.dtype) for m in range(B)]
                    eng.set_far_profile(*(np.stack([t[k] for t in tabs]) for k in range(3)))

                upload()
                done = 0
                while done < total:
                    n = min(int(vortex_every), total - done)
                    quiet = min(n, max(warmup_steps - done, 0))    # the chunk's steps that still belong to the warm-up take no sample
                    if quiet:
                        eng.step(quiet, tau, ux0)
                    if n > quiet:
                        eng.step(n - quiet, tau, ux0, sample_every=sample_every)
                    done += n
                    count = eng.step_count
                    if count >= after:
                        fx, fy, _, _ = eng.forces()
                        strength, source, clipped = vortex_update(strength, source, fx, fy, alpha_far, u0, vortex_relax, bound,
                                                                  with_source=far_field == "vortex+source")
                        upload()
                        for k, v in zip(vh, (count, fx, fy, strength, source, clipped)):
                            vh[k].append(v)
                U = len(vh["step"])
                vortex_history = {"step": np.asarray(vh["step"], np.int64), **{k: np.asarray(vh[k], np.float64).reshape(U, B) for k in ("fx", "fy", "strength", "source")},
                                  "clipped": np.asarray(vh["clipped"], bool).reshape(U, B)}
        h = eng.history()
        rho_ev, u_ev = eng.clamp_events()
        surfaces = [surface_cp(eng.surface(m), 0.0 if wind else a, u0) for m, a in enumerate(alphas)] if loads else [None] * len(alphas)
        means = [mean_flow(eng.mean_sums(m), u0) for m in range(len(alphas))] if mean_fields else [None] * len(alphas)
        probe_sums = [eng.probe_sums(m) for m in range(len(alphas))] if boundary_layer else None
        state = eng.state() if keep_state else None
        if vortex and state is not None:
            state["vortex"] = {"strength": strength.copy(), "source": source.copy()}
    if wind:                                                   # lattice axes -> wind axes, every sample of every member
        h["fx"], h["fy"] = wind_axes(h["fx"], h["fy"], alphas)
        if total_forces:
            h["fx_mex"], h["fy_mex"] = wind_axes(h["fx_mex"], h["fy_mex"], alphas)
    points = [polar_point(a, h["step"], h["fx"][:, m], h["fy"][:, m], h["surf"][:, m], h["rev"][:, m], u0, nx, (rho_ev[m], u_ev[m]),
                          mz=h["mz"][:, m] if loads else None, surface=surfaces[m],
                          **({k: h[k][:, m] for k in ("fx_mex", "fy_mex", "mz_mex", "links")} if total_forces else {}))
              for m, a in enumerate(alphas)]
    for p, mean in zip(points, means):
        p.mean = mean
    if vortex:
        for m, p in enumerate(points):
            p.vortex_strength, p.vortex_source = float(strength[m]), float(source[m])
    if boundary_layer:
        for m, p in enumerate(points):
            n = probe_sums[m]["n"]
            with np.errstate(invalid="ignore", divide="ignore"):
                means = {k: probe_sums[m][k] / n for k in ("rho", "ux", "uy")}
            p.boundary_layer = _boundary_layer_of(stations[m], means, rakes[m][2], u0, tau)
    return PolarResult(points=points, nx=nx, ny=ny, tau=tau, u0=u0, warmup_steps=warmup_steps, sample_every=int(sample_every), les=les,
                       walls=walls, frame=frame, storage=storage, state=state, collision=collision, magic=magic if trt else None,
                       far_field=far_field, vortex_history=vortex_history if vortex else None,
                       slot=dict(slot, links=np.array(slot["links"], np.int64)) if slot is not None else None)


def sweep_alphas(start: float, end: float, step: float) -> List[float]:
    """The page's angles of a sweep (pages/Airfoil_Analysis.py:930-932): rounded to 2 decimals, end included up to 1e-9."""
    return [round(start + i * step, 2)
            for i in range(int(round((end - start) / step)) + 1)
            if round(start + i * step, 2) <= end + 1e-9]


def _with_separation(result: PolarResult, rows: List[dict]) -> List[dict]:
    """polar_rows' rows with x_sep_upper and x_sep_lower in front of Status where every point carries a boundary layer
    (run_polar(boundary_layer=True)); the rows as they are otherwise.  "—" where the flow stays attached or the point failed."""
    if any(getattr(p, "boundary_layer", None) is None for p in result.points):
        return rows
    out = []
    for p, row in zip(result.points, rows):
        row = dict(row)
        status = row.pop("Status")
        for side in ("upper", "lower"):
            x = p.boundary_layer[side]["x_sep"]
            row["x_sep_" + side] = round(x, 3) if p.converged and math.isfinite(x) else "—"
        row["Status"] = status
        out.append(row)
    return out


def polar_rows(result: PolarResult, forces: str = "pressure") -> List[dict]:
    """The page's sweep table (pages/Airfoil_Analysis.py:950-966), one row per angle.  Cm is the mean moment coefficient of a
    point that carries one (run_polar(loads=True)), "—" otherwise.
    A point converged when every sample is finite and the stability net held no site at a bound; a failed one shows "—"
    throughout, as the page's failed rows do.
    forces="total" (every point must carry the momentum exchange, run_polar(total_forces=True), else ValueError): CL, CD, L/D
    and Cm from the totals, and between CD and L/D the pressure drag CDp and the friction drag CDf = CD - CDp.
    Where every point carries a boundary layer (run_polar(boundary_layer=True)) the rows also hold x_sep_upper and x_sep_lower, the
    x/c at which the skin friction of that surface first turns negative ("—": attached); without it the rows are what they always were."""
    if forces not in ("pressure", "total"):
        raise ValueError(f'forces must be "pressure" or "total", got {forces!r}')
    rows = []
    if forces == "total":
        if any(p.cd_total_mean is None for p in result.points):
            raise ValueError('forces="total" needs the momentum exchange of every point: run_polar(total_forces=True)')
        for p in result.points:
            if p.converged:
                ld = p.cl_total_mean / p.cd_total_mean if p.cd_total_mean != 0 else None
                rows.append({"α (°)": p.alpha, "CL": round(p.cl_total_mean, 4), "CD": round(p.cd_total_mean, 5),
                             "CDp": round(p.cd_mean, 5), "CDf": round(p.cd_friction_mean, 5),
                             "L/D": round(ld, 2) if ld is not None else "—", "Cm": round(p.cm_total_mean, 4), "Status": "✅ Converged"})
            else:
                rows.append({"α (°)": p.alpha, "CL": "—", "CD": "—", "CDp": "—", "CDf": "—", "L/D": "—", "Cm": "—",
                             "Status": "❌ Failed"})
        return _with_separation(result, rows)
    for p in result.points:
        if p.converged:
            ld = p.cl_mean / p.cd_mean if p.cd_mean != 0 else None
            rows.append({"α (°)": p.alpha, "CL": round(p.cl_mean, 4), "CD": round(p.cd_mean, 5),
                         "L/D": round(ld, 2) if ld is not None else "—",
                         "Cm": round(p.cm_mean, 4) if p.cm_mean is not None else "—", "Status": "✅ Converged"})
        else:
            rows.append({"α (°)": p.alpha, "CL": "—", "CD": "—", "L/D": "—", "Cm": "—", "Status": "❌ Failed"})
    return _with_separation(result, rows)
