#!/usr/bin/env python3
"""Batched sweeps (libwtpolar.so) against the same member-steps on sequential single handles: one JSON line per (lattice, B).

    python tools/polar_bench.py [--sizes 320x160,1024x512] [--members 1,8,32,64] [--steps 200] [--warmup 50]

Per line: us per batched step and member-steps per second (host clock around wtp_step + wtp_sync, after a warm-up), aggregate
GLUPS, algorithmic bytes per step (72 B per site fp32, + 12 B per site on the emitting last step of a call) over the time as a
fraction of 8 TB/s, and the same member-steps taken by B libwindtunnel handles stepped one after another (library defaults),
timed in the same process.

    python tools/polar_bench.py --loads [--sizes 320x160] [--members 32] [--steps 1200] [--sample-every 12] [--repeats 7]

The sampled batched step with and without surface loads (wtp_enable_loads: one k_loads_batch behind every k_forces_batch): the two
variants are timed in turn, `repeats` times each in the same process, and the line gives the median and the range of each.

    python tools/polar_bench.py --mex [--loads] [--lib PATH] [the same options]

The same protocol for the momentum-exchange readout (wtp_enable_mex: one k_mex_batch behind the other reductions); with --loads the
surface loads are on in both variants.  --lib loads another build of libwtpolar.so (such as one compiled with -DWTP_MEX_WINDOW=0,
which visits every interior column).

    python tools/polar_bench.py --mean [--loads] [--mex] [--lib PATH] [the same options]

The same protocol for the mean fields (wtp_enable_mean: one k_mean_batch behind the reductions); with --loads / --mex those read-outs
are on in both variants.  The line also gives the bytes one sample moves (3 sizeof(T) + 2 * 56 per site and member: derived, not
measured) and what the added time per sample makes of them against 8 TB/s.

    python tools/polar_bench.py --les CS [--repeats 5] [the options of the first form]

The batched step with the Smagorinsky subgrid viscosity (wtp_enable_les, Smagorinsky constant CS in every member): the COLLIDE_LES
instantiation of k_step_batch in place of the plain one.  The line gives `repeats` timings of the same window and their median; without --les the same repeats time the
BGK step, so that two lines compare.  No sequential leg: a single handle has no such collision.  With --loads / --mex / --mean the
model is on in both variants of those protocols.

    python tools/polar_bench.py --ibb [--les CS] [--repeats 5] [the options of the first form]

The batched step with interpolated bounce-back (wtp_enable_ibb, every member with the wall distances of its own airfoil):
the WALL_INTERP instantiation of k_step_batch with the collision the other switches select.  The line has the shape of --les's; no
sequential leg either.  With --loads / --mex / --mean the model is on in both variants of those protocols (and --mex then times k_mex_batch with LinkInterp).

    python tools/polar_bench.py --wall-velocity [--les CS] [--wind] [--trt MAGIC] [--profile] [--repeats 5] [the options of the first form]

The batched step with moving walls (wtp_enable_wall_velocity on top of --ibb's wall distances; every member's body turns rigidly about the
lattice's centre, so that every link carries a term): the WALL_MOVING instantiation of k_step_batch with the collision and the far field the other switches select.  The
line has the shape of --les's; no sequential leg either.  Not with --storage half.  With --mex the model is on in both variants of that
protocol (and --mex then times k_mex_batch with LinkMoving); not with --loads, --mean or --probes.  Without --wall-velocity, --lib may name a build from
before the entry points existed.

    python tools/polar_bench.py --wind [--les CS] [--ibb] [--repeats 5] [the options of the first form]

The batched step with an inclined free stream (wtp_enable_wind): the FAR_INCLINED instantiation of the kernel the other switches select.
The masks stay those of the other forms, so that the tile classes are the same; member m's cross-flow is U0 sin(alpha_m).  The line
has the shape of --les's; no sequential leg either.  With --loads / --mex / --mean the model is on in both variants of those protocols.

    python tools/polar_bench.py --storage half [--les CS] [--wind] [--repeats 5] [the options of the first form]

The batched step of a half batch (PolarEngine(storage="half")): k_step_half_batch, with the collision and the far field the other switches
select, on lattices of binary16 deviations from the weights.  The line has the shape of --les's and counts 37 B per site (nine 2-byte loads,
nine 2-byte stores and the mask byte) in place of 72; no sequential leg.  Not with --ibb.  With --loads / --mex / --mean the batch is
a half batch in both variants of those protocols (and --mex then times k_mex_batch on half_t elements).

    python tools/polar_bench.py --trt MAGIC [--les CS] [--ibb] [--wind] [--storage half] [--repeats 5] [the options of the first form]

The batched step with the two-relaxation-time collision (wtp_enable_trt, magic number MAGIC in every member): the COLLIDE_TRT (with --les
COLLIDE_TRT_LES) instantiation of k_step_batch, in a half batch of k_step_half_batch, with the inclined far field.  The line has the shape of --les's; no sequential
leg either.  With --loads / --mex / --mean the model is on in both variants of those protocols.  Without --trt, --lib may name a
build from before the collision existed, so that a parent commit's library is timed by the same script.

    python tools/polar_bench.py --profile [--les CS] [--ibb] [--wind] [--trt MAGIC] [--repeats 5] [the options of the first form]

The batched step with a prescribed far-field profile (wtp_enable_far_profile; every member with the tables of its free stream plus a
point vortex at the quarter chord that induces 0.01 at the nearest far-field cell): the FAR_PROFILE instantiation of the kernel the other
switches select.  The line has the shape of --les's; no sequential leg either.  Not with --storage half.  Without --profile,
--lib may name a build from before the entry points existed.

    python tools/polar_bench.py --probes [--loads] [--mex] [--mean] [--lib PATH] [the same options as --loads]

The same protocol for the probe points (wtp_enable_probes: one k_probe_batch behind the other read-outs) with run_polar's default
boundary-layer rake on every member's airfoil (160 stations, a point every 0.5 cells up to 0.15 chords: 8320 points per member at
320x160); with --loads / --mex / --mean those read-outs are on in both variants.  With --lib naming a build from before the entry points
existed only the variant without probes is timed, so that a parent commit's library gives its figure by the same script and protocol.

Tracing: run under `rocprofv3 --kernel-trace --stats -- python tools/polar_bench.py ...`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import airfoil_cfd_tool_amd as pkg       # noqa: E402

PEAK_BPS = 8.0e12
TAU, U0 = 0.58, 0.06


def _alphas(b):
    return np.linspace(-4.0, 12.0, b) if b > 1 else np.array([6.0])


def _masks(nx, ny, b):
    return np.stack([pkg.geometry.build_geometry(nx, ny, float(a), None, "naca2412").mask for a in _alphas(b)])


def _interpolated_walls(eng, nx, ny, b):
    """Switch interpolated bounce-back on and give every member the wall distances of its airfoil (_masks' geometries)."""
    eng.enable_interpolated_walls()
    for m, a in enumerate(_alphas(b)):
        g = pkg.geometry.build_geometry(nx, ny, float(a), None, "naca2412")
        eng.set_wall_distances(pkg.geometry.wall_distances(g.xp, g.yp, g.mask, nx, ny), first=m)


def _wall_velocity(eng, nx, ny, b):
    """Switch the wall velocity on and turn every member's body rigidly about the lattice's centre, so that every link carries a term:
    a rim speed of 0.02 at half a chord's distance."""
    eng.enable_wall_velocity()
    omega = 0.02 / (0.5 * pkg.windtunnel.chord_cells(nx))
    for m, a in enumerate(_alphas(b)):
        g = pkg.geometry.build_geometry(nx, ny, float(a), None, "naca2412")
        q = pkg.geometry.wall_distances(g.xp, g.yp, g.mask, nx, ny)
        eng.set_wall_velocity(pkg.geometry.rigid_wall_velocity(g.mask, q, 0.0, 0.0, omega, 0.5 * nx, 0.5 * ny), first=m)


def _cross_flow(b):
    return U0 * np.sin(np.radians(_alphas(b)))


def _far_profile(eng, nx, ny, b, wind):
    """Switch the prescribed far-field profile on: member m's free stream plus a vortex that induces 0.01 at the nearest far-field cell."""
    xc, yc = pkg.polar.quarter_chord(nx, ny)
    strength = 0.01 * pkg.polar.vortex_bound(nx, ny, xc, yc)
    v0 = _cross_flow(b) if wind else np.zeros(b)
    tabs = [pkg.polar.far_profile(nx, ny, U0, v0[m], strength, 0.0, xc, yc) for m in range(b)]
    eng.enable_far_profile()
    eng.set_far_profile(*(np.stack([t[k] for t in tabs]) for k in range(3)))


def bench_batch(nx, ny, b, steps, warmup, masks, les=None, repeats=1, ibb=False, wind=False, storage="native", trt=None, profile=False,
                wall_velocity=False):
    """Seconds of `steps` steps after a warm-up, one figure per repeat; les: the Smagorinsky constant of every member (None: BGK);
    ibb: interpolated bounce-back with every airfoil's wall distances; wind: an inclined free stream, U0 sin(alpha) across;
    trt: the magic number of the two-relaxation-time collision in every member (None: one relaxation time); profile: a prescribed
    far-field profile, the free stream plus a weak vortex; wall_velocity: interpolated bounce-back with a rigid rotation of every body
    as its wall velocity."""
    out = []
    with pkg.PolarEngine(nx, ny, b, storage=storage) as eng:
        eng.set_masks(masks)
        if wind:
            eng.enable_wind(_cross_flow(b))
        eng.init_equilibrium(U0)
        if les is not None:
            eng.enable_les(les)
        if ibb or wall_velocity:
            _interpolated_walls(eng, nx, ny, b)
        if wall_velocity:
            _wall_velocity(eng, nx, ny, b)
        if trt is not None:
            eng.enable_trt(trt)
        if profile:
            _far_profile(eng, nx, ny, b, wind)
        eng.step(warmup, TAU, U0)
        eng.sync()
        for _ in range(repeats):
            t0 = time.perf_counter()
            eng.step(steps, TAU, U0)
            eng.sync()
            out.append(time.perf_counter() - t0)
    return out


LES = None      # --les: the Smagorinsky constant the sampled protocols run with (None: BGK)
IBB = False     # --ibb: the sampled protocols run with interpolated bounce-back
WIND = False    # --wind: the sampled protocols run with an inclined free stream
STORAGE = "native"      # --storage: the sampled protocols run on a batch of this storage
TRT = None      # --trt: the magic number the sampled protocols run the two-relaxation-time collision with (None: off)
WALLVEL = False         # --wall-velocity: the sampled protocols run with interpolated bounce-back and a wall velocity


def _default_rakes(nx, ny, b):
    """(x, y) [b][P]: run_polar's default boundary-layer rake on every member's airfoil (_masks' geometries)."""
    pts = []
    for a in _alphas(b):
        st = pkg.geometry.surface_stations(pkg.geometry.build_geometry(nx, ny, float(a), None, "naca2412"), nx, ny)
        pts.append(pkg.polar.boundary_layer_points(st, pkg.polar.BL_HEIGHT_DEFAULT * st["chord_cells"], pkg.polar.BL_SPACING_DEFAULT)[:2])
    return np.stack([p[0] for p in pts]), np.stack([p[1] for p in pts])


def bench_sampled(nx, ny, b, steps, warmup, masks, every, loads, repeats, mex=False, mean=False, probes=None):
    """Seconds of `steps` sampled steps, one figure per repeat; the history is emptied between repeats.  probes: (x, y) [b][P], the
    probe points of every member (None: off)."""
    out = []
    with pkg.PolarEngine(nx, ny, b, history_cap=steps // every + 1, storage=STORAGE) as eng:
        eng.set_masks(masks)
        if WIND:
            eng.enable_wind(_cross_flow(b))
        eng.init_equilibrium(U0)
        if loads:
            eng.enable_loads(*pkg.polar.quarter_chord(nx, ny))
        if mex:
            eng.enable_momentum_exchange(*pkg.polar.quarter_chord(nx, ny))
        if mean:
            eng.enable_mean_fields()
        if probes is not None:
            eng.enable_probes(probes[0].shape[1])
            eng.set_probes(*probes)
        if LES is not None:
            eng.enable_les(LES)
        if IBB or WALLVEL:
            _interpolated_walls(eng, nx, ny, b)
        if WALLVEL:
            _wall_velocity(eng, nx, ny, b)
        if TRT is not None:
            eng.enable_trt(TRT)
        eng.step(warmup - warmup % every, TAU, U0)
        eng.sync()
        for _ in range(repeats):
            eng.clear_history()
            eng.sync()
            t0 = time.perf_counter()
            eng.step(steps, TAU, U0, sample_every=every)
            eng.sync()
            out.append(time.perf_counter() - t0)
    return out


def loads_cost(a):
    for size in a.sizes.split(","):
        nx, ny = (int(v) for v in size.split("x"))
        for b in (int(v) for v in a.members.split(",")):
            masks = _masks(nx, ny, b)
            t = {False: [], True: []}
            for r in range(a.repeats):                 # in turn, so that a drift of the clocks lands on both
                for loads in (False, True):
                    t[loads] += bench_sampled(nx, ny, b, a.steps, a.warmup, masks, a.sample_every, loads, 1)
            us = {k: np.array(v) / a.steps * 1e6 for k, v in t.items()}
            med = {k: float(np.median(v)) for k, v in us.items()}
            samples = a.steps // a.sample_every
            print(json.dumps({"tool": "polar_bench --loads", "nx": nx, "ny": ny, "dtype": "float32", "members": b, "steps": a.steps,
                              "sample_every": a.sample_every, "repeats": a.repeats,
                              "us_per_step_plain_median": round(med[False], 3), "us_per_step_plain_range": [round(float(us[False].min()), 3), round(float(us[False].max()), 3)],
                              "us_per_step_loads_median": round(med[True], 3), "us_per_step_loads_range": [round(float(us[True].min()), 3), round(float(us[True].max()), 3)],
                              "loads_us_per_sample": round((med[True] - med[False]) * a.steps / samples, 3),
                              "loads_fraction_of_step": round(med[True] / med[False] - 1.0, 5)}), flush=True)


def mex_cost(a):
    variants = (False, True)
    for size in a.sizes.split(","):
        nx, ny = (int(v) for v in size.split("x"))
        for b in (int(v) for v in a.members.split(",")):
            masks = _masks(nx, ny, b)
            t = {v: [] for v in variants}
            for r in range(a.repeats):                 # in turn, so that a drift of the clocks lands on both
                for mex in variants:
                    t[mex] += bench_sampled(nx, ny, b, a.steps, a.warmup, masks, a.sample_every, a.loads, 1, mex=mex)
            us = {k: np.array(v) / a.steps * 1e6 for k, v in t.items()}
            med = {k: float(np.median(v)) for k, v in us.items()}
            samples = a.steps // a.sample_every
            line = {"tool": "polar_bench --mex", "lib": a.lib or "default", "storage": a.storage, "loads": bool(a.loads), "nx": nx, "ny": ny, "dtype": "float32",
                    "members": b, "steps": a.steps, "sample_every": a.sample_every, "repeats": a.repeats,
                    "us_per_step_plain_median": round(med[False], 3),
                    "us_per_step_plain_range": [round(float(us[False].min()), 3), round(float(us[False].max()), 3)],
                    "us_per_step_mex_median": round(med[True], 3),
                    "us_per_step_mex_range": [round(float(us[True].min()), 3), round(float(us[True].max()), 3)],
                    "mex_us_per_sample": round((med[True] - med[False]) * a.steps / samples, 3),
                    "mex_fraction_of_step": round(med[True] / med[False] - 1.0, 5)}
            print(json.dumps(line), flush=True)


def mean_cost(a):
    variants = (False, True)
    for size in a.sizes.split(","):
        nx, ny = (int(v) for v in size.split("x"))
        for b in (int(v) for v in a.members.split(",")):
            masks = _masks(nx, ny, b)
            t = {v: [] for v in variants}
            for r in range(a.repeats):                 # in turn, so that a drift of the clocks lands on both
                for mean in variants:
                    t[mean] += bench_sampled(nx, ny, b, a.steps, a.warmup, masks, a.sample_every, a.loads, 1, mex=a.mex, mean=mean)
            us = {k: np.array(v) / a.steps * 1e6 for k, v in t.items()}
            med = {k: float(np.median(v)) for k, v in us.items()}
            samples = a.steps // a.sample_every
            per_sample = (med[True] - med[False]) * a.steps / samples
            bytes_sample = b * nx * ny * (3 * 4 + 2 * 56)
            line = {"tool": "polar_bench --mean", "lib": a.lib or "default", "storage": a.storage, "loads": bool(a.loads), "mex": bool(a.mex), "nx": nx, "ny": ny,
                    "dtype": "float32", "members": b, "steps": a.steps, "sample_every": a.sample_every, "repeats": a.repeats,
                    "us_per_step_plain": [round(float(v), 3) for v in us[False]], "us_per_step_plain_median": round(med[False], 3),
                    "us_per_step_mean": [round(float(v), 3) for v in us[True]], "us_per_step_mean_median": round(med[True], 3),
                    "mean_us_per_sample": round(per_sample, 3), "mean_fraction_of_step": round(med[True] / med[False] - 1.0, 5),
                    "mean_bytes_per_sample": bytes_sample,
                    "mean_fraction_of_8TBps_host_clock": round(bytes_sample / (per_sample * 1e-6) / PEAK_BPS, 4) if per_sample > 0 else None}
            print(json.dumps(line), flush=True)


def probes_cost(a):
    variants = (False, True) if hasattr(pkg.polar.load_polar_library(), "wtp_enable_probes") else (False,)
    for size in a.sizes.split(","):
        nx, ny = (int(v) for v in size.split("x"))
        for b in (int(v) for v in a.members.split(",")):
            masks = _masks(nx, ny, b)
            rakes = _default_rakes(nx, ny, b) if True in variants else None
            t = {v: [] for v in variants}
            for r in range(a.repeats):                 # in turn, so that a drift of the clocks lands on both
                for on in variants:
                    t[on] += bench_sampled(nx, ny, b, a.steps, a.warmup, masks, a.sample_every, a.loads, 1, mex=a.mex, mean=a.mean,
                                           probes=rakes if on else None)
            us = {k: np.array(v) / a.steps * 1e6 for k, v in t.items()}
            med = {k: float(np.median(v)) for k, v in us.items()}
            samples = a.steps // a.sample_every
            line = {"tool": "polar_bench --probes", "lib": a.lib or "default", "storage": a.storage, "loads": bool(a.loads), "mex": bool(a.mex),
                    "mean": bool(a.mean), "nx": nx, "ny": ny, "dtype": "float32", "members": b, "steps": a.steps, "sample_every": a.sample_every,
                    "repeats": a.repeats, "us_per_step_plain": [round(float(v), 3) for v in us[False]], "us_per_step_plain_median": round(med[False], 3)}
            if True in variants:
                per_sample = (med[True] - med[False]) * a.steps / samples
                line.update({"points_per_member": int(rakes[0].shape[1]), "us_per_step_probes": [round(float(v), 3) for v in us[True]],
                             "us_per_step_probes_median": round(med[True], 3), "probes_us_per_sample": round(per_sample, 3),
                             "probes_fraction_of_step": round(med[True] / med[False] - 1.0, 5)})
            print(json.dumps(line), flush=True)


def bench_sequential(nx, ny, b, steps, warmup, masks):
    hs = []
    try:
        for m in range(b):
            e = pkg.Engine(nx, ny)
            hs.append(e)
            e.set_mask(masks[m])
            e.init_equilibrium(U0)
        for e in hs:
            e.step(warmup, TAU, U0)
        for e in hs:
            e.sync()
        t0 = time.perf_counter()
        for e in hs:
            e.step(steps, TAU, U0)
        for e in hs:
            e.sync()
        return time.perf_counter() - t0
    finally:
        for e in hs:
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="320x160,1024x512")
    ap.add_argument("--members", default="1,8,32,64")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--no-sequential", action="store_true", help="time the batch only")
    ap.add_argument("--loads", action="store_true", help="the sampled step with and without surface loads")
    ap.add_argument("--mex", action="store_true", help="the sampled step with and without the momentum-exchange readout")
    ap.add_argument("--mean", action="store_true", help="the sampled step with and without the mean fields")
    ap.add_argument("--probes", action="store_true", help="the sampled step with and without probe points (run_polar's default boundary-layer rake)")
    ap.add_argument("--les", type=float, default=None, metavar="CS", help="step with the Smagorinsky subgrid viscosity, constant CS in every member")
    ap.add_argument("--ibb", action="store_true", help="step with interpolated bounce-back, every member with its airfoil's wall distances")
    ap.add_argument("--wall-velocity", action="store_true", help="step with interpolated bounce-back and a wall velocity, a rigid rotation of every member's body")
    ap.add_argument("--wind", action="store_true", help="step with an inclined free stream, U0 sin(alpha) across in every member")
    ap.add_argument("--storage", default="native", choices=pkg.polar.STORAGES, help="how the batch stores its populations (half: binary16 deviations)")
    ap.add_argument("--trt", type=float, default=None, metavar="MAGIC", help="step with the two-relaxation-time collision, magic number MAGIC in every member")
    ap.add_argument("--profile", action="store_true", help="step with a prescribed far-field profile, the free stream plus a weak vortex in every member")
    ap.add_argument("--lib", default=None, help="another build of libwtpolar.so to load instead of the package's")
    ap.add_argument("--sample-every", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=None, help="timed windows per variant (default 7; 1 for the first form)")
    a = ap.parse_args()
    plain = not (a.mean or a.mex or a.loads or a.probes)
    if a.repeats is None:
        a.repeats = 1 if plain else 7
    if a.lib:
        unused = (("wtp_enable_trt", a.trt is None), ("wtp_enable_far_profile", not a.profile), ("wtp_set_far_profile", not a.profile),
                  # the device-side far-field vortex and the tables' read-back: nothing here calls them
                  ("wtp_read_far_profile", True), ("wtp_enable_far_vortex", True), ("wtp_set_far_vortex", True), ("wtp_far_vortex", True),
                  ("wtp_far_vortex_update", True), ("wtp_far_vortex_log", True),
                  # the probe points: only --probes calls them, and with an older build it times the variant without them alone
                  ("wtp_enable_probes", True), ("wtp_set_probes", True), ("wtp_probe_sums", True), ("wtp_probe_sample", True),
                  ("wtp_enable_wall_velocity", not a.wall_velocity), ("wtp_set_wall_velocity", not a.wall_velocity))
        pkg.polar.load_polar_library(a.lib, optional=tuple(name for name, free in unused if free))
    if a.storage == "half" and (a.ibb or a.wall_velocity):
        ap.error("--storage half does not combine with --ibb or --wall-velocity")
    if a.wall_velocity and (a.loads or a.mean or a.probes):
        ap.error("--wall-velocity times the plain stepping form and --mex only")
    half = a.storage == "half"
    if half and a.profile:
        ap.error("--storage half does not combine with --profile")
    if a.profile and not plain:
        ap.error("--profile times the plain stepping form only")
    global LES, IBB, WIND, STORAGE, TRT, WALLVEL
    LES, IBB, WIND, STORAGE, TRT, WALLVEL = a.les, a.ibb, a.wind, a.storage, a.trt, a.wall_velocity
    if a.probes:
        return probes_cost(a)
    if a.mean:
        return mean_cost(a)
    if a.mex:
        return mex_cost(a)
    if a.loads:
        return loads_cost(a)
    for size in a.sizes.split(","):
        nx, ny = (int(v) for v in size.split("x"))
        for b in (int(v) for v in a.members.split(",")):
            masks = _masks(nx, ny, b)
            sites = nx * ny
            ts = bench_batch(nx, ny, b, a.steps, a.warmup, masks, les=a.les, repeats=a.repeats, ibb=a.ibb, wind=a.wind, storage=a.storage, trt=a.trt,
                             profile=a.profile, wall_velocity=a.wall_velocity)
            t = float(np.median(ts))
            us = t / a.steps * 1e6
            ms_per_s = b * a.steps / t
            bytes_step = b * sites * ((37 if half else 72) + 12 / a.steps)
            line = {"tool": "polar_bench", "nx": nx, "ny": ny, "dtype": "float32", "members": b, "steps": a.steps,
                    "us_per_batched_step": round(us, 2), "member_steps_per_s": round(ms_per_s, 1),
                    "glups": round(ms_per_s * sites / 1e9, 3), "hbm_fraction_of_8TBps": round(bytes_step / (t / a.steps) / PEAK_BPS, 4)}
            if a.les is not None or a.ibb or a.wall_velocity or a.wind or half or a.trt is not None or a.profile or a.repeats > 1:
                line["les"] = a.les
                if a.trt is not None:
                    line["trt"] = a.trt
                if a.lib:
                    line["lib"] = a.lib
                if half:
                    line["storage"] = "half"
                if a.ibb:
                    line["ibb"] = True
                if a.wall_velocity:
                    line["wall_velocity"] = True
                if a.wind:
                    line["wind"] = True
                if a.profile:
                    line["profile"] = True
                line["us_per_batched_step_repeats"] = [round(v / a.steps * 1e6, 2) for v in ts]
            if not a.no_sequential and a.les is None and not a.ibb and not a.wall_velocity and not a.wind and not half and a.trt is None and not a.profile:
                ts = bench_sequential(nx, ny, b, a.steps, a.warmup, masks)
                line["sequential_us_per_member_step"] = round(ts / (b * a.steps) * 1e6, 2)
                line["sequential_member_steps_per_s"] = round(b * a.steps / ts, 1)
                line["speedup_vs_sequential"] = round(ts / t, 2)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
