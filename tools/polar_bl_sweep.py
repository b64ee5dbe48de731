#!/usr/bin/env python3
"""What does the boundary-layer read-out of a sweep give?  A NACA 2412 from 0 to 14 degrees, and a thin flat plate beside Blasius.

    python tools/polar_bl_sweep.py [--size 320x160] [--samples 256] [--out profiles/polar_bl_sweep.txt]

run_polar(boundary_layer=True) with its default rake (160 stations, a point every 0.5 cells up to 0.15 chords) and run_polar's defaults
otherwise (body frame, staircase walls, BGK, the default tau, warm-up of two flow-throughs).
Case 1: NACA 2412, 0 to 14 degrees in steps of 2.  Per angle CL, CD, the page's separation count and x_sep / x_reattach of both
surfaces; then Cf and H of the upper surface at a few stations.
Case 2: a flat plate of 1.2 % thickness (two rows of cells at 320x160) at 0 degrees.  Per station delta* sqrt(Re_x) / x,
Cf sqrt(Re_x) and H beside Blasius' 1.72, 0.664 and 2.59, with Re_x = U0 x / nu and x the distance from the leading edge.
Nothing is fitted and nothing is left out: at a chord Reynolds number of a few hundred on this lattice the figures are what they are.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import airfoil_cfd_tool_amd as pkg       # noqa: E402
from airfoil_cfd_tool_amd.windtunnel import chord_cells       # noqa: E402

STATIONS = (0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9, 0.97)
PLATE_T = 0.012
PLATE = [(1.0, PLATE_T / 2), (0.0, PLATE_T / 2), (0.0, -PLATE_T / 2), (1.0, -PLATE_T / 2), (1.0, PLATE_T / 2)]


def nearest(side, xc):
    return int(np.argmin(np.abs(side["x_over_c"] - xc)))


def fmt(x):
    return f"{x:8.4f}" if np.isfinite(x) else "       -"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="320x160")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_bl_sweep.txt"))
    a = ap.parse_args()
    nx, ny = (int(v) for v in a.size.split("x"))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    alphas = [2.0 * k for k in range(8)]
    res = pkg.run_polar(alphas, shape="naca2412", nx=nx, ny=ny, samples=a.samples, boundary_layer=True)
    nu = (res.tau - 0.5) / 3.0
    say(f"# naca2412 {nx}x{ny} float32, U0 {res.u0}, tau {res.tau} (Re_c = U0 chord / nu = {res.u0 * chord_cells(nx) / nu:.0f}), warm-up {res.warmup_steps} steps, "
        f"{a.samples} samples every {res.sample_every} steps; rake: {res.points[0].boundary_layer['heights'].size} points per station, "
        f"{res.points[0].boundary_layer['heights'][0]:g} to {res.points[0].boundary_layer['heights'][-1]:g} cells")
    say("# case 1: x/c at which Cf first turns negative going from the leading edge (x_sep) and where it turns back (x_re); - : none")
    say("#  alpha        CL        CD  rev/surf  upper x_sep     x_re  lower x_sep     x_re  converged")
    for p in res.points:
        up, lo = p.boundary_layer["upper"], p.boundary_layer["lower"]
        say(f"{p.alpha:8.2f}  {p.cl_mean:8.5f}  {p.cd_mean:8.5f}  {p.sep_frac:8.4f}     {fmt(up['x_sep'])} {fmt(up['x_reattach'])}     {fmt(lo['x_sep'])} {fmt(lo['x_reattach'])}  {p.converged}")
    for name, key in (("Cf", "cf"), ("H", "H"), ("Ue/U0", "ue"), ("delta*/c", "dstar")):
        say(f"# upper surface, {name} at the station nearest x/c = " + ", ".join(f"{x:g}" for x in STATIONS))
        for p in res.points:
            side = p.boundary_layer["upper"]
            say(f"{p.alpha:8.2f}  " + "  ".join(fmt(side[key][nearest(side, x)]) for x in STATIONS))
    say("# lower surface, Cf at the same stations")
    for p in res.points:
        side = p.boundary_layer["lower"]
        say(f"{p.alpha:8.2f}  " + "  ".join(fmt(side["cf"][nearest(side, x)]) for x in STATIONS))

    plate = pkg.run_polar([0.0], coords=PLATE, nx=nx, ny=ny, samples=a.samples, boundary_layer=True)
    p = plate.points[0]
    chord = chord_cells(nx)
    solid_rows = int((pkg.geometry.build_geometry(nx, ny, 0.0, pkg.geometry.round_coords(PLATE)).mask != 0).any(axis=1).sum())
    say(f"# case 2: a flat plate, thickness {PLATE_T} chords ({solid_rows} rows of cells), 0 degrees; CL {p.cl_mean:.5f}, CD {p.cd_mean:.5f}, converged {p.converged}")
    say("# Blasius: delta* sqrt(Re_x) / x = 1.72, Cf sqrt(Re_x) = 0.664, H = 2.59; Re_x = U0 x / nu, x from the leading edge in cells")
    say("#  side     x/c      Re_x   Ue/U0  delta* sqrt(Re_x)/x  Cf sqrt(Re_x)         H  delta* (cells)")
    for name in ("upper", "lower"):
        side = p.boundary_layer[name]
        for xc in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9):
            k = nearest(side, xc)
            x = side["x_over_c"][k] * chord
            re_x = plate.u0 * x / nu
            say(f"  {name}  {side['x_over_c'][k]:6.3f}  {re_x:8.1f}  {side['ue'][k]:6.3f}  {side['dstar'][k] * chord * np.sqrt(re_x) / x:19.3f}  "
                f"{side['cf'][k] * np.sqrt(re_x):13.3f}  {side['H'][k]:8.3f}  {side['dstar'][k] * chord:14.3f}")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
