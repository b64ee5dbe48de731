#!/usr/bin/env python3
"""A fine sweep under both wall rules: does interpolated bounce-back give the smoother polar?

    python tools/polar_ibb_sweep.py [--shape naca2412] [--start 4] [--end 6] [--step 0.25] [--size 320x160] [--samples 256]

run_polar(total_forces=True) over the angles, once with walls="staircase" and once with walls="interpolated" (same lattice, tau, U0,
warm-up and samples: run_polar's defaults).  Per angle: the mean total (momentum-exchange) CL and CD of both runs and their second
differences in alpha, d2[i] = v[i-1] - 2 v[i] + v[i+1] (interior angles); then the r.m.s. and the largest |d2| of each column and
the number of wall links of each member.  A smooth polar has small second differences: what remains is the curvature of the true
polar over one step of alpha, which both rules share, plus whatever the wall's description adds from one angle to the next.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import airfoil_cfd_tool_amd as pkg       # noqa: E402


def second_differences(v):
    v = np.asarray(v, np.float64)
    return v[:-2] - 2.0 * v[1:-1] + v[2:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="naca2412")
    ap.add_argument("--start", type=float, default=4.0)
    ap.add_argument("--end", type=float, default=6.0)
    ap.add_argument("--step", type=float, default=0.25)
    ap.add_argument("--size", default="320x160")
    ap.add_argument("--samples", type=int, default=256)
    a = ap.parse_args()
    nx, ny = (int(v) for v in a.size.split("x"))
    alphas = pkg.polar.sweep_alphas(a.start, a.end, a.step)
    res = {w: pkg.run_polar(alphas, shape=a.shape, nx=nx, ny=ny, samples=a.samples, total_forces=True, walls=w)
           for w in ("staircase", "interpolated")}
    r0 = res["staircase"]
    print(f"# {a.shape} {nx}x{ny} float32, tau {r0.tau}, U0 {r0.u0}, warm-up {r0.warmup_steps} steps, {a.samples} samples every "
          f"{r0.sample_every} steps; total (momentum-exchange) coefficients, means over the samples")
    cols = {}
    for w, r in res.items():
        for p in r.points:
            if not p.converged:
                print(f"# {w}: alpha {p.alpha} did not converge (finite {p.finite}, clamp events {p.clamp_events})")
        cols[w, "cl"] = np.array([p.cl_total_mean for p in r.points])
        cols[w, "cd"] = np.array([p.cd_total_mean for p in r.points])
        cols[w, "cl_std"] = np.array([p.cl_total_std for p in r.points])
        cols[w, "links"] = np.array([int(p.history["links"][-1]) for p in r.points])
    d2 = {k: second_differences(v) for k, v in cols.items() if k[1] in ("cl", "cd")}
    print("# alpha | staircase: CL_total  d2 CL     CD_total  d2 CD     CL std   links | interpolated: CL_total  d2 CL     CD_total  d2 CD     "
          "CL std   links")
    for i, al in enumerate(alphas):
        cells = [f"{al:7.2f}"]
        for w in ("staircase", "interpolated"):
            inner = 0 < i < len(alphas) - 1
            dcl = f"{d2[w, 'cl'][i - 1]:+9.5f}" if inner else "        —"
            dcd = f"{d2[w, 'cd'][i - 1]:+9.5f}" if inner else "        —"
            cells.append(f"{cols[w, 'cl'][i]:9.5f} {dcl} {cols[w, 'cd'][i]:9.5f} {dcd} {cols[w, 'cl_std'][i]:8.5f} {cols[w, 'links'][i]:6d}")
        print(" | ".join(cells))
    for w in ("staircase", "interpolated"):
        for v in ("cl", "cd"):
            d = d2[w, v]
            print(f"# {w:12s} d2 {v.upper()}_total: r.m.s. {float(np.sqrt((d * d).mean())):.5f}, largest |d2| {float(np.abs(d).max()):.5f}")
    for v in ("cl", "cd"):
        s, t = d2["staircase", v], d2["interpolated", v]
        print(f"# r.m.s. d2 {v.upper()}_total, interpolated / staircase: {float(np.sqrt((t * t).mean()) / np.sqrt((s * s).mean())):.3f}")


if __name__ == "__main__":
    main()
