#!/usr/bin/env python3
"""A fine sweep in both frames and under both wall rules: does turning the free stream remove the saw-tooth, and what does it cost?

    python tools/polar_wind_sweep.py [--shape naca2412] [--start 4] [--end 6] [--step 0.25] [--size 320x160] [--samples 256]

run_polar(total_forces=True) over the angles, four times: frame="body" and frame="wind", each with walls="staircase" and
walls="interpolated" (same lattice, tau, |U|, warm-up and samples: run_polar's defaults).  Per angle: the mean total
(momentum-exchange) CL and CD of each run and their second differences in alpha, d2[i] = v[i-1] - 2 v[i] + v[i+1] (interior
angles); then, per run, the r.m.s. and the largest |d2| and the lift-curve slope (CL(end) - CL(start)) / (end - start); and, per
wall rule, the offset of the wind-frame CL and CD from the body-frame ones at each angle.  The body frame's values are themselves
scattered by the raster from angle to angle; the wind frame's top and bottom rows carry inflow and outflow.  The offset is printed,
not explained away.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import airfoil_cfd_tool_amd as pkg       # noqa: E402
from airfoil_cfd_tool_amd.polar import FRAMES, WALLS       # noqa: E402


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
    runs = [(f, w) for w in WALLS for f in FRAMES]
    res = {k: pkg.run_polar(alphas, shape=a.shape, nx=nx, ny=ny, samples=a.samples, total_forces=True, frame=k[0], walls=k[1]) for k in runs}
    r0 = res[runs[0]]
    print(f"# {a.shape} {nx}x{ny} float32, tau {r0.tau}, |U| {r0.u0}, warm-up {r0.warmup_steps} steps, {a.samples} samples every "
          f"{r0.sample_every} steps; total (momentum-exchange) coefficients, means over the samples")
    cl, cd, std, links = {}, {}, {}, {}
    for k, r in res.items():
        for p in r.points:
            if not p.converged:
                print(f"# {k}: alpha {p.alpha} did not converge (finite {p.finite}, clamp events {p.clamp_events})")
        cl[k] = np.array([p.cl_total_mean for p in r.points])
        cd[k] = np.array([p.cd_total_mean for p in r.points])
        std[k] = np.array([p.cl_total_std for p in r.points])
        links[k] = np.array([int(p.history["links"][-1]) for p in r.points])
    for k in runs:
        dcl, dcd = second_differences(cl[k]), second_differences(cd[k])
        print(f"# frame {k[0]}, walls {k[1]}")
        print("#  alpha  CL_total     d2 CL  CD_total     d2 CD   CL std  links")
        for i, al in enumerate(alphas):
            inner = 0 < i < len(alphas) - 1
            a1 = f"{dcl[i - 1]:+9.5f}" if inner else "        —"
            a2 = f"{dcd[i - 1]:+9.5f}" if inner else "        —"
            print(f"{al:8.2f} {cl[k][i]:9.5f} {a1} {cd[k][i]:9.5f} {a2} {std[k][i]:8.5f} {links[k][i]:6d}")
        slope = (cl[k][-1] - cl[k][0]) / (alphas[-1] - alphas[0])
        print(f"# {k[0]:4s} {k[1]:12s} d2 CL_total: r.m.s. {float(np.sqrt((dcl * dcl).mean())):.5f}, largest |d2| {float(np.abs(dcl).max()):.5f}; "
              f"d2 CD_total: r.m.s. {float(np.sqrt((dcd * dcd).mean())):.5f}, largest |d2| {float(np.abs(dcd).max()):.5f}; "
              f"slope {slope:.5f} per degree")
    for w in WALLS:
        for name, v in (("CL", cl), ("CD", cd)):
            b, s = second_differences(v["body", w]), second_differences(v["wind", w])
            print(f"# walls {w}: r.m.s. d2 {name}_total, wind / body: {float(np.sqrt((s * s).mean()) / np.sqrt((b * b).mean())):.4f}")
        off_cl, off_cd = cl["wind", w] - cl["body", w], cd["wind", w] - cd["body", w]
        print(f"# walls {w}: wind - body per angle, CL_total: " + " ".join(f"{x:+.4f}" for x in off_cl))
        print(f"# walls {w}: wind - body per angle, CD_total: " + " ".join(f"{x:+.5f}" for x in off_cd))
        print(f"# walls {w}: mean offset CL_total {float(off_cl.mean()):+.4f} ({100.0 * float((off_cl / cl['body', w]).mean()):+.1f} %), "
              f"CD_total {float(off_cd.mean()):+.5f} ({100.0 * float((off_cd / cd['body', w]).mean()):+.1f} %)")


if __name__ == "__main__":
    main()
