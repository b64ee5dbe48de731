#!/usr/bin/env python3
"""A fine sweep with native and with half-precision population storage: what does storing binary16 deviations do to CL and CD?

    python tools/polar_half_sweep.py [--shape naca2412] [--start 4] [--end 6] [--step 0.25] [--size 320x160] [--samples 256]

run_polar over the angles twice, storage="native" and storage="half" (same lattice, tau, U0, warm-up and samples: run_polar's
defaults).  Per angle: the mean pressure CL and CD of each run, the difference half - native, and beside it the angle's own standard
deviation over the samples (of the native run), the yardstick the difference is read against.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import airfoil_cfd_tool_amd as pkg       # noqa: E402
from airfoil_cfd_tool_amd.polar import STORAGES       # noqa: E402


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
    res = {s: pkg.run_polar(alphas, shape=a.shape, nx=nx, ny=ny, samples=a.samples, storage=s) for s in STORAGES}
    n, h = res["native"], res["half"]
    print(f"# {a.shape} {nx}x{ny} float32, tau {n.tau}, U0 {n.u0}, warm-up {n.warmup_steps} steps, {a.samples} samples every "
          f"{n.sample_every} steps; pressure coefficients, means over the samples")
    for s, r in res.items():
        for p in r.points:
            if not p.converged:
                print(f"# {s}: alpha {p.alpha} did not converge (finite {p.finite}, clamp events {p.clamp_events})")
    print("#  alpha CL native   CL half   half-native  CL std   CD native   CD half   half-native   CD std")
    dcl, dcd = [], []
    for p, q in zip(n.points, h.points):
        dcl.append(q.cl_mean - p.cl_mean)
        dcd.append(q.cd_mean - p.cd_mean)
        print(f"{p.alpha:8.2f} {p.cl_mean:9.5f} {q.cl_mean:9.5f} {dcl[-1]:+12.5f} {p.cl_std:8.5f} {p.cd_mean:10.5f} {q.cd_mean:9.5f} "
              f"{dcd[-1]:+12.6f} {p.cd_std:9.6f}")
    dcl, dcd = np.array(dcl), np.array(dcd)
    cl, cd = np.array([p.cl_mean for p in n.points]), np.array([p.cd_mean for p in n.points])
    sl, sd = np.array([p.cl_std for p in n.points]), np.array([p.cd_std for p in n.points])
    print(f"# largest |half - native|: CL {float(np.abs(dcl).max()):.5f} ({100 * float(np.abs(dcl / cl).max()):.3f} % of CL, "
          f"{float(np.abs(dcl / sl).max()):.3f} of the angle's CL std), CD {float(np.abs(dcd).max()):.6f} "
          f"({100 * float(np.abs(dcd / cd).max()):.3f} % of CD, {float(np.abs(dcd / sd).max()):.3f} of the angle's CD std)")


if __name__ == "__main__":
    main()
