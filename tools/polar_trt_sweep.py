#!/usr/bin/env python3
"""What does the two-relaxation-time collision do to a polar?  A fine sweep at the default tau, and one angle at three tau.

    python tools/polar_trt_sweep.py [--shape naca2412] [--start 4] [--end 6] [--step 0.25] [--size 320x160] [--samples 256]
                                    [--angle 5] [--taus 0.52,0.58,0.8]

run_polar(total_forces=True) with collision="bgk", collision="trt" at magic 3/16 and collision="trt" at magic 1/4 (same lattice,
|U|, warm-up and samples: run_polar's defaults).  Part one: the angles of the sweep at the default tau; per angle the mean total
(momentum-exchange) CL and CD of each collision, their standard deviation over the samples and the clamp events, then the offsets of
the two TRT runs from BGK.  Part two: one angle at each tau; the same columns, then per collision the spread of CL and CD over the
tau values.  With one relaxation time the effective wall position moves with (tau - 1/2)^2; with two it is set by the magic number.
A change of tau also changes the Reynolds number, so the coefficients move with tau under every collision: the figures are printed,
not explained away.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import airfoil_cfd_tool_amd as pkg       # noqa: E402

COLLISIONS = (("bgk", None), ("trt", 3.0 / 16.0), ("trt", 1.0 / 4.0))


def label(c):
    return "bgk" if c[0] == "bgk" else f"trt {c[1]:.4f}"


def run(alphas, c, **kw):
    extra = {} if c[0] == "bgk" else {"collision": "trt", "magic": c[1]}
    return pkg.run_polar(alphas, total_forces=True, **extra, **kw)


def table(res, alphas_or_taus, first):
    print(f"# {first:>6s}  " + "  ".join(f"{label(c):>10s} CL_total  CD_total   CL std  clamps" for c in COLLISIONS))
    for i, x in enumerate(alphas_or_taus):
        cells = []
        for c in COLLISIONS:
            p = res[c][i]
            cells.append(f"{'':10s} {p.cl_total_mean:8.5f} {p.cd_total_mean:9.5f} {p.cl_total_std:8.5f} {p.clamp_events[0] + p.clamp_events[1]:7d}")
        print(f"{x:8.3f}  " + "  ".join(cells))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="naca2412")
    ap.add_argument("--start", type=float, default=4.0)
    ap.add_argument("--end", type=float, default=6.0)
    ap.add_argument("--step", type=float, default=0.25)
    ap.add_argument("--size", default="320x160")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--angle", type=float, default=5.0)
    ap.add_argument("--taus", default="0.52,0.58,0.8")
    a = ap.parse_args()
    nx, ny = (int(v) for v in a.size.split("x"))
    kw = dict(shape=a.shape, nx=nx, ny=ny, samples=a.samples)
    alphas = pkg.polar.sweep_alphas(a.start, a.end, a.step)
    sweep = {c: run(alphas, c, **kw) for c in COLLISIONS}
    r0 = sweep[COLLISIONS[0]]
    print(f"# {a.shape} {nx}x{ny} float32, |U| {r0.u0}, warm-up {r0.warmup_steps} steps, {a.samples} samples every {r0.sample_every} steps; "
          f"total (momentum-exchange) coefficients, means over the samples; clamps = density + speed clamp events of the last state")
    print(f"# part one: the sweep at tau {r0.tau}")
    pts = {c: r.points for c, r in sweep.items()}
    table(pts, alphas, "alpha")
    for c in COLLISIONS[1:]:
        dcl = np.array([p.cl_total_mean - q.cl_total_mean for p, q in zip(pts[c], pts[COLLISIONS[0]])])
        dcd = np.array([p.cd_total_mean - q.cd_total_mean for p, q in zip(pts[c], pts[COLLISIONS[0]])])
        print(f"# {label(c)} - bgk per angle, CL_total: " + " ".join(f"{x:+.5f}" for x in dcl))
        print(f"# {label(c)} - bgk per angle, CD_total: " + " ".join(f"{x:+.5f}" for x in dcd))
        print(f"# {label(c)} - bgk, mean: CL_total {float(dcl.mean()):+.5f}, CD_total {float(dcd.mean()):+.5f}")
    taus = [float(t) for t in a.taus.split(",")]
    print(f"# part two: alpha {a.angle} at tau " + ", ".join(f"{t:g}" for t in taus) + " (Re = |U| chord / ((tau - 1/2) / 3) changes with tau)")
    one = {c: [run([a.angle], c, tau=t, **kw).points[0] for t in taus] for c in COLLISIONS}
    table(one, taus, "tau")
    for c in COLLISIONS:
        cl = np.array([p.cl_total_mean for p in one[c]])
        cd = np.array([p.cd_total_mean for p in one[c]])
        print(f"# {label(c):>10s}: over the tau values CL_total spans {float(cl.max() - cl.min()):.5f}, CD_total spans {float(cd.max() - cd.min()):.5f}; "
              f"converged: {[p.converged for p in one[c]]}")


if __name__ == "__main__":
    main()
