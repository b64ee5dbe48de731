#!/usr/bin/env python
"""What the far-field vortex of a sweep costs, updated by the host and updated on the device (run_polar(vortex_on=)).

The configuration of profiles/polar_profile_cost.txt: the wind frame, 32 angles from -4 to 11.5 degrees, NACA 2412, 320x160 fp32,
9024 warm-up steps and 512 samples every 12 steps (15168 steps), loads off.  The time is the wall clock of the whole run_polar call
(masks, engine, steps, history), which ends in read-backs that wait for the device.  Uniform far field, vortex on the host and vortex
on the device, three calls each, alternating in one process after one untimed call of each; then the two vortex modes once more at
vortex_every = 12, an update behind every sample.  One JSON line per call.

    python tools/polar_vortex_cost.py [--every 96] [--dense 12] [--repeats 3]

--trace: one call of the device mode at --every and nothing else, to run under a kernel trace (the profiler slows the host, so its
run gives kernel durations and no wall clock).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import airfoil_cfd_tool_amd as pkg  # noqa: E402

ALPHAS = [-4.0 + 0.5 * k for k in range(32)]
RUN = dict(shape="naca2412", nx=320, ny=160, frame="wind", warmup_steps=9024, samples=512, sample_every=12, loads=False)
STEPS = RUN["warmup_steps"] + RUN["samples"] * RUN["sample_every"]
MODES = {"uniform": dict(far_field="uniform"), "vortex on the host": dict(far_field="vortex", vortex_on="host"),
         "vortex on the device": dict(far_field="vortex", vortex_on="device")}


def timed(mode, every):
    t0 = time.perf_counter()
    r = pkg.run_polar(ALPHAS, vortex_every=every, **MODES[mode], **RUN)
    dt = time.perf_counter() - t0
    vh = r.vortex_history
    line = {"tool": "polar_vortex_cost", "members": len(ALPHAS), "mode": mode, "vortex_every": every if vh is not None else None, "steps": STEPS,
            "seconds": round(dt, 4), "us_per_step_whole_call": round(dt / STEPS * 1e6, 2), "updates": 0 if vh is None else int(vh["step"].size),
            "clipped": 0 if vh is None else int(vh["clipped"].sum()), "cl_mean_6deg": round(r.points[20].cl_mean, 6)}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--every", type=int, default=96)
    ap.add_argument("--dense", type=int, default=12, help="the second vortex_every, timed for the two vortex modes only (0: skip)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="one device-mode call only, for a kernel trace")
    a = ap.parse_args()
    if a.trace:
        return timed("vortex on the device", a.every)
    warm = dict(RUN, warmup_steps=96, samples=8)
    for kw in MODES.values():                                              # code objects, allocator, first touches
        pkg.run_polar(ALPHAS, vortex_every=a.every, vortex_after=0, **kw, **warm)
    for _ in range(a.repeats):
        for mode in MODES:
            timed(mode, a.every)
    if a.dense:
        for _ in range(a.repeats):
            for mode in ("vortex on the host", "vortex on the device"):
                timed(mode, a.dense)


if __name__ == "__main__":
    main()
