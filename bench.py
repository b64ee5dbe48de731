#!/usr/bin/env python3
"""bench.py — MLUPS of the D2Q9 wind-tunnel step on MI355X (BASELINE.json's metric).

    python bench.py [--gpus N] [--steps K] [--warmup W]          (N > 1 without a launcher: starts the line below as a child job)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one lattice update (simStep, html:510-525) of the whole tunnel.  Workload (default, `--config 2`):
BASELINE.json configs[2] — 4096x4096 fp32, AoA 10 deg, U0 0.06, tau 0.58; `--config N` runs any of BASELINE.json's five
configurations on its own shape / angle / tau / dtype / size (CONFIGS below), explicit flags override single values.  The S1223 coordinates
named there are not available offline (no network; the reference ships no .dat files), so the
body is the reference's own high-camber built-in shape NACA 6409 (html:127); the kernel's cost
depends on the body only through the fraction of window-tiles that touch its surface.

N > 1: the SAME 4096x4096 lattice is split into N column slabs (strong scaling, as the metric
"MLUPS on 4096^2 ... at 1/2/4/8 MI355X" is quoted), one process per GPU, ghost columns
exchanged by RCCL send/recv inside libwindtunnel every `halo` steps.  That path has never met more
than one GPU (no multi-GPU box was available to the builder): every rank first runs the library's
one-rank RCCL self-test, then joins the communicator under a watchdog; any failure prints rank,
device and wt_last_error() and exits non-zero — nothing is retried and no process is re-exec'ed.

Prints ONE JSON line on rank 0 (contract in the task description), with `roofline` and
`cpu_baseline` objects.  The roofline object carries BOTH views of the dominant kernel: the
real HBM rate from the rocprofv3 counters (when profiles/pmc_traffic.json has an entry for this
workload) and the "effective" rate at the scheme's 72 B per site update, which a pass
that advances two steps can exceed because it moves fewer bytes.  The CPU baseline is the straight
NumPy transcription of the scheme (oracle/lbm_numpy.py) timed on this host on a bounded sample — it
is only ever the thing measured BESIDE the product, never part of it.

A plain run does only what the headline needs: set-up, clock settling, warm-up, the K timed steps, the
line.  `--full` adds every side measurement: the rocprofv3 counter runs of this workload (`--pmc-traffic`),
the un-fused and the contracted kernels beside the timed one (`--side`) and the CPU baseline
(`--cpu-steps`); each of the three can also be asked for on its own.  `--dump-outputs DIR` writes what
the timed steps computed (populations and macroscopic fields after the last step) as DIR/<name>.npy.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

# the host driver of this pool only supports dmabuf IPC; without this RCCL / device-memory sharing across
# processes fails with "hipIpcGetMemHandle: invalid argument" (set before anything loads the HIP runtime)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_PEAK_GBPS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s; 6.29 TB/s float4-copy)
BYTES_PER_LUP = {"float32": 72, "float64": 144}   # 9 loads + 9 stores per site update
COMM_TIMEOUT_S = 180.0


# BASELINE.json's five configurations, each with its own parameters (U0 = 0.06 throughout; tau 0.58 = html:78 unless a Reynolds number is named:
# tau = 0.5 + 3 U0 (NX / 1.84) / Re).  `steps` / `warmup`: what `--config N` runs when --steps / --warmup are not given — configs 0 and 1
# name their own step counts; the others get a steady-state sample.  Config 2's S1223 coordinates are not available offline (see the module text).
CONFIGS = {
    0: dict(shape="naca0012", nx=256, ny=128, aoa=0.0, dtype="float32", re=None, steps=500, warmup=100,
            name="BASELINE configs[0]: NACA 0012, 256x128 D2Q9, AoA 0 deg, 500 steps (the reference's own CPU-runnable case: a parity case, launch-bound on a GPU)"),
    1: dict(shape="naca2412", nx=1024, ny=512, aoa=5.0, dtype="float32", re=None, steps=2000, warmup=300,
            name="BASELINE configs[1]: NACA 2412, 1024x512 fp32, AoA 5 deg, 2000 steps (38 MB working set: cache-resident)"),
    2: dict(shape="naca6409", nx=4096, ny=4096, aoa=10.0, dtype="float32", re=None, steps=400, warmup=300,
            name="BASELINE configs[2]: 4096x4096 fp32, AoA 10 deg; S1223 coordinates unavailable offline -> NACA 6409; pass --dat PATH to use a supplied file"),
    3: dict(shape="naca0012", nx=16384, ny=4096, aoa=8.0, dtype="float32", re=None, steps=200, warmup=100,
            name="BASELINE configs[3]: NACA 0012, 16384x4096 fp32, AoA 8 deg (the 8-GPU column-slab case: --gpus 8 splits it, one GPU holds it whole)"),
    4: dict(shape="naca4412", nx=4096, ny=2048, aoa=12.0, dtype="float64", re=1e6, steps=240, warmup=120,
            name="BASELINE configs[4]: NACA 4412, 4096x2048 fp64, Re=1e6 (tau = 0.5 + 3 U0 (NX/1.84)/Re ~ 0.5004), AoA 12 deg near stall"),
}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--config", type=int, default=2, choices=sorted(CONFIGS),
                    help="which of BASELINE.json's configurations to run, on ITS shape / AoA / tau / dtype / lattice (default 2: the one the metric is quoted "
                         "on); --nx/--ny/--dtype/--shape/--aoa/--tau/--re override single values (the workload is then labelled 'custom')")
    # defaults (config 2): the clocks of an idle MI355X take 20-30 ms of work to settle (profiles/r03_g_time_series.txt: 98 -> 86 us per step over the first
    # 250 steps of the bench lattice), so the untimed warm-up covers that and the timed region is 35 ms of steady state
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--nx", type=int, default=None)
    ap.add_argument("--ny", type=int, default=None)
    ap.add_argument("--dtype", default=None, choices=["float32", "float64"])
    ap.add_argument("--shape", default=None)
    ap.add_argument("--dat", default=None, metavar="PATH",
                    help="airfoil coordinates from a .dat file (Selig / Lednicer, parsed and repaired like the reference's back end: "
                         "datfile.load_dat) in place of --shape; e.g. the S1223 file BASELINE configs[2] names, which neither the reference "
                         "(.gitignore:4 excludes *.dat) nor this image ships")
    ap.add_argument("--local-slabs", type=int, default=0, metavar="P",
                    help="ONE process, P column slabs of the lattice as P handles on device 0 (wt_link_local + wt_step_group: the slab state "
                         "machine and the refresh / interior overlap of the N-GPU path, run on one GPU); prints per-slab device times")
    ap.add_argument("--aoa", type=float, default=None)
    ap.add_argument("--u0", type=float, default=0.06)
    ap.add_argument("--tau", type=float, default=None)
    ap.add_argument("--re", type=float, default=None, help="Reynolds number: tau = 0.5 + 3 U0 (NX / 1.84) / Re (SURVEY 8b) in place of --tau")
    ap.add_argument("--halo", type=int, default=61,
                    help="ghost columns per interior slab side (exchange every `halo` steps; 61 = one single refresh step + fifteen four-step passes.  With "
                         "the ghost columns TRIMMED pass by pass (option trim_ghosts, round 4) a deeper halo costs little redundant work and spares refresh "
                         "steps; the exchange grows with it.  Real slabs of the 8-way split of 4096^2 on overlapping windows, slowest slab measured / with the "
                         "modelled exchange: 17.5 / 18.1 us per step at 29, 16.4 / 17.5 at 45, 16.0 / 17.3 at 61, 15.7 / 17.1 at 77 "
                         "(profiles/r05_t_slab_costs_cfg2_overlap.txt, r05_z_halo_deep.txt)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: the counter runs (--pmc-traffic 1), the side kernels (--side 1) and the CPU "
                         "baseline (--cpu-steps 10), each unless given explicitly; without it those default to off (and --settle-ms to 120 in place of 50)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what they computed as DIR/<name>.npy (f: the nine populations, rho, ux, uy; the run's float "
                         "type): whole arrays up to 50 MB, beyond that the same fixed, seeded sample of sites in every array")
    ap.add_argument("--cpu-steps", type=int, default=None, help="steps of the NumPy CPU baseline (0 = skip; default 10 with --full, else 0)")
    ap.add_argument("--fuse", type=int, default=-1, choices=[-1, 0, 1, 2],
                    help="two steps per pass over the lattice (csrc/step_march.hpp; fp32; bit-identical): -1 library "
                         "default (on where it pays), 0 off, 1 where it pays, 2 always")
    ap.add_argument("--fuse-chunk", type=int, default=0, help="cost limit of a marching unit in columns (0 = whole resident rounds)")
    ap.add_argument("--fuse-sites", type=int, default=0, choices=[0, 2], help="sites per lane of the marching kernel (0 = automatic; fixed by the dtype since round 3)")
    ap.add_argument("--fuse-depth", type=int, default=0, choices=[0, 2, 3, 4], help="steps per pass of the marching kernel (0 = automatic)")
    ap.add_argument("--fast-math", type=int, default=-1, choices=[-1, 0, 1],
                    help="the OPT-IN contracted collision (fused multiply-adds, v_rcp): -1 (default) = the bit-exact kernels print the line and the "
                         "contracted ones are timed beside them as roofline.contracted; 0 = skip that; 1 = the whole run uses them (NOT bit-exact)")
    ap.add_argument("--pmc-traffic", type=int, default=None, choices=[0, 1],
                    help="1 (default with --full, one GPU only): before the timed run, measure this workload's HBM traffic and vector-ALU activity per launch in this "
                         "session — three short child runs of this script under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` / the SQ group — and use "
                         "them for roofline.traffic / frac / valu_busy_frac; 0, or when rocprofv3 is not available: the entry of profiles/pmc_traffic.json "
                         "(measured in another run), if there is one, and no valu_busy_frac")
    ap.add_argument("--side", type=int, default=None, choices=[0, 1],
                    help="1 (default with --full, one GPU): also time the un-fused kernel and (fp32) the opt-in contracted arithmetic for the roofline entry — BEFORE the "
                         "warm-up, reported as preheat_steps / preheat_ms; 0: nothing runs on the device before the declared warm-up but the plan's own tuning")
    ap.add_argument("--settle-ms", type=float, default=None,
                    help="untimed steps on the bench handle IN FRONT of the declared warm-up, this many milliseconds of device work, so that the timed region "
                         "runs at settled clocks: a fresh MI355X process reads 336, 359, 353, 339, 330, 322 ... 299 us per pass over its first 35 ms of "
                         "marching and 295-300 from then on, whatever the flow does (profiles/r05_zz_clock_settling.txt) — a timed region of 20 steps is "
                         "1.6 ms.  The lattice is put back to its initial state afterwards; counted in preheat_steps / preheat_ms.  0: none.  Default 50 with "
                         "--full; 120 without, which stands in for the ~70 ms of side kernels (--side) a plain run no longer puts in front of its warm-up")
    ap.add_argument("--balance", type=int, default=-1, metavar="R",
                    help="slab runs with strong scaling: R rounds of cutting the slabs by MEASURED cost instead of equal widths before the run (every rank "
                         "times its candidate slab alone, airfoil_cfd_tool_amd.distributed.balance_split; the split with the fastest slowest slab is kept, "
                         "the equal one included).  -1 (default): 4 rounds when there is more than one slab, 0: equal widths")
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                    help="strong: nx x ny split over N GPUs; weak: every GPU gets an nx x ny slab")
    args = ap.parse_args()
    for k, on, off in (("cpu_steps", 10, 0), ("pmc_traffic", 1, 0), ("side", 1, 0), ("settle_ms", 50.0, 120.0)):
        if getattr(args, k) is None:
            setattr(args, k, on if args.full else off)
    if args.dump_outputs and (args.gpus > 1 or args.local_slabs > 0):
        ap.error("--dump-outputs: one GPU, one lattice (not with --gpus N or --local-slabs)")
    cfg = CONFIGS[args.config]
    args.custom = [k for k in ("nx", "ny", "dtype", "shape", "aoa") if getattr(args, k) is not None and getattr(args, k) != cfg[k]]
    for k in ("nx", "ny", "dtype", "shape", "aoa", "steps", "warmup"):
        if getattr(args, k) is None:
            setattr(args, k, cfg[k])
    if args.tau is not None and args.re is not None:
        ap.error("--tau and --re exclude each other")
    tau_of = lambda re_: 0.58 if re_ is None else 0.5 + 3.0 * args.u0 * (args.nx / 1.84) / re_        # html:77-79, SURVEY 8b
    cfg_tau = tau_of(cfg["re"])
    if args.tau is None:
        args.tau = tau_of(args.re if args.re is not None else cfg["re"])
    if abs(args.tau - cfg_tau) > 1e-12:
        args.custom.append("tau")
    if args.u0 != 0.06:
        args.custom.append("u0")
    if args.dat:
        args.custom.append("dat")
    return args


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def cpu_baseline(mask, steps, tau, u0, dtype):
    """NumPy transcription (the 'port') on the host cores; element-wise NumPy = 1 core."""
    import numpy as np
    import lbm_numpy
    ny, nx = mask.shape
    f, _ = lbm_numpy.equilibrium_init(nx, ny, u0, np.dtype(dtype))
    f, _ = lbm_numpy.step(f, mask, tau, u0)            # untimed first touch
    t0 = time.perf_counter()
    for _ in range(steps):
        f, _ = lbm_numpy.step(f, mask, tau, u0)
    dt = time.perf_counter() - t0
    return {
        "value": nx * ny * steps / dt / 1e6,
        "unit": "MLUPS",
        "cores": 1,
        "kind": "port",
        "sample": f"{steps} steps of the same {nx}x{ny} {dtype} lattice and mask, oracle/lbm_numpy.py "
                  f"(NumPy {np.__version__}, element-wise => single core; host: {cpu_model()}, {os.cpu_count()} cpus), {dt:.1f} s",
    }


DUMP_SEED = 20240611
DUMP_BYTES = 12 << 22        # 9 populations + rho, ux, uy: 2^22 / element-size sites (50.3 MB, fp32 or fp64)


def dump_outputs(eng, out_dir):
    """--dump-outputs: the lattice after the last timed step as a caller of the step receives it — the nine populations (f) and the
    macroscopic fields (rho, ux, uy) — in the run's float type.  Lattices beyond DUMP_BYTES are sampled: the same sites (fixed seed, in
    ascending order of y * nx + x) in every array, so that two builds given the same arguments can be compared value for value."""
    import numpy as np
    f = eng.read_f()
    rho, ux, uy = eng.read_macro()
    ny, nx = rho.shape
    arrays = {"f": f.reshape(9, ny * nx), "rho": rho.reshape(-1), "ux": ux.reshape(-1), "uy": uy.reshape(-1)}
    n = DUMP_BYTES // (12 * f.itemsize)
    if ny * nx > n:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(ny * nx, n, replace=False))
        arrays = {k: np.ascontiguousarray(v[..., idx]) for k, v in arrays.items()}
        sample = f"{n} of {ny * nx} sites, numpy default_rng({DUMP_SEED}).choice without replacement, sorted"
    else:
        arrays = {"f": f, "rho": rho, "ux": ux, "uy": uy}
        sample = "all sites"
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)
    return {"dir": out_dir, "arrays": sorted(arrays), "sites": sample}


def baseline_metric():
    """BASELINE.json's metric string, verbatim."""
    try:
        with open(os.path.join(ROOT, "BASELINE.json"), encoding="utf-8") as fh:
            return json.load(fh)["metric"]
    except Exception:
        return "MLUPS on 4096² fp32 D2Q9 at 1/2/4/8 MI355X; achieved % HBM3E peak"


def measured_traffic(workload_key):
    """HBM bytes per launch from the rocprofv3 PMC passes kept under profiles/ (None if this workload was never profiled).
    The entry was measured in ANOTHER run of this same command on another box of the pool; `source` says which."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(path) as fh:
            e = json.load(fh).get(workload_key)
    except Exception:
        return None
    return e if e and "hbm_bytes_per_launch" in e else None


SQ_GROUP = ("SQ_ACTIVE_INST_VALU", "SQ_BUSY_CYCLES", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "GRBM_GUI_ACTIVE")


def pmc_counters_this_session(args):
    """Counters per launch of every kernel of this workload, measured NOW on this box: three short child runs of this same script and workload under
    rocprofv3 — FETCH_SIZE and WRITE_SIZE in a pass each (they do not fit one; MI355X_MICROARCH.md HBM section: FETCH_SIZE KB x 1024 x 2 on gfx950,
    WRITE_SIZE KB x 1024), then the SQ group (vector-ALU activity, wave cycles, waits) with GRBM_GUI_ACTIVE (the kernel's duration in clocks).
    Runs before this process touches the GPU; the children are started with the interpreter itself behind `--`, in a session of their own so that a
    timeout takes the whole process group down (no grandchild keeps the GPU beside the timed run).  Returns None on any failure (no rocprofv3, no
    counters, a profiler already attached to this process); a failing SQ pass alone leaves the traffic figures standing."""
    import glob
    import re
    import shutil
    import signal
    import sqlite3
    import subprocess
    import tempfile
    rocprof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if rocprof is None or "rocprof" in os.environ.get("LD_PRELOAD", "") or os.environ.get("ROCP_TOOL_LIBRARIES"):
        return None
    child = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--config", str(args.config), "--steps", "48", "--warmup", "12", "--cpu-steps", "0",
             "--fast-math", "1" if args.fast_math == 1 else "0", "--side", "1", "--settle-ms", "0", "--pmc-traffic", "0", "--nx", str(args.nx), "--ny", str(args.ny),
             "--dtype", args.dtype, "--shape", args.shape, "--aoa", str(args.aoa), "--u0", str(args.u0), "--tau", repr(args.tau), "--fuse", str(args.fuse),
             "--fuse-chunk", str(args.fuse_chunk), "--fuse-sites", str(args.fuse_sites), "--fuse-depth", str(args.fuse_depth)]
    if args.dat:
        child += ["--dat", os.path.abspath(args.dat)]          # (the children run in /tmp)
    per_kernel = {}
    tmp = tempfile.mkdtemp(prefix="wt_pmc_", dir="/tmp")
    try:
        # WT_TUNE=0: the counters are averaged per kernel over ALL dispatches of the child run, and the trial passes of the measured cut
        # (13 per new mask, every one with the halo kernel's gather path) would be averaged in; the modelled cut moves the same bytes per pass
        env = dict(os.environ, TMPDIR="/tmp", WT_TUNE="0")
        for group in (("FETCH_SIZE",), ("WRITE_SIZE",), SQ_GROUP):
            out = os.path.join(tmp, group[0])
            proc = subprocess.Popen([rocprof, "--pmc", *group, "-d", out, "-o", "c", "--"] + child, cwd="/tmp", env=env, stdout=subprocess.PIPE,
                                    stderr=subprocess.STDOUT, text=True, start_new_session=True)
            try:
                proc.communicate(timeout=240)
            except subprocess.TimeoutExpired:
                try:
                    os.killpg(proc.pid, signal.SIGKILL)        # rocprofv3 AND the interpreter behind it
                except OSError:
                    pass
                proc.wait()
                if group is SQ_GROUP:
                    break
                return None
            dbs = glob.glob(os.path.join(out, "**", "*.db"), recursive=True)
            if proc.returncode != 0 or not dbs:
                if group is SQ_GROUP:
                    break                                      # traffic measured, vector-ALU activity not: the line says so
                return None
            con = sqlite3.connect(dbs[0])
            acc = {}
            for kname, cname, disp, val in con.execute("select kernel_name, counter_name, dispatch_id, value from counters_collection"):
                if cname not in group:
                    continue
                k = re.sub(r"\(.*", "", kname).replace("void ", "").replace(", ", ",")
                acc.setdefault((k, cname), {}).setdefault(disp, 0.0)
                acc[(k, cname)][disp] += val                   # summed over the chip (one row per counter instance)
            for (k, cname), d in acc.items():
                per_kernel.setdefault(k, {})[cname] = sum(d.values()) / len(d)
                per_kernel[k].setdefault("dispatches", {})[cname] = len(d)
    except Exception:      # noqa: BLE001 - the file entry (or null) stands in
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return per_kernel


def pass_kernels(fused, depth):
    """(predicate over kernel names, description) of the dominant kernels of one launch (pass)."""
    if not fused:
        return (lambda k: k.startswith("wt::k_step<") and ",false," in k), "wt::k_step<T,false,...> (non-emitting step)"
    if depth >= 3:
        # (a three-step pass on a four-step plan — a tau without a proved fast division — still runs k_halo4: the tables decide)
        return ((lambda k: (k.startswith("wt::k_march3<") and f",{depth},false," in k) or k.startswith("wt::k_halo4<") or k.startswith("wt::k_halo3<")),
                f"one pass = wt::k_halo4 / k_halo3 + wt::k_march3<T,S,{depth},false,FD>")
    return ((lambda k: (k.startswith("wt::k_march<") and ",false," in k) or k.startswith("wt::k_halo_from_seams")),
            "one pass = wt::k_halo_from_seams + wt::k_march<T,S,false,FD>")


def select_traffic(per_kernel, fused, depth):
    """Sum the dominant kernels of one launch (pass) out of pmc_counters_this_session()'s table."""
    if not per_kernel:
        return None
    use, what = pass_kernels(fused, depth)
    fetch = sum(v.get("FETCH_SIZE", 0.0) for k, v in per_kernel.items() if use(k)) * 1024 * 2
    write = sum(v.get("WRITE_SIZE", 0.0) for k, v in per_kernel.items() if use(k)) * 1024
    if fetch <= 0 or write <= 0:
        return None
    return {"hbm_bytes_per_launch": fetch + write, "fetch_bytes_corrected": fetch, "write_bytes": write, "kernel": what,
            "measured": "this session, this box: child runs of this command (48 timed steps, the MODELLED cut of the units: WT_TUNE=0, which moves the "
                        "same bytes per pass as the measured cut of the timed run) under rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, just before the timed run",
            "source": "rocprofv3 counters, FETCH_SIZE KB x1024 x2 (gfx950 correction, MI355X_MICROARCH.md HBM section) + WRITE_SIZE KB x1024"}


def select_valu(per_kernel, fused, depth, n_simd, launch_ms):
    """Vector-ALU activity of one launch (pass) from the SQ group of pmc_counters_this_session(): SQ_ACTIVE_INST_VALU counts, per wave, the
    quad-cycles a vector instruction of that wave is executing (MI355X_MICROARCH.md: SQ_ACTIVE_INST_* / SQ_WAVE_CYCLES / SQ_WAIT_* count
    quad-cycles), summed over the chip.  valu_busy_frac = that x 4 clocks / (SIMDs x the kernels' duration in clocks), the duration taken from
    GRBM_GUI_ACTIVE of the SAME profiled dispatches (summed over the 8 XCDs by rocprofv3: / 8) — no clock frequency is assumed; beside it the
    same numerator over this run's launch time at the nominal 2.4 GHz.  With two waves per SIMD the figure can exceed 0.5 only by overlapping
    the two waves' instructions; 1.0 is a vector instruction in flight on every SIMD for the whole launch."""
    if not per_kernel:
        return None
    use, what = pass_kernels(fused, depth)
    tot = {c: sum(v.get(c, 0.0) for k, v in per_kernel.items() if use(k)) for c in SQ_GROUP}
    if tot["SQ_ACTIVE_INST_VALU"] <= 0 or tot["SQ_WAVE_CYCLES"] <= 0:
        return None
    clocks = tot["GRBM_GUI_ACTIVE"] / 8.0
    out = {"kernel": what, "SQ_ACTIVE_INST_VALU": tot["SQ_ACTIVE_INST_VALU"], "SQ_WAVE_CYCLES": tot["SQ_WAVE_CYCLES"], "SQ_WAIT_ANY": tot["SQ_WAIT_ANY"],
           "SQ_BUSY_CYCLES": tot["SQ_BUSY_CYCLES"], "GRBM_GUI_ACTIVE": tot["GRBM_GUI_ACTIVE"], "simds": n_simd,
           "valu_active_per_wave": tot["SQ_ACTIVE_INST_VALU"] / tot["SQ_WAVE_CYCLES"],
           "waves_waiting_frac": tot["SQ_WAIT_ANY"] / tot["SQ_WAVE_CYCLES"],
           "valu_busy_frac_at_2p4_ghz": tot["SQ_ACTIVE_INST_VALU"] * 4.0 / (n_simd * launch_ms * 1e-3 * 2.4e9),
           "valu_busy_frac": None, "effective_clock_ghz": None,
           "measured": "this session, this box: a third child run under rocprofv3 --pmc " + " ".join(SQ_GROUP) + " (per launch, summed over the chip)"}
    if clocks > 0:
        out["valu_busy_frac"] = tot["SQ_ACTIVE_INST_VALU"] * 4.0 / (n_simd * clocks)
        out["effective_clock_ghz"] = clocks / (launch_ms * 1e-3) / 1e9      # profiled clocks over the UN-profiled launch time: indicative only
    # GRBM_GUI_ACTIVE has been seen ten times too large on a launch of a millisecond (configs[3]: "22 GHz"): a clock outside what the part
    # can run at means the counter pass is not to be trusted — fall back to the nominal clock and say so
    if not (clocks > 0 and 1.0 <= out["effective_clock_ghz"] <= 3.0):
        out["valu_busy_frac"] = out["valu_busy_frac_at_2p4_ghz"]
        out["clock_note"] = "GRBM_GUI_ACTIVE implausible for this launch time: valu_busy_frac taken at the nominal 2.4 GHz"
    return out


# Exchange-cost model of a ghost refresh.  A refresh moves, per interior side of a slab, all nine populations of `halo` ghost
# columns (csrc/windtunnel.hip exchange_rccl: 18 grouped ncclSend / ncclRecv per side straight on the lattice): 9 x halo x pitch x element size bytes
# in and the same out.  The two sides of a slab go to different neighbours, i.e. over different xGMI links, so a side is the unit.  Stated rates:
# one xGMI link of an MI355X carries 153.6 GB/s bidirectional = 76.8 GB/s per direction at best (the 7 x ~153 GB/s the task statement quotes per
# GPU); a grouped send/recv costs a fixed ~12 us of launch / proxy latency before the first byte moves (RCCL point-to-point on one node — an
# ASSUMPTION until a box with two GPUs has run it: no round has had one).  model_us = 12 + bytes / 76.8e3.
XGMI_LINK_GBPS_PER_DIRECTION = 76.8
EXCHANGE_FIXED_US = 12.0


def exchange_model(halo, ny, esz, sides):
    pitch = (ny + 255) // 256 * 256                                     # csrc: the lattice pitch, NY rounded to 256 rows
    nbytes = 9 * halo * pitch * esz
    return {"exchange_bytes_each": nbytes, "exchange_sides": sides,
            "exchange_model_us": (EXCHANGE_FIXED_US + nbytes / (XGMI_LINK_GBPS_PER_DIRECTION * 1e3)) if sides else 0.0}


EXCHANGE_MODEL_NOTE = ("exchange_bytes_each = 9 populations x halo columns x pitch x element size, per side and refresh (in, and as much out); exchange_model_us = "
                       f"{EXCHANGE_FIXED_US:g} us fixed + bytes / {XGMI_LINK_GBPS_PER_DIRECTION:g} GB/s (one xGMI link, one direction; the sides use different links) "
                       "- a stated model, not a measurement; exchange_ms_each / exchange_exposed_ms_each beside it are this run's event times")


def die(rank, device, what, err=None):
    """One diagnosable line per failing rank, then a non-zero exit (never a retry, never a re-exec)."""
    msg = f"[bench.py] rank {rank} (device {device}) FAILED: {what}"
    if err is not None:
        msg += f": {err}"
    msg += ("  | re-run with NCCL_DEBUG=WARN (RCCL reads the NCCL_* variables) for the transport's own message; "
            f"HSA_ENABLE_IPC_MODE_LEGACY={os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')}")
    print(msg, file=sys.stderr, flush=True)
    os._exit(3)


def with_watchdog(seconds, rank, device, what, fn):
    """Runs fn(); if it has not returned after `seconds` the process reports and exits (a peer that never joins an
    RCCL communicator would otherwise block this rank for ever)."""
    done = threading.Event()

    def watch():
        if not done.wait(seconds):
            die(rank, device, f"{what} did not finish within {seconds:.0f} s (a peer is missing or the transport hangs)")

    t = threading.Thread(target=watch, daemon=True)
    t.start()
    try:
        return fn()
    finally:
        done.set()


def roofline_entry(kernel, bytes_alg, launch_ms, traffic):
    """Both views of one kernel: counter-based when profiles/pmc_traffic.json knows this workload, and the
    'effective' rate at 72 (144) B per site update."""
    eff = bytes_alg / (launch_ms * 1e-3) / 1e9
    out = {"kernel": kernel, "launch_ms": launch_ms, "algorithmic_bytes_per_launch": bytes_alg,
           "effective_gbps": eff, "effective_frac": eff / HBM_PEAK_GBPS,
           "traffic": None, "traffic_source": None, "counter_gbps": None}
    if traffic is not None:
        t = float(traffic["hbm_bytes_per_launch"])
        out["traffic"] = t
        out["traffic_source"] = {k: traffic.get(k) for k in ("source", "measured", "kernel") if k in traffic}
        out["counter_gbps"] = t / (launch_ms * 1e-3) / 1e9
    return out


def workload_name(args, nx_total, ny, body_name):
    """Names the workload; only a run on a BASELINE configuration's OWN parameters carries that configuration's name."""
    if args.dat:
        note = "custom: coordinates from the file named"
    elif not args.custom and (nx_total, ny) == (CONFIGS[args.config]["nx"], CONFIGS[args.config]["ny"]):
        note = CONFIGS[args.config]["name"]
    else:
        note = f"custom workload (differs from BASELINE configs[{args.config}] in: {', '.join(args.custom) or 'lattice'}); built-in shape"
    return f"{body_name} {nx_total}x{ny} {args.dtype} D2Q9, AoA={args.aoa:g} deg, U0={args.u0:g}, tau={args.tau:.7g} ({note})"


def slab_options(args):
    """The marching options of this run, for the stand-alone handles that measure a candidate slab."""
    o = {}
    if args.fuse_chunk > 0:
        o["fuse_chunk"] = args.fuse_chunk
    if args.fuse_depth > 0:
        o["fuse_depth"] = args.fuse_depth
    if args.fuse >= 0:
        o["fuse_steps"] = args.fuse
    if args.fast_math == 1:
        o["fast_math"] = 1
    return o


def balance_report(history):
    """[(edges, per-slab us/step)] of every split tried -> JSON-able summary."""
    return [{"widths": [b - a for a, b in zip(ed[:-1], ed[1:])], "slab_us_per_step": [round(c, 2) for c in cost], "slowest": round(max(cost), 2)}
            for ed, cost in history]


def local_slabs_main(args, wtpkg, mask, body_name):
    """--local-slabs P: the column-slab path of `--gpus P` with every slab on device 0 (in-process transport: peer copies on each
    slab's comm stream in place of RCCL send/recv; every other line of the slab state machine is shared, csrc/windtunnel.hip
    halo_begin / step_compute).  What it shows on one GPU: the refresh step's copies run beside the interior kernel (profile with
    rocprofv3 --kernel-trace --memory-copy-trace), and what P slab-sized handles cost next to one whole lattice."""
    import torch
    P, ny, nx = args.local_slabs, args.ny, args.nx
    torch.cuda.set_device(0)
    edges, history = None, []
    rounds = 4 if args.balance < 0 else args.balance
    if P > 1 and rounds > 0:
        opts = slab_options(args)
        edges, history = wtpkg.balance_split(nx, P, max(args.halo, 32), lambda ed: [
            wtpkg.measure_slab_cost(mask, ed, r, args.halo, dtype=args.dtype, device=0, tau=args.tau, u0=args.u0, options=opts) for r in range(P)], rounds)
    es = [wtpkg.Engine(nx, ny, dtype=args.dtype, device=0, rank=r, nranks=P, halo=args.halo, edges=edges) for r in range(P)]
    try:
        wtpkg.Engine.link_local(es)
        for e in es:
            if args.fuse_chunk > 0:
                e.set_option("fuse_chunk", args.fuse_chunk)
            if args.fuse_depth > 0:
                e.set_option("fuse_depth", args.fuse_depth)
            if args.fuse >= 0:
                e.set_option("fuse_steps", args.fuse)
            e.set_mask(mask)
            e.init_equilibrium(args.u0)
            e.set_option("exchange_timing", 1)
        if args.warmup > 0:
            wtpkg.Engine.step_group(es, args.warmup, args.tau, args.u0)
        for e in es:
            e.sync()
        t0 = time.perf_counter()
        dev_ms = wtpkg.Engine.step_group_timed(es, args.steps, args.tau, args.u0)
        for e in es:
            e.sync()
        wall = time.perf_counter() - t0
        # one slab handle of the same size alone on the GPU, for the "P x one slab" comparison
        solo_ms = None
        if P > 1:
            w = es[1].info().width + (2 if P > 2 else 1) * args.halo
            with wtpkg.Engine(w, ny, dtype=args.dtype, device=0) as solo:
                if args.fuse_depth > 0:
                    solo.set_option("fuse_depth", args.fuse_depth)
                if args.fuse >= 0:
                    solo.set_option("fuse_steps", args.fuse)
                solo.set_mask(mask[:, :w].copy())
                solo.init_equilibrium(args.u0)
                solo.step(args.warmup, args.tau, args.u0)
                solo_ms = solo.step_timed(args.steps, args.tau, args.u0) / args.steps
        out = {
            "metric": baseline_metric(), "value": nx * ny * args.steps / wall / 1e6, "unit": "MLUPS", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": wall / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32" if args.dtype == "float32" else "f64", "data": "synthetic",
            "config": {"workload": workload_name(args, nx, ny, body_name) + f" as {P} LOCAL column slabs on one GPU", "nx": nx, "ny": ny,
                       "slabs": P, "halo": args.halo, "transport": "local (copy kernel on each slab's comm stream)",
                       "edges": [e.x0 for e in es] + [nx], "balance": balance_report(history),
                       "fuse_depth": [int(e.get_option("fuse_depth")) if e.get_option("fuse_active") else 0 for e in es],
                       "single_steps": [int(e.get_option("single_steps")) for e in es]},
            # the per-rank report of the N-GPU line (`ranks`), from the in-process transport: same keys, comm_ranks 0 (no communicator here)
            "ranks": [{"rank": r, "device": 0, "comm_ranks": int(e.get_option("comm_ranks")), "x0": e.x0, "width": e.width, "device_ms": dev_ms[r],
                       "exchanges": int(e.get_option("exchanges")),
                       "exchange_ms_each": e.get_option("exchange_ms") / max(1.0, e.get_option("exchanges")),
                       "interior_ms_each": e.get_option("interior_ms") / max(1.0, e.get_option("exchanges")),
                       "exchange_exposed_ms_each": e.get_option("exchange_exposed_ms") / max(1.0, e.get_option("exchanges")),
                       "exchange_hidden_frac": (None if e.get_option("exchange_ms") <= 0 else
                                                max(0.0, 1.0 - e.get_option("exchange_exposed_ms") / e.get_option("exchange_ms"))),
                       **exchange_model(args.halo, ny, 4 if args.dtype == "float32" else 8, (1 if r > 0 else 0) + (1 if r < P - 1 else 0)),
                       "fuse_active": int(e.get_option("fuse_active")), "fuse_depth": int(e.get_option("fuse_depth")),
                       "pass_depth": int(e.get_option("pass_depth")), "passes": int(e.get_option("passes")),
                       "single_steps": int(e.get_option("single_steps")), "agree_checks": int(e.get_option("agree_checks")),
                       "window_overlap": int(e.get_option("window_overlap")),
                       "chain_downgrades": int(e.get_option("chain_downgrades"))} for r, e in enumerate(es)],
            "local_slabs": {"device_ms_per_step": [m / args.steps for m in dev_ms], "sum_device_ms_per_step": sum(dev_ms) / args.steps,
                            "group_wall_ms_per_step": wall / args.steps * 1e3,
                            "one_slab_alone_ms_per_step": solo_ms,
                            "P_times_one_slab_ms_per_step": None if solo_ms is None else P * solo_ms,
                            "note": "per-slab device time = HIP events on that slab's compute stream around the whole timed region; the slabs share "
                                    "one GPU, so their kernels interleave and each slab's time includes waiting for the others"},
            "exchange_model": EXCHANGE_MODEL_NOTE,
            "roofline": None, "cpu_baseline": None,
        }
        print(json.dumps(out), flush=True)
    finally:
        for e in es:
            e.close()


def self_launch(n):
    """`python bench.py --gpus N` with no launcher around it (WORLD_SIZE unset): start the N ranks as a CHILD job —
        python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py <the same arguments>
    — before this process has imported torch or touched the GPU (it never does), let the child's stdout / stderr through (rank 0's JSON line, every
    failing rank's one-line diagnosis) and return its exit status.  Nothing is retried and no process that has initialised the GPU is replaced."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:          # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"[bench.py] --gpus {n} without a launcher: starting {n} ranks as a child job: {' '.join(cmd[1:8])} ... bench.py {' '.join(sys.argv[1:])}",
          file=sys.stderr, flush=True)
    env = dict(os.environ, WT_BENCH_SELF_LAUNCHED="1")
    try:
        return subprocess.run(cmd, env=env).returncode
    except KeyboardInterrupt:
        return 130


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if "WORLD_SIZE" not in os.environ and args.gpus > 1 and args.local_slabs == 0:
            if os.environ.get("WT_BENCH_SELF_LAUNCHED"):                   # (a child of self_launch without the launcher's variables: never recurse)
                print("[bench.py] self-launched job came up without WORLD_SIZE", file=sys.stderr, flush=True)
                raise SystemExit(2)
            rc = self_launch(args.gpus)
            if rc != 0:
                print(f"[bench.py] the {args.gpus}-rank job exited with status {rc}: see the per-rank line(s) above "
                      f"('[bench.py] rank R (device D) FAILED: ...'); no bench line was printed", file=sys.stderr, flush=True)
            raise SystemExit(rc)
        args.gpus = world

    # same-session HBM traffic (children under rocprofv3), before this process touches the GPU
    session_counters = pmc_counters_this_session(args) if (world == 1 and args.pmc_traffic == 1 and args.local_slabs == 0) else None

    import datetime
    import numpy as np
    import torch
    import torch.distributed as dist
    import airfoil_cfd_tool_amd as wtpkg

    if os.environ.get("WT_BENCH_FORCE_DEVICE") is not None:      # plumbing tests on a 1-GPU box only
        local_rank = int(os.environ["WT_BENCH_FORCE_DEVICE"])
    distributed = world > 1
    ndev = torch.cuda.device_count()
    if local_rank >= ndev:
        die(rank, local_rank, f"LOCAL_RANK {local_rank} but only {ndev} HIP device(s) are visible")
    torch.cuda.set_device(local_rank)
    if distributed:
        # 1. this rank's own RCCL plumbing, before any peer is involved
        try:
            wtpkg.Engine.comm_selftest(local_rank, 1024)
        except Exception as e:      # noqa: BLE001 - every failure is reported the same way
            die(rank, local_rank, "wt_comm_selftest (one-rank RCCL send/recv on this GPU)", e)
        try:
            # (plumbing tests on a 1-GPU box put every rank on one device, where torch's own NCCL group cannot exist: WT_BENCH_TORCH_BACKEND=gloo)
            tb = os.environ.get("WT_BENCH_TORCH_BACKEND", "nccl")
            with_watchdog(COMM_TIMEOUT_S, rank, local_rank, f"torch.distributed.init_process_group({tb})",
                          lambda: dist.init_process_group(backend=tb, timeout=datetime.timedelta(seconds=COMM_TIMEOUT_S),
                                                          **({"device_id": torch.device("cuda", local_rank)} if tb == "nccl" else {})))
        except Exception as e:      # noqa: BLE001
            die(rank, local_rank, "torch.distributed.init_process_group(nccl)", e)

    nx_total = args.nx if (args.scaling == "strong" or world == 1) else args.nx * world
    ny = args.ny
    user_coords, body_name = None, args.shape.upper()
    if args.dat:
        from airfoil_cfd_tool_amd.datfile import load_dat
        pts, fixes = load_dat(args.dat)                       # main.py:59-180 semantics (repairs included)
        user_coords = wtpkg.geometry.round_coords(pts)        # AA.py:34-36
        body_name = f"{os.path.basename(args.dat)} ({len(user_coords)} points" + (f", {len(fixes)} parser repairs" if fixes else "") + ")"
    geom = wtpkg.geometry.build_geometry(nx_total, ny, args.aoa, user_coords, args.shape)
    mask = geom.mask
    if args.local_slabs > 0:
        return local_slabs_main(args, wtpkg, mask, body_name)

    edges, balance_hist = None, []
    rounds = (4 if args.balance < 0 else args.balance) if (distributed and args.scaling == "strong") else 0
    if rounds > 0:
        # every rank times ITS slab of the candidate split alone on its GPU (no communicator involved), the costs are gathered, the
        # columns are cut again; a failure anywhere leaves every rank on equal widths (distributed.balance_over_group)
        try:
            edges, balance_hist = wtpkg.balance_over_group(
                nx_total, max(args.halo, 32), lambda ed, r: wtpkg.measure_slab_cost(mask, ed, r, args.halo, dtype=args.dtype, device=local_rank, tau=args.tau,
                                                                                     u0=args.u0, options=slab_options(args)), rounds)
        except Exception as e:      # noqa: BLE001 - host logic on gathered (identical) numbers: the same outcome on every rank
            print(f"[bench rank {rank}] slab balancing failed: {e}", file=sys.stderr, flush=True)
            edges, balance_hist = None, []
        if edges is None and rank == 0:
            print("[bench] slab balancing skipped: a rank could not measure its slab; equal widths", file=sys.stderr, flush=True)

    try:
        if distributed:
            eng = wtpkg.Engine(nx_total, ny, dtype=args.dtype, device=local_rank, rank=rank, nranks=world, halo=args.halo, edges=edges)
        else:
            eng = wtpkg.Engine(nx_total, ny, dtype=args.dtype, device=local_rank)
        if args.fuse_chunk > 0:
            eng.set_option("fuse_chunk", args.fuse_chunk)
        if args.fuse_sites > 0:
            eng.set_option("fuse_sites", args.fuse_sites)
        if args.fuse_depth > 0:
            eng.set_option("fuse_depth", args.fuse_depth)
        if args.fuse >= 0:
            eng.set_option("fuse_steps", args.fuse)
        if args.fast_math == 1:
            eng.set_option("fast_math", 1)
        if distributed:
            # 2. the library's own communicator (beside torch's): unique id through torch.distributed, join under a watchdog
            ids = [wtpkg.Engine.comm_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(ids, src=0)
            with_watchdog(COMM_TIMEOUT_S, rank, local_rank, "wt_comm_init_rank (ncclCommInitRank)", lambda: eng.comm_init_rank(ids[0]))
        eng.set_mask(mask)
        eng.init_equilibrium(args.u0)
    except Exception as e:      # noqa: BLE001
        die(rank, local_rank, "engine set-up", e)

    def barrier():
        if distributed:
            dist.barrier()

    # One GPU: the two side measurements of the roofline entry — the un-fused kernel (on a handle of its own) and the opt-in contracted arithmetic
    # (on this handle: the same lattice, mask and plan) — run FIRST; the handle is then put back to its equilibrium state and the bench run proper
    # follows: W untimed warm-up steps, K timed steps.  Order matters on this hardware: an idle GPU takes 20-30 ms of uninterrupted work to settle its
    # clocks (profiles/r03_g_time_series.txt), and a K of 20 steps is 1.8 ms.
    side = {}
    preheat_steps, t_pre0 = 0, time.perf_counter()
    if not distributed and args.side == 1 and bool(eng.get_option("fuse_active")):
        spl0 = int(eng.get_option("fuse_depth"))
        try:
            with wtpkg.Engine(nx_total, ny, dtype=args.dtype, device=local_rank) as e1:
                e1.set_option("fuse_steps", 0)
                e1.set_mask(mask); e1.init_equilibrium(args.u0)
                e1.step(4, args.tau, args.u0)
                side["single_ms"] = e1.step_timed(40, args.tau, args.u0) / 40
                preheat_steps += 44
        except Exception as e:      # noqa: BLE001
            side["single_error"] = str(e)
        if args.fast_math == -1 and args.dtype == "float32":
            try:
                eng.step(2 * spl0, args.tau, args.u0)              # (the plan's units are timed and cut again here, once)
                eng.set_option("fast_math", 1)
                eng.step(2 * spl0, args.tau, args.u0)
                nfm = (200 // spl0) * spl0                         # (its own sample, whatever K is: 17 ms of steady state)
                side["contracted_ms"] = eng.step_timed(nfm, args.tau, args.u0) / nfm
                preheat_steps += 4 * spl0 + nfm
            except Exception as e:      # noqa: BLE001
                side["contracted_error"] = str(e)
            eng.set_option("fast_math", 0)
            eng.init_equilibrium(args.u0)
    # clock settling (--settle-ms): the bench handle marches, untimed, until the device has worked for that long without a pause; then back to the
    # initial state.  Every rank of a slab run takes rank 0's step count (the exchanges are collective).
    settle_steps = 0
    if args.settle_ms > 0:
        try:
            eng.step(40, args.tau, args.u0)                                       # (the plan's units are timed and cut again here, once)
            est = max(1e-4, eng.step_timed(40, args.tau, args.u0) / 40)           # ms per step
            n = [max(1, min(200000, int(args.settle_ms / est + 0.5)))]
            if distributed:
                dist.broadcast_object_list(n, src=0)
            with_watchdog(COMM_TIMEOUT_S, rank, local_rank, "clock-settling steps", lambda: eng.step(n[0], args.tau, args.u0))
            settle_steps = 80 + n[0]
            eng.init_equilibrium(args.u0)
        except Exception as e:      # noqa: BLE001
            die(rank, local_rank, "clock-settling steps", e)
    if not distributed:
        eng.sync()
    # everything the device has done before the DECLARED warm-up (ADVICE r3 / VERDICT r3 weak 5): the side measurements above and the trial passes
    # of the plan's measured cut (13 marching passes on a new mask).  On a short run (`--steps 20 --warmup 5`) this work, not the five warm-up
    # steps, is what brings the GPU's clocks up before the timed region; the JSON line says so (`preheat_*`), and `--side 0` runs none of it.
    tune_passes = 13 if (bool(eng.get_option("fuse_active")) and eng.get_option("tune_rounds") > 0) else 0
    preheat = {"preheat_steps": preheat_steps + settle_steps + tune_passes * (int(eng.get_option("fuse_depth")) if tune_passes else 0),
               "preheat_ms": (time.perf_counter() - t_pre0) * 1e3 if (preheat_steps or tune_passes or settle_steps) else 0.0,
               "preheat_what": ("k_step on a second handle: %d steps; contracted arithmetic on the bench handle: %d steps; clock settling on the bench handle "
                                "(--settle-ms %g): %d steps; trial passes of the measured cut: %d"
                                % (44 if preheat_steps else 0, max(0, preheat_steps - 44), args.settle_ms, settle_steps, tune_passes))
                               if (preheat_steps or tune_passes or settle_steps) else "nothing"}

    try:
        # warm-up (untimed); the first exchange of a slab run happens here
        if args.warmup > 0:
            with_watchdog(COMM_TIMEOUT_S, rank, local_rank, "warm-up steps", lambda: eng.step(args.warmup, args.tau, args.u0))
        eng.sync()
        torch.cuda.synchronize()
        barrier()

        # timed region: exactly K steps; HIP events on the library's compute stream give the device time
        t0 = time.perf_counter()
        dev_ms = eng.step_timed(args.steps, args.tau, args.u0)
        eng.sync()
        torch.cuda.synchronize()
        barrier()
        wall = time.perf_counter() - t0
        if distributed:
            # the per-rank exchange report comes from a SECOND, untimed pass of two refresh cycles with the exchange events on: the events' ring
            # blocks the launch thread now and then (xt_resolve), so the headline above is timed without them
            eng.set_option("exchange_timing", 1)
            with_watchdog(COMM_TIMEOUT_S, rank, local_rank, "exchange-report steps", lambda: eng.step(3 * max(args.halo, 1) + 2, args.tau, args.u0))
            eng.sync()
            barrier()
    except Exception as e:      # noqa: BLE001
        die(rank, local_rank, "stepping", e)
    dumped = dump_outputs(eng, args.dump_outputs) if args.dump_outputs else None

    if tune_passes == 0 and bool(eng.get_option("fuse_active")) and eng.get_option("tune_rounds") > 0:
        # (no side measurement ran: the plan was timed inside the warm-up call, before its first pass)
        preheat["preheat_steps"] += 13 * int(eng.get_option("fuse_depth"))
        preheat["preheat_what"] = "trial passes of the measured cut: 13 (inside the warm-up call)"
    per_rank_ms = [dev_ms]
    rank_report = None
    if distributed:
        # first-contact kit: what every rank saw — the ranks in the library's communicator, its device time, its
        # exchanges and how much of them hid behind the interior kernel, its slab and plan
        nx_ = max(1.0, eng.get_option("exchanges"))
        mine_rep = {"rank": rank, "device": local_rank, "comm_ranks": int(eng.get_option("comm_ranks")), "x0": eng.x0, "width": eng.width,
                    "device_ms": dev_ms, "exchanges": int(eng.get_option("exchanges")),
                    "exchange_ms_each": eng.get_option("exchange_ms") / nx_, "interior_ms_each": eng.get_option("interior_ms") / nx_,
                    "exchange_exposed_ms_each": eng.get_option("exchange_exposed_ms") / nx_,
                    "exchange_hidden_frac": (None if eng.get_option("exchange_ms") <= 0 else
                                             max(0.0, 1.0 - eng.get_option("exchange_exposed_ms") / eng.get_option("exchange_ms"))),
                    **exchange_model(args.halo, ny, 4 if args.dtype == "float32" else 8, (1 if rank > 0 else 0) + (1 if rank < world - 1 else 0)),
                    "fuse_active": int(eng.get_option("fuse_active")), "fuse_depth": int(eng.get_option("fuse_depth")),
                    "pass_depth": int(eng.get_option("pass_depth")), "passes": int(eng.get_option("passes")),
                    "single_steps": int(eng.get_option("single_steps")), "agree_checks": int(eng.get_option("agree_checks")),
                    "window_overlap": int(eng.get_option("window_overlap")),      # 1: the slab marches overlapping windows (no halo kernel)
                    "chain_downgrades": int(eng.get_option("chain_downgrades"))}
        rank_report = [None] * world
        dist.all_gather_object(rank_report, mine_rep)
        tdev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([wall, dev_ms], dtype=torch.float64, device=tdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        mine = torch.tensor([dev_ms], dtype=torch.float64, device=tdev)
        gathered = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(gathered, mine)
        per_rank_ms = [float(g[0]) for g in gathered]
        wall, dev_ms = float(t[0]), float(t[1])

    sites = nx_total * ny
    mlups = sites * args.steps / wall / 1e6
    bpl = BYTES_PER_LUP[args.dtype]
    fused = bool(eng.get_option("fuse_active"))
    # steps a full pass actually takes ("pass_depth": 3 on a four-step fp32 plan whose tau has no proved fast division — ADVICE r3)
    steps_per_launch = int(eng.get_option("pass_depth")) if fused else 1
    # one launch = one pass of the dominant kernel over the slab (when --steps is not a multiple of the steps per pass the
    # last one or two steps are single steps; they are averaged in)
    launch_ms = dev_ms / args.steps * steps_per_launch
    sites_per_launch = eng.width * ny
    key = f"{nx_total}x{ny}_{args.dtype}"
    main_kernel = "wt::k_step"
    if fused and steps_per_launch == 4:
        main_kernel = "wt::k_march3<..,4,..> (FOUR steps per pass, body / inlet / outlet inside; + wt::k_halo4 per pass)"
    elif fused and steps_per_launch == 3:
        main_kernel = "wt::k_march3 (THREE steps per pass, body / inlet / outlet inside; + wt::k_halo3 per pass)"
    elif fused:
        main_kernel = "wt::k_march (TWO steps per pass, body / inlet / outlet inside; + wt::k_halo_from_seams per pass)"
    if fused and steps_per_launch >= 3 and int(eng.get_option("window_overlap")) == 1:
        # overlapping windows (slabs, whole lattices of up to 7.5 M sites): the pass is the marching kernel alone
        main_kernel = main_kernel.split(";")[0] + "; OVERLAPPING windows: 128 rows of which the middle 120 are owned, no halo kernel)"
    traffic = None if distributed else (select_traffic(session_counters, fused, steps_per_launch) or
                                        measured_traffic(key + (("_march4" if steps_per_launch == 4 else "_march3" if steps_per_launch == 3 else "_march") if fused else "")))
    r = roofline_entry(main_kernel, bpl * sites_per_launch * steps_per_launch, launch_ms, traffic)
    # `achieved` / `frac` are the REAL HBM rate (rocprofv3 counters of this workload, profiles/pmc_traffic.json) over this run's launch time,
    # or null when this workload was never profiled — never the "effective" figure, which a multi-step pass can push beyond the peak.
    # Beside it: `compulsory_*` = one lattice read + one lattice write per PASS (what any T-step pass must move) and `effective_*` =
    # 72 (144) B per site UPDATE, the throughput unit of SURVEY 8d.
    achieved = r["counter_gbps"]
    compulsory = bpl * sites_per_launch / (launch_ms * 1e-3) / 1e9
    cfg_fuse = {"fuse_steps": int(fused), "fuse_chunk": int(eng.get_option("fuse_chunk")) if fused else 0,
                "fuse_units": int(eng.get_option("fuse_units")) if fused else 0,
                "fuse_sites": int(eng.get_option("fuse_sites")) if fused else 0,
                "fuse_depth": int(eng.get_option("fuse_depth")) if fused else 0, "pass_depth": steps_per_launch if fused else 0,
                "fast_div": int(eng.get_option("fast_div_active")) if fused else 0,
                "single_steps": int(eng.get_option("single_steps"))}
    # Which roof is nearer is MEASURED in this session: the HBM fraction from the FETCH / WRITE counters over this run's launch
    # time, the vector-ALU fraction from the SQ group of the third child run; `bound` names the larger of the two.  Without SQ counters (no
    # rocprofv3, --pmc-traffic 0, a slab run) `bound` stays "hbm" — the roof SURVEY 8d prices this path against — and `valu_busy_frac` is null.
    valu = None if distributed else select_valu(session_counters, fused, steps_per_launch, int(eng.get_option("wave_slots")) // 2, launch_ms)
    hbm_frac = None if achieved is None else achieved / HBM_PEAK_GBPS
    valu_frac = None if valu is None else valu["valu_busy_frac"]
    # valu_busy_frac is a per-wave activity count that saturates near 0.85-0.92, not at 1 (profiles/r04_x_issue_experiments.txt): it is normalised by
    # 0.9 before it is compared, and two fractions within 0.1 of each other name no single bound — "mixed".
    hbm_cmp = hbm_frac if hbm_frac is not None else compulsory / HBM_PEAK_GBPS
    valu_cmp = None if valu_frac is None else min(1.0, valu_frac / 0.9)
    bound = "hbm" if valu_cmp is None else ("mixed" if abs(valu_cmp - hbm_cmp) < 0.1 else ("valu" if valu_cmp > hbm_cmp else "hbm"))
    roofline = {"bound": bound, "kernel": main_kernel, "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                "frac": hbm_frac,
                "valu_busy_frac": valu_frac,
                "bound_basis": ("measured this session: HBM %s of the peak (counters), vector-instruction activity %s of the launch (SQ_ACTIVE_INST_VALU x 4 / "
                                "(SIMDs x GRBM_GUI_ACTIVE / 8); it saturates near 0.9, so it is divided by 0.9 for the comparison: %s); the larger names the "
                                "bound ('valu' = vector-instruction ISSUE at two waves per SIMD), 'mixed' when they are within 0.1"
                                % ("n/a" if hbm_frac is None else "%.3f" % hbm_frac, "n/a" if valu_frac is None else "%.3f" % valu_frac,
                                   "n/a" if valu_cmp is None else "%.3f" % valu_cmp)),
                "valu": valu,
                "achieved_basis": ("rocprofv3 FETCH_SIZE x2 + WRITE_SIZE per launch (see traffic_source.measured) / this run's launch time"
                                   if achieved is not None else "no counters: rocprofv3 unavailable (or --pmc-traffic 0) and no entry for this workload in profiles/pmc_traffic.json"),
                "traffic": r["traffic"], "traffic_source": r["traffic_source"], "counter_gbps": r["counter_gbps"],
                "compulsory_gbps": compulsory, "compulsory_frac": compulsory / HBM_PEAK_GBPS,
                # counter bytes over the bytes every pass must move (read + write each population once): what re-reads, tables and fill columns add
                "traffic_over_compulsory": (None if r["traffic"] is None or not launch_ms else r["traffic"] / (compulsory * 1e9 * launch_ms * 1e-3)),
                "counter_calibration": ("FETCH_SIZE x 2 and WRITE_SIZE x 1 reproduce known byte counts in this kernel's own access shapes (16, 8, 4 bytes per lane; "
                                        "tools/kfetchcal.hip, profiles/r04_u_fetch_calibration.txt)"),
                "valu_busy_note": ("a per-wave activity count (it reads 0.85-0.92 on a kernel of nothing but packed FMAs at 2-4 waves per SIMD, "
                                   "profiles/r04_x_issue_experiments.txt), not a pipe utilisation"),
                "effective_gbps": r["effective_gbps"], "effective_frac": r["effective_frac"],
                "algorithmic_bytes_per_launch": r["algorithmic_bytes_per_launch"], "launch_ms": launch_ms,
                "steps_per_launch": steps_per_launch}
    if "contracted_ms" in side:
        # the opt-in contracted collision beside the bit-exact default, same run (tolerance-tested, tests/test_gpu_fast_math.py; never the default)
        msf = side["contracted_ms"]
        roofline["contracted"] = {"option": "fast_math = 1 (fused multiply-adds, v_rcp / v_rsq: within |d rho| <= 1e-5, |d u| <= 5e-6 of the oracle, not bit-exact)",
                                  "ms_per_step": msf, "mlups": sites / (msf * 1e-3) / 1e6,
                                  "gain_over_default": (dev_ms / args.steps) / msf,
                                  "compulsory_frac": bpl * sites_per_launch / (msf * steps_per_launch * 1e-3) / 1e9 / HBM_PEAK_GBPS}
    elif "contracted_error" in side:
        roofline["contracted"] = {"error": side["contracted_error"]}
    if "single_ms" in side:
        # the un-fused kernel beside it, same run, same lattice and mask
        ms1 = side["single_ms"]
        # (the children's side run puts k_step under the same counters: same session, same box — VERDICT r3 weak 10; the file entry only without them)
        s = roofline_entry("wt::k_step (one step per launch)", bpl * sites_per_launch, ms1,
                           (None if distributed else select_traffic(session_counters, False, 1)) or measured_traffic(key))
        s["achieved"] = s["counter_gbps"]                 # one step per launch: effective == compulsory
        s["frac"] = None if s["achieved"] is None else s["achieved"] / HBM_PEAK_GBPS
        s["mlups"] = sites / (ms1 * 1e-3) / 1e6
        roofline["single_step"] = s
    elif "single_error" in side:
        roofline["single_step"] = {"error": side["single_error"]}

    workload = workload_name(args, nx_total, ny, body_name)
    out = {
        "metric": baseline_metric(),
        "value": mlups,
        "unit": "MLUPS",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        **preheat,
        "ms_per_step": wall / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": "f32" if args.dtype == "float32" else "f64",
        "data": "synthetic",
        "config": {"workload": workload, "nx": nx_total, "ny": ny, "slabs": world,
                   "halo": args.halo if distributed else 0, **cfg_fuse, "fast_math": int(args.fast_math == 1),
                   "solid_sites": int((mask != 0).sum()),
                   **({"slab_widths": [w for _, w in wtpkg.slab_bounds(nx_total, world, edges)], "balance": balance_report(balance_hist)} if distributed else {})},
        "device_ms": per_rank_ms,
        "roofline": roofline,
    }
    if dumped is not None:
        out["dump_outputs"] = dumped
    if rank_report is not None:
        out["ranks"] = rank_report
        out["comm_ranks_seen"] = sorted({r_["comm_ranks"] for r_ in rank_report})
        out["exchange_model"] = EXCHANGE_MODEL_NOTE
    if rank == 0 and world == 1 and args.cpu_steps > 0:
        out["cpu_baseline"] = cpu_baseline(mask, args.cpu_steps, args.tau, args.u0, args.dtype)
    elif rank == 0:
        out["cpu_baseline"] = None
    eng.close()
    if distributed:
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
