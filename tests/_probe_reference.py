"""NumPy reference of the probe points of batched sweeps (wtp_enable_probes, include/wt_polar.h "Probe points"), and the point sets that
tests/test_polar_probe_host.py (CPU) and tests/test_gpu_polar_probe.py (GPU) both use.

Definition: a point (x, y) in lattice units has the base cell and the weights of airfoil_cfd_tool_amd.polar.probe_weights, the rule the
library applies on the host.  For each of the three planes a in (rho, ux, uy) that wtp_read_macro returns, converted exactly to double,
    v = ((w00*a00 + w10*a10) + w01*a01) + w11*a11
with the cells (i0, j0), (i0+1, j0), (i0, j0+1), (i0+1, j0+1), one rounding per operation.  The device keeps the sum of v over the
samples, added in sample order, and a count.  An inactive point (x = NaN) is never sampled: NaN in a sample, +0 in the sums.
"""
import numpy as np

from airfoil_cfd_tool_amd.polar import probe_weights

PLANES = ("rho", "ux", "uy")
EPS = 2.0 ** -53
GPU_CASE = dict(nx=160, ny=80, alphas=(0.0, 8.0))          # the lattice and the angles of the GPU run_polar test, whose rakes the CPU test checks


def gather(plane, i0, j0, w, di=0, dj=0, swap=False):
    """The formula on one [NY][NX] plane.  di, dj and swap are the misreads a comparison has to notice: the base cell shifted by columns or
    rows, w10 and w01 exchanged."""
    a = np.asarray(plane).astype(np.float64)                               # (exact)
    i, j = i0 + di, j0 + dj
    w00, w10, w01, w11 = (w[0], w[2], w[1], w[3]) if swap else w
    return ((w00 * a[j, i] + w10 * a[j, i + 1]) + w01 * a[j + 1, i]) + w11 * a[j + 1, i + 1]


def sample(macro, x, y, planes=(0, 1, 2), **misread):
    """{"rho", "ux", "uy"}: one sample of macro = (rho, ux, uy) at the points, [P] float64, NaN at inactive points.  planes: which of the
    three fields each output reads (another order is a misread)."""
    ny, nx = np.asarray(macro[0]).shape
    i0, j0, w = probe_weights(x, y, nx, ny)
    on = i0 >= 0
    out = {}
    for name, k in zip(PLANES, planes):
        v = np.full(np.shape(x), np.nan)
        v[on] = gather(macro[k], i0[on], j0[on], w[:, on], **misread)
        out[name] = v
    return out


def accumulate(samples, x, y):
    """n and the three sums over a list of (rho, ux, uy) triples, added in list order; +0 at inactive points."""
    s = {k: np.zeros(np.shape(x)) for k in PLANES}
    on = ~np.isnan(np.asarray(x, np.float64))
    for macro in samples:
        one = sample(macro, x, y)
        for k in PLANES:
            s[k][on] = s[k][on] + one[k][on]
    return {"n": len(samples), **s}


def abs_terms(samples, x, y, k):
    """The sum over the samples and the four cells of |w a| for plane k at every point: what the rounding bounds scale with."""
    ny, nx = np.asarray(samples[0][0]).shape
    i0, j0, w = probe_weights(x, y, nx, ny)
    t = np.zeros(np.shape(x))
    for macro in samples:
        t += gather(np.abs(np.asarray(macro[k]).astype(np.float64)), np.maximum(i0, 0), np.maximum(j0, 0), w)
    return t


def point_set(nx, ny, npoints, mask, seed):
    """(x, y) [npoints]: the four extreme corners of the valid rectangle, a point on a cell centre, one on a vertical and one on a
    horizontal face, up to twenty points whose stencil touches solid cells of `mask`, three inactive points (their y holds what must
    not be read: NaN, a value far outside, a valid value) and points drawn uniformly from the rectangle, the last one among them.  With
    fewer than 40 points only the first of these fit; npoints = 1 is one random point."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, nx - 0.5, npoints)
    y = rng.uniform(0.5, ny - 0.5, npoints)
    if npoints < 40:
        return x, y
    fixed = [(0.5, 0.5), (nx - 0.5, 0.5), (0.5, ny - 0.5), (nx - 0.5, ny - 0.5),
             (nx // 3 + 0.5, ny // 3 + 0.5), (nx // 2 + 1.0, ny // 4 + 0.5), (nx // 4 + 0.5, ny // 2 + 1.0)]
    jj, ii = np.nonzero(np.asarray(mask)[1:-1, 1:-1])
    pick = rng.permutation(jj.size)[:20]
    fixed += [(ii[k] + 1 + rng.uniform(0.05, 0.95), jj[k] + 1 + rng.uniform(0.05, 0.95)) for k in pick]     # inside a solid cell: it is in the stencil
    for k, (px, py) in enumerate(fixed):
        x[8 + k], y[8 + k] = px, py
    for k, bad_y in zip((5, npoints // 2, npoints - 2), (np.nan, 1e9, 1.5)):
        x[k], y[k] = np.nan, bad_y
    return x, y


def touches_solid(x, y, mask):
    """Per point: its stencil holds a solid cell."""
    ny, nx = np.asarray(mask).shape
    i0, j0, _ = probe_weights(x, y, nx, ny)
    m = np.asarray(mask) != 0
    i, j = np.maximum(i0, 0), np.maximum(j0, 0)
    return (i0 >= 0) & (m[j, i] | m[j, i + 1] | m[j + 1, i] | m[j + 1, i + 1])
