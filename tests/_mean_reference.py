"""NumPy reference of the mean fields of batched sweeps (wtp_enable_mean, include/wt_polar.h).

Definition: for member m and cell (i, j), let rho, ux, uy be what wtp_read_macro would return after a sampled step, converted
exactly to double.  Solid and boundary cells are included; no cell is special-cased.  The device keeps seven running sums per
cell, in double, added in sample order: sum rho, sum ux, sum uy, sum rho*rho, sum ux*ux, sum uy*uy, sum ux*uy.  Each product is
one double multiplication, added as a separate operation; nothing is fused.  For fp32 members the products are exact in double;
for fp64 members they round once, as NumPy's do.  In both cases the seven sums are bit-identical to a NumPy loop over
wtp_read_macro at the sampled steps.  The device also keeps a per-member sample count n (int64).
"""
import numpy as np

SUMS = ("rho", "ux", "uy", "rho2", "ux2", "uy2", "uxuy")
EPS = 2.0 ** -53


def accumulate(samples):
    """The seven sums and n of a list of (rho, ux, uy) triples ([NY][NX] each, float32 or float64), added in list order."""
    first = np.asarray(samples[0][0])
    s = {k: np.zeros(first.shape, np.float64) for k in SUMS}
    n = 0
    for rho, ux, uy in samples:
        r, u, v = (np.asarray(a).astype(np.float64) for a in (rho, ux, uy))      # (exact)
        s["rho"] = s["rho"] + r
        s["ux"] = s["ux"] + u
        s["uy"] = s["uy"] + v
        s["rho2"] = s["rho2"] + r * r
        s["ux2"] = s["ux2"] + u * u
        s["uy2"] = s["uy2"] + v * v
        s["uxuy"] = s["uxuy"] + u * v
        n += 1
    return {"n": n, **s}


def moment_bound(n, a_abs_max, b_abs_max):
    """Bound on |(S_ab / n - mean_a mean_b) - cov(a, b)| where cov is the two-pass central moment mean((a - mean a)(b - mean b))
    (np.var for a = b), for n samples with |a| <= A, |b| <= B, every operation in double with unit roundoff u = 2^-53:
      * one pass.  A sum of n terms added in order errs by at most (n - 1) u times the sum of the terms' magnitudes, each product
        a_k b_k by u A B more: |dS_ab| <= n u (n A B), so S_ab / n errs by (n + 1) u A B with its division; the means err by
        n u A and n u B, their product by (2 n + 1) u A B; the subtraction rounds a value of at most 2 A B: (3 n + 4) u A B.
        The difference S_ab / n - mean_a mean_b cancels, so these absolute errors stay whatever the moment's size.
      * two passes.  The mean errs by at most n u A, a deviation (magnitude <= 2 A) by (n + 2) u A, a product of deviations
        (magnitude <= 4 A B) by (4 n + 12) u A B, their mean by (4 n + 4) u A B more: (8 n + 16) u A B.
    Together (11 n + 20) u A B to first order in u, rounded up to 12 (n + 2) u A B.  It is the noise floor of the one-pass
    formula: at U0 = 0.06 and n = 256 about 1e-15, against u'u' of 1e-6 and more in a wake."""
    return 12.0 * (n + 2) * EPS * a_abs_max * b_abs_max


def mean_bound(n, a_abs_max):
    """|S_a / n - np.mean(a)| <= 2 n u A: either side adds n terms of magnitude <= A in some order and divides once."""
    return 2.0 * n * EPS * a_abs_max


def mean_flow_reference(samples, u0):
    """mean_flow's fields by NumPy's own two-pass mean and var over the stacked samples (the closed form the one-pass sums are
    checked against)."""
    r, u, v = (np.stack([np.asarray(s[k]).astype(np.float64) for s in samples]) for k in range(3))
    rho, ux, uy = r.mean(axis=0), u.mean(axis=0), v.mean(axis=0)
    uu, vv, rho_var = u.var(axis=0), v.var(axis=0), r.var(axis=0)
    uv = ((u - ux) * (v - uy)).mean(axis=0)
    q = 1.5 * u0 * u0
    return {"n": len(samples), "rho": rho, "ux": ux, "uy": uy, "uu": uu, "vv": vv, "uv": uv, "rho_var": rho_var,
            "cp_mean": (rho - 1.0) / q, "cp_rms": np.sqrt(rho_var) / q, "speed": np.hypot(ux, uy), "tke": 0.5 * (uu + vv)}
