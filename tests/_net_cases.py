"""Batched sweeps at the stability net: the cases, their inputs and the reference runs that tests/test_polar_net_host.py pins and
tests/test_gpu_polar_net.py compares the kernels with.  Test infrastructure only.

A case is a lattice (chosen by step_tile's tile classes, as in tests/test_gpu_polar_les.py), a configuration is a pair of wall rule
and collision: "les" (half-way walls, k_step_batch with COLLIDE_LES), "ibb-bgk" and "ibb-les" (interpolated walls, k_step_batch with WALL_INTERP and either
collision).  Every batch has the same three kinds of member: one driven onto the net with a weak model (cs > 0), one driven onto it
with cs = 0, one healthy.  These cases reach the net by stepping from equilibrium, as a sweep does: tau - 0.5 of 4e-4 and an inflow
of 0.31 against the velocity bound of 0.35, started impulsively on a body of blocks, slots and single cells.  (They were written when
the library had no way to write a state; since wtp_write_f, tests/_net_rough_cases.py puts every step kernel on the net in its first
step from a written start, on these masks and wall distances.)

The reference of a member is lbm_numpy.run (cs = 0, half-way walls), _les_reference or _ibb_reference, stepped one step at a time so
that the events of every step are seen: an event is an interior fluid cell whose stored moments sit at a bound (rho == 0.5, rho == 2.0
in the lattice's precision; |u|^2 >= 0.35^2 (1 - 1e-6) in double: lbm_numpy.clamp_events' rules).
"""
import functools

import numpy as np

import lbm_numpy
import _ibb_reference as ibb
import _les_reference as les
from _mex_reference import link_masks

CASES = {
    "96x48-f32": (96, 48, "float32"),            # ragged tiles only: site_general
    "40x300-f32": (40, 300, "float32"),          # a FAST tile of 256 rows and a ragged one per column
    "37x299-f32": (37, 299, "float32"),          # the same with odd NX and NY
    "24x140-f64": (24, 140, "float64"),          # a FAST tile of 128 rows and a ragged one
}
CONFIGS = ("les", "ibb-bgk", "ibb-les")
# (tau, u0, cs): driven with a weak model, driven with cs = 0 (BGK inside the LES kernel), healthy.  cs is used by the "les" and
# "ibb-les" configurations only.
MEMBERS = [(0.5004, 0.31, 0.02), (0.5004, 0.32, 0.0), (0.9, 0.03, 0.1)]
DRIVEN, HEALTHY = (0, 1), 2
KINDS = ("u", "rho_max", "rho_min")              # in the order in which the checkpoints meet them
# Steps from equilibrium at the checkpoints: by the first every driven member has met the velocity bound, by the second rho = 2.0,
# by the third rho = 0.5, in every tile class of its lattice (tests/test_polar_net_host.py).
CHECKPOINTS = {name: (6, 60, 170) for name in CASES}


def net_mask(nx, ny, rng):
    """A body with narrow gaps, like test_gpu_polar_ibb._blob_mask: a block cut by one-cell slots (cells with a wall on either side,
    where a short link has no fluid cell behind it) and sprinkled with single solid cells.  Unlike that mask, the sprinkle around the
    block keeps to the block's columns and three either side, so the columns up- and downstream of it stay free of solid cells:
    their full tiles are TILE_FAST.  A second sprinkle in the last ten rows, across the lattice, lies in the ragged tile of the tall
    lattices.  The border cells stay fluid."""
    mask = np.zeros((ny, nx), np.uint8)
    j0, i0 = ny // 2 - 9 + int(rng.integers(0, 5)), nx // 3 + int(rng.integers(0, 3))
    h, w = 17, max(7, nx // 4)
    mask[j0:j0 + h, i0:i0 + w] = 255
    mask[j0 + 4, i0:i0 + w - 2] = 0                                    # a horizontal slot, open upstream
    mask[j0 + 9:j0 + h, i0 + 3] = 0                                    # a vertical slot, open at the top
    mask[j0 + 12, i0 + 5:i0 + w] = 0                                   # and one open downstream
    ja, jb, ia, ib = max(j0 - 5, 2), min(j0 + h + 5, ny - 2), max(i0 - 3, 2), min(i0 + w + 3, nx - 2)
    mask[ja:jb, ia:ib][rng.random((jb - ja, ib - ia)) < 0.12] = 255
    mask[ny - 11:ny - 2, 2:nx - 2][rng.random((9, nx - 4)) < 0.12] = 255
    mask[[0, 1, ny - 2, ny - 1], :] = 0
    mask[:, [0, 1, nx - 2, nx - 1]] = 0
    return mask


def random_q(nx, ny, dtype, rng):
    """Wall distances of test_gpu_polar_ibb._random_q's kind: (0, 1] in every entry, with exact 0.5, exact 1, values close to 0 and
    values either side of 0.5 among them."""
    q = 1.0 - rng.random((8, ny, nx))
    pick = rng.random(q.shape)
    q[pick < 0.10] = 0.5
    q[(pick >= 0.10) & (pick < 0.20)] = 1.0
    q[(pick >= 0.20) & (pick < 0.25)] = 2.0 ** -12
    q[(pick >= 0.25) & (pick < 0.30)] = np.nextafter(0.5, 0.0)
    q = q.astype(dtype)
    assert (q > 0).all() and (q <= 1).all()
    return q


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(masks [B][NY][NX], q [B][8][NY][NX] of the case's dtype), read-only."""
    nx, ny, dtype = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 101)
    masks = np.stack([net_mask(nx, ny, rng) for _ in MEMBERS])
    q = np.stack([random_q(nx, ny, dtype, rng) for _ in MEMBERS])
    masks.setflags(write=False)
    q.setflags(write=False)
    return masks, q


def interior_fluid(mask):
    inner = np.zeros(mask.shape, bool)
    inner[1:-1, 1:-1] = True
    return inner & (np.asarray(mask) == 0)


def fast_cells(mask, dtype):
    """[NY][NX] bool: the cells of TILE_FAST tiles, by k_classify's rule (csrc/step_fast.hpp).  A tile is TJ = 64 * (16 / sizeof(T))
    consecutive rows of one column; it is FAST when it is full (its rows end inside the lattice), its column is neither the inlet nor
    the outlet column, and no cell of columns i - 1 .. i + 1 in rows j0 - 1 .. j0 + TJ (those inside the lattice) is solid."""
    solid = np.asarray(mask) != 0
    ny, nx = solid.shape
    tj = 64 * (16 // np.dtype(dtype).itemsize)
    fast = np.zeros((ny, nx), bool)
    for j0 in range(0, ny - tj + 1, tj):
        rows = slice(max(j0 - 1, 0), min(j0 + tj, ny - 1) + 1)
        for i in range(1, nx - 1):
            if not solid[rows, i - 1:i + 2].any():
                fast[j0:j0 + tj, i] = True
    return fast


def cell_classes(mask, dtype):
    """{"fast", "general", "link"} -> [NY][NX] bool among the interior fluid cells: the cells that collide in the straight-line path
    of step_tile, those that collide in site_general, and those that own a link (all of them general)."""
    fluid, fast = interior_fluid(mask), fast_cells(mask, dtype)
    owner = np.zeros(fluid.shape, bool)
    for o in link_masks(mask)[1:]:
        owner |= o
    assert not (owner & fast).any()
    return {"fast": fluid & fast, "general": fluid & ~fast, "link": owner}


def event_cells(macro):
    """{"u", "rho_max", "rho_min"} -> [NY][NX] bool: the cells whose stored moments sit at that bound (lbm_numpy.clamp_events' rules)."""
    rho, ux, uy = macro
    T = rho.dtype.type
    u, v = ux.astype(np.float64), uy.astype(np.float64)
    return {"u": (u * u + v * v) >= lbm_numpy.U_MAX * lbm_numpy.U_MAX * (1 - 1e-6), "rho_max": rho == T(lbm_numpy.RHO_MAX),
            "rho_min": rho == T(lbm_numpy.RHO_MIN)}


def one_step(config, f, mask, tau, u0, cs, q, dtype):
    """One step of the member's reference.  Returns (f, macro, acts): acts [NY][NX] bool, where the model changed the relaxation
    (te != tau), None for a member without the model."""
    c = les.les_constant(cs, dtype)
    if config == "les":
        if cs == 0.0:
            fo, macro = lbm_numpy.step(f, mask, tau, u0)              # the BGK oracle itself
            return fo, macro, None
        fo, macro, te = les.step(f, mask, tau, u0, c)
        return fo, macro, te != te.dtype.type(tau)
    if config == "ibb-bgk" or cs == 0.0:
        fo, macro = ibb.step(f, mask, tau, u0, q, None if config == "ibb-bgk" else c)
        return fo, macro, None
    fo, macro = ibb.step(f, mask, tau, u0, q, c)
    # _ibb_reference does not return te: fo = fin - n / te differs from BGK's fin - n / tau on the same input exactly where te != tau
    # (and n != 0, which it is at a bound)
    plain, _ = ibb.step(f, mask, tau, u0, q, None)
    return fo, macro, (fo != plain).any(axis=0)


class MemberRun:
    """One member's reference run: states[k] = (f, (rho, ux, uy)) at checkpoint k; first[kind][cls] = the first step (1-based) after
    which a cell of that class sat at that bound, None if none did up to the last checkpoint; counted[k][kind][cls] = the number of
    (step, cell) pairs of that class at that bound up to checkpoint k; at_bound / acted = the number of (step, cell) pairs at a bound
    and of those where the model acted (cs > 0 members); finite = every population of every step was; max_abs = the largest |f|."""

    def __init__(self):
        self.states, self.finite, self.at_bound, self.acted, self.max_abs = [], True, 0, 0, 0.0
        self.first = {kind: {"fast": None, "general": None, "link": None} for kind in KINDS}
        self.counted = []


@functools.lru_cache(maxsize=None)
def reference(name, config):
    """[MemberRun] of the case's members under the configuration, every array read-only."""
    nx, ny, dtype = CASES[name]
    masks, q = inputs(name)
    marks = CHECKPOINTS[name]
    out = []
    for m, (tau, u0, cs) in enumerate(MEMBERS):
        if config == "ibb-bgk":
            cs = 0.0
        run = MemberRun()
        classes = cell_classes(masks[m], dtype)
        f, macro = lbm_numpy.equilibrium_init(nx, ny, u0, np.dtype(dtype))
        total = {kind: {cls: 0 for cls in classes} for kind in KINDS}
        for step in range(1, marks[-1] + 1):
            f, macro, acts = one_step(config, f, masks[m], tau, u0, cs, q[m], dtype)
            run.finite = run.finite and bool(np.isfinite(f).all())
            run.max_abs = max(run.max_abs, float(np.abs(f).max()))
            ev = event_cells(macro)
            for kind in KINDS:
                for cls, cells in classes.items():
                    n = int((ev[kind] & cells).sum())
                    total[kind][cls] += n
                    if run.first[kind][cls] is None and n:
                        run.first[kind][cls] = step
            if acts is not None:
                bound = (ev["u"] | ev["rho_max"] | ev["rho_min"]) & (classes["fast"] | classes["general"])
                run.at_bound += int(bound.sum())
                run.acted += int((bound & acts).sum())
            if step in marks:
                for a in (f, *macro):
                    a.setflags(write=False)
                run.states.append((f, macro))
                run.counted.append({kind: dict(total[kind]) for kind in KINDS})
        out.append(run)
    return out
