"""Sample reductions of batched sweeps past 1024 columns: the lattice, its members and what splits a reference's terms by the trip
of the kernels' final sum that adds them.  Test infrastructure only.

k_loads_batch, k_mex_batch and k_mex_ibb_batch end in a loop that passes NT = 1024 column partials at a time through LDS: the
partials of k_loads_batch are indexed by the column, those of the momentum exchange by the column's place in the member's window
(from the column before its first solid column, not below 1, to the one after its last, not above NX - 2).  A member whose partials
reach past index 1023 takes a second trip: the running sums are carried, the last trip is partial, the LDS array is used again.
"""
import math

import numpy as np

from _loads_reference import DIRS
from _mex_reference import link_masks

NT = 1024
NX, NY = 1100, 24
EVERY, CALLS = 12, 3
# (tau, u0) of: the long body, the short one, the member without a body
MEMBERS = [(0.6, 0.05), (0.7, 0.06), (0.58, 0.04)]


def masks():
    """[3][NY][NX]: a plate of four rows over columns 20 .. 1079 that is asymmetric past column 1024 (a step of four more rows on its
    upper side from column 1050 on, a notch in its lower side at columns 1060 .. 1069); a block of 20 x 8 cells; nothing."""
    m = np.zeros((len(MEMBERS), NY, NX), np.uint8)
    m[0, 10:14, 20:1080] = 1
    m[0, 14:18, 1050:1080] = 1
    m[0, 10:12, 1060:1070] = 0
    m[1, 8:16, 400:420] = 1
    return m


def short_mask():
    """What replaces the long body: a block whose window is 22 columns wide, far from member 1's."""
    m = np.zeros((NY, NX), np.uint8)
    m[7:13, 700:720] = 1
    return m


def refs():
    """A different off-centre reference point per member, none on a cell centre or a face."""
    n = len(MEMBERS)
    return [0.3641 * NX + 1.7 * m for m in range(n)], [0.5 * NY - 0.85 * m - 1.3 for m in range(n)]


def window(mask):
    """(first column, columns) of the member's momentum-exchange window; (1, 0) without a body."""
    cols = np.flatnonzero((np.asarray(mask) != 0).any(axis=0))
    if cols.size == 0:
        return 1, 0
    c0, c1 = max(int(cols[0]) - 1, 1), min(int(cols[-1]) + 1, mask.shape[1] - 2)
    return c0, c1 - c0 + 1


def loads_columns(mask):
    """The column (of the fluid cell, which is the partial's index) of every term of _loads_reference.loads_reference, in its order."""
    solid = np.asarray(mask) != 0
    ny, nx = solid.shape
    cols = []
    for dx, dy in DIRS:
        nb = np.zeros_like(solid)
        nb[max(-dy, 0):ny + min(-dy, 0), max(-dx, 0):nx + min(-dx, 0)] = solid[max(dy, 0):ny + min(dy, 0), max(dx, 0):nx + min(dx, 0)]
        cols.append(np.nonzero(~solid & nb)[1])
    return np.concatenate(cols)


def mex_columns(mask):
    """The column of every term of _mex_reference.mex_reference and _ibb_reference.mex_reference, in their order."""
    return np.concatenate([np.nonzero(own)[1] for own in link_masks(mask)[1:]])


def second_trip_loads(ref, mask):
    """The sum of the terms of a Loads whose column partial the second trip adds."""
    cols = loads_columns(mask)
    assert cols.size == ref.n
    return math.fsum(ref.tm[cols >= NT])


def second_trip_mex(ref, mask):
    """(fx, fy, mz): the sums of the terms of a Mex whose window partial the second trip adds."""
    idx = mex_columns(mask) - window(mask)[0]
    assert idx.size == ref.links and (idx >= 0).all() and (idx < window(mask)[1]).all()
    late = idx >= NT
    return math.fsum(ref.tx[late]), math.fsum(ref.ty[late]), math.fsum((ref.ta - ref.tb)[late])
