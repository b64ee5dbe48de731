"""The gfx950 code object of csrc/polar.hip for the host tests that inspect it: compiled once per session, whichever test
module asks first."""
import functools
import os
import re
import sys

import pytest

from conftest import ROOT

BGK, LES, TRT, TRT_LES = range(4)       # COLL, d2q9.hpp
HALFWAY, INTERP = range(2)              # WALL
AXIAL, INCLINED, PROFILE = range(3)     # FAR
_STEP = re.compile(r"^_Z\d+k_step_(half_)?batchI([fd]?)((?:L[bi]\d+E)+)E")


def step_variant(name):
    """(storage, T, EMIT, COLL, WALL, FAR) of a mangled k_step_batch<T, EMIT, LOADMODE, COLL, WALL, FAR> or k_step_half_batch<EMIT, COLL, FAR>
    symbol, read from its template arguments: storage "native" or "half", T "f" or "d"; None for any other symbol."""
    m = _STEP.match(name)
    if not m:
        return None
    args = [int(a) for a in re.findall(r"L[bi](\d+)E", m.group(3))]
    if m.group(1):
        assert not m.group(2) and len(args) == 3, name
        return ("half", "f", args[0], args[1], HALFWAY, args[2])
    assert m.group(2) and len(args) == 5, name
    return ("native", m.group(2), args[0], args[2], args[3], args[4])


def step_variants_built():
    """The step kernels the library is to hold, no more and no fewer: native, both dtypes, emitting and not, every collision with either wall
    rule and every far field but the two-relaxation-time collisions with the axial one (80); half, every collision with the inclined far
    field and the single-relaxation-time ones with the axial one too (12)."""
    native = {("native", t, e, c, w, f) for t in "fd" for e in (0, 1) for c in range(4) for w in range(2) for f in range(3)
              if not (c >= TRT and f == AXIAL)}
    half = {("half", "f", e, c, HALFWAY, f) for e in (0, 1) for c in range(4) for f in (AXIAL, INCLINED) if not (c >= TRT and f == AXIAL)}
    return native | half


def step_kernels(chk, files, select=lambda v: True):
    """{symbol: (variant, resources)} of the step kernels of the code object whose variant `select` accepts."""
    out = {}
    for f in files:
        for name, r in chk.resources(f).items():
            v = step_variant(name)
            if v is not None and select(v):
                out[name] = (v, r)
    return out


@functools.lru_cache(maxsize=None)
def polar_isa():
    """(tools/check_store_hazard module, the device .s files of polar.hip); skips where hipcc is absent."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_store_hazard as chk
    return chk, chk.build(os.path.join(ROOT, "airfoil-cfd-tool_amd", "csrc", "polar.hip"))
