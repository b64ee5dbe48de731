"""The gfx950 code object of csrc/polar.hip for the host tests that inspect it: compiled once per session, whichever test
module asks first."""
import functools
import os
import sys

import pytest

from conftest import ROOT


@functools.lru_cache(maxsize=None)
def polar_isa():
    """(tools/check_store_hazard module, the device .s files of polar.hip); skips where hipcc is absent."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_store_hazard as chk
    return chk, chk.build(os.path.join(ROOT, "airfoil-cfd-tool_amd", "csrc", "polar.hip"))
