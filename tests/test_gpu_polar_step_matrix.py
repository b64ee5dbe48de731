"""GPU: every step variant of batched sweeps (libwtpolar.so) that wtp_step can select - every (COLL, WALL, FAR) instantiation of
k_step_batch in fp32 and fp64 and of k_step_half_batch, emitting and not - on a batch of three members, bits against the NumPy
references of tests/_step_matrix_cases.py.  The suites of each feature do not visit every combination; this one does, so that a
variant selected wrongly, or handed another variant's arguments, is seen (tests/test_polar_step_matrix_host.py shows on the references
alone that no two variants agree on these inputs).
"""
import numpy as np
import pytest

import _half_reference as half
import _many_cases as mc
import _many_model_cases as mm
import _step_matrix_cases as sm
from test_gpu_polar_many_models import _assert_state, _read

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("run", sm.RUNS, ids=[sm.run_id(r) for r in sm.RUNS])
def test_every_step_variant_is_its_reference(pkg, run):
    mdl, name = run
    nx, ny, dtype, *_ = mc.CASES[name]
    mem, B = mc.members(name), len(sm.MEMBERS)
    want = sm.reference(mdl, name)
    with pkg.PolarEngine(nx, ny, B, dtype=dtype, history_cap=2, storage="half" if mdl.stored else "native") as b:
        b.set_masks(mem.masks[:B])
        if mdl.ibb:
            b.enable_interpolated_walls()
            b.set_wall_distances(mem.q[:B])
        if mdl.les:
            b.enable_les(mem.cs[:B])
        if mdl.wind:
            b.enable_wind(mem.v0[:B])
        if mdl.trt:
            b.enable_trt(mm.magic(name)[:B])
        if mdl.profile:
            b.enable_far_profile()
            b.set_far_profile(*mm.stacked_tables(name, sm.MEMBERS))
        b.init_equilibrium(mem.u0[:B])
        for m in sm.MEMBERS:
            f = mm.start(name, m)
            if mdl.stored and m & 1:
                b.write_stored(m, half.store(f).view(np.uint16))
            else:
                b.write_f(m, f)
        done = 0
        for n in sm.CALLS:
            b.step(n, mem.tau[:B], mem.u0[:B], sample_every=sm.EVERY)
            done += n
            assert b.step_count == done
            for m in sm.MEMBERS:
                _assert_state(_read(b, m), want[done][m], (sm.run_id(run), "step", done, "member", m))
        assert list(b.history()["step"]) == [sm.EVERY]
    assert done == sm.MARKS[-1]
