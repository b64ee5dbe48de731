"""Host: the references of tests/_step_matrix_cases.py can tell the step variants apart.  After the first step from the members' rough
start states, the populations of any two variants of the same case and storage differ in at least one of the three members, so a batch
that ran another variant's kernel, or its own with another variant's arguments, does not compare equal in
tests/test_gpu_polar_step_matrix.py."""
import itertools

import numpy as np
import pytest

import _step_matrix_cases as sm


def test_the_runs_are_every_switch_combination():
    native = [r for r in sm.RUNS if not r[0].stored]
    stored = [r for r in sm.RUNS if r[0].stored]
    assert len(native) == 2 * 2 * 2 * 2 * 3 and len(stored) == 8 and len(set(sm.RUNS)) == len(sm.RUNS)
    assert {name for _, name in native} == set(sm.NATIVE_CASES) and {name for _, name in stored} == {sm.HALF_CASE}
    assert not any(m.wind and m.profile for m, _ in sm.RUNS) and not any(m.stored and (m.ibb or m.profile) for m, _ in sm.RUNS)
    assert len(sm.MEMBERS) % 2 == 1 and sm.MARKS == (1, 5, 8)


@pytest.mark.parametrize("stored,name", [(False, n) for n in sm.NATIVE_CASES] + [(True, sm.HALF_CASE)])
def test_no_two_variants_share_a_reference(stored, name):
    runs = [r for r in sm.RUNS if r[0].stored == stored and r[1] == name]
    first = {mdl: [np.asarray(state) for state, _ in sm.reference(mdl, name, upto=1)[1]] for mdl, _ in runs}
    fewest = len(sm.MEMBERS)
    for a, b in itertools.combinations(first, 2):
        differing = sum(x.tobytes() != y.tobytes() for x, y in zip(first[a], first[b]))
        fewest = min(fewest, differing)
        assert differing >= 1, (a, b)
    print(f"{name}{' half' if stored else ''}: {len(first)} variants, every pair differs in at least {fewest} of {len(sm.MEMBERS)} members after one step")
