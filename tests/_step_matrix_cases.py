"""Every step variant that wtp_step can select, on one small batch each: the runs and the cached references that
tests/test_polar_step_matrix_host.py pins and tests/test_gpu_polar_step_matrix.py compares the kernels with.  Test infrastructure only.

A run is a set of switches (tests/_many_model_cases.py Model) on a case: native storage with les x trt x ibb x {axial, wind, profile} in
fp32 and in fp64, half storage with les x trt x wind.  That is every (COLL, WALL, FAR) instantiation of k_step_batch and of
k_step_half_batch, emitting and not.  The batch is members 0..2 of the case, with their own masks, tau, U0, Cs, V0, wall distances
(tests/_many_cases.py members), magic numbers, far-field tables and rough start states (tests/_many_model_cases.py): three members, an
odd count, so that the reversed member walk differs from the forward one.  The lattices are 24x300 (fp32, half) and 24x140 (fp64): one
whole tile and a ragged one, so that the GENERAL, FAST, INLET and outlet paths all run.  A batch runs CALLS = (1, 4, 3) steps with
sample_every = 8 and is read back after each call, at steps 1, 5 and 8: both walk directions, emitting and non-emitting steps.  The
reference is _many_model_cases.advance with the run's Model, which composes the references of the features' own tests.
"""
import functools
import itertools

import numpy as np

import _many_cases as mc
import _many_model_cases as mm
from _many_model_cases import Model

MEMBERS = (0, 1, 2)
CALLS = (1, 4, 3)
EVERY = 8
MARKS = tuple(int(v) for v in np.cumsum(CALLS))
NATIVE_CASES = ("67-24x300-f32", "35-24x140-f64")
HALF_CASE = "67-24x300-f32"
FARS = ("axial", "wind", "profile")


def _native():
    for les, trt, ibb, far in itertools.product((False, True), (False, True), (False, True), FARS):
        yield Model(les=les, trt=trt, ibb=ibb, wind=far == "wind", profile=far == "profile")


def _half():
    for les, trt, wind in itertools.product((False, True), repeat=3):
        yield Model(stored=True, les=les, trt=trt, wind=wind)


RUNS = [(mdl, name) for name in NATIVE_CASES for mdl in _native()] + [(mdl, HALF_CASE) for mdl in _half()]


def run_id(run):
    mdl, name = run
    on = [k for k in ("stored", "les", "trt", "ibb", "wind", "profile") if getattr(mdl, k)]
    return "+".join(on or ["plain"]) + "-" + name.split("-")[-1]


def start_state(mdl, name, m):
    """What member m starts from: its rough state, or Store of it in a half batch."""
    return mm.start_state("half" if mdl.stored else "trt", name, m)


@functools.lru_cache(maxsize=None)
def reference(mdl, name, upto=MARKS[-1]):
    """{mark: [(state, (rho, ux, uy)) of members 0..2]} at the marks up to `upto`, read-only."""
    out = {mark: [] for mark in MARKS if mark <= upto}
    for m in MEMBERS:
        state, done = start_state(mdl, name, m), 0
        for mark in out:
            (state, macro), _ = mm.advance(None, name, m, state, mark - done, mdl=mdl)
            done = mark
            out[mark].append((state, macro))
    return out
