"""Half storage, the two-relaxation-time collision, prescribed far-field profiles and state upload at many members: the families, the
per-member inputs and the cached reference runs that tests/test_polar_many_models_host.py pins and tests/test_gpu_polar_many_models.py
compares the kernels with.  Test infrastructure only.

The batches are tests/_many_cases.py's (67, 35 and 1024 members; masks, tau, U0, Cs, V0, wall distances and reference points from
mc.members, unchanged).  Added here per member, from generators of their own: a magic number, a rough start state
(_rough_start.rough_state at _restart_cases.AMPS, a seed per member), far-field tables (_profile_reference.random_tables), and a second
start state and a second set of tables for the members that a test overwrites in the middle of a run.

A family is a set of models and the cases it runs on.  Its reference is one step at a time and continued from its own states, composed
of what the tests of each feature use: _trt_reference.step with les_constant(cs) and q where walls interpolate, _half_reference.windy
and half_step for the inclined stream and half storage, _profile_reference.profile_step for the profile.  A batch runs calls(name) =
(1, 4, 3, 8, 8) steps with sample_every = 8 and is read back after each call, at steps 1, 5, 8, 16 and 24: step 1 is the first step
after an upload, and the marks fall on odd and even counts, so states written by either walk of the members are compared, after emitting
and non-emitting steps.  The 1024 batch runs (1, 6, 7, 7) with sample_every = 7.
"""
import functools
from dataclasses import dataclass

import numpy as np

import lbm_numpy
import _half_reference as half
import _ibb_reference as ibb
import _les_reference as les
import _many_cases as mc
import _profile_reference as prof
import _restart_cases as rc
import _trt_reference as trt
from _rough_start import rough_state


@dataclass(frozen=True)
class Model:
    """What a family switches on.  `stored`: a storage="half" batch."""
    stored: bool = False
    trt: bool = False
    wind: bool = False
    les: bool = False
    ibb: bool = False
    profile: bool = False


HALF_CASES = ("67-96x48-f32", "67-24x300-f32")
# family -> (its models, the cases it runs on, the step kernel)
FAMILIES = {
    "half": (Model(stored=True, wind=True, les=True), HALF_CASES),                              # k_step_half_batch<COLLIDE_LES, FAR_INCLINED>
    "half-trt": (Model(stored=True, trt=True, wind=True, les=True), HALF_CASES),                # k_step_half_batch<COLLIDE_TRT_LES, FAR_INCLINED>
    "trt": (Model(trt=True, wind=True, les=True, ibb=True), mc.BODY),                           # k_step_batch<COLLIDE_TRT_LES, WALL_INTERP, FAR_INCLINED>
    "profile": (Model(profile=True, trt=True, les=True, ibb=True), ("67-96x48-f32", "35-24x140-f64")),      # k_step_batch<FAR_PROFILE> (TRT, interpolated)
    "profile-plain": (Model(profile=True), ("67-24x300-f32",)),                                 # k_step_batch<FAR_PROFILE> (BGK, half-way walls)
    "max-half-trt": (Model(stored=True, trt=True, wind=True, les=True), (mc.MAX,)),             # both at WTP_MAX_MEMBERS
    "max-profile": (Model(profile=True, trt=True, les=True), (mc.MAX,)),
}
MAX_FAMILIES = ("max-half-trt", "max-profile")
RUNS = [(fam, name) for fam, (_, names) in FAMILIES.items() for name in names]
BODY_RUNS = [(fam, name) for fam, name in RUNS if fam not in MAX_FAMILIES]
READOUT_RUNS = (("half-trt", "67-96x48-f32"), ("profile", "35-24x140-f64"))      # the batches of the read-out and the overwrite tests
SUB_RUN = ("profile", "67-96x48-f32")                                           # of the profile sub-range test
SUB_TABLES = (43, 2)                                                            # ... set_far_profile(first=43) with 2 members' second tables
ARG_RUN = ("trt", "67-96x48-f32")                                               # of the argument checks at late indices
RESTART_RUN = ("half-trt", "67-24x300-f32")                                     # of the checkpoint test
WRITE_AFTER = 8                                                                 # the step after whose sample members are overwritten


def model(family):
    return FAMILIES[family][0]


def calls(name):
    return (1, 6, 7, 7) if name == mc.MAX else (1, 4, 3, 8, 8)


def every(name):
    return 7 if name == mc.MAX else 8


def marks(name):
    """The step counts at which a batch is read back: after every call."""
    return tuple(int(v) for v in np.cumsum(calls(name)))


def sample_marks(name):
    return tuple(s for s in marks(name) if s % every(name) == 0)


def compared(name):
    """The members whose state is compared: all of them, or mc.listed_members() of the 1024 batch."""
    return mc.listed_members() if name == mc.MAX else tuple(range(mc.CASES[name][3]))


def subset(name):
    """The members of the sensitivity checks: 0, either side of 64 and B - 1 among them."""
    B = mc.CASES[name][3]
    if name == mc.MAX:
        return (0, 2, 63, 64, 65, 511, 512, 1023)
    return (0, 1, 31, 41, 63, 64, 65, 66) if B == 67 else (0, 1, 6, 16, 17, 31, 33, 34)


def overwritten(family, name):
    """{member: "f" or "stored"}: the members the overwrite test writes after the sample at WRITE_AFTER, and by which call.  Member 41
    and the last one by write_f (6 = 41 - 35 in the batch of 35, which has no member 41); on a half batch also member 0 by write_stored."""
    B = mc.CASES[name][3]
    out = {41 if B > 41 else 41 - B: "f", B - 1: "f"}
    if model(family).stored:
        out[0] = "stored"
    return out


def upload_order(name):
    """The fixed scrambled order in which a test writes the members' start states."""
    return tuple(np.random.default_rng(611).permutation(mc.CASES[name][3]).tolist())


def _seed(name, kind, m, which):
    return (7301, sorted(mc.CASES).index(name), kind, int(m), int(which))


@functools.lru_cache(maxsize=None)
def magic(name):
    """[B] doubles, read-only: uniform in [1/16, 1/2], with 3/16 planted on members 0 and 64 mod B and 1/4 on members 7 and B - 1."""
    B = mc.CASES[name][3]
    lam = np.random.default_rng(_seed(name, 0, 0, 0)).uniform(1.0 / 16.0, 0.5, B)
    lam[[0, 64 % B]] = 3.0 / 16.0
    lam[[7, B - 1]] = 0.25
    lam.setflags(write=False)
    return lam


@functools.lru_cache(maxsize=None)
def start(name, m, which=0):
    """Member m's rough start state [9][NY][NX] of the case's dtype, read-only; which = 1: the state it is overwritten with."""
    nx, ny, dtype, *_ = mc.CASES[name]
    f = rough_state(nx, ny, float(mc.members(name).u0[m]), np.dtype(dtype), _seed(name, 1, m, which), **rc.AMPS)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def tables(name, m, which=0):
    """Member m's far-field tables (left [3][NY], bottom [3][NX], top [3][NX]), read-only; which = 1: its second set."""
    nx, ny, dtype, *_ = mc.CASES[name]
    t = prof.random_tables(nx, ny, dtype, _seed(name, 2, m, which))
    for a in t:
        a.setflags(write=False)
    return t


def stacked_tables(name, members, which=0):
    """(left [n][3][NY], bottom [n][3][NX], top [n][3][NX]) of `members`, as set_far_profile takes them."""
    return tuple(np.stack([tables(name, m, which)[k] for m in members]) for k in range(3))


def start_state(family, name, m, which=0):
    """What the reference of member m starts from: the rough state, or Store of it in a half family."""
    f = start(name, m, which)
    if not model(family).stored:
        return f
    h = half.store(f)
    h.setflags(write=False)
    return h


def base_of(mdl, name, m, lam=None, v0=None):
    """(base step, its extra arguments) of member m under the models `mdl`, without the profile and the half wrappers.  lam, v0: the
    member's own magic number and cross-flow unless given."""
    mem = mc.members(name)
    dtype = mc.CASES[name][2]
    _, _, cs, own_v0 = mem.params(m)
    c = les.les_constant(cs, np.dtype(dtype)) if mdl.les else None
    q = mem.q[m] if mdl.ibb else None
    if mdl.trt:
        base, extra = trt.step, (float(magic(name)[m]) if lam is None else lam, c, q)
    elif mdl.ibb:
        base, extra = ibb.step, (q, c)
    elif mdl.les:
        base, extra = les.step, (c,)
    else:
        base, extra = lbm_numpy.step, ()
    if mdl.wind:
        base, extra = half.windy(base), (own_v0 if v0 is None else v0, *extra)
    return base, extra


def advance(family, name, m, state, steps, which=0, lam=None, v0=None, tabs=None, mdl=None):
    """`steps` steps of member m's reference from `state` (populations, or halves in a half family).  which: the set of its tables in
    use; lam, v0, tabs, mdl: another magic number, cross-flow, tables or set of models than its own (the sensitivity checks).  Returns
    ((state, (rho, ux, uy)), (density events, speed events) summed over the steps), the arrays read-only."""
    mdl = model(family) if mdl is None else mdl
    mem = mc.members(name)
    mask = mem.masks[m]
    tau, u0, _, _ = mem.params(m)
    base, extra = base_of(mdl, name, m, lam, v0)
    if mdl.profile and tabs is None:
        tabs = tables(name, m, which)
    events, out = [0, 0], None
    for _ in range(steps):
        if mdl.profile:
            out = prof.profile_step(base, state, mask, tau, u0, tabs, *extra)
        elif mdl.stored:
            out = half.half_step(base, state, mask, tau, u0, *extra)
        else:
            out = base(state, mask, tau, u0, *extra)
        state = out[0]
        e = lbm_numpy.clamp_events(*out[1], mask)
        events[0] += e[0]
        events[1] += e[1]
    return mc.frozen(out), tuple(events)


def continued(family, name, m, state, done, **kw):
    """[(state, macro)] of member m at the marks after `done`, continued from `state` at step `done`."""
    out = []
    for mark in marks(name):
        if mark > done:
            (state, macro), _ = advance(family, name, m, state, mark - done, **kw)
            done = mark
            out.append((state, macro))
    return out


class Reference:
    """states[k][m] = (state, (rho, ux, uy)) of member m at marks(name)[k], for m in compared(name); events[m] = its clamp events summed
    over every step."""

    def __init__(self, states, events):
        self.states, self.events = states, events


@functools.lru_cache(maxsize=None)
def reference(family, name):
    states = [{} for _ in marks(name)]
    events = {}
    for m in compared(name):
        state, done, ev = start_state(family, name, m), 0, (0, 0)
        for k, mark in enumerate(marks(name)):
            (state, macro), e = advance(family, name, m, state, mark - done)
            done, ev = mark, (ev[0] + e[0], ev[1] + e[1])
            states[k][m] = (state, macro)
        events[m] = ev
    return Reference(states, events)


def at(family, name, mark):
    """{m: (state, macro)} of the family's reference at step `mark`."""
    return reference(family, name).states[marks(name).index(mark)]


@functools.lru_cache(maxsize=None)
def overwrite_reference(family, name):
    """{m: [(state, macro) at the marks after WRITE_AFTER]} of the members overwritten with their second start state at WRITE_AFTER."""
    return {m: continued(family, name, m, start_state(family, name, m, 1), WRITE_AFTER) for m in overwritten(family, name)}


@functools.lru_cache(maxsize=None)
def sub_tables_reference():
    """{m: [(state, macro) at the marks after WRITE_AFTER]} of the members of SUB_RUN that take their second tables at WRITE_AFTER."""
    family, name = SUB_RUN
    first, count = SUB_TABLES
    return {m: continued(family, name, m, at(family, name, WRITE_AFTER)[m][0], WRITE_AFTER, which=1) for m in range(first, first + count)}


@functools.lru_cache(maxsize=None)
def axial_reference():
    """[m] = (state, macro) of ARG_RUN's members 8 steps after step 16 with a cross-flow of 0."""
    family, name = ARG_RUN
    return [advance(family, name, m, at(family, name, 16)[m][0], 8, v0=0.0)[0] for m in range(mc.CASES[name][3])]
