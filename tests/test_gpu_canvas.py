"""GPU: the device canvas (csrc/canvas.hpp: k_canvas_stroke, k_canvas_compose) pixel for pixel on crafted inputs, driven through
Engine.canvas_stroke and Engine.canvas_compose, against the NumPy compositor's primitives (tests/_canvas_cases.py: the inputs, the
reference, the rule of comparison and where its bound comes from).  The field image under the canvas is computed from the handle's own
read_macro() by oracle/lbm_numpy.py, as tests/test_gpu_readouts.py does, so that only the canvas is under test.

Field only (nothing touches hypot): byte for byte, the whole canvas.  Strokes, foil, everything together: a byte may differ by one level
only at a hypot-dependent pixel whose reference value lies within 1e-6 of a rounding tie, of which a reference holds at most 16.
Every comparison prints one line `canvas: <case> differ=<bytes> near=<pixels>` (pytest -s shows them)."""
import ctypes

import numpy as np
import pytest

import _canvas_cases as cc
from airfoil_cfd_tool_amd import compose
from test_gpu_readouts import CLAMP_TAU, CLAMP_U0, LATTICES, TAU, U0, VORT_SCALE, _mask, _run

pytestmark = pytest.mark.gpu

LAT = {(l[0], l[1]): l for l in LATTICES}
ERR_ARG, ERR_STATE = -1, -5


class _Tunnel:
    """A stepped handle with what the reference needs of it."""

    def __init__(self, pkg, oracle_np, key):
        nx, ny, dtype, shape, aoa, clamp = LAT[key]
        assert (nx, ny, dtype) in cc.FIELD_LATTICES
        self.mask = _mask(pkg, nx, ny, shape, aoa)
        self.tau, self.u0 = (CLAMP_TAU, CLAMP_U0) if clamp else (TAU, U0)
        self.e = pkg.Engine(nx, ny, dtype=dtype)
        if nx * ny > 2_000_000:                         # 30 steps are enough for a picture
            self.e.set_mask(self.mask)
            self.e.init_equilibrium(self.u0)
            self.e.step(30, self.tau, self.u0)
        else:
            _run(self.e, self.mask, self.tau, self.u0, clamp)
        self.oracle_np = oracle_np
        self.refresh()

    def refresh(self):
        self.macro = self.e.read_macro()
        self.params = tuple(self.oracle_np.ranges_from_macro(*self.macro, self.mask, self.u0)) + (VORT_SCALE,)
        self._fields = {}

    def field(self, mode, params=None):
        key = (mode, params)
        if key not in self._fields:
            self._fields[key] = cc.field_image(mode, self.macro, self.mask, self.u0, params or self.params)
        return self._fields[key]

    def clear(self):
        """An empty particle layer: the handle's canvas may then change its scale."""
        s = int(self.e.get_option("canvas_scale"))
        if s:
            self.e.canvas_stroke(s, 2)

    def strokes(self, s, calls):
        self.clear()
        for fade, rec in calls:
            self.e.canvas_stroke(s, fade, rec)

    def compose(self, s, mode, poly=None, text=None, trails=False, params=None):
        return self.e.canvas_compose(s, mode, self.u0, *(params or self.params), np.zeros((0, 2)) if poly is None else poly,
                                     compose.bar_rows(mode, s), text, trails)


@pytest.fixture(scope="module")
def tunnels(pkg, oracle_np):
    made = {}

    def get(key):
        if key not in made:
            made[key] = _Tunnel(pkg, oracle_np, key)
        return made[key]
    yield get
    for t in made.values():
        t.e.close()


def _equal(img, ref, what):
    bad = np.argwhere((img != ref.rgba).any(axis=-1))
    assert bad.size == 0, (what, len(bad), [(int(y), int(x), img[y, x].tolist(), ref.rgb[y, x].tolist()) for y, x in bad[:4]])
    assert not ref.dep.any()


# --------------------------------------------------------------------------------------------------------------------------------------------
# field only: resampling, the clamps of x0 / x1 / y0 / y1, field_value and the stability net seen through the canvas, background, bar
# --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", cc.FIELD_LATTICES, ids=lambda l: f"{l[0]}x{l[1]}-{l[2]}")
def test_field_only_is_byte_identical(pkg, oracle_np, tunnels, lattice):
    key = lattice[:2]
    scaled = key in cc.SCALED_LATTICES
    t = tunnels(key) if key in ((37, 29), (200, 131), (65, 130)) else _Tunnel(pkg, oracle_np, key)
    try:
        t.clear()
        assert t.e.dtype == np.dtype(lattice[2])
        sets = [None] + ([tuple(float(v) for v in p) for p in cc.floor_params(t.macro, t.mask, t.u0)] if scaled else [])
        n = 0
        for s in cc.SCALES if scaled else (1,):
            for mode in (0, 1, 2):
                for params in sets if s == 1 else sets[:1]:
                    ref = cc.reference(s, t.field(mode, params), None, None, compose.bar_rows(mode, s), cc.no_text(s))
                    img = t.compose(s, mode, text=cc.no_text(s), params=params)
                    _equal(img, ref, (s, mode, params))
                    n += 1
        print(f"canvas: field-{key[0]}x{key[1]} images={n} differ=0 near=0")
        # the picture is one: the field shows in the plot rectangle, solids are drawn flat, the background keeps its colour
        assert (ref.rgba[0, 0, :3] == compose.BG).all() and len(np.unique(ref.rgba[26:334, 54:638].reshape(-1, 4), axis=0)) > (3 if key != (3, 3) else 1)
    finally:
        if t.e is not None and key not in ((37, 29), (200, 131), (65, 130)):
            t.e.close()


# --------------------------------------------------------------------------------------------------------------------------------------------
# strokes, foil, everything together: the cases of _canvas_cases
# --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.cases(), ids=cc.case_id)
def test_case_against_the_compositor(tunnels, case):
    t, s = tunnels(case.lattice[:2]), case.scale
    calls = cc.stroke_scenarios(s)[case.strokes] if case.strokes else []
    t.strokes(s, calls[:-1])
    text, poly = cc.case_text(case), cc.polygons(s)[case.poly] if case.poly else None
    before = t.compose(s, case.mode, poly, text, bool(case.strokes))
    if calls:
        t.e.canvas_stroke(s, *calls[-1])
    img = t.compose(s, case.mode, poly, None, bool(case.strokes))                    # None: the map of the call before
    ref = cc.case_reference(case, t.field(case.mode))
    differ, near = cc.judge(img, ref)
    print(f"canvas: {cc.case_id(case)} differ={differ} near={near}")
    live = t.e.get_option("canvas_layer_live")
    bare = t.compose(s, case.mode, poly, None, False)
    if case.strokes in ("far_outside_only", "fades_then_clear"):                     # an empty layer: as if there were none, byte for byte
        assert np.array_equal(img, bare)
        assert live == (1.0 if case.strokes == "far_outside_only" else 0.0)          # (strokes were submitted / the layer was cleared)
    elif case.strokes:
        assert live == 1.0 and (img != bare).any(axis=-1).sum() > 100
    if case.strokes == "fades":                                                      # its last call is fade 0 with no segment: nothing changes
        assert calls[-1] == (0, None) and np.array_equal(img, before)
    if case.poly in cc.NO_FOIL:                                                      # fewer than 3 points draw no foil
        assert np.array_equal(bare, t.compose(s, case.mode, None, None, False))
    elif case.poly:
        assert (bare != t.compose(s, case.mode, None, None, False)).any(axis=-1).sum() > 50


@pytest.mark.parametrize("s", cc.SCALES)
def test_strokes_blend_in_the_order_given(tunnels, s):
    t = tunnels((37, 29))
    imgs = []
    for name in ("stack", "stack_reversed"):
        t.strokes(s, cc.stroke_scenarios(s)[name])
        imgs.append(t.compose(s, 0, None, cc.no_text(s), True))
        cc.judge(imgs[-1], cc.reference(s, t.field(0), cc.layer_of(s, name), None, compose.bar_rows(0, s), cc.no_text(s)))
    y, x = int(150.5 * s), int(300.5 * s)
    assert (imgs[0][y, x] != imgs[1][y, x]).any() and (imgs[0] != imgs[1]).any(axis=-1).sum() > 20


def test_the_fill_is_half_open_on_the_device(tunnels):
    """k_canvas_compose alone, no reference: the rectangle with x edges at 100.5 and 110.5 and y edges at 50.5 and 60.5 fills columns
    100 .. 109 and rows 50 .. 59."""
    t = tunnels((37, 29))
    t.clear()
    rect = cc.polygons(1)["rect_on_centres"]
    img = t.compose(1, 0, rect, cc.no_text(1), False).astype(int)
    field = t.compose(1, 0, None, cc.no_text(1), False).astype(int)
    # column 109 and row 59 lie 1.0 inside the edges at 110.5 and 60.5, under 1.2 - 1.0 = 0.2 of the outline: the fill shows through it
    shade = [int(np.rint(c * (1 - 0.2 * 0.85) + o * 0.2 * 0.85)) for c, o in zip(compose.FOIL_FILL, compose.FOIL_STROKE[:3])]
    assert (img[52:59, 109, :3] == shade).all() and (img[59, 102:109, :3] == shade).all()
    assert (np.abs(field[52:59, 109, :3] - compose.FOIL_FILL) > 2).any() and (np.abs(field[59, 102:109, :3] - compose.FOIL_FILL) > 2).any()
    # column 110 and row 60 lie on those edges, under the whole outline: not filled, the field shows through it
    want = field[..., :3] * (1 - 0.85) + np.array(compose.FOIL_STROKE[:3]) * 0.85
    assert (np.abs(img[52:59, 110, :3] - want[52:59, 110]) <= 0.5 + 0.5 * 0.15 + 1e-9).all()
    assert (np.abs(img[60, 102:109, :3] - want[60, 102:109]) <= 0.5 + 0.5 * 0.15 + 1e-9).all()
    filled = np.array(compose.FOIL_FILL) * (1 - 0.85) + np.array(compose.FOIL_STROKE[:3]) * 0.85
    assert (np.abs(want[52:59, 110] - filled) > 1.1).any() and (np.abs(want[60, 102:109] - filled) > 1.1).any()      # (it would show)
    # column 100 and row 50 lie on the near edges: filled under the whole outline; the inside proper is the fill's colour
    assert (np.abs(img[52:59, 100, :3] - filled) <= 0.5).all() and (np.abs(img[50, 102:109, :3] - filled) <= 0.5).all()
    assert (img[52:59, 102:109, :3] == compose.FOIL_FILL).all()


def test_natural_strokes_on_a_tall_fp64_lattice(pkg, oracle_np):
    """Tracers' own strokes: the same particles through a DeviceTrailLayer and a TrailLayer, 25 frames, then the whole frame."""
    from airfoil_cfd_tool_amd.tracers import Tracers
    nx, ny, s = 65, 130, 1
    with pkg.WindTunnel(shape="naca4412", nx=nx, ny=ny, aoa_deg=9.0, dtype="float64", field="speed") as wt:
        host_layer, dev_layer = compose.TrailLayer(s), wt.trail_layer(s)
        assert isinstance(dev_layer, compose.DeviceTrailLayer)
        tr_h, tr_d = Tracers(wt, n=700, seed=11), Tracers(wt, n=700, seed=11)
        for _ in range(25):
            wt.frame(render=False)
            sh, _ = tr_h.draw(host_layer, 16.0)
            sd, _ = tr_d.draw(dev_layer, 16.0)
            assert np.array_equal(sh, sd)
        img = wt.compose_frame(trails=dev_layer, scale=s)
        mask = (wt.geometry.mask != 0).astype(np.uint8)
        params = (wt.max_s, wt.cp_min, wt.cp_max, VORT_SCALE)
        field = cc.field_image(0, wt.engine.read_macro(), mask, wt.u0, params)
        yh = wt.y_half_world()
        cx, cy = compose.Canvas(s, alloc=False).w2c(wt.geometry.xp, wt.geometry.yp, yh)
        ref = cc.reference(s, field, host_layer, np.column_stack([cx, cy]), compose.bar_rows(0, s), compose.text_alpha_map(s, wt.aoa_deg, 0, yh))
        differ, near = cc.judge(img, ref)
        print(f"canvas: natural-65x130-f64 differ={differ} near={near}")
        assert (host_layer.a > 0.3).sum() > 200


@pytest.mark.parametrize("lattice", cc.COMBINED_LATTICES, ids=lambda l: f"{l[0]}x{l[1]}-{l[2]}")
def test_the_layer_survives_a_new_mask_and_further_steps(pkg, oracle_np, lattice):
    nx, ny = lattice[:2]
    t = _Tunnel(pkg, oracle_np, (nx, ny))
    try:
        case = cc.survival_case(lattice)
        s, mode = case.scale, case.mode
        t.strokes(s, cc.stroke_scenarios(s)["crafted"])
        poly, text = cc.polygons(s)[case.poly], cc.case_text(case)
        seen = [t.compose(s, mode, poly, text, True)]
        stats = [cc.judge(seen[0], cc.case_reference(case, t.field(mode)))]
        t.mask = _mask(pkg, nx, ny, "naca2412", 3.0, seed=4)                      # another body, other border runs: the old planes under a new mask
        t.e.set_mask(t.mask)
        t._fields = {}
        seen.append(t.compose(s, mode, poly, None, True))
        stats.append(cc.judge(seen[1], cc.case_reference(case, t.field(mode))))
        t.e.step(40, t.tau, t.u0)
        params = t.params
        t.refresh()
        t.params = params                                                           # the picture's ranges stay: only the state moved on
        seen.append(t.compose(s, mode, poly, None, True))
        stats.append(cc.judge(seen[2], cc.case_reference(case, t.field(mode))))
        print(f"canvas: survive-{nx}x{ny} differ={[d for d, _ in stats]} near={[n for _, n in stats]}")
        assert (seen[0] != seen[1]).any() and (seen[1] != seen[2]).any() and t.e.get_option("canvas_layer_live") == 1.0
    finally:
        t.e.close()


# --------------------------------------------------------------------------------------------------------------------------------------------
# the label map: NULL keeps the previous one, or draws none
# --------------------------------------------------------------------------------------------------------------------------------------------
def test_a_null_text_map_means_the_previous_one_or_none(tunnels):
    t = tunnels((37, 29))
    t.clear()
    t.compose(2, 0, None, cc.crafted_text(2), False)
    assert t.e.get_option("canvas_text_set") == 1.0 and t.e.get_option("canvas_scale") == 2.0
    bar = compose.bar_rows(0, 1)
    img = t.compose(1, 0, None, None, False)                                        # a canvas new at this scale has no map: no text
    assert t.e.get_option("canvas_text_set") == 0.0 and t.e.get_option("canvas_scale") == 1.0
    _equal(img, cc.reference(1, t.field(0), None, None, bar, None), "no map yet")
    with_text = cc.reference(1, t.field(0), None, None, bar, cc.crafted_text(1))
    _equal(t.compose(1, 0, None, cc.crafted_text(1), False), with_text, "crafted map")
    assert t.e.get_option("canvas_text_set") == 1.0
    _equal(t.compose(1, 0, None, None, False), with_text, "the previous map")
    assert (with_text.rgba != cc.reference(1, t.field(0), None, None, bar, None).rgba).any(axis=-1).sum() > 1000
    real = cc.real_text(1, 9.0, 0, 37, 29)
    _equal(t.compose(1, 0, None, real, False), cc.reference(1, t.field(0), None, None, bar, real), "real labels")
    _equal(t.compose(1, 0, None, cc.no_text(1), False), cc.reference(1, t.field(0), None, None, bar, None), "an all-zero map")


# --------------------------------------------------------------------------------------------------------------------------------------------
# arguments and state
# --------------------------------------------------------------------------------------------------------------------------------------------
def _raw_stroke(e, scale, fade, n, seg):
    return e._lib.wt_canvas_stroke(e._h, scale, fade, n, None if seg is None else seg.ctypes.data_as(ctypes.c_void_p))


def _raw_compose(e, scale, mode, npoly, poly, bar, out, u0=U0):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    return e._lib.wt_canvas_compose(e._h, scale, mode, u0, 0.1, -1.0, 1.0, VORT_SCALE, p(poly), npoly, p(bar), None, 0, p(out))


def test_bad_arguments_are_refused_and_leave_the_layer_alone(pkg, tunnels):
    t = tunnels((37, 29))
    e = t.e
    good = cc.short_records(1, 40, 5)
    t.strokes(1, [(0, good)])
    before = t.compose(1, 0, None, cc.no_text(1), True)
    seg = np.ascontiguousarray(good)
    assert _raw_stroke(e, 0, 0, 0, None) == ERR_ARG and _raw_stroke(e, 9, 0, 0, None) == ERR_ARG
    assert _raw_stroke(e, 1, 3, 0, None) == ERR_ARG and _raw_stroke(e, 1, -1, 0, None) == ERR_ARG
    assert _raw_stroke(e, 1, 0, -1, seg) == ERR_ARG and _raw_stroke(e, 1, 0, 5, None) == ERR_ARG
    for ns in (1.0, 65537.0, float("nan")):
        bad = seg.copy()
        bad[17, 4] = ns
        assert _raw_stroke(e, 1, 1, len(bad), bad) == ERR_ARG, ns
        with pytest.raises(pkg.WTError) as ei:
            e.canvas_stroke(1, 0, bad)
        assert ei.value.code == ERR_ARG and "segment 17" in str(ei.value)
    assert np.array_equal(t.compose(1, 0, None, cc.no_text(1), True), before)       # neither faded nor stroked
    edge = seg.copy()
    edge[3, 4], edge[4, 4] = 2.0, 65536.0                                           # the bounds themselves are valid
    assert _raw_stroke(e, 1, 0, len(edge), edge) == 0
    bar, out, poly = compose.bar_rows(0, 1), np.empty((360, 680, 4), np.uint8), np.zeros((cc.CV_MAX_POLY + 1, 2))
    assert _raw_compose(e, 1, 3, 0, None, bar, out) == ERR_ARG and _raw_compose(e, 1, -1, 0, None, bar, out) == ERR_ARG
    assert _raw_compose(e, 1, 0, cc.CV_MAX_POLY + 1, poly, bar, out) == ERR_ARG and _raw_compose(e, 1, 0, 3, None, bar, out) == ERR_ARG
    assert _raw_compose(e, 1, 0, -1, poly, bar, out) == ERR_ARG
    assert _raw_compose(e, 1, 0, 0, None, None, out) == ERR_ARG and _raw_compose(e, 1, 0, 0, None, bar, None) == ERR_ARG
    assert _raw_compose(e, 0, 0, 0, None, bar, out) == ERR_ARG and _raw_compose(e, 9, 0, 0, None, bar, out) == ERR_ARG
    assert _raw_compose(e, 1, 0, cc.CV_MAX_POLY, poly, bar, out) == 0 and _raw_compose(e, 1, 0, 0, None, bar, out) == 0


def test_a_slab_handle_refuses_the_canvas(pkg):
    nx, ny, edges = 96, 48, [0, 40, 96]
    mask = _mask(pkg, nx, ny, "naca2412", 6.0)
    es = [pkg.Engine(nx, ny, dtype="float32", rank=r, nranks=2, halo=2, edges=edges) for r in range(2)]
    try:
        pkg.Engine.link_local(es)
        for e in es:
            e.set_mask(mask)
            e.init_equilibrium(U0)
        pkg.Engine.step_group(es, 4, TAU, U0)
        for e in es:
            with pytest.raises(pkg.WTError) as ei:
                e.canvas_stroke(1, 0, cc.short_records(1, 3, 21))
            assert ei.value.code == ERR_STATE and "whole lattice" in str(ei.value)
            with pytest.raises(pkg.WTError) as ei:
                e.canvas_compose(1, 0, U0, 0.1, -1.0, 1.0, VORT_SCALE, np.zeros((0, 2)), compose.bar_rows(0, 1), None, False)
            assert ei.value.code == ERR_STATE and "whole lattice" in str(ei.value)
            assert e.get_option("canvas_scale") == 0.0
    finally:
        for e in es:
            e.close()


def test_compose_wants_planes_that_describe_the_state(pkg, oracle_np):
    """require_macro: no state or no mask is refused; equilibrium before any step is a state like another; after wt_write_f the planes
    are stale until a step has emitted them again."""
    nx, ny = 37, 29
    mask = _mask(pkg, nx, ny, "naca4412", 24.0)
    bar, args = compose.bar_rows(0, 1), (U0, 0.1, -1.0, 1.0, VORT_SCALE)
    with pkg.Engine(nx, ny, dtype="float32") as e:
        for ready in (lambda: None, lambda: e.set_mask(mask)):
            ready()
            with pytest.raises(pkg.WTError) as ei:
                e.canvas_compose(1, 0, *args, np.zeros((0, 2)), bar, None, False)
            assert ei.value.code == ERR_STATE and "state or mask missing" in str(ei.value)
        assert e.get_option("canvas_scale") == 0.0                                  # refused before a canvas was made
        e.canvas_stroke(1, 0, cc.short_records(1, 3, 21))                           # the layer needs no state
        assert e.get_option("canvas_scale") == 1.0 and e.get_option("canvas_layer_live") == 1.0
        e.init_equilibrium(U0)
        img = e.canvas_compose(1, 0, *args, np.zeros((0, 2)), bar, None, False)      # a fresh handle before any step: the equilibrium
        _equal(img, cc.reference(1, cc.field_image(0, e.read_macro(), mask, U0, args[1:]), None, None, bar, None), "before any step")
        e.step(5, TAU, U0)
        f = e.read_f()
        e.write_f(f)
        with pytest.raises(pkg.WTError) as ei:
            e.canvas_compose(1, 0, *args, np.zeros((0, 2)), bar, None, False)
        assert ei.value.code == ERR_STATE and "wt_write_f" in str(ei.value)
        e.step(1, TAU, U0)
        img = e.canvas_compose(1, 0, *args, np.zeros((0, 2)), bar, None, False)
        _equal(img, cc.reference(1, cc.field_image(0, e.read_macro(), mask, U0, args[1:]), None, None, bar, None), "after the next step")


def test_scale_text_and_layer_flags_follow_the_calls(pkg, tunnels):
    t = tunnels((37, 29))
    e = t.e
    opt = lambda: tuple(e.get_option(k) for k in ("canvas_scale", "canvas_layer_live", "canvas_text_set"))
    t.clear()
    t.compose(3, 0, None, None, False)
    assert opt()[:2] == (3.0, 0.0)
    e.canvas_stroke(3, 1)                                                           # a fade alone draws nothing
    e.canvas_stroke(3, 0)
    assert opt()[:2] == (3.0, 0.0)
    t.compose(2, 0, None, None, False)                                              # so the canvas may change its scale; its map is gone
    assert opt() == (2.0, 0.0, 0.0)
    t.compose(2, 0, None, cc.crafted_text(2), False)
    assert opt() == (2.0, 0.0, 1.0)
    e.canvas_stroke(2, 0, cc.short_records(2, 10, 23))
    assert opt() == (2.0, 1.0, 1.0)
    kept = t.compose(2, 0, None, None, True)
    for call in (lambda: t.compose(1, 0, None, None, True), lambda: e.canvas_stroke(3, 0, cc.short_records(3, 3, 21)), lambda: e.canvas_stroke(1, 2)):
        with pytest.raises(pkg.WTError) as ei:                                       # another scale while strokes live on the layer
            call()
        assert ei.value.code == ERR_STATE and "wipe" in str(ei.value)
    assert opt() == (2.0, 1.0, 1.0) and np.array_equal(t.compose(2, 0, None, None, True), kept)
    e.canvas_stroke(2, 1)                                                           # fading does not clear
    assert opt()[1] == 1.0
    e.canvas_stroke(2, 2)
    assert opt() == (2.0, 0.0, 1.0)
    img = t.compose(1, 0, None, None, True)                                         # allowed now; the new canvas has neither strokes nor labels
    assert opt() == (1.0, 0.0, 0.0)
    _equal(img, cc.reference(1, t.field(0), None, None, compose.bar_rows(0, 1), None), "after the change of scale")
