"""Host side of the device-canvas comparison (tests/_canvas_cases.py, tests/test_gpu_canvas.py): the reference is alive — it changes
when a stroke category is dropped, a stack is reversed, a texel or a tile-border stroke is shifted — it is the product's compositor, and
its inputs keep under the cap of hypot-dependent near-tie pixels that the rule of comparison rests on.  No GPU: the field under the canvas
is a made-up flow (synthetic_state)."""
import numpy as np
import pytest

import _canvas_cases as cc
from airfoil_cfd_tool_amd import compose


@pytest.fixture(scope="module")
def fields():
    cache = {}

    def get(lattice, mode):
        key = (lattice, mode)
        if key not in cache:
            macro, mask, params = cc.synthetic_state(*lattice)
            cache[key] = cc.field_image(mode, macro, mask, cc.U0, params)
        return cache[key]
    return get


@pytest.mark.parametrize("case", cc.cases(), ids=cc.case_id)
def test_near_tie_count_of_every_case(fields, case):
    """At most MAX_NEAR hypot-dependent pixels of a reference lie within TIE of a rounding tie: counted from the reference alone."""
    ref = cc.case_reference(case, fields(case.lattice, case.mode))
    n = int(cc.near_ties(ref).any(axis=-1).sum())
    assert n <= cc.MAX_NEAR, n
    if case.strokes not in (None, "far_outside_only", "fades_then_clear"):
        assert (cc.layer_of(case.scale, case.strokes).a > 0).sum() > 100
    if case.poly and case.poly not in cc.NO_FOIL:
        assert ref.dep.sum() > 50
    cc.judge(ref.rgba, ref)                                                  # the reference passes its own rule


@pytest.mark.parametrize("s", (1, 2))
def test_dropping_a_stroke_category_changes_the_reference(s):
    rec, cat = cc.crafted_records(s)
    assert set(cat) == set(cc.STROKE_CATEGORIES)
    full = cc.layer_of(s, "crafted")
    for name in cc.STROKE_CATEGORIES:
        part = cc.run_layer(s, [(0, rec[cat != name])])
        same = np.array_equal(part.rgb, full.rgb) and np.array_equal(part.a, full.a)
        assert same == (name == cc.CHANGES_NOTHING), name
    empty = cc.layer_of(s, "far_outside_only")
    assert not empty.a.any() and not empty.rgb.any()
    # the edge categories reach the pixels they are named for
    assert full.a[0, 0] > 0 and full.a[-1, -1] > 0
    only = cc.run_layer(s, [(0, rec[cat == "near_outside"])])
    assert only.a[:, 0].any() and only.a[:, -1].any() and only.a[0].any() and only.a[-1].any()
    assert not only.a[4 * s:-4 * s, 4 * s:-4 * s].any()


@pytest.mark.parametrize("s", cc.SCALES)
def test_reversing_the_stack_changes_the_reference(s):
    a, b = cc.layer_of(s, "stack"), cc.layer_of(s, "stack_reversed")
    y, x = int(150.5 * s), int(300.5 * s)
    assert a.a[y, x] > 0.99 and not np.array_equal(a.rgb[y, x], b.rgb[y, x])
    bar = compose.bar_rows(0, s)
    assert not np.array_equal(cc.reference(s, None, a, None, bar).rgba, cc.reference(s, None, b, None, bar).rgba)


@pytest.mark.parametrize("s", cc.SCALES)
def test_shifting_a_tile_border_stroke_changes_the_reference(s):
    rec, cat = cc.crafted_records(s)
    t = rec[cat == "tile"]
    full = cc.run_layer(s, [(0, t)])
    for i in range(0, len(t), 5):
        for dx, dy in ((1.0, 0.0), (0.0, 1.0)):
            moved = t.copy()
            moved[i, [0, 2]] += dx
            moved[i, [1, 3]] += dy
            assert not np.array_equal(cc.run_layer(s, [(0, moved)]).a, full.a), (i, dx, dy)
    r = cc.brush_r(s)
    off = np.concatenate([t[:, 0], t[:, 1]])
    gap = np.abs(np.abs(off - 8 * np.round(off / 8)) - r)                    # every crafted end point lies at 8 k +- r, or 1e-9 beside it
    assert (gap < 2e-9).all() and (gap > 5e-10).sum() >= 20 and (gap < 1e-12).sum() >= 20


def _draw_field_shifted(cv, rgba_top_first):
    """Canvas.draw_field sampling texel x0 + 1 where it should sample x0: what a kernel one column off would draw."""
    img = np.asarray(rgba_top_first, dtype=np.float64)[..., :3]
    ny, nx = img.shape[:2]
    fx = (np.arange(cv.pw) + 0.5) / cv.pw * nx - 0.5
    fy = (np.arange(cv.ph) + 0.5) / cv.ph * ny - 0.5
    x0 = np.clip(np.floor(fx).astype(int), 0, nx - 1); tx = np.clip(fx - x0, 0, 1)[None, :, None]
    x0 = np.clip(x0 + 1, 0, nx - 1); x1 = np.clip(x0 + 1, 0, nx - 1)
    y0 = np.clip(np.floor(fy).astype(int), 0, ny - 1); y1 = np.clip(y0 + 1, 0, ny - 1); ty = np.clip(fy - y0, 0, 1)[:, None, None]
    top = img[y0][:, x0] * (1 - tx) + img[y0][:, x1] * tx
    bot = img[y1][:, x0] * (1 - tx) + img[y1][:, x1] * tx
    cv.rgb[cv.py:cv.py + cv.ph, cv.px:cv.px + cv.pw] = top * (1 - ty) + bot * ty


@pytest.mark.parametrize("lattice", cc.FIELD_LATTICES, ids=lambda l: f"{l[0]}x{l[1]}")
def test_a_texel_one_column_off_changes_the_field_reference(fields, lattice):
    for mode in (0, 1, 2):
        img = fields(lattice, mode)
        assert img.shape == (lattice[1], lattice[0], 4)
        good, bad = compose.Canvas(1), compose.Canvas(1)
        good.draw_field(img)
        _draw_field_shifted(bad, img)
        assert (good.to_rgba8() != bad.to_rgba8()).any(axis=-1).sum() > 50, mode
        ref =cc.reference(1, img, None, None, compose.bar_rows(mode, 1), cc.no_text(1))
        keep = np.ones(ref.rgba.shape[:2], bool)
        keep[26:26 + 309, 680 - 32:680 - 22] = False                           # all but the bar: the helper draws the field as the canvas does
        assert np.array_equal(ref.rgba[keep], good.to_rgba8()[keep]) and not ref.dep.any()


@pytest.mark.parametrize("s,mode,aoa", [(1, 0, 9.0), (2, 1, -4.5), (1, 2, 9.0)])
def test_the_helper_equals_compose_on_the_natural_case(fields, s, mode, aoa):
    """Field, tracer-like strokes, NACA 4412, bar and the real labels: reference() draws what compose.compose draws."""
    from airfoil_cfd_tool_amd import geometry
    nx, ny = 200, 131
    img = fields((nx, ny, "float32"), mode)
    g = geometry.build_geometry(nx, ny, aoa, None, "naca4412")
    yh = geometry.domain_y_half(nx, ny)
    rng = np.random.default_rng(3)
    seg = np.column_stack([rng.uniform(-0.4, 1.3, 300), rng.uniform(-yh, yh, 300)])
    seg = np.column_stack([seg, seg + rng.uniform(-0.01, 0.02, (300, 2))])
    layer = compose.TrailLayer(s)
    for k in range(3):
        layer.fade()
        layer.stroke(compose.Canvas(s, alloc=False), seg[100 * k:100 * k + 100], rng.uniform(0, 1, 100), yh)
    want = compose.compose(img, g.xp, g.yp, aoa, mode, yh, trails=layer, scale=s)
    cx, cy = compose.Canvas(s, alloc=False).w2c(g.xp, g.yp, yh)
    ref = cc.reference(s, img, layer, np.column_stack([cx, cy]), compose.bar_rows(mode, s), compose.text_alpha_map(s, aoa, mode, yh))
    differ = (want != ref.rgba).any(axis=-1)
    assert differ.sum() == 0, (int(differ.sum()), np.argwhere(differ)[:4].tolist())
    assert (layer.a > 0.3).sum() > 100 and ref.dep.sum() > (layer.a > 0).sum()


@pytest.mark.parametrize("s", (1, 3))
def test_the_fill_is_half_open_in_x_and_in_y(s):
    """A rectangle with its vertices on pixel centres fills the centres a <= c < b on both axes (as k_canvas_compose does)."""
    for name in ("rect_on_centres", "rect_on_centres_turned", "diamond_on_centres"):
        p = cc.polygons(s)[name]
        cv = compose.Canvas(s)
        cv.fill_polygon(p[:, 0], p[:, 1], compose.FOIL_FILL)
        ys, xs = np.nonzero((cv.rgb == np.array(compose.FOIL_FILL, float)).all(axis=-1))
        x0, x1, y0, y1 = (int(v - 0.5) for v in (p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max()))
        if name.startswith("rect"):
            assert (xs.min(), xs.max(), ys.min(), ys.max()) == (x0, x1 - 1, y0, y1 - 1), name
            assert len(xs) == (x1 - x0) * (y1 - y0)
        else:       # the diamond: row y0 + k holds the centres from xc - k to xc + k - 1; the top apex's row [xc, xc) is empty
            xc = (x0 + x1) // 2
            for k in range(1, (y1 - y0) // 2 + 1):
                row = xs[ys == y0 + k]
                assert (row.min(), row.max(), len(row)) == (xc - k, xc + k - 1, 2 * k), (name, k)
            assert not (ys == y0).any() and not (ys == y1).any()
