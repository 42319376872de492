"""Greyscale and crop in the transcode, the host contract (include/mij_host.h, mjw_tplan_grey / mjw_tplan_cropped /
mjh_transcode_memory_window): plans, units, streams and refusals against the numpy model (window_coef_model.py) for every transcodable
layout, orientation, edge mode, grey on and off and the named windows; pixels through the oracle; codability in window order; the mirror
that only a grey picture can take.  No GPU."""
import functools

import numpy as np
import pytest

import header_cases as hc
import orient_coef_model as om
import transcode_planes as tp
import window_coef_model as wm

LAYOUTS = list(tp.LAYOUTS)
EDGES = (False, True)  # trim
QT = {0: [1 + (3 * k) % 200 for k in range(64)], 1: [2 + (7 * k) % 250 for k in range(64)]}


def sizes(layout):
    """an exact multiple of the MCU with mcu_x != mcu_y, and a partial MCU on both axes"""
    a, v = tp.LAYOUTS[layout][0]
    mw, mh = 8 * a, 8 * v
    return [(4 * mw, 3 * mh), (3 * mw + 5, 4 * mh - 2)]


@functools.lru_cache(maxsize=None)
def picture(layout, w, h):
    hv = tp.LAYOUTS[layout]
    planes = tp.address_planes(w, h, hv)
    return planes, hc.plain(w, h, hv, planes, qt=QT if len(hv) == 3 else {0: QT[0]}).bytes()


@functools.lru_cache(maxsize=None)
def source_units(ica_mod, layout, w, h):
    desc, region = ica_mod.host_decode_staged(picture(layout, w, h)[1], 0, want_compact=False)
    t, why = ica_mod.transcode_plan(desc)
    assert t is not None, why
    return t, ica_mod.units_from_region(desc, region, False)


def _host(ica, layout, w, h, o, trim, crop, grey):
    """the contract's steps one by one -> (plan, units, kept rectangle) or (None, reason, None)"""
    t, du = source_units(ica, layout, w, h)
    if grey:
        du = ica.units_grey(t, du)
        t = ica.transcode_plan_grey(t)
    dst, why = ica.transcode_plan_oriented(t, o, trim)
    if dst is None:
        return None, why, None
    du = ica.units_orient(t, du, o, trim)
    t, rect = dst, None
    if crop is not None:
        dst, rect = ica.transcode_plan_cropped(t, crop)
        if dst is None:
            return None, rect, None
        du = ica.units_crop(t, du, rect)
        t = dst
    return t, du, rect


@pytest.mark.parametrize("trim", EDGES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_plans_and_units_equal_the_model(ica, layout, trim):
    hv = tp.LAYOUTS[layout]
    seen, grown = set(), 0
    for w, h in sizes(layout):
        planes, data = picture(layout, w, h)
        for grey in (False, True):
            for o in om.ORIENTATIONS:
                try:
                    whole = wm.window(w, h, hv, planes, o, trim, None, grey)
                except om.Refused as e:
                    t, why, _ = _host(ica, layout, w, h, o, trim, None, grey)
                    assert t is None and ("%s axis" % e.axis) in why and ("MCU size %d" % e.mcu) in why, (w, h, o, grey, why)
                    assert ica.transcode_memory(data, orientation=o, trim=trim, grey=grey, crop=(0, 0, 1, 1))[0] is None
                    seen.add("edge")
                    continue
                assert whole.hv[0] == ((1, 1) if grey else whole.hv[0]) and whole.greyed == (grey and len(hv) == 3)
                for name, crop in [(None, None)] + list(wm.windows(whole.w, whole.h, whole.hv).items()):
                    want = wm.window(w, h, hv, planes, o, trim, crop, grey)
                    t, du, rect = _host(ica, layout, w, h, o, trim, crop, grey)
                    what = (w, h, o, grey, name, crop)
                    assert t is not None, what + (du,)
                    assert rect == want.rect, what
                    g = want.geom
                    assert (t.plan.width, t.plan.height, t.plan.mcu_x, t.plan.mcu_y) == (want.w, want.h, g.mcu_x, g.mcu_y), what
                    assert (t.lh, t.lv, t.ncomp, t.plan.du_per_mcu, t.plan.comp) == (want.hv[0][0], want.hv[0][1], len(want.hv), g.dpm, len(want.hv)), what
                    assert t.plan.subsample == (1 if want.hv[0] == (2, 2) else 0)
                    assert list(t.plan.ytab) == list(om.orient_table(QT[0], o)), what
                    assert list(t.plan.ctab) == list(om.orient_table(QT[1 if len(want.hv) == 3 else 0], o)), what
                    assert du.shape == want.units.shape and np.array_equal(du, want.units), what
                    if name == "unaligned":
                        assert rect[0] < crop[0] and rect[1] < crop[1] and rect[0] + rect[2] == crop[0] + crop[2] and rect[1] + rect[3] == crop[1] + crop[3]
                        assert rect[0] % (8 * want.hv[0][0]) == 0 and rect[1] % (8 * want.hv[0][1]) == 0
                        grown += 1
                    # the whole chain's stream is the emission of these units, and the whole picture is the call without a crop
                    for optimize in (False, True):
                        got, why = ica.transcode_memory(data, optimize=optimize, orientation=o, trim=trim, crop=crop, grey=grey)
                        assert got is not None and got == ica.emit_transcoded(t, du, optimize), what + (why,)
                        if name == "whole":
                            assert got == ica.transcode_memory(data, optimize=optimize, orientation=o, trim=trim, grey=grey)[0], what
                            if not whole.greyed:
                                assert got == ica.transcode_memory(data, optimize=optimize, orientation=o, trim=trim)[0], what
                    seen.add("ok")
                for bad in wm.REFUSALS:
                    crop = bad(whole.w, whole.h)
                    with pytest.raises(wm.Outside):
                        wm.window(w, h, hv, planes, o, trim, crop, grey)
                    t, why, _ = _host(ica, layout, w, h, o, trim, crop, grey)
                    assert t is None and ("%dx%d+%d+%d" % (crop[2], crop[3], crop[0], crop[1])) in why and ("(%d x %d)" % (whole.w, whole.h)) in why, why
                    got, why2 = ica.transcode_memory(data, orientation=o, trim=trim, crop=crop, grey=grey)
                    assert got is None and why2 == why
                    seen.add("outside")
    assert seen == ({"ok", "outside"} if trim else {"ok", "edge", "outside"}) and grown > 0  # the trim leaves nothing to refuse at these sizes


def _smooth(layout, w, h, seed, flat=False):
    """small DCs and a few small ACs under mild tables: pixels stay inside 0..255, so no clamp hides a wrong block.  flat: DCs only"""
    hv = tp.LAYOUTS[layout]
    planes = hc.blank(w, h, hv)
    rng = np.random.default_rng(seed)
    for p in planes:
        p[:, :, 0] = rng.integers(-40, 41, size=p.shape[:2])
        if not flat:
            p[:, :, 1:6] = rng.integers(-6, 7, size=p.shape[:2] + (5,))
    qt = {0: [8] + [4] * 63, 1: [8] + [5] * 63}
    return hc.plain(w, h, hv, planes, qt=qt if len(hv) == 3 else {0: qt[0]}).bytes()


@pytest.mark.parametrize("layout", ["grey", "444"])
def test_cropped_pixels_are_the_crop_of_the_pixels(ica, oracle, layout):
    """no upsampling in these layouts and every block decodes on its own: with the origin on the MCU grid the cropped stream decodes to
    exactly the crop of the source's decode.  Under an orientation the same holds for DC-only blocks, which decode flat (a decoder's
    integer IDCT of a mirrored or transposed block is not the mirrored or transposed IDCT to the last bit)"""
    w, h = 45, 38
    for flat in (False, True):
        _cropped_pixels(ica, oracle, _smooth(layout, w, h, 7, flat), w, h, om.ORIENTATIONS if flat else (1,))


def _cropped_pixels(ica, oracle, data, w, h, orientations):
    kind, src_px, _ = oracle.load(data, 0)
    assert kind == "ok" and len(np.unique(src_px)) > 20
    for o in orientations:
        disp = om.orient_pixels(src_px[:h // 8 * 8 if o in om.MIRROR_Y else h, :w // 8 * 8 if o in om.MIRROR_X else w], o)
        dh, dw = disp.shape[:2]
        for crop in ((8, 16, 24, 8), (16, 8, dw - 16, dh - 8), (0, 0, 9, 5), (dw - dw % 8 - 8, dh - dh % 8 - 8, 8, 8)):
            out, why = ica.transcode_memory(data, orientation=o, trim=True, crop=crop)
            assert out is not None, (o, crop, why)
            kind, px, _ = oracle.load(out, 0)
            x0, y0, cw, ch = crop
            assert kind == "ok" and np.array_equal(px, disp[y0:y0 + ch, x0:x0 + cw]), (o, crop)


@pytest.mark.parametrize("layout", ["444", "422", "440", "420"])
def test_grey_keeps_the_luma_pixels(ica, oracle, layout):
    a, v = tp.LAYOUTS[layout][0]
    w, h = 3 * 8 * a - 3, 2 * 8 * v + 5
    data = _smooth(layout, w, h, 9)
    kind, want, _ = oracle.load(data, 1)
    assert kind == "ok" and len(np.unique(want)) > 50
    out, why = ica.transcode_memory(data, grey=True)
    assert out is not None, why
    kind, px, _ = oracle.load(out, 1)
    assert kind == "ok" and np.array_equal(px, want)
    desc = ica.HostDecoder.probe(out, 0)
    assert (desc.ncomp, desc.width, desc.height) == (1, w, h)
    # and a window of it, origin on the 8 x 8 grid that a grey picture has whatever the source's MCU was
    out, why = ica.transcode_memory(data, grey=True, crop=(8, 8, w - 8, h - 8))
    assert out is not None, why
    kind, px, _ = oracle.load(out, 1)
    assert kind == "ok" and np.array_equal(px, want[8:, 8:])


# [[A, B], [C, D]]: raster order is codable, but B follows 0 once the left column is cut away; and the reverse
DC_CUT_BREAKS = (1500, 3000, 1500, 3000)
DC_CUT_MENDS = (-1024, 1024, 0, 1024)
RIGHT_COLUMN = (8, 0, 8, 16)


@pytest.mark.parametrize("layout", ["grey", "444"])
def test_codability_is_judged_in_window_order(ica, layout):
    hv = tp.LAYOUTS[layout]
    for values, whole_ok, window_ok in ((DC_CUT_BREAKS, True, False), (DC_CUT_MENDS, False, True)):
        planes, data = om.dc_grid(layout, values)
        assert om.codable(om.orient(16, 16, hv, planes, 1)) == whole_ok
        assert wm.codable(wm.window(16, 16, hv, planes, crop=RIGHT_COLUMN)) == window_ok
        out, why = ica.transcode_memory(data)
        assert (out is not None) == whole_ok and (whole_ok or "DC" in why)
        out, why = ica.transcode_memory(data, crop=RIGHT_COLUMN)
        assert (out is not None) == window_ok and (window_ok or "DC" in why)
        if window_ok:
            d2, r2 = ica.host_decode_staged(out, 0, want_compact=False)
            assert np.array_equal(ica.units_from_region(d2, r2, False), wm.window(16, 16, hv, planes, crop=RIGHT_COLUMN).units)


def test_grey_rescues_a_mirror(ica):
    """a 4:2:0 picture whose mirrored axis is a multiple of 8 but not of 16: refused as it is under edge="perfect", exact once grey.
    Orientation 4 mirrors y, so the axis that matters is the height: 20 x 24; the same picture lying down (24 x 20) under orientation 2"""
    hv = tp.LAYOUTS["420"]
    for (w, h), o, axis in (((20, 24), 4, "y"), ((24, 20), 2, "x")):
        planes, data = picture("420", w, h)
        out, why = ica.transcode_memory(data, orientation=o)
        assert out is None and ("%s axis" % axis) in why and "MCU size 16" in why
        out, why = ica.transcode_memory(data, orientation=o, grey=True)
        assert out is not None, why
        want = wm.window(w, h, hv, planes, o, False, None, True)
        assert (want.w, want.h) == (w, h)  # nothing trimmed
        d2, r2 = ica.host_decode_staged(out, 0, want_compact=False)
        assert d2.ncomp == 1 and np.array_equal(ica.units_from_region(d2, r2, False), want.units)
        # the other axis is no multiple of 8: mirroring it stays refused, grey or not
        assert ica.transcode_memory(data, orientation=3, grey=True)[0] is None


def test_markers_and_requant_compose(ica):
    """crop and grey with copied markers and new tables: the chain is requant(crop(orient(grey(source)))), and the no-crop, no-grey call
    stays byte for byte what it was"""
    import requant_model as rm
    planes, data = picture("420", 53, 38)
    tables = rm.quality_tables(60)
    com = b"\xff\xfe\x00\x07hello"
    src = data[:2] + com + data[2:]
    for o in (1, 6):
        plain = ica.transcode_memory(src, optimize=True, copy_markers=True, orientation=o, trim=True, tables=tables)[0]
        assert plain is not None and com in plain
        w2, h2 = (53, 38) if o == 1 else (32, 53)
        assert ica.transcode_memory(src, optimize=True, copy_markers=True, orientation=o, trim=True, tables=tables, crop=(0, 0, w2, h2))[0] == plain
        out, why = ica.transcode_memory(src, optimize=True, copy_markers=True, orientation=o, trim=True, tables=tables, crop=(16, 16, 10, 9), grey=True)
        assert out is not None and com in out, why
        want = wm.window(53, 38, tp.LAYOUTS["420"], planes, o, True, (16, 16, 10, 9), True)
        s = om.orient_table(QT[0], o)
        d = rm.dest_tables((s, s), tables)
        d2, r2 = ica.host_decode_staged(out, 0, want_compact=False)
        assert np.array_equal(ica.units_from_region(d2, r2, False), rm.requant_units(want.units, 1, 1, (s, s), (d[0], d[0])))
