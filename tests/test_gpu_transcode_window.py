"""Lossless crop and greyscale in the GPU transcode (mij_enc_add_coef_window, Transcoder.transcode(crop=, grey=)) against the host
contract (mjh_transcode_memory_window, pinned by tests/test_transcode_window_host.py) and the numpy model (window_coef_model.py):
streams byte for byte for every layout, window, orientation, edge mode, grey on and off, table kind, plane format and front end; units
and plans at block level with plain and windowed slots mixed on one encoder; requantising with a window; the DC predecessor at the cut;
escaped blocks; a progressive source; the culled work list, counted; the arena overflow.

Pictures are test_gpu_transcode_orient.py's: luma planes of 77 to 96 blocks -- one tile seam, a last tile with dead lanes, strides that
do not divide 64 -- in both grid orders, whole and short of the MCU multiple, and the one-MCU picture, with address content."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before the library is first loaded: one HIP runtime for both (tensor_out._one_hip_runtime)

import header_cases as hc
import orient_coef_model as om
import requant_model as rm
import test_gpu_transcode_orient as O
import test_gpu_transcode_requant as R
import transcode_cases as tc
import transcode_planes as tp
import window_coef_model as wm

pytestmark = pytest.mark.gpu

ARENA = 16 << 20
LAYOUTS = list(tp.LAYOUTS)
EDGES = ("perfect", "trim")
OUTSIDE = (0, 0, 10 ** 6, 1)
pictures = O.pictures


@functools.lru_cache(maxsize=None)
def model(layout, i, o, trim, crop, grey):
    """the numpy model of one picture's transcode, computed once: Windowed, or the exception that refuses it"""
    p = pictures(layout)[i]
    try:
        return wm.window(p.w, p.h, p.hv, p.planes, o, trim, crop, grey)
    except (om.Refused, wm.Outside) as e:
        return e


def plane_tiles(w, h, hv):
    """every 64-block tile of every plane: what a plain slot queues"""
    return sum((bh * bw + 63) // 64 for bh, bw in hc.geometry(w, h, hv)[2])


def queued_tiles(w, h, hv, whole, m):
    """the tiles a slot's conversion reads: those that hold a kept block (the model's own count) for a windowed slot -- crop or grey
    changed the picture -- and every tile of the source's planes for a plain one, which is converted as it always was"""
    windowed = m.greyed or (m.rect is not None and m.rect != (0, 0, whole.w, whole.h))
    return m.tiles if windowed else plane_tiles(w, h, hv)


@functools.lru_cache(maxsize=None)
def cases(layout, o, trim, grey):
    """[(picture index, window name, crop)] for one orientation, edge mode and grey: every named window of every picture in the frame
    it is displayed in, one window for a picture the edge mode refuses, and one window outside its picture"""
    out = []
    for i in range(len(pictures(layout))):
        whole = model(layout, i, o, trim, None, grey)
        if isinstance(whole, Exception):
            out.append((i, "edge", (0, 0, 1, 1)))
            continue
        out += [(i, name, crop) for name, crop in wm.windows(whole.w, whole.h, whole.hv).items()]
    out.append((0, "outside", OUTSIDE))
    return out


@functools.lru_cache(maxsize=None)
def host_stream(ica_mod, layout, i, o, trim, crop, grey, optimize):
    return ica_mod.transcode_memory(pictures(layout)[i].data, optimize=optimize, orientation=o, trim=trim, crop=crop, grey=grey)


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_streams_equal_the_host_contract(ica, layout, fmt):
    """window x orientation x edge mode x grey x table kind x front end: one call per combination over every picture and window"""
    pics = pictures(layout)
    t = ica.Transcoder()
    try:
        t.set_coef_format(fmt)
        t.reserve_arena(8 << 20)
        refused = culled = 0
        for gpu_entropy in (False, True):
            for optimize in (False, True):
                for o in om.ORIENTATIONS:
                    for edge in EDGES:
                        for grey in (False, True):
                            trim = edge == "trim"
                            todo = cases(layout, o, trim, grey)
                            got = t.transcode([pics[i].data for i, _, _ in todo], optimize=optimize, copy_markers="none", gpu_entropy=gpu_entropy,
                                              orientation=o, edge=edge, crop=[c for _, _, c in todo], grey=grey)
                            assert t.last_host_emitted == 0  # otherwise the host would be compared with itself
                            tiles = 0
                            for k, (i, name, crop) in enumerate(todo):
                                what = (pics[i].name, name, crop, o, edge, grey, gpu_entropy, optimize)
                                want, why = host_stream(ica, layout, i, o, trim, crop, grey, optimize)
                                m = model(layout, i, o, trim, crop, grey)
                                assert got[k] == want and (want is None) == isinstance(m, Exception), what
                                if want is None:
                                    assert t.last_reasons[k].endswith(why) and ("axis" in why) == isinstance(m, om.Refused), what + (why,)
                                    assert name in ("edge", "outside") and ("1000000x1+0+0" in why) == isinstance(m, wm.Outside), what + (why,)
                                    refused += 1
                                    continue
                                assert t.last_reasons[k] is None and t.last_crops[k] == m.rect and t.last_greyed[k] == m.greyed, what
                                n = queued_tiles(pics[i].w, pics[i].h, pics[i].hv, model(layout, i, o, trim, None, grey), m)
                                culled += n < plane_tiles(pics[i].w, pics[i].h, pics[i].hv)
                                tiles += n
                            assert t._enc.coef_tiles() == tiles, (o, edge, grey, gpu_entropy, optimize)
        assert refused > 0 and culled > 0
    finally:
        t.close()


def _assert_units(got, want, what):
    if got.shape != want.shape:
        pytest.fail("%s: %s units, want %s" % (what, got.shape, want.shape))
    if not np.array_equal(got, want):
        diff = np.argwhere(got != want)
        u, k = (int(x) for x in diff[0])
        pytest.fail("%s: first difference at unit %d, k %d: got %d, want %d (%d coefficients in %d units differ)"
                    % (what, u, k, got[u, k], want[u, k], len(diff), len(set(diff[:, 0].tolist()))))


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_units_at_block_level(ica, gpu_ctx, layout, fmt):
    """every (picture, window, orientation, edge mode, grey) as a slot of ONE encoder -- plain and windowed conversion groups of every
    orientation in one upload: plan, kept rectangle and units of each slot are the model's, the refused ones are refused at add_coef,
    and a plain slot among them is what add_coef always made"""
    pics = pictures(layout)
    b = ica.Batch(gpu_ctx, len(pics), ARENA, ARENA, ARENA)
    enc = None
    try:
        b.set_coef_format(fmt)
        ok, sl, why = b.decode_jpegs([p.data for p in pics], 0, threads=4, gpu_entropy=False)
        assert ok == len(pics), why
        b.upload()
        combos = [(i, o, trim, grey, name, crop) for o in om.ORIENTATIONS for trim in (False, True) for grey in (False, True)
                  for i, name, crop in cases(layout, o, trim, grey)]
        want = {c: model(layout, c[0], c[1], c[2], c[5], c[3]) for c in combos}
        du_bytes = sum((w.units.shape[0] * 128 + 255) // 256 * 256 for w in want.values() if not isinstance(w, Exception))
        plain_want = tp.expected_units(pics[0])
        enc = ica.Encoder(gpu_ctx, len(combos) + 1, 0, du_bytes + plain_want.shape[0] * 128 + (1 << 20), stage_bytes=0)
        slots, tiles = {}, 0
        for n, c in enumerate(combos):
            i, o, trim, grey, name, crop = c
            if n == len(combos) // 2:
                plain = enc.add_coef(b, sl[0])
                tiles += plane_tiles(pics[0].w, pics[0].h, pics[0].hv)
            if isinstance(want[c], Exception):
                with pytest.raises(ica.MijError, match="axis" if isinstance(want[c], om.Refused) else "not croppable"):
                    enc.add_coef(b, sl[i], o, trim, crop=crop, grey=grey)
                continue
            slots[c] = enc.add_coef(b, sl[i], o, trim, crop=crop, grey=grey)
            tiles += queued_tiles(pics[i].w, pics[i].h, pics[i].hv, model(layout, i, o, trim, None, grey), want[c])
        assert 0 < len(slots) < len(combos)
        enc.upload()
        assert enc.coef_tiles() == tiles
        enc.launch()
        enc.wait()
        _assert_units(enc.fetch(plain), plain_want, "the plain slot")
        assert enc.slot_rect(plain) == (0, 0, pics[0].w, pics[0].h) and not enc.slot_windowed(plain) and not enc.slot_greyed(plain)
        ctab = O.QT[1 if len(pics[0].hv) == 3 else 0]
        for c, slot in slots.items():
            w, plan = want[c], enc.tplan(slot)
            assert (plan.plan.width, plan.plan.height, plan.plan.mcu_x, plan.plan.mcu_y, plan.lh, plan.lv, plan.ncomp, plan.plan.du_per_mcu) == \
                (w.w, w.h, w.geom.mcu_x, w.geom.mcu_y, w.hv[0][0], w.hv[0][1], len(w.hv), w.geom.dpm), c
            assert list(plan.plan.ytab) == list(om.orient_table(O.QT[0], c[1])), c
            assert list(plan.plan.ctab) == list(om.orient_table(ctab if len(w.hv) == 3 else O.QT[0], c[1])), c
            whole = model(layout, c[0], c[1], c[2], None, c[3])
            assert enc.slot_rect(slot) == (w.rect or (0, 0, whole.w, whole.h)) and enc.slot_greyed(slot) == w.greyed, c
            _assert_units(enc.fetch(slot), w.units, "%s %s o %d trim %s grey %s (%s)" % (pics[c[0]].name, c[4], c[1], c[2], c[3], fmt))
    finally:
        if enc is not None:
            enc.close()
        b.close()


@pytest.mark.parametrize("fmt", ["compact", "int16"])
def test_requantising_with_a_window(ica, gpu_ctx, fmt):
    """quality 75 and an explicit pair taken as it is, under orientation 6, a window and grey together and apart: units are requant_model
    over the window model's, tables the destination's; and a value that only the coarser step makes codable, inside the window"""
    pics = [R.pictures("420")[1], R.pictures("422")[0], R.pictures("444")[3], R.pictures("grey")[0], R.special("420")]
    targets = (R._tables_of(ica, {"quality": 75}), (R.EXPLICIT, False))
    b = ica.Batch(gpu_ctx, len(pics), ARENA, ARENA, ARENA)
    enc = None
    try:
        b.set_coef_format(fmt)
        ok, sl, why = b.decode_jpegs([p.data for p in pics], 0, threads=4, gpu_entropy=False)
        assert ok == len(pics), why
        b.upload()
        combos = []
        for i, p in enumerate(pics):
            for o, grey in ((6, True), (6, False), (1, True), (3, False)):
                whole = wm.window(p.w, p.h, p.hv, p.planes, o, True, None, grey)
                wins = wm.windows(whole.w, whole.h, whole.hv)
                combos += [(i, o, grey, wins[name], tgt) for name in ("unaligned", "last row", "whole") for tgt in targets]
        enc = ica.Encoder(gpu_ctx, len(combos), 0, 8 << 20, stage_bytes=0)
        slots = {c: enc.add_coef(b, sl[c[0]], c[1], True, c[4][0], c[4][1], crop=c[3], grey=c[2]) for c in combos}
        enc.upload()
        enc.launch()
        enc.wait()
        for c, slot in slots.items():
            i, o, grey, crop, (tables, coarsen) = c
            p = pics[i]
            w = wm.window(p.w, p.h, p.hv, p.planes, o, True, crop, grey)
            s = (om.orient_table(R.QT[0], o), om.orient_table(R.QT[1 if len(w.hv) == 3 else 0], o))
            d = rm.dest_tables(s, tables, coarsen)
            if len(w.hv) == 1:
                d = (d[0], d[0])
            plan = enc.tplan(slot)
            assert list(plan.plan.ytab) == list(d[0]) and list(plan.plan.ctab) == list(d[1]) and enc.slot_requantized(slot), c[:4]
            assert (plan.plan.width, plan.plan.height, plan.ncomp) == (w.w, w.h, len(w.hv)), c[:4]
            _assert_units(enc.fetch(slot), rm.requant_units(w.units, w.geom.ny, w.geom.dpm, s, d), "%s o %d grey %s crop %s (%s)" % (p.name, o, grey, crop, fmt))
    finally:
        if enc is not None:
            enc.close()
        b.close()
    # AC 1500 at step 1 in luma block 1: beyond the range as it is, 750 at step 2; the window holds that block alone
    big = R._one_value(5, 1500, 1)
    t = ica.Transcoder()
    try:
        t.set_coef_format(fmt)
        kw = {"optimize": False, "copy_markers": "none", "gpu_entropy": False, "crop": (8, 0, 8, 8), "grey": True}
        assert t.transcode([big], **kw) == [None] and "not codable" in t.last_reasons[0]
        assert ica.transcode_memory(big, crop=(8, 0, 8, 8), grey=True)[0] is None
        got = t.transcode([big], qtables=R.TWOS, **kw)
        want = ica.transcode_memory(big, tables=R.TWOS, crop=(8, 0, 8, 8), grey=True)[0]
        assert want is not None and got == [want] and t.last_host_emitted == 0 and t.last_requantized == [True]
        assert t.last_crops == [(8, 0, 8, 8)] and t.last_greyed == [True]
    finally:
        t.close()


# [[A, B], [C, D]] in every component: raster order is codable, but B follows 0 once the left column is cut away; and the reverse
DC_CUT_BREAKS = (1500, 3000, 1500, 3000)
DC_CUT_MENDS = (-1024, 1024, 0, 1024)


@pytest.mark.parametrize("fmt", ["compact", "int16"])
def test_dc_predecessor_at_the_cut(ica, fmt):
    """the first unit of a window predicts from 0, whatever lies left of the cut: the device's verdict is the host's, window by window"""
    srcs = [om.dc_grid(layout, values)[1] for layout in ("grey", "444") for values in (DC_CUT_BREAKS, DC_CUT_MENDS)]
    good = pictures("420")[4].data
    wins = [None, (8, 0, 8, 16), (0, 0, 8, 16), (0, 8, 16, 8), (8, 8, 8, 8)]
    t = ica.Transcoder()
    try:
        t.set_coef_format(fmt)
        t.reserve_arena(1 << 20)
        verdicts = set()
        for o in (1, 5, 3):
            for win in wins:
                datas = [good] + [d for s in srcs for d in (s, good)]
                got = t.transcode(datas, optimize=False, copy_markers="none", gpu_entropy=False, orientation=o, crop=[None] + [win, None] * len(srcs))
                assert t.last_host_emitted == 0
                want_good = ica.transcode_memory(good, orientation=o)[0]
                assert want_good is not None and all(g == want_good for g in got[0::2])
                for k, s in enumerate(srcs):
                    want, why = ica.transcode_memory(s, orientation=o, crop=win)
                    assert got[2 * k + 1] == want, (k, o, win)
                    if want is None:
                        assert "DC" in why and "not codable" in t.last_reasons[2 * k + 1], (k, o, win)
                    verdicts.add((k % 2, o, win, want is not None))
        assert {(0, 1, None, True), (0, 1, (8, 0, 8, 16), False), (1, 1, None, False), (1, 1, (8, 0, 8, 16), True)} <= verdicts
    finally:
        t.close()


def _tiles_of(ica, data, o, trim, crop, grey):
    """the tiles a source without known planes queues, from its frame header and the model's bookkeeping alone"""
    d = ica.HostDecoder.probe(data, 0)
    hv = [(d.comp[c].h, d.comp[c].v) for c in range(d.ncomp)]
    blank = hc.blank(d.width, d.height, hv)
    m = wm.window(d.width, d.height, hv, blank, o, trim, crop, grey)
    return queued_tiles(d.width, d.height, hv, wm.window(d.width, d.height, hv, blank, o, trim, None, grey), m), m


def _generic_source(ica, src, fmt, escapes):
    t = ica.Transcoder()
    try:
        t.set_coef_format(fmt)
        d = ica.HostDecoder.probe(src, 0)
        for o in (1, 6):
            for grey in (False, True):
                w, h = (d.width, d.height) if o == 1 else (d.height // 16 * 16, d.width)
                for crop in ((0, 0, w, h), (16, 16, 16, 16), (19, 5, w - 30, h - 9), (w - 1, h - 1, 1, 1)):
                    for gpu_entropy in (False, True):
                        got = t.transcode([src], copy_markers="none", gpu_entropy=gpu_entropy, orientation=o, edge="trim", crop=crop, grey=grey)
                        want = ica.transcode_memory(src, optimize=True, orientation=o, trim=True, crop=crop, grey=grey)[0]
                        assert got == [want] and want is not None and t.last_host_emitted == 0, (o, grey, crop, gpu_entropy)
                        n, m = _tiles_of(ica, src, o, True, crop, grey)
                        assert t._enc.coef_tiles() == n and t.last_crops == [m.rect] and t.last_greyed == [m.greyed]
                        if escapes:
                            assert t._batch.slot_escapes(0) > 0
    finally:
        t.close()


def test_escaped_blocks_inside_and_outside_the_window(ica):
    _generic_source(ica, tc.escaped_source(), "compact", True)


@pytest.mark.parametrize("fmt", ["compact", "int16"])
def test_progressive_source(ica, fmt):
    """the planes of a progressive source: blocks a non-interleaved scan never coded hold zeros, inside the window and outside"""
    src = dict(tc.layout_sources())["progressive 4:2:0 50x38"]
    _generic_source(ica, src, fmt, False)


def test_culling_of_a_large_picture(ica):
    """4:2:0, 40 x 40 MCUs: the whole picture queues 100 luma tiles and 25 for each chroma plane.  A one-MCU window in the last MCU row
    keeps luma blocks (78..79, 2..3) of a plane 80 blocks wide -- raster indices 6242, 6243, 6322 and 6323, which lie 80 apart and so
    in two tiles, 97 and 98 -- and block (39, 1) of each chroma plane: four tiles; grey, the two luma tiles alone"""
    hv = tp.LAYOUTS["420"]
    planes = hc.blank(640, 640, hv)
    for c, p in enumerate(planes):
        p[:, :, 0] = (np.arange(p.shape[0])[:, None] * 3 + np.arange(p.shape[1])[None] * 5 + c) % 200 - 100
        p[:, :, 1] = (np.arange(p.shape[0])[:, None] + np.arange(p.shape[1])[None]) % 7 - 3
    src = hc.plain(640, 640, hv, planes).bytes()
    crop = (16, 624, 16, 16)
    assert {(by * 80 + bx) // 64 for by in (78, 79) for bx in (2, 3)} == {97, 98} and (39 * 40 + 1) // 64 == 24
    t = ica.Transcoder()
    try:
        for kw, tiles in (({}, 150), ({"crop": crop}, 4), ({"crop": crop, "grey": True}, 2), ({"grey": True}, 100),
                          ({"crop": crop, "orientation": 3}, 4), ({"crop": (0, 0, 640, 640)}, 150)):
            got = t.transcode([src], copy_markers="none", gpu_entropy=False, **kw)
            want = ica.transcode_memory(src, optimize=True, orientation=kw.get("orientation"), crop=kw.get("crop"), grey=kw.get("grey", False))[0]
            assert got == [want] and want is not None, kw
            assert t._enc.coef_tiles() == tiles, kw
            m = wm.window(640, 640, hv, planes, kw.get("orientation", 1), False, kw.get("crop"), kw.get("grey", False))
            assert queued_tiles(640, 640, hv, wm.window(640, 640, hv, planes, 1, False, None, kw.get("grey", False)), m) == tiles
    finally:
        t.close()


def test_arena_overflow_is_finished_on_the_host(ica):
    pics = pictures("420")[:4] + pictures("422")[:4]
    datas = [p.data for p in pics]
    orients = [5, 6, 7, 8, 2, 3, 4, 1]
    crops = [(16, 16, 20, 9), None, (3, 3, 17, 17), (16, 0, 16, 16), None, (0, 8, 30, 30), (17, 9, 8, 8), (32, 8, 40, 30)]
    greys = [False, True, True, False, True, False, True, False]
    want = [ica.transcode_memory(d, optimize=True, orientation=o, trim=True, crop=c, grey=g)[0] for d, o, c, g in zip(datas, orients, crops, greys)]
    assert all(w is not None for w in want)
    t = ica.Transcoder()
    try:
        t.reserve_arena(2048)
        got = t.transcode(datas, copy_markers="none", orientation=orients, edge="trim", crop=crops, grey=greys)
        assert t.last_host_emitted > 0 and got == want
        got = t.transcode(datas, copy_markers="none", orientation=orients, edge="trim", crop=crops, grey=greys)
        assert t.last_host_emitted == 0 and got == want
    finally:
        t.close()


def test_arguments_and_mixed_call(ica):
    """badly shaped crop / grey raise before any device call; per-source windows with None among them, a window outside its picture
    and a file that is no JPEG each get their own stream or reason; only_if_smaller never hands back the source of a changed picture"""
    p420 = pictures("420")
    srcs = [p420[0].data, p420[1].data, b"not a jpeg", p420[0].data, p420[2].data, pictures("grey")[0].data]
    t = ica.Transcoder()
    try:
        for bad in ({"crop": (0, 0, 8)}, {"crop": (0, 0, 8, 0)}, {"crop": (0, 0, 0, 8)}, {"crop": (0.0, 0, 8, 8)}, {"crop": "0,0,8,8"}, {"crop": 5},
                    {"crop": [(0, 0, 8, 8)] * 2}, {"crop": [None] * 5 + [(0, 0, True, 8)]}, {"grey": 1}, {"grey": None}, {"grey": [True] * 5},
                    {"grey": [True] * 5 + [0]}, {"grey": "yes"}):
            with pytest.raises(ValueError):
                t.transcode(srcs, **bad)
        assert t._ctx is None  # refused before a device was touched
        crops = [(16, 16, 16, 16), None, (0, 0, 8, 8), (90, 0, 16, 16), (0, 0, p420[2].w, p420[2].h), (8, 8, 16, 16)]
        greys = [False, True, True, False, False, True]
        got = t.transcode(srcs, copy_markers="all", only_if_smaller=True, optimize=False, crop=crops, grey=greys)
        assert t.last_host_emitted == 0
        for i, s in enumerate(srcs):
            want, why = ica.transcode_memory(s, copy_markers=True, crop=crops[i], grey=greys[i])
            changed = i in (0, 1, 5)  # source 4's window is its whole picture, and colour: nothing changed
            assert got[i] == (want if want is None or changed or len(want) < len(s) else s), i
            assert (t.last_reasons[i] is None) == (want is not None), i
        assert [g is not None for g in got] == [True, True, False, False, True, True]
        assert "96x64" in t.last_reasons[3].replace(" x ", "x") and "16x16+90+0" in t.last_reasons[3]
        assert t.last_crops == [(16, 16, 16, 16), None, None, None, (0, 0, p420[2].w, p420[2].h), (8, 8, 16, 16)]
        assert t.last_greyed == [False, True, False, False, False, False]
    finally:
        t.close()


@pytest.mark.parametrize("fmt", ["compact", "int16"])
def test_windowed_slots_past_4_gib(ica, gpu_ctx, oracle, fmt):
    """in the manner of test_gpu_far_slots.test_transcode_from_far_planes_into_far_units: windowed and grey slots whose planes lie
    behind byte 2^32 of the coefficient arena and whose units lie behind byte 2^32 of the unit arena (the first straddles it), so that
    the origin's block offsets and the DC predecessor's index are added to 64-bit plane offsets.  Units are the model's, streams the
    host's, and the spacers in front of the line are untouched"""
    import far_slots as F

    class FarWindowEncoder(F.FarEncoder):
        def add_coef_window(self, batch, slot, orientation, trim, crop, grey):
            s = self.enc.add_coef(batch, slot, orientation, trim, crop=crop, grey=grey)
            p = self.enc.plan(s)
            return self._under_test(s, p.width, p.height, p.comp, 0, False)

    pics = [pictures("420")[0], pictures("422")[1], pictures("444")[2], pictures("grey")[0]]
    fb = F.FarBatch(ica, gpu_ctx, oracle, 3, fmt, [(p.data, 0) for p in pics])  # req_comp 0, as Transcoder decodes
    fe = None
    try:
        b = fb.b
        b.upload()
        b.wait()
        combos = [(0, 1, (16, 16, 80, 48), False)]  # 5 x 3 MCUs of 4:2:0: 90 units, more than the 4096 bytes in front of the line
        for i, p in enumerate(pics):
            for o, grey in ((1, True), (6, False), (3, True)):
                whole = wm.window(p.w, p.h, p.hv, p.planes, o, True, None, grey)
                wins = wm.windows(whole.w, whole.h, whole.hv)
                combos += [(i, o, wins[name], grey) for name in ("last row", "unaligned", "whole")]
        fe = FarWindowEncoder(ica, gpu_ctx, len(combos))
        slots = [(c, fe.add_coef_window(b, fb.slots[c[0]], c[1], True, c[2], c[3])) for c in combos]
        fe.premise()
        optimized = {s for k, s in enumerate(fe.slots) if k & 1}
        for s in optimized:
            fe.enc.set_optimize(s)
        fe.enc.upload()
        fe.enc.launch()
        fe.enc.fetch_streams()
        for (i, o, crop, grey), slot in slots:
            p = pics[i]
            w = wm.window(p.w, p.h, p.hv, p.planes, o, True, crop, grey)
            _assert_units(fe.enc.fetch(slot), w.units, "%s o %d crop %s grey %s (%s) unit offset %d" % (p.name, o, crop, grey, fmt, fe.du_off[slot]))
            host = ica.transcode_memory(p.data, optimize=slot in optimized, orientation=o, trim=True, crop=crop, grey=grey)[0]
            assert host is not None and fe.enc.slot_status(slot) == "ok" and fe.enc.stream(slot)[0] == host, (p.name, o, crop, grey)
        fe.check_spacers()
    finally:
        if fe is not None:
            fe.close()
        fb.close()
