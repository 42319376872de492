"""Lossless rotate / flip / transpose in the GPU transcode (mij_enc_add_coef_oriented, Transcoder.transcode(orientation=, edge=)) against
the host contract (mjh_transcode_memory_oriented, pinned by tests/test_transcode_orient_host.py) and the numpy model
(orient_coef_model.py): streams byte for byte for every layout, orientation, edge mode, plane format, front end and table kind; units at
block level; codability judged in destination order; mixed calls; the arena overflow; mixed slots on one encoder.

Shapes: per layout an MCU grid whose luma plane has more than 64 blocks and no multiple of 64 (a tile seam, dead lanes in the last
tile), the swapped grid (mcu_x != mcu_y either way), both also 3 px / 1 px short of the multiple, and the one-MCU picture."""
import functools

import numpy as np
import pytest
import torch  # before the library is first loaded: one HIP runtime for both (tensor_out._one_hip_runtime)

import exif_build as xb
import header_cases as hc
import orient_coef_model as om
import transcode_cases as tc
import transcode_planes as tp

pytestmark = pytest.mark.gpu

ARENA = 16 << 20
LAYOUTS = list(tp.LAYOUTS)
EDGES = ("perfect", "trim")
# luma planes of 77, 77, 84, 88 and 96 blocks
GRIDS = {"grey": (11, 7), "444": (11, 7), "422": (6, 7), "440": (11, 4), "420": (6, 4)}
QT = {0: [1 + (3 * k) % 200 for k in range(64)], 1: [2 + (7 * k) % 250 for k in range(64)]}

Pic = tp.Source


@functools.lru_cache(maxsize=None)
def pictures(layout):
    hv = tp.LAYOUTS[layout]
    g = GRIDS[layout]
    out = []
    for grid, short in ((g, False), (g, True), (g[::-1], False), (g[::-1], True), ((1, 1), False)):
        w, h = tp.size(layout, grid, short)
        planes = tp.address_planes(w, h, hv)
        data = hc.plain(w, h, hv, planes, qt=QT if len(hv) == 3 else {0: QT[0]}).bytes()
        out.append(Pic("%s %dx%d" % (layout, w, h), layout, w, h, hv, planes, data))
    assert 64 < out[0].planes[0].shape[0] * out[0].planes[0].shape[1] < 128
    return out


@functools.lru_cache(maxsize=None)
def host_stream(ica_mod, layout, i, o, trim, optimize):
    """the host contract's stream of picture i of a layout (None where it is refused) and its reason, computed once"""
    return ica_mod.transcode_memory(pictures(layout)[i].data, optimize=optimize, orientation=o, trim=trim)


def _model(pic, o, trim):
    try:
        return om.orient(pic.w, pic.h, pic.hv, pic.planes, o, trim)
    except om.Refused:
        return None


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_streams_equal_the_host_contract(ica, layout, fmt):
    """every orientation x edge mode x front end x table kind: one call per combination over the layout's five pictures"""
    pics = pictures(layout)
    datas = [p.data for p in pics]
    t = ica.Transcoder()
    try:
        t.set_coef_format(fmt)
        t.reserve_arena(4 << 20)
        refused = 0
        for gpu_entropy in (False, True):
            for optimize in (False, True):
                for o in om.ORIENTATIONS:
                    for edge in EDGES:
                        got = t.transcode(datas, optimize=optimize, copy_markers="none", gpu_entropy=gpu_entropy, orientation=o, edge=edge)
                        assert t.last_host_emitted == 0  # otherwise the host would be compared with itself
                        for i, p in enumerate(pics):
                            want, why = host_stream(ica, layout, i, o, edge == "trim", optimize)
                            assert got[i] == want, (p.name, o, edge, gpu_entropy, optimize)
                            assert (want is None) == (_model(p, o, edge == "trim") is None)
                            if want is None:
                                assert t.last_reasons[i].endswith(why) and "axis" in why, (p.name, o, edge)
                                refused += 1
                            else:
                                assert t.last_reasons[i] is None
        assert refused > 0
    finally:
        t.close()


def test_escaped_blocks_in_compact_planes(ica):
    src = tc.escaped_source()
    t = ica.Transcoder()
    try:
        t.set_coef_format("compact")
        for o in om.ORIENTATIONS:
            got = t.transcode([src], copy_markers="none", gpu_entropy=False, orientation=o, edge="trim")
            assert got == [ica.transcode_memory(src, optimize=True, orientation=o, trim=True)[0]] and got[0] is not None, o
            assert t._batch.slot_escapes(0) > 0
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
    """every (picture, orientation, edge mode) as a slot of ONE encoder -- sixteen conversion groups in one upload: plan and units of
    each slot are the model's, and the pictures the model refuses are refused at add_coef with the axis in the reason"""
    pics = pictures(layout)
    b = ica.Batch(gpu_ctx, len(pics), ARENA, ARENA, ARENA)
    enc = None
    try:
        b.set_coef_format(fmt)
        ok, sl, why = b.decode_jpegs([p.data for p in pics], 0, threads=4, gpu_entropy=False)
        assert ok == len(pics), why
        b.upload()
        combos = [(i, o, trim) for o in om.ORIENTATIONS for trim in (False, True) for i in range(len(pics))]
        want = {c: _model(pics[c[0]], c[1], c[2]) for c in combos}
        du_bytes = sum((w.units.shape[0] * 128 + 255) // 256 * 256 for w in want.values() if w is not None)
        enc = ica.Encoder(gpu_ctx, len(combos), 0, du_bytes + (1 << 20), stage_bytes=0)
        slots = {}
        for c in combos:
            i, o, trim = c
            if want[c] is None:
                with pytest.raises(ica.MijError, match="axis"):
                    enc.add_coef(b, sl[i], o, trim)
            else:
                slots[c] = enc.add_coef(b, sl[i], o, trim)
        assert len(slots) < len(combos)
        with pytest.raises(ica.MijError, match="1..8"):
            enc.add_coef(b, sl[0], 9)
        with pytest.raises(ica.MijError, match="1..8"):
            enc.add_coef(b, sl[0], 0, True)
        enc.upload()
        enc.launch()
        enc.wait()
        for c, slot in slots.items():
            w, plan = want[c], enc.tplan(slot)
            assert (plan.plan.width, plan.plan.height, plan.plan.mcu_x, plan.plan.mcu_y, plan.lh, plan.lv) == \
                (w.w, w.h, w.geom.mcu_x, w.geom.mcu_y, w.hv[0][0], w.hv[0][1]), c
            assert list(plan.plan.ytab) == list(om.orient_table(QT[0], c[1])), c
            _assert_units(enc.fetch(slot), w.units, "%s o %d trim %s (%s)" % (pics[c[0]].name, c[1], c[2], fmt))
    finally:
        if enc is not None:
            enc.close()
        b.close()


@pytest.mark.parametrize("fmt", ["compact", "int16"])
def test_codability_follows_the_destination(ica, fmt):
    """DC steps within +-2047 in source order and beyond it in a transposed order, and the converse: the device's verdict is the host's"""
    cases = [(layout, name, om.dc_grid(layout, values)) for layout in ("grey", "444") for name, values in (("rows", om.DC_ROWS_OK), ("cols", om.DC_COLS_OK))]
    good = pictures("420")[4].data
    datas = [good]
    for _, _, (_, data) in cases:
        datas += [data, good]
    t = ica.Transcoder()
    try:
        t.set_coef_format(fmt)
        t.reserve_arena(1 << 20)
        verdicts = set()
        for o in om.ORIENTATIONS:
            got = t.transcode(datas, optimize=False, copy_markers="none", gpu_entropy=False, orientation=o)
            assert t.last_host_emitted == 0
            want_good = ica.transcode_memory(good, orientation=o)[0]
            assert want_good is not None and all(g == want_good for g in got[0::2])
            for k, (layout, name, (planes, data)) in enumerate(cases):
                want, why = ica.transcode_memory(data, orientation=o)
                assert (want is not None) == om.codable(om.orient(16, 16, tp.LAYOUTS[layout], planes, o)), (layout, name, o)
                assert got[2 * k + 1] == want, (layout, name, o)
                if want is None:
                    assert "DC" in why and "not codable" in t.last_reasons[2 * k + 1], (layout, name, o)
                verdicts.add((name, o, want is not None))
        assert {("rows", 1, True), ("rows", 5, False), ("cols", 1, False), ("cols", 5, True)} <= verdicts
    finally:
        t.close()


def test_mixed_call(ica):
    """per-source orientations in one call: the file's tag, explicit ones, None, a refused non-perfect picture and an undecodable file;
    every source gets its own stream or its own reason, and the untransformed slots are today's bytes"""
    p420 = pictures("420")
    p422 = pictures("422")
    tagged6 = xb.tagged(p420[0].data, 6)
    tagged3 = xb.tagged(p422[2].data, 3, le=False)
    srcs = [p420[0].data, tagged6, p420[1].data, b"not a jpeg", p422[0].data, tagged3, p420[1].data, tagged6, p420[4].data]
    orients = [None, "exif", 2, 6, 5, "exif", 4, 1, 7]
    fixed = [1, 6, 2, 6, 5, 3, 4, 1, 7]
    t = ica.Transcoder()
    try:
        plain = t.transcode(srcs, copy_markers="all")
        got = t.transcode(srcs, copy_markers="all", orientation=orients, edge="perfect")
        reasons = list(t.last_reasons)
        assert t.last_host_emitted == 0
        for i, (s, o) in enumerate(zip(srcs, fixed)):
            want, why = ica.transcode_memory(s, optimize=True, copy_markers=True, orientation=o, trim=False)
            assert got[i] == want, i
            assert (reasons[i] is None) == (want is not None), i
            if o == 1:
                assert got[i] == plain[i] == ica.transcode_memory(s, optimize=True, copy_markers=True)[0], i
        assert [g is not None for g in got] == [True, True, False, False, True, True, False, True, True]
        assert "x axis" in reasons[2] and "y axis" in reasons[6] and "axis" not in reasons[3]
        assert [ica.exif_orientation(g) for g in (got[1], got[5], got[7])] == [1, 1, 6]
        # trim takes the two refused pictures; only_if_smaller never hands back the source of a picture that was turned
        trimmed = t.transcode(srcs, copy_markers="all", orientation=orients, edge="trim", only_if_smaller=True, optimize=False)
        for i, (s, o) in enumerate(zip(srcs, fixed)):
            want = ica.transcode_memory(s, optimize=False, copy_markers=True, orientation=o, trim=True)[0]
            assert trimmed[i] == (want if o != 1 or want is None or len(want) < len(s) else s), i
        assert [g is not None for g in trimmed] == [True, True, True, False, True, True, True, True, True]
        for bad in ({"orientation": 0}, {"orientation": 9}, {"orientation": "auto"}, {"orientation": [1, 2]}, {"orientation": True},
                    {"orientation": [1.5] * len(srcs)}, {"edge": "crop"}, {"edge": None}):
            with pytest.raises(ValueError):
                t.transcode(srcs, **bad)
    finally:
        t.close()


def test_arena_overflow_is_finished_on_the_host(ica):
    pics = pictures("420")[:4] + pictures("422")[:4]
    datas = [p.data for p in pics]
    orients = [5, 6, 7, 8, 2, 3, 4, 5]
    want = [ica.transcode_memory(d, optimize=True, orientation=o, trim=True)[0] for d, o in zip(datas, orients)]
    assert all(w is not None for w in want)
    t = ica.Transcoder()
    try:
        t.reserve_arena(4096)
        got = t.transcode(datas, copy_markers="none", orientation=orients, edge="trim")
        assert t.last_host_emitted > 0 and got == want
        got = t.transcode(datas, copy_markers="none", orientation=orients, edge="trim")
        assert t.last_host_emitted == 0 and got == want
    finally:
        t.close()


def test_one_encoder_mixed_slots(ica, gpu_ctx):
    """coefficient slots of two orientations from two batches (one compact, one int16), a pixel slot and a unit slot on one encoder:
    every coefficient slot's units are the model's and its stream the host's; the pixel and unit slots' streams are what they are alone"""
    A, B = pictures("420")[:2], pictures("440")[2:4]
    img = np.ascontiguousarray(np.random.default_rng(4).integers(0, 256, size=(40, 56, 3)).astype(np.uint8))
    plan, du = ica.host_transform(img, 90)
    alone = ica.emit_jpeg(plan, du)
    batches = []
    enc = None
    try:
        for fmt, pics in (("compact", A), ("int16", B)):
            b = ica.Batch(gpu_ctx, len(pics), ARENA, ARENA, ARENA)
            batches.append(b)
            b.set_coef_format(fmt)
            ok, sl, why = b.decode_jpegs([p.data for p in pics], 0, threads=2, gpu_entropy=False)
            assert ok == len(pics), why
            b.upload()
        enc = ica.Encoder(gpu_ctx, 8, 1 << 20, 4 << 20)
        enc.stream_reserve(4 << 20)
        s_px = enc.add(img, 90)
        c0 = enc.add_coef(batches[0], 0, 6, True)
        c1 = enc.add_coef(batches[1], 0, 3, True)
        s_du = enc.add_units(56, 40, 3, 90, du)
        c2 = enc.add_coef(batches[0], 1, 3, True)
        c3 = enc.add_coef(batches[1], 1, 6, True)
        c4 = enc.add_coef(batches[0], 0)
        enc.upload()
        enc.launch()
        enc.fetch_streams()
        for slot, pic, o in ((c0, A[0], 6), (c1, B[0], 3), (c2, A[1], 3), (c3, B[1], 6), (c4, A[0], 1)):
            _assert_units(enc.fetch(slot), om.orient(pic.w, pic.h, pic.hv, pic.planes, o, True).units, "%s o %d" % (pic.name, o))
            assert enc.slot_status(slot) == "ok"
            assert enc.stream(slot)[0] == ica.transcode_memory(pic.data, orientation=o, trim=True)[0], (pic.name, o)
        assert enc.stream(s_px)[0] == alone and enc.stream(s_du)[0] == alone
    finally:
        if enc is not None:
            enc.close()
        for b in batches:
            b.close()
