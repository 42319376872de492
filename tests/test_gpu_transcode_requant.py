"""Requantisation in the GPU transcode (mij_enc_add_coef_requant, Transcoder.transcode(quality=, qtables=, coarsen_only=)) against the
host contract (mjh_transcode_memory_requant, pinned by tests/test_transcode_requant_host.py) and the numpy model (requant_model.py):
streams byte for byte for every layout, orientation, edge mode, plane format and front end; units and plans at block level with ties,
values that vanish, the codable edge and the clamp; codability judged on the result; mixed calls; the arena overflow.

Shapes are test_gpu_transcode_orient.py's: per layout an MCU grid whose luma plane has 77 to 96 blocks (a tile seam, dead lanes in the
last tile), the swapped grid, both also short of the MCU multiple, and the one-MCU picture."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before the library is first loaded: one HIP runtime for both (tensor_out._one_hip_runtime)

import header_cases as hc
import orient_coef_model as om
import requant_model as rm
import transcode_cases as tc
import transcode_planes as tp

pytestmark = pytest.mark.gpu

ARENA = 16 << 20
LAYOUTS = list(tp.LAYOUTS)
GRIDS = {"grey": (11, 7), "444": (11, 7), "422": (6, 7), "440": (11, 4), "420": (6, 4)}
# two distinct tables whose entries stay within 8..20, so that the explicit target below is finer by less than four times wherever it
# is finer, whatever the transposition: with coefficients within +-128 every result stays codable
QT = {0: [8 + (5 * k) % 9 for k in range(64)], 1: [10 + (7 * k) % 11 for k in range(64)]}
EXPLICIT = (tuple(6 if k % 2 == 0 else 40 for k in range(64)), tuple(7 if k % 2 == 0 else 50 for k in range(64)))
ONES = ((1,) * 64, (1,) * 64)
TWOS = ((2,) * 64, (2,) * 64)
# (name, Transcoder arguments): quality 50, the explicit pair taken as it is, and the identity (every entry 1, coarsened to the source's)
TARGETS = (("q50", {"quality": 50}), ("explicit", {"qtables": EXPLICIT, "coarsen_only": False}), ("identity", {"quality": 100}))

Pic = tp.Source


def _tables_of(ica_mod, kw):
    """the (luma, chroma) target and coarsen_only that Transcoder arguments stand for, hashable"""
    if "quality" in kw:
        return tuple(tuple(int(v) for v in t) for t in ica_mod.quality_tables(kw["quality"])), kw.get("coarsen_only", True)
    return kw["qtables"], kw.get("coarsen_only", True)


def _write(name, layout, w, h, planes, qt=QT):
    hv = tp.LAYOUTS[layout]
    return Pic(name, layout, w, h, hv, planes, hc.plain(w, h, hv, planes, qt=qt if len(hv) == 3 else {0: qt[0]}).bytes())


@functools.lru_cache(maxsize=None)
def pictures(layout):
    """address content scaled into -128..127"""
    hv = tp.LAYOUTS[layout]
    g = GRIDS[layout]
    out = []
    for grid, short in ((g, False), (g, True), (g[::-1], False), (g[::-1], True), ((1, 1), False)):
        w, h = tp.size(layout, grid, short)
        planes = [p >> 3 for p in tp.address_planes(w, h, hv)]
        out.append(_write("%s %dx%d" % (layout, w, h), layout, w, h, planes))
    assert 64 < out[0].planes[0].shape[0] * out[0].planes[0].shape[1] < 128
    return out


@functools.lru_cache(maxsize=None)
def special(layout):
    """the layout's first grid, short of the multiple, with chosen AC values: for source step a and explicit step b at position k, the
    integers on both sides of the ties |c| a = (j + 1/2) b (j = 0 gives the values that round to zero), of the results +-1023 / +-1024,
    and +-32767, which needs the clamp wherever b < a; block L takes candidate (L + k) mod n at k.  DCs are the address ones."""
    hv = tp.LAYOUTS[layout]
    w, h = tp.size(layout, GRIDS[layout], True)
    planes = [p >> 3 for p in tp.address_planes(w, h, hv)]
    for c, p in enumerate(planes):
        a = np.array(QT[0 if c == 0 else 1], np.int64)[1:]
        b = np.array(EXPLICIT[0 if c == 0 else 1], np.int64)[1:]
        cand = []
        for j in (0, 1, 7):
            lo = ((2 * j + 1) * b) // (2 * a)
            cand += [lo, lo + 1]
        edge = (2047 * b) // (2 * a)  # |c| a / b = 1023.5
        cand += [edge - 1, edge, edge + 1, edge + 2, np.full_like(a, 32767)]
        cand = np.stack([s * np.minimum(x, 32767) for x in cand for s in (1, -1)])  # [n, 63]
        L = np.arange(p.shape[0] * p.shape[1]).reshape(p.shape[0], p.shape[1])
        idx = (L[:, :, None] + np.arange(1, 64)[None, None]) % cand.shape[0]
        p[:, :, 1:] = cand[idx, np.arange(63)[None, None]]
    return _write("special %s %dx%d" % (layout, w, h), layout, w, h, planes)


@functools.lru_cache(maxsize=None)
def host_stream(ica_mod, layout, i, o, trim, optimize, tables, coarsen):
    return ica_mod.transcode_memory(pictures(layout)[i].data, optimize=optimize, orientation=o, trim=trim, tables=tables, coarsen_only=coarsen)


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_streams_equal_the_host_contract(ica, layout, fmt):
    """every orientation x edge mode x front end x target, optimised tables; the Annex-K tables as well at orientation 1"""
    pics = pictures(layout)
    datas = [p.data for p in pics]
    t = ica.Transcoder()
    try:
        t.set_coef_format(fmt)
        t.reserve_arena(4 << 20)
        refused = emitted = 0
        for gpu_entropy in (False, True):
            for o in om.ORIENTATIONS:
                for edge in ("perfect", "trim"):
                    for name, kw in TARGETS:
                        tables, coarsen = _tables_of(ica, kw)
                        for optimize in ((True, False) if o == 1 and edge == "perfect" else (True,)):
                            got = t.transcode(datas, optimize=optimize, copy_markers="none", gpu_entropy=gpu_entropy, orientation=o, edge=edge, **kw)
                            assert t.last_host_emitted == 0  # otherwise the host would be compared with itself
                            for i, p in enumerate(pics):
                                want, why = host_stream(ica, layout, i, o, edge == "trim", optimize, tables, coarsen)
                                assert got[i] == want, (p.name, o, edge, gpu_entropy, optimize, name)
                                if want is None:
                                    assert t.last_reasons[i].endswith(why) and "axis" in why, (p.name, o, edge, name)
                                    refused += 1
                                else:
                                    assert t.last_reasons[i] is None and t.last_requantized[i] == (name != "identity")
                                    emitted += 1
                                    if name == "identity":
                                        assert want == ica.transcode_memory(p.data, optimize=optimize, orientation=o, trim=edge == "trim")[0]
        assert refused > 0 and emitted > refused
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


def _model(ica, pic, o, trim, target):
    """-> (Oriented, destination tables, units) of the numpy models; target None: no requantisation"""
    w = om.orient(pic.w, pic.h, pic.hv, pic.planes, o, trim)
    s = (om.orient_table(QT[0], o), om.orient_table(QT[1 if len(pic.hv) == 3 else 0], o))
    if target is None:
        return w, s, w.units
    tables, coarsen = target
    d = rm.dest_tables(s, tables, coarsen)
    if len(pic.hv) == 1:
        d = (d[0], d[0])
    return w, d, rm.requant_units(w.units, w.geom.ny, w.geom.dpm, s, d)


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_units_at_block_level(ica, gpu_ctx, layout, fmt):
    """plain, oriented and requantising slots of ONE encoder in one upload: plan, tables and units of every slot are the models'.  The
    special picture holds ties in both signs, values that round to zero, results on both sides of +-1023 and values that need the clamp."""
    pics = pictures(layout)[:4] + [special(layout)]
    sp = pics[-1]
    explicit = (EXPLICIT, False)
    q50 = _tables_of(ica, {"quality": 50})
    # the content is what the docstring says, by the model: ties, zeros from non-zero values, +-1023, +-1024 and clamped results
    m = _model(ica, sp, 1, True, explicit)[2].astype(np.int64)
    src = om.orient(sp.w, sp.h, sp.hv, sp.planes, 1, True).units.astype(np.int64)
    assert ((m == 0) & (src != 0)).any() and all((m[:, 1:] == v).any() for v in (1023, -1023, 1024, -1024, 32767, -32767))
    a = np.array(QT[0])[None]
    b = np.array(EXPLICIT[0])[None]
    lum = src[np.arange(src.shape[0]) % _model(ica, sp, 1, True, None)[0].geom.dpm < _model(ica, sp, 1, True, None)[0].geom.ny]
    ties = (2 * np.abs(lum * a)) % (2 * b) == b
    assert (ties & (lum > 0)).any() and (ties & (lum < 0)).any()
    b_ = ica.Batch(gpu_ctx, len(pics), ARENA, ARENA, ARENA)
    enc = None
    try:
        b_.set_coef_format(fmt)
        ok, sl, why = b_.decode_jpegs([p.data for p in pics], 0, threads=4, gpu_entropy=False)
        assert ok == len(pics), why
        b_.upload()
        combos = [(i, o, True, tgt) for i in range(len(pics)) for o in om.ORIENTATIONS for tgt in (explicit,)]
        combos += [(i, o, True, q50) for i in (0, 4) for o in (1, 6)]
        combos += [(i, o, True, None) for i in (0, 4) for o in (1, 3, 5)]
        combos += [(4, 1, False, (ONES, True)), (4, 7, True, (ONES, True))]  # identity: plain slots
        want = {c: _model(ica, pics[c[0]], c[1], c[2], c[3]) for c in combos}
        du_bytes = sum((w[2].shape[0] * 128 + 255) // 256 * 256 for w in want.values())
        enc = ica.Encoder(gpu_ctx, len(combos), 0, du_bytes + (1 << 20), stage_bytes=0)
        slots = {}
        for c in combos:
            i, o, trim, tgt = c
            slots[c] = enc.add_coef(b_, sl[i], o, trim) if tgt is None else enc.add_coef(b_, sl[i], o, trim, tgt[0], tgt[1])
        with pytest.raises(ica.MijError, match="axis"):
            enc.add_coef(b_, sl[1], 2, False, EXPLICIT, False)
        enc.upload()
        enc.launch()
        enc.wait()
        for c, slot in slots.items():
            (w, d, units), plan = want[c], enc.tplan(slot)
            assert (plan.plan.width, plan.plan.height, plan.plan.mcu_x, plan.plan.mcu_y, plan.lh, plan.lv) == \
                (w.w, w.h, w.geom.mcu_x, w.geom.mcu_y, w.hv[0][0], w.hv[0][1]), c[:3]
            assert list(plan.plan.ytab) == list(d[0]) and list(plan.plan.ctab) == list(d[1]), c[:3]
            assert enc.slot_requantized(slot) == (c[3] is not None and c[3][0] is not ONES), c[:3]
            _assert_units(enc.fetch(slot), units, "%s o %d trim %s target %s (%s)" % (pics[c[0]].name, c[1], c[2], "none" if c[3] is None else c[3][1], fmt))
    finally:
        if enc is not None:
            enc.close()
        b_.close()


def test_escaped_blocks_in_compact_planes(ica):
    src = tc.escaped_source()
    t = ica.Transcoder()
    try:
        t.set_coef_format("compact")
        for o in (1, 6):
            for name, kw in TARGETS[:2]:
                tables, coarsen = _tables_of(ica, kw)
                got = t.transcode([src], copy_markers="none", gpu_entropy=False, orientation=o, edge="trim", **kw)
                want = ica.transcode_memory(src, optimize=True, orientation=o, trim=True, tables=tables, coarsen_only=coarsen)[0]
                assert got == [want] and want is not None and t.last_requantized == [True], (o, name)
                assert t._batch.slot_escapes(0) > 0 and t.last_host_emitted == 0
    finally:
        t.close()


def _one_value(k, value, q):
    """a 4:4:4 16x8 picture, all zero but coefficient k of luma block 1 and of Cb block 0, every table entry q"""
    hv = tp.LAYOUTS["444"]
    planes = hc.blank(16, 8, hv)
    planes[0][0, 1, k] = value
    planes[1][0, 0, k] = value
    return hc.plain(16, 8, hv, planes, qt={0: [q] * 64, 1: [q] * 64}).bytes()


@pytest.mark.parametrize("fmt", ["compact", "int16"])
def test_codability_is_judged_on_the_result(ica, fmt):
    """beyond the range at a = 1 and inside it at b = 2; inside it at a = 2 and beyond it at b = 1; AC and DC difference, both signs"""
    cases = [(5, 1500, 1000), (63, -1500, -1000), (0, 3000, 1500), (0, -3000, -1500)]
    big = [_one_value(k, v, 1) for k, v, _ in cases]
    fine = [_one_value(k, v, 2) for k, _, v in cases]
    t = ica.Transcoder()
    try:
        t.set_coef_format(fmt)
        t.reserve_arena(1 << 20)
        kw = {"optimize": False, "copy_markers": "none", "gpu_entropy": False}
        got = t.transcode(big + fine, **kw)
        assert t.last_host_emitted == 0
        assert got == [None] * 4 + [ica.transcode_memory(s)[0] for s in fine] and all(g is not None for g in got[4:])
        assert all("not codable" in r for r in t.last_reasons[:4]) and t.last_reasons[4:] == [None] * 4
        got = t.transcode(big + fine, qtables=TWOS, **kw)
        assert t.last_host_emitted == 0 and t.last_reasons == [None] * 8
        assert got == [ica.transcode_memory(s, tables=TWOS)[0] for s in big + fine] and all(g is not None for g in got)
        assert t.last_requantized == [True] * 4 + [False] * 4
        got = t.transcode(big + fine, qtables=ONES, coarsen_only=False, **kw)
        assert t.last_host_emitted == 0
        assert got == [None] * 8 and all("not codable" in r for r in t.last_reasons)
        assert all(ica.transcode_memory(s, tables=ONES, coarsen_only=False)[0] is None for s in big + fine)
        assert t.last_requantized == [False] * 4 + [True] * 4
    finally:
        t.close()


@pytest.mark.parametrize("layout", ["444", "420"])
def test_dc_pairs_across_a_tile_seam(ica, layout):
    """a block and its MCU-order predecessor in an earlier plane tile whose DCs differ by +-2048: uncodable as they are, codable once
    both DCs -- the predecessor's too -- have gone through b = 2"""
    srcs = [s for s, accepted in tp.dc_pairs(layout) if not accepted and "earlier tile" in s.name]
    assert len(srcs) >= 4
    datas = [s.data for s in srcs]
    t = ica.Transcoder()
    try:
        kw = {"optimize": False, "copy_markers": "none", "gpu_entropy": False}
        assert t.transcode(datas, **kw) == [None] * len(datas)
        got = t.transcode(datas, qtables=TWOS, **kw)
        assert t.last_host_emitted == 0
        for s, g in zip(srcs, got):
            want = ica.transcode_memory(s.data, tables=TWOS)[0]
            assert want is not None and g == want, s.name
    finally:
        t.close()


def test_mixed_call(ica):
    """per-source qualities with None among them, a source that is not transcodable and a file that is no JPEG"""
    p420, p422 = pictures("420"), pictures("422")
    srcs = [p420[0].data, p420[1].data, b"not a jpeg", tc.different_chroma_tables(), p422[0].data, p420[4].data, p422[2].data]
    quality = [50, None, 75, 60, None, 30, 100]
    t = ica.Transcoder()
    try:
        plain = t.transcode(srcs, copy_markers="all")
        plain_reasons = list(t.last_reasons)
        got = t.transcode(srcs, copy_markers="all", quality=quality)
        assert t.last_host_emitted == 0
        for i, (s, q) in enumerate(zip(srcs, quality)):
            tables = None if q is None else ica.quality_tables(q)
            want, why = ica.transcode_memory(s, optimize=True, copy_markers=True, tables=tables)
            assert got[i] == want, i
            assert (t.last_reasons[i] is None) == (want is not None), i
            if q is None or q == 100:
                assert got[i] == plain[i] and got[i] is not None, i
        assert [g is not None for g in got] == [True, True, False, False, True, True, True]
        assert t.last_reasons[2] == plain_reasons[2] and t.last_reasons[3] == plain_reasons[3] and "Cb and Cr" in t.last_reasons[3]
        assert t.last_requantized == [True, False, False, False, False, True, False]
        assert len(got[0]) < len(plain[0]) and len(got[5]) < len(plain[5])
        # only_if_smaller keeps its meaning at orientation 1
        small = t.transcode(srcs, copy_markers="all", quality=quality, only_if_smaller=True)
        assert small == [g if g is None or len(g) < len(s) else s for g, s in zip(got, srcs)]
    finally:
        t.close()


def test_arena_overflow_is_finished_on_the_host(ica):
    pics = pictures("420")[:4] + pictures("422")[:4]
    datas = [p.data for p in pics]
    orients = [5, 6, 7, 8, 1, 3, 4, 5]
    q50 = ica.quality_tables(50)
    want = [ica.transcode_memory(d, optimize=True, orientation=o, trim=True, tables=q50)[0] for d, o in zip(datas, orients)]
    assert all(w is not None for w in want)
    t = ica.Transcoder()
    try:
        t.reserve_arena(4096)
        got = t.transcode(datas, copy_markers="none", orientation=orients, edge="trim", quality=50)
        assert t.last_host_emitted > 0 and got == want
        got = t.transcode(datas, copy_markers="none", orientation=orients, edge="trim", quality=50)
        assert t.last_host_emitted == 0 and got == want
    finally:
        t.close()
