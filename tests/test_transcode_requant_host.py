"""Requantisation in the transcode, the host contract (include/mij_host.h, mjw_tplan_requant): the rounding rule against exact rational
rounding, the division constants the kernel's table is filled with, the quality tables against the writer's own DQT, identity, streams
read back, composition with the eight orientations, codability judged on the result, and the Python arguments.  No GPU."""
import functools

import numpy as np
import pytest

import header_cases as hc
import orient_coef_model as om
import requant_model as rm
import transcode_cases as tc
import transcode_model as model
import transcode_planes as tp

LAYOUTS = list(tp.LAYOUTS)
# two distinct asymmetric tables (zigzag order) within 8..20, and an explicit target that is finer than they are at even k (by less than
# four times, whatever the transposition: coefficients within +-128 stay codable) and coarser at odd k, luma and chroma
QT = {0: [8 + (5 * k) % 9 for k in range(64)], 1: [10 + (7 * k) % 11 for k in range(64)]}
TARGET = ([6 if k % 2 == 0 else 40 for k in range(64)], [7 if k % 2 == 0 else 50 for k in range(64)])
SPECIAL = (0, 1, -1, 2, -2, 1023, -1023, 1024, -1024, 32767, -32767, -32768)


def _exact(c, a, b):
    """round(c * a / b), halves away from zero, in exact integer arithmetic on doubled values; then the int16 clamp of the contract"""
    x = np.asarray(c, np.int64) * a
    y = np.sign(x) * ((2 * np.abs(x) + b) // (2 * b))
    return np.clip(y, -32767, 32767)


def _values(a, b):
    """the special values and, for steps (a, b) [broadcast arrays], the c on both sides of the first ties and of the tie nearest 1023"""
    shape = np.broadcast(a, b).shape
    vals = [np.full(shape, v, np.int64) for v in SPECIAL]
    for j in (0, 1, 2, 511, 1023):  # |c| * a = (j + 1/2) * b is a tie: the integers around (2j + 1) * b / (2a)
        lo = ((2 * j + 1) * b) // (2 * a)
        for c in (lo, lo + 1):
            c = np.minimum(c, 32767)
            vals += [c, -c]
    return np.stack(vals)


def test_rounding_rule_is_exact_rational_rounding():
    a, b = np.mgrid[1:256, 1:256].astype(np.int64)
    c = _values(a, b)
    got = rm.requant(c, a[None], b[None])
    want = _exact(c, a[None], b[None])
    assert np.array_equal(got, want)
    # ties exist and go away from zero: c = 1, a = 1, b = 2 -> 1; c = -3, a = 1, b = 2 -> -2; and a value that needs the clamp
    assert rm.requant(1, 1, 2) == 1 and rm.requant(-3, 1, 2) == -2 and rm.requant(-1, 1, 2) == -1
    assert rm.requant(32767, 255, 1) == 32767 and rm.requant(-32768, 255, 1) == -32767 and rm.requant(-32768, 1, 1) == -32767


def _plan(ica, ncomp, ytab, ctab, units=2):
    t = ica.TranscodePlan()
    t.ncomp, t.lh, t.lv = ncomp, 1, 1
    t.plan.width, t.plan.height, t.plan.comp = 8 * units, 8, ncomp
    t.plan.mcu_x, t.plan.mcu_y, t.plan.du_per_mcu = units, 1, 1 if ncomp == 1 else 3
    for k in range(64):
        t.plan.ytab[k], t.plan.ctab[k] = int(ytab[k]), int(ctab[k])
    return t


def test_units_requant_equals_the_model(ica):
    rng = np.random.default_rng(7)
    for trial in range(24):
        s = (rng.integers(1, 256, 64), rng.integers(1, 256, 64))
        d = (rng.integers(1, 256, 64), rng.integers(1, 256, 64))
        if trial == 0:
            s, d = (np.full(64, 255), np.full(64, 255)), (np.full(64, 1), np.full(64, 2))
        n_mcu = 40
        du = rng.integers(-32768, 32768, size=(n_mcu * 3, 64)).astype(np.int16)
        a = np.where(((np.arange(n_mcu * 3) % 3) >= 1)[:, None], s[1][None], s[0][None])
        b = np.where(((np.arange(n_mcu * 3) % 3) >= 1)[:, None], d[1][None], d[0][None])
        sv = _values(a, b)  # [n values, units, 64]: a few rows of them replace random ones
        for i in range(min(sv.shape[0], 32)):
            du[i * 3:(i + 1) * 3] = np.clip(sv[i, i * 3:(i + 1) * 3], -32768, 32767)
        got = ica.units_requant(_plan(ica, 3, *s, units=n_mcu), _plan(ica, 3, *d, units=n_mcu), du)
        assert got is not None
        assert np.array_equal(got, rm.requant_units(du, 1, 3, s, d)), trial
        assert np.array_equal(got, _exact(du, a, b)), trial
    # grey: the luma table only
    du = rng.integers(-32768, 32768, size=(5, 64)).astype(np.int16)
    got = ica.units_requant(_plan(ica, 1, QT[0], QT[0], units=5), _plan(ica, 1, TARGET[0], TARGET[0], units=5), du)
    assert np.array_equal(got, rm.requant(du, np.array(QT[0])[None], np.array(TARGET[0])[None]))


def _quotients(n, magic):
    """what the kernel computes for dividends n (uint64 array) with the constants (m, inc) of mjw_requant_magic: the high half of the
    64-bit product (n + inc) * m"""
    m, inc = magic
    assert 0 < m < 1 << 32 and inc in (0, 1)
    return ((n + np.uint64(inc)) * np.uint64(m)) >> np.uint64(32)


def test_division_constants_around_every_multiple(ica):
    """every b in 1..255, every n in {k * b - 1, k * b} below 2^24: where a quotient computed by a too small or too large constant first
    goes wrong"""
    for b in range(1, 256):
        m = ica.requant_magic(b)
        assert m == (((1 << 32) - 1, 1) if b == 1 else ((1 << 32) // b + 1, 0))
        kb = np.arange(b, 1 << 24, b, dtype=np.uint64)
        n = np.concatenate([kb - np.uint64(1), kb])
        assert np.array_equal(_quotients(n, m), n // np.uint64(b)), b
    assert ica.requant_magic(0)[0] == 0 and ica.requant_magic(256)[0] == 0


@pytest.mark.parametrize("b", [1, 2, 3, 127, 128, 254, 255])
def test_division_constants_for_every_dividend(ica, b):
    n = np.arange(1 << 24, dtype=np.uint64)
    assert np.array_equal(_quotients(n, ica.requant_magic(b)), n // np.uint64(b))


def _dqt(stream):
    qt = {}
    for m, a, b in model.segments(stream):
        p = stream[a + 4:b]
        while m == 0xDB and p:
            assert p[0] >> 4 == 0
            qt[p[0] & 15] = list(p[1:65])
            p = p[65:]
    return qt


def _sof(stream):
    for m, a, b in model.segments(stream):
        if m == 0xC0:
            p = stream[a + 4:b]
            return (p[3] << 8 | p[4], p[1] << 8 | p[2], [p[6 + 3 * c + 1] for c in range(p[5])])


@pytest.mark.parametrize("q", [1, 10, 49, 50, 51, 90, 91, 100])
def test_quality_tables_are_the_writers(ica, q):
    img = ica.synth_rgb(24, 16, seed=q)
    qt = _dqt(ica.stbi_write_jpg_to_memory(img, q))
    luma, chroma = ica.quality_tables(q)
    assert list(luma) == qt[0] and list(chroma) == qt[1]
    mine = rm.quality_tables(q)
    assert np.array_equal(luma, mine[0]) and np.array_equal(chroma, mine[1])


def test_quality_tables_refuse_what_is_no_quality(ica):
    assert ica.quality_tables(0) is None and ica.quality_tables(101) is None and ica.quality_tables(-5) is None


def _source_units(ica, data):
    desc, region = ica.host_decode_staged(data, 0, want_compact=False)
    t, why = ica.transcode_plan(desc)
    assert t is not None, why
    return t, ica.units_from_region(desc, region, False)


def _tables(t):
    return np.array(list(t.plan.ytab)), np.array(list(t.plan.ctab))


def test_identity_targets_change_nothing(ica):
    """quality 100 (every entry 1) with coarsen_only, and the source's own tables either way: a plain lossless slot, today's bytes"""
    for name, data in tc.layout_sources():
        want, why = ica.transcode_memory(data)
        assert want is not None, (name, why)
        t, _ = _source_units(ica, data)
        own = _tables(t)
        for tables, coarsen in ((ica.quality_tables(100), True), (own, True), (own, False)):
            assert ica.transcode_memory(data, tables=tables, coarsen_only=coarsen)[0] == want, name
            dst, changed = ica.transcode_plan_requant(t, tables, coarsen)
            assert dst is not None and changed is False and bytes(dst) == bytes(t), name
        for optimize in (False, True):
            assert ica.transcode_memory(data, optimize=optimize, copy_markers=True, tables=own)[0] == \
                ica.transcode_memory(data, optimize=optimize, copy_markers=True)[0], name


@pytest.mark.parametrize("which", ["quality 50", "explicit"])
def test_streams_read_back_as_the_model(ica, which):
    changed_any = 0
    for name, data in tc.layout_sources():
        t, du = _source_units(ica, data)
        s = _tables(t)
        target, coarsen = (ica.quality_tables(50), True) if which == "quality 50" else (TARGET, False)
        d = rm.dest_tables(s, target, coarsen)
        if t.ncomp == 1:
            d = (d[0], d[0])
        dst, changed = ica.transcode_plan_requant(t, target, coarsen)
        assert dst is not None and changed == (not all(np.array_equal(x, y) for x, y in zip(s, d))), name
        assert np.array_equal(_tables(dst)[0], d[0]) and np.array_equal(_tables(dst)[1], d[1]), name
        changed_any += changed
        ny = 1 if t.ncomp == 1 else t.lh * t.lv
        want_units = rm.requant_units(du, ny, t.plan.du_per_mcu, s, d)
        assert np.array_equal(ica.units_requant(t, dst, du), want_units), name
        for optimize in (False, True):
            out, why = ica.transcode_memory(data, optimize=optimize, tables=target, coarsen_only=coarsen)
            assert out is not None, (name, why)
            assert out == ica.emit_transcoded(dst, want_units, optimize), (name, optimize)
            qt = _dqt(out)
            assert qt[0] == list(d[0]) and (t.ncomp == 1 or qt[1] == list(d[1])), name
            assert _sof(out) == _sof(ica.transcode_memory(data)[0]), name  # the size and the sampling bytes stay
            t2, du2 = _source_units(ica, out)
            assert np.array_equal(du2, want_units), (name, optimize)
            assert (t2.lh, t2.lv, t2.ncomp, t2.plan.width, t2.plan.height) == (t.lh, t.lv, t.ncomp, t.plan.width, t.plan.height)
    assert changed_any > 0


@functools.lru_cache(maxsize=None)
def picture(layout, w, h):
    hv = tp.LAYOUTS[layout]
    planes = [p >> 3 for p in tp.address_planes(w, h, hv)]
    return planes, hc.plain(w, h, hv, planes, qt=QT if len(hv) == 3 else {0: QT[0]}).bytes()


def _sizes(layout):
    a, v = tp.LAYOUTS[layout][0]
    return [(3 * 8 * a, 2 * 8 * v), (2 * 8 * a + 5, 3 * 8 * v - 2), (8 * a - 3, 8 * v)]


@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_composition_with_the_orientations(ica, layout, trim):
    """one call == requantising the oriented units with the transposed tables; what is refused is what the orientation refuses"""
    hv = tp.LAYOUTS[layout]
    seen = set()
    for w, h in _sizes(layout):
        planes, data = picture(layout, w, h)
        t, du = _source_units(ica, data)
        for o in om.ORIENTATIONS:
            got, why = ica.transcode_memory(data, orientation=o, trim=trim, tables=TARGET, coarsen_only=False)
            plain, why_plain = ica.transcode_memory(data, orientation=o, trim=trim)
            try:
                want = om.orient(w, h, hv, planes, o, trim)
            except om.Refused:
                assert got is None and plain is None and why == why_plain and "axis" in why, (w, h, o)
                seen.add("refused")
                continue
            op, _ = ica.transcode_plan_oriented(t, o, trim)
            s = (om.orient_table(QT[0], o), om.orient_table(QT[1 if len(hv) == 3 else 0], o))
            assert np.array_equal(_tables(op)[0], s[0]) and np.array_equal(_tables(op)[1], s[1])
            d = (np.array(TARGET[0]), np.array(TARGET[1] if len(hv) == 3 else TARGET[0]))
            dst, changed = ica.transcode_plan_requant(op, TARGET, False)
            assert changed and np.array_equal(_tables(dst)[0], d[0]) and np.array_equal(_tables(dst)[1], d[1])
            units = rm.requant_units(ica.units_orient(t, du, o, trim), want.geom.ny, want.geom.dpm, s, d)
            assert np.array_equal(units, rm.requant_units(want.units, want.geom.ny, want.geom.dpm, s, d))
            if not model.codable(want.geom, units):
                assert got is None and "outside" in why, (w, h, o, why)
                seen.add("uncodable")
                continue
            assert got == ica.emit_transcoded(dst, units), (w, h, o, why)
            seen.add("ok")
    assert "ok" in seen and "uncodable" not in seen and (trim or "refused" in seen)


def _one_value(k, value, q):
    """a 4:4:4 16x8 picture, all zero but coefficient k of luma block 1 and of Cb block 0, every table entry q"""
    hv = tp.LAYOUTS["444"]
    planes = hc.blank(16, 8, hv)
    planes[0][0, 1, k] = value
    planes[1][0, 0, k] = value
    return hc.plain(16, 8, hv, planes, qt={0: [q] * 64, 1: [q] * 64}).bytes()


@pytest.mark.parametrize("k, big, fine", [(5, 1500, 1000), (63, -1500, -1000), (0, 3000, 1500), (0, -3000, -1500)])
def test_codability_is_judged_on_the_result(ica, k, big, fine):
    twos, ones = ([2] * 64, [2] * 64), ([1] * 64, [1] * 64)
    # beyond the range at a = 1: refused plain, codable at b = 2
    src = _one_value(k, big, 1)
    out, why = ica.transcode_memory(src)
    assert out is None and "outside" in why, why
    out, why_ok = ica.transcode_memory(src, tables=twos)
    assert out is not None, why_ok
    _, du = _source_units(ica, out)
    assert du[1, k] == big // 2 and du[3, k] == big // 2 and _dqt(out)[0] == [2] * 64
    # inside the range at a = 2: codable plain and under coarsen_only, refused at b = 1
    src = _one_value(k, fine, 2)
    plain = ica.transcode_memory(src)[0]
    assert plain is not None and ica.transcode_memory(src, tables=ones, coarsen_only=True)[0] == plain
    out, why2 = ica.transcode_memory(src, tables=ones, coarsen_only=False)
    assert out is None and why2 == why, (why2, why)


def test_zero_entries_are_refused(ica):
    t, _ = _source_units(ica, picture("444", 24, 16)[1])
    bad = np.array(TARGET[0], np.uint8)
    bad[17] = 0
    for tables in ((bad, TARGET[1]), (TARGET[0], bad)):
        dst, why = ica.transcode_plan_requant(t, tables, True)
        assert dst is None and "zero" in why


BAD_ARGS = [{"quality": 0}, {"quality": 101}, {"quality": True}, {"quality": 50.0}, {"quality": "50"}, {"quality": [50, 60, 70]},
            {"quality": [50, True]}, {"quality": [50, 0]}, {"quality": 50, "qtables": TARGET}, {"qtables": TARGET[0]},
            {"qtables": (TARGET[0], TARGET[1][:63])}, {"qtables": (TARGET[0], [0] + TARGET[1][1:])}, {"qtables": (TARGET[0], [256] + TARGET[1][1:])},
            {"qtables": (TARGET[0], [True] + TARGET[1][1:])}, {"qtables": (TARGET[0], [1.0] + TARGET[1][1:])}, {"qtables": 50},
            {"coarsen_only": 1}, {"coarsen_only": None}, {"quality": 50, "coarsen_only": "yes"}]


@pytest.mark.parametrize("bad", BAD_ARGS, ids=[str(i) for i in range(len(BAD_ARGS))])
def test_bad_arguments_raise_before_a_device_is_touched(ica, bad):
    t = ica.Transcoder()
    with pytest.raises(ValueError):
        t.transcode([b"not a jpeg", b"nor this"], **bad)
    assert t._ctx is None and t._batch is None and t._enc is None
    with pytest.raises(ValueError):
        ica.transcode_memory(b"not a jpeg", tables=(TARGET[0], [0] * 64))


def test_new_symbols_are_declared_and_exported(ica):
    import os
    import re
    import helpers
    L = ica.lib()
    for header, names in (("mij_host.h", ("mjw_quality_tables", "mjw_tplan_requant", "mjw_units_requant", "mjw_requant_magic",
                                         "mjw_transcode_memory_requant_at", "mjh_transcode_memory_requant")),
                          ("mij.h", ("mij_enc_add_coef_requant", "mij_enc_slot_requantized"))):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(helpers.ROOT, "include", header)).read(), flags=re.S)
        for name in names:
            assert re.search(r"\b%s\s*\(" % name, src), name
            assert hasattr(L, name), name
    assert L.mij_abi_version() == 1
