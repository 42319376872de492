"""Lossless rotate / flip / transpose in the transcode, the host contract (include/mij_host.h, mjw_tplan_oriented): the numpy model
(orient_coef_model.py) is anchored on the DCT itself, and plans, units, streams, refusals and the EXIF tag reset are held against it for
every transcodable layout, orientation and edge mode.  No GPU."""
import functools
import struct

import numpy as np
import pytest

import exif_build as xb
import header_cases as hc
import helpers
import orient_coef_model as om
import transcode_model as model
import transcode_planes as tp

LAYOUTS = list(tp.LAYOUTS)
EDGES = (False, True)  # trim
# asymmetric tables (zigzag order): a transposed table differs from the source's at every off-diagonal entry
QT = {0: [1 + (3 * k) % 200 for k in range(64)], 1: [2 + (7 * k) % 250 for k in range(64)]}


def sizes(layout):
    """exact multiples with mcu_x != mcu_y; a partial MCU on the right only, on the bottom only, on both; one MCU; narrower / lower than
    one MCU, where the trim leaves nothing"""
    a, v = tp.LAYOUTS[layout][0]
    mw, mh = 8 * a, 8 * v
    return [(3 * mw, 2 * mh), (3 * mw - 3, 2 * mh), (3 * mw, 2 * mh - 1), (2 * mw + 5, 3 * mh - 2), (mw, mh), (mw - 3, mh), (2 * mw, mh - 1)]


@functools.lru_cache(maxsize=None)
def picture(layout, w, h):
    hv = tp.LAYOUTS[layout]
    planes = tp.address_planes(w, h, hv)
    return planes, hc.plain(w, h, hv, planes, qt=QT if len(hv) == 3 else {0: QT[0]}).bytes()


def _dct_matrix():
    k, n = np.mgrid[0:8, 0:8]
    c = np.cos((2 * n + 1) * k * np.pi / 16) * 0.5
    c[0] /= np.sqrt(2.0)
    return c


def test_coefficient_rule_is_the_dct_of_the_oriented_block():
    """seeded integer blocks x: dct2(orient(x)) == the model's rule applied to dct2(x).  Values stay below 2^12 and float64 errors
    around 1e-12, so 1e-6 separates right from wrong whatever the block.  Rows of dct2 are the vertical frequency v, columns u."""
    C = _dct_matrix()
    assert np.allclose(C @ C.T, np.eye(8), atol=1e-12)
    x = np.random.default_rng(5).integers(-255, 256, size=(16, 8, 8)).astype(np.float64)
    dct2 = lambda b: C @ b @ C.T
    for o in om.ORIENTATIONS:
        for b in x:
            want = dct2(om.orient_pixels(b, o))
            got = om.orient_block(dct2(b), o)
            assert np.abs(want - got).max() < 1e-6, o
    # and the eight rules differ from one another on such a block: no orientation can stand in for another
    outs = [om.orient_block(dct2(x[0]), o) for o in om.ORIENTATIONS]
    assert all(np.abs(outs[i] - outs[j]).max() > 1 for i in range(8) for j in range(i))


def _host(ica, data, o, trim):
    """-> (source plan, destination plan or None, reason, destination units or None) by the host calls"""
    desc, region = ica.host_decode_staged(data, 0, want_compact=False)
    t, why = ica.transcode_plan(desc)
    assert t is not None, why
    dst, why = ica.transcode_plan_oriented(t, o, trim)
    if dst is None:
        return t, None, why, None
    return t, dst, None, ica.units_orient(t, ica.units_from_region(desc, region, False), o, trim)


def _assert_refusal(why, e):
    assert ("%s axis" % e.axis) in why and (" %d)" % e.size) in why and ("MCU size %d" % e.mcu) in why, (why, str(e))
    assert ("not perfect" in why) == (e.kind == "perfect") and ("nothing left" in why) == (e.kind == "nothing left"), (why, str(e))


@pytest.mark.parametrize("trim", EDGES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_plans_and_units_equal_the_model(ica, layout, trim):
    hv = tp.LAYOUTS[layout]
    seen = set()
    for w, h in sizes(layout):
        planes, data = picture(layout, w, h)
        for o in om.ORIENTATIONS:
            try:
                want = om.orient(w, h, hv, planes, o, trim)
            except om.Refused as e:
                _, dst, why, _ = _host(ica, data, o, trim)
                assert dst is None, (w, h, o)
                _assert_refusal(why, e)
                assert ica.transcode_memory(data, orientation=o, trim=trim)[0] is None
                seen.add(e.kind)
                continue
            src, dst, why, du = _host(ica, data, o, trim)
            assert dst is not None, (w, h, o, why)
            g = want.geom
            assert (dst.plan.width, dst.plan.height, dst.plan.mcu_x, dst.plan.mcu_y) == (want.w, want.h, g.mcu_x, g.mcu_y), (w, h, o)
            assert (dst.lh, dst.lv, dst.ncomp, dst.plan.du_per_mcu, dst.plan.comp) == (want.hv[0][0], want.hv[0][1], len(hv), g.dpm, len(hv))
            assert dst.plan.subsample == (1 if want.hv[0] == (2, 2) else 0)
            assert list(dst.plan.ytab) == list(om.orient_table(QT[0], o)), (w, h, o)
            assert list(dst.plan.ctab) == list(om.orient_table(QT[1 if len(hv) == 3 else 0], o)), (w, h, o)
            assert du.shape == want.units.shape and np.array_equal(du, want.units), (w, h, o, trim)
            seen.add("ok")
    assert seen == ({"ok", "nothing left"} if trim else {"ok", "perfect"})


def _header_of(stream):
    """-> (width, height, [(h, v) per component], {Tq: 64 zigzag bytes}) as the stream's SOF0 and DQT segments say"""
    qt, sof = {}, None
    for m, a, b in model.segments(stream):
        p = stream[a + 4:b]
        if m == 0xDB:
            while p:
                assert p[0] >> 4 == 0
                qt[p[0] & 15] = list(p[1:65])
                p = p[65:]
        elif m == 0xC0:
            hgt, wid, n = struct.unpack(">HHB", p[1:6])
            sof = (wid, hgt, [(p[6 + 3 * c + 1] >> 4, p[6 + 3 * c + 1] & 15) for c in range(n)])
    return sof + (qt,)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_streams_read_back_as_the_model(ica, layout):
    """the emitted stream's SOF size, sampling bytes and DQT entries are the transposed / trimmed ones, and its units, read back by the
    host decoder, the model's"""
    hv = tp.LAYOUTS[layout]
    for w, h in sizes(layout)[:5]:
        planes, data = picture(layout, w, h)
        for o in om.ORIENTATIONS:
            want = om.orient(w, h, hv, planes, o, True)
            for optimize in (False, True):
                out, why = ica.transcode_memory(data, optimize=optimize, orientation=o, trim=True)
                assert out is not None, (w, h, o, why)
                wid, hgt, fac, qt = _header_of(out)
                assert (wid, hgt, fac) == (want.w, want.h, want.hv), (w, h, o)
                assert qt[0] == list(om.orient_table(QT[0], o)) and (len(hv) == 1 or qt[1] == list(om.orient_table(QT[1], o)))
                d2, r2 = ica.host_decode_staged(out, 0, want_compact=False)
                assert np.array_equal(ica.units_from_region(d2, r2, False), want.units), (w, h, o, optimize)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_algebra(ica, layout):
    """o = 1 is mjh_transcode_memory byte for byte; on MCU multiples o and then its inverse, and o = 3 twice, give back the source's
    units and tables: the stream of the plain transcode"""
    for w, h in sizes(layout)[:4]:
        _, data = picture(layout, w, h)
        for optimize in (False, True):
            for markers in (False, True):
                plain = ica.transcode_memory(data, optimize=optimize, copy_markers=markers)[0]
                assert plain is not None
                for trim in EDGES:
                    assert ica.transcode_memory(data, optimize=optimize, copy_markers=markers, orientation=1, trim=trim)[0] == plain
    w, h = sizes(layout)[0]
    _, data = picture(layout, w, h)
    plain = ica.transcode_memory(data)[0]
    for o in om.ORIENTATIONS:
        once = ica.transcode_memory(data, orientation=o)[0]
        assert (once == plain) == (o == 1)
        assert ica.transcode_memory(once, orientation=om.INVERSE[o])[0] == plain, o
    assert ica.transcode_memory(ica.transcode_memory(data, orientation=3)[0], orientation=3)[0] == plain


@pytest.mark.parametrize("layout", ["grey", "444"])
def test_pixels_of_flat_blocks(ica, oracle, layout):
    """DC-only blocks decode flat and these layouts have no upsampling, so the decoded transform IS the numpy orientation of the decoded
    source, byte for byte"""
    hv = tp.LAYOUTS[layout]
    w, h = 40, 24
    planes = hc.blank(w, h, hv)
    rng = np.random.default_rng(3)
    for p in planes:
        p[:, :, 0] = rng.integers(-100, 101, size=p.shape[:2])
    data = hc.plain(w, h, hv, planes, qt={0: [8] + QT[0][1:], 1: [8] + QT[1][1:]} if len(hv) == 3 else {0: [8] + QT[0][1:]}).bytes()
    kind, src_px, _ = oracle.load(data, 0)
    assert kind == "ok" and len(np.unique(src_px)) > 10  # 15 blocks of their own grey each, or nearly
    for o in om.ORIENTATIONS:
        out, why = ica.transcode_memory(data, orientation=o)
        assert out is not None, why
        kind, px, _ = oracle.load(out, 0)
        assert kind == "ok" and np.array_equal(px, om.orient_pixels(src_px, o)), o


@pytest.mark.parametrize("layout", ["grey", "444"])
def test_codability_follows_the_destination(ica, layout):
    hv = tp.LAYOUTS[layout]
    verdicts = {}
    for name, values in (("rows", om.DC_ROWS_OK), ("cols", om.DC_COLS_OK)):
        planes, data = om.dc_grid(layout, values)
        for o in om.ORIENTATIONS:
            want = om.codable(om.orient(16, 16, hv, planes, o))
            _, dst, _, du = _host(ica, data, o, False)
            ok, why = ica.units_codable(dst, du)
            out, why2 = ica.transcode_memory(data, orientation=o)
            assert ok == want and (out is not None) == want, (name, o)
            assert want or ("DC" in why and "DC" in why2)
            verdicts[(name, o)] = want
    # the transpose exchanges the two pictures' fates: codable in source order and not in the destination's, and the converse
    assert verdicts[("rows", 1)] and not verdicts[("rows", 5)] and not verdicts[("cols", 1)] and verdicts[("cols", 5)], verdicts

def test_refusals_carry_their_reasons(ica):
    w, h = 45, 32   # 4:2:0: x is no multiple of 16, y is
    _, data = picture("420", w, h)
    for o in om.ORIENTATIONS:
        out, why = ica.transcode_memory(data, orientation=o)
        assert (out is None) == (o in om.MIRROR_X), o
        if out is None:
            assert "x axis" in why and "width 45" in why and "MCU size 16" in why and "y axis" not in why
    _, data = picture("422", 32, 13)   # 4:2:2: the MCU is 16 x 8; y is no multiple
    for o in om.ORIENTATIONS:
        out, why = ica.transcode_memory(data, orientation=o)
        assert (out is None) == (o in om.MIRROR_Y), o
        if out is None:
            assert "y axis" in why and "height 13" in why and "MCU size 8" in why and "x axis" not in why
    for o in (-1, 9, 100):
        for trim in EDGES:
            out, why = ica.transcode_memory(data, orientation=o, trim=trim)
            assert out is None and "1..8" in why
    src, _, _, _ = _host(ica, data, 1, False)
    for o in (0, 9):
        assert "1..8" in ica.transcode_plan_oriented(src, o)[1]


def test_exif_set_orientation_patches_two_bytes(ica):
    _, base = picture("420", 48, 32)
    for le in (True, False):
        for old in (1, 3, 6, 8):
            src = xb.tagged(base, old, le)
            assert ica.exif_orientation(src) == old
            for new in (1, 5, 8):
                got, ok = ica.exif_set_orientation(src, new)
                assert ok and ica.exif_orientation(got) == new and len(got) == len(src)
                diff = [i for i in range(len(src)) if src[i] != got[i]]
                at = src.index(struct.pack("<HHI" if le else ">HHI", 0x0112, 3, 1)) + 8
                assert set(diff) <= {at, at + 1} and (diff or new == old)
                assert got[at:at + 2] == struct.pack("<H" if le else ">H", new)
            assert ica.exif_set_orientation(src, 0) == (src, False) and ica.exif_set_orientation(src, 9) == (src, False)
    # no readable tag: untouched
    ifd1_only = xb.insert(base, xb.app1(xb.tiff(entries=[(0x0100, 3, 1, 48)], ifd1=[(0x0112, 3, 1, 6)])))
    cases = [base, xb.insert(base, xb.app1(xb.tiff(6), exif=False)), xb.insert(base, xb.app1(xb.tiff(entries=[(0x0112, 4, 1, 6)]))),
             xb.insert(base, xb.app1(xb.tiff(6, count=200))), xb.insert(base, xb.app1(xb.tiff(6)), after_sof=False)[:30], ifd1_only, b"", b"\xff\xd8"]
    for src in cases:
        assert ica.exif_orientation(src) == 1
        assert ica.exif_set_orientation(src, 3) == (bytes(src), False)


@pytest.mark.parametrize("le", [True, False])
def test_exif_transcode_resets_the_tag_and_nothing_else(ica, le):
    planes, base = picture("420", 48, 32)
    com = b"\xff\xfe\x00\x07hello"
    for tag in om.ORIENTATIONS:
        src = xb.insert(base, xb.app1(xb.tiff(tag, le)), com)
        for optimize in (False, True):
            out, why = ica.transcode_memory(src, optimize=optimize, copy_markers=True, orientation="exif")
            assert out is not None, why
            assert ica.exif_orientation(out) == 1
            # the stream: the fixed orientation's; the copied bytes: the source's but for the tag
            bare = ica.transcode_memory(src, optimize=optimize, orientation=tag)[0]
            spliced = model.splice_markers(src, bare)
            want, patched = ica.exif_set_orientation(spliced, 1)
            assert out == want and len(out) == len(spliced)
            diff = [i for i in range(len(out)) if out[i] != spliced[i]]
            assert len(diff) == (0 if tag == 1 else 1) and com in out
            assert np.array_equal(ica.units_from_region(*_staged(ica, out)), om.orient(48, 32, tp.LAYOUTS["420"], planes, tag).units)
    # an explicit orientation resets the tag as well; without copied markers there is none
    src = xb.tagged(base, 6, le)
    assert ica.exif_orientation(ica.transcode_memory(src, copy_markers=True, orientation=3)[0]) == 1
    assert ica.exif_orientation(ica.transcode_memory(src, copy_markers=True, orientation=1)[0]) == 6
    assert ica.exif_orientation(ica.transcode_memory(src, copy_markers=True)[0]) == 6
    assert b"Exif" not in ica.transcode_memory(src, orientation="exif")[0]


def _staged(ica, data):
    d, r = ica.host_decode_staged(data, 0, want_compact=False)
    return d, r, False


def test_host_orientation_under_sanitizers(tmp_path):
    """tests/support/san_orient.c: the plan, unit and whole-file calls for every MCU shape, orientation and edge mode, and the EXIF patch
    on every prefix of a tagged file, on exact-size heap blocks under ASan + UBSan, as a stand-alone CPU program"""
    import os
    import subprocess
    root = helpers.ROOT
    exe = str(tmp_path / "san_orient")
    csrc = root + "/image-codecs_amd/csrc/"
    cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-I" + root + "/include", "-I" + root + "/image-codecs_amd/csrc", "-o", exe, root + "/tests/support/san_orient.c",
           csrc + "jpeg_write_host.c", csrc + "transcode_host.c", csrc + "transcode_orient.c", csrc + "exif.c", csrc + "jpeg_entropy.c", "-lm", "-lpthread"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("no address sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-2000:]
    assert "orientation harness: 20 cases, 0 failures" in run.stdout
