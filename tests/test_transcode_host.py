"""Lossless transcode, the host contract (include/mij_host.h, mjw_tplan): the writer's own files are fixed points, every transcodable
layout comes back with the same coefficients and the same pixels, the units equal the numpy model on both plane formats, refusals carry
their reasons, and the marker copy equals the model.  No GPU."""
import numpy as np
import pytest

import helpers
import header_cases as hc
import transcode_cases as tc
import transcode_model as model


def _c_table(path, name):
    import os
    import re
    src = open(os.path.join(helpers.ROOT, path)).read()
    body = re.search(name + r"\[64\]\s*=\s*\{(.*?)\}", src, re.S).group(1)
    return [int(v) for v in re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("\n", " ").split(",") if v.strip()]


def test_zigzag_tables_agree():
    """mij_zigzag_pos (plane position of zigzag index k) against the model's zigzag order, and the conversion kernel's inverse table"""
    pos = _c_table("include/mij.h", "mij_zigzag_pos")
    inv = _c_table("image-codecs_amd/csrc/mij_transcode_kernels.h", "k_zigzag_of_pos")
    assert len(pos) == 64 and sorted(pos) == list(range(64)) and len(inv) == 64
    for k, nat in enumerate(model.ZIGZAG_NATURAL):
        row, col = divmod(int(nat), 8)
        assert pos[k] == 8 * col + (0, 4, 2, 5, 1, 6, 3, 7)[row]
        assert inv[pos[k]] == k


@pytest.mark.parametrize("case", range(12))
def test_writer_files_are_fixed_points(ica, case):
    name, src, img, q = tc.writer_sources()[case]
    got, why = ica.transcode_memory(src)
    assert why is None and got == src, name
    plan, du = ica.host_transform(img, q)
    got, why = ica.transcode_memory(src, optimize=True)
    assert why is None and got == ica.emit_jpeg(plan, du, True), name
    # the header alone: mjw_theader is mjw_header byte for byte given the writer's tables
    desc, _ = ica.HostDecoder.decode(src, 0)
    t, _ = ica.transcode_plan(desc)
    assert ica.transcode_header(t) == src[:607]


def _lossless(ica, oracle, ref, name, src):
    desc, arena = ica.HostDecoder.decode(src, 0)
    want_blocks = model.blocks_in_planes(desc, ica.detile_coefficients(desc, arena))
    want_coef = helpers._dequantised_in_call_order(ica, desc, arena)  # what a decoder of the OUTPUT (baseline, one scan) sees
    kind, want_px, _ = oracle.load(src, 0)
    assert kind == "ok", name
    for optimize in (False, True):
        out, why = ica.transcode_memory(src, optimize=optimize)
        assert out is not None, (name, why)
        d2, a2 = ica.HostDecoder.decode(out, 0)
        assert (d2.width, d2.height, d2.ncomp) == (desc.width, desc.height, desc.ncomp), name
        for c, (a, b) in enumerate(zip(want_blocks, model.blocks_in_planes(d2, ica.detile_coefficients(d2, a2)))):
            assert np.array_equal(a, b), (name, optimize, c)
            assert d2.comp[c].h == desc.comp[c].h and d2.comp[c].v == desc.comp[c].v
            assert list(d2.dequant[d2.comp[c].tq]) == list(desc.dequant[desc.comp[c].tq]), (name, c)
        assert np.array_equal(oracle.coef(out, 0), want_coef), (name, optimize)
        k2, px, _ = oracle.load(out, 0)
        assert k2 == "ok" and np.array_equal(px, want_px), (name, optimize)
        if ref is not None:
            kr, pr, _ = ref.load(out, 0)
            ks, ps, _ = ref.load(src, 0)
            assert kr == "ok" and ks == "ok" and np.array_equal(pr, ps), (name, optimize)
            assert np.array_equal(pr, want_px), (name, optimize)
        if optimize:
            plain, _ = ica.transcode_memory(src)
            assert len(out) <= len(plain), name


@pytest.fixture(scope="module")
def ref():
    return helpers.Reference() if helpers.Reference.available() else None


def test_every_layout_is_lossless(ica, oracle, ref):
    cases = tc.layout_sources()
    assert len(cases) >= 23
    for name, src in cases:
        _lossless(ica, oracle, ref, name, src)


def test_transcodable_goldens_are_lossless(ica, oracle, ref, golden):
    cases = tc.golden_sources(golden)
    names = [n for n, _ in cases]
    for must in ("b420_17x33_q75", "b444_9x7_q100", "b422_37x21", "s12_35x19", "prog_422_50x30", "prog_grey_40x40", "rst_blocks_64x48", "grey_33x20",
                 "pil420_130x50", "cmyk_transform1_40x30"):
        if must.startswith("cmyk"):
            assert "golden " + must not in names
        else:
            assert "golden " + must in names, must
    for name, src in cases:
        _lossless(ica, oracle, ref, name, src)


def test_units_equal_the_model_on_both_plane_formats(ica):
    srcs = [s for _, s in tc.layout_sources()] + [tc.escaped_source(), tc.writer_sources()[5][1]]
    escapes = 0
    for src in srcs:
        seen = []
        for compact in (False, True):
            desc, region = ica.host_decode_staged(src, 0, want_compact=compact)
            is_compact = bool(desc.flags & 4)
            arena = ica.expand_compact_region(desc, region) if is_compact else region.view(np.int16)[:desc.coef_elems()]
            want = model.units_from_planes(desc, ica.detile_coefficients(desc, arena))
            got = ica.units_from_region(desc, region, is_compact)
            assert got is not None and np.array_equal(got, want)
            seen.append(is_compact)
            if src is tc.escaped_source() and is_compact:
                offs, _ = ica.compact_offsets(desc)
                for c, (lo, _, _) in enumerate(offs):
                    nblk = desc.comp[c].bw * desc.comp[c].bh
                    L = np.arange(nblk)
                    escapes += int((region[lo + ((L >> 6) << 12) + ((L & 63) << 3)] & 1).sum())
        assert seen[0] is False
    assert escapes > 0


def _reason(ica, data, **kw):
    out, why = ica.transcode_memory(data, **kw)
    assert out is None and why
    return why


def test_refusals_carry_their_reasons(ica, golden):
    assert "4:1:1" in _reason(ica, hc.plain(35, 19, [(4, 1), (1, 1), (1, 1)]).bytes())
    assert "4:1:1" in _reason(ica, golden.jpg("s41_35x19"))
    assert "CMYK" in _reason(ica, golden.jpg("cmyk_40x30"))
    assert "CMYK" in _reason(ica, golden.jpg("cmyk_transform2_40x30"))
    assert "RGB-tagged" in _reason(ica, hc.plain(24, 24, [(2, 2), (1, 1), (1, 1)], app14=0).bytes())
    assert "RGB-tagged" in _reason(ica, golden.jpg("rgb_tagged_24x24"))
    assert "different quantisation tables" in _reason(ica, tc.different_chroma_tables())
    # a third pair of Huffman tables is no obstacle: the contract speaks of quantisation tables
    src = tc.writer_sources()[9][1]
    assert ica.transcode_memory(helpers.third_tables(src))[0] == src
    # a table entry above 255: the contract function, and a 16-bit DQT file whatever stage refuses it
    desc, _ = ica.HostDecoder.decode(src, 0)
    desc.dequant[desc.comp[0].tq][9] = 256
    t, why = ica.transcode_plan(desc)
    assert t is None and "255" in why
    assert "255" in _reason(ica, tc.wide_table_entry())
    assert ica.transcode_memory(golden.jpg("sixteen_bit_dqt"))[0] is not None  # 16-bit precision with 8-bit values is written as 8-bit
    # truncated streams
    for cut in (len(src) // 2, 300, 3):
        _reason(ica, src[:cut])
    _reason(ica, b"")
    for name in ("trunc_header", "garbage", "empty", "soi_only"):
        _reason(ica, golden.jpg(name))


@pytest.mark.parametrize("what,value,ok", [("ac", 1023, True), ("ac", -1023, True), ("ac", 1024, False), ("ac", -1024, False),
                                           ("dc", 2047, True), ("dc", -2047, True), ("dc", 2048, False), ("dc", -2048, False)])
def test_codable_ranges(ica, what, value, ok):
    """at the unit emitter, and through a whole file whose tables can code any magnitude"""
    for hv in ([(2, 1), (1, 1), (1, 1)], [(1, 1)]):
        w, h = 40, 24

        def edit(planes, hv=hv):
            p = planes[len(hv) - 1]
            if what == "ac":
                p[1, 2, 17] = value
            else:  # the DC difference between two neighbours in MCU order
                p[:, :, 0] = 0
                p[1, 2, 0] = value // 2
                p[1, 1, 0] = value // 2 - value
        src = tc.planes_source(w, h, hv, edit)
        desc, region = ica.host_decode_staged(src, 0, want_compact=False)
        t, _ = ica.transcode_plan(desc)
        du = ica.units_from_region(desc, region, False)
        assert model.codable(desc, du) == ok
        assert ica.units_codable(t, du)[0] == ok
        for optimize in (False, True):
            assert (ica.emit_transcoded(t, du, optimize) is not None) == ok
            out, why = ica.transcode_memory(src, optimize=optimize)
            assert (out is not None) == ok
            if ok:
                d2, r2 = ica.host_decode_staged(out, 0, want_compact=False)
                assert np.array_equal(ica.units_from_region(d2, r2, False), du)
            else:
                assert ("AC" in why) if what == "ac" else ("DC" in why)


def _with_segments(src, segs, drop_app0=False):
    body = src[20:] if drop_app0 else src[2:]
    return src[:2] + b"".join(b"\xff" + bytes([m, (len(p) + 2) >> 8, (len(p) + 2) & 255]) + p for m, p in segs) + body


def test_marker_copy_equals_the_model(ica):
    src = tc.writer_sources()[3][1]
    exif = b"Exif\0\0II*\0" + bytes(range(40))
    adobe = b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 1])
    sources = {
        "jfif + exif + com": src[:20] + _with_segments(src, [(0xE1, exif), (0xFE, b"a comment")], True)[2:],
        "adobe only": _with_segments(src, [(0xEE, adobe)], True),
        "no appn": _with_segments(src, [], True),
        "com and app2 without jfif": _with_segments(src, [(0xFE, b"x"), (0xE2, b"MPF\0" + bytes(30))], True),
    }
    for name, s in sources.items():
        for optimize in (False, True):
            plain, why = ica.transcode_memory(s, optimize=optimize)
            assert plain is not None, (name, why)
            want = model.splice_markers(s, plain)
            assert want is not None
            got, why = ica.copy_markers(s, plain)
            assert got == want, name
            assert ica.transcode_memory(s, optimize=optimize, copy_markers=True)[0] == want, name
            d, a = ica.HostDecoder.decode(got, 0)
            d0, a0 = ica.HostDecoder.decode(s, 0)
            assert np.array_equal(a, a0), name
    assert model.splice_markers(sources["jfif + exif + com"], src).count(b"JFIF\0") == 1
    assert model.splice_markers(sources["adobe only"], src).count(b"JFIF\0") == 0
    assert model.splice_markers(sources["no appn"], src) == src
    # a segment whose length runs past the end: refused by both
    bad = src[:2] + b"\xff\xe1\xff\xf0" + b"Exif" + src[2:300]
    assert model.splice_markers(bad, src) is None
    got, why = ica.copy_markers(bad, src)
    assert got is None and "length" in why
    got, why = ica.copy_markers(src[:2] + b"\xff\xe1\x00", src)
    assert got is None and why
    got, why = ica.copy_markers(src[:2] + b"\xff\xe1\x00\x01" + src[2:], src)
    assert got is None and why


def test_host_transcode_under_sanitizers(tmp_path):
    """tests/support/san_transcode.c: both plane formats, every MCU shape, every emitter, every prefix of a stream through
    mjh_transcode_memory and mjw_copy_markers, on exact-size heap blocks under ASan + UBSan, as a stand-alone CPU program"""
    import os
    import subprocess
    root = helpers.ROOT
    exe = str(tmp_path / "san_transcode")
    csrc = root + "/image-codecs_amd/csrc/"
    cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-I" + root + "/include", "-I" + root + "/image-codecs_amd/csrc", "-o", exe, root + "/tests/support/san_transcode.c",
           csrc + "jpeg_write_host.c", csrc + "transcode_host.c", csrc + "jpeg_entropy.c", "-lm", "-lpthread"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("no address sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-2000:]
    assert "transcode harness: 20 cases, 0 failures" in run.stdout
