"""Lossless transcode, the host contract (include/mij_host.h, mjw_tplan): the writer's own files are fixed points, every transcodable
layout comes back with the same coefficients and the same pixels, the units equal the numpy model on both plane formats, refusals carry
their reasons, and the marker copy equals the model.  No GPU."""
import numpy as np
import pytest

import emit_model as em
import helpers
import header_cases as hc
import hufopt_model as hm
import transcode_cases as tc
import transcode_model as model
import transcode_planes as tp


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


# ---------------------------------------------------------------- sources made from chosen coefficient planes (transcode_planes.py)

def test_units_to_planes_inverts_the_model():
    rng = np.random.default_rng(7)
    for layout, hv in tp.LAYOUTS.items():
        w, h = tp.size(layout, (5, 3), True)
        g = tp.Geom(w, h, hv)
        du = rng.integers(-1023, 1024, size=(g.n_du, 64)).astype(np.int16)
        planes = tp.units_to_planes(du, w, h, hv)
        assert [p.shape for p in planes] == [(c.bh, c.bw, 64) for c in g.comp]
        assert np.array_equal(model.units_from_planes(g, tp.natural(planes)), du), layout


def test_chosen_planes_are_what_they_claim():
    """the properties the sources are built for, in numpy, before anything decodes them"""
    for layout, hv in tp.LAYOUTS.items():
        for s in tp.address(layout):
            g = tp.Geom(s.w, s.h, s.hv)
            assert (g.mcu_x, g.mcu_y) in tp.GRIDS
            for c, p in enumerate(s.planes):
                assert np.abs(p.astype(np.int64)).max() <= 1023
                plain = (np.arange(p.shape[0] * p.shape[1]) % 3 == 0).reshape(p.shape[:2])
                assert p[plain].min() >= -128 and p[plain].max() <= 127
                if (~plain).any():
                    assert ((p[~plain][:, 1:] > 127) | (p[~plain][:, 1:] < -128)).any(axis=1).all()
        assert len(tp.address(layout)) == 20 and max(s.w for s in tp.address(layout)) <= 1040
        e = tp.edge_values(layout)
        for p in e.planes:
            flat = p.reshape(-1, 64)
            for v in tp.EDGE_VALUES:
                assert (flat[:, 1:] == v).any(axis=0).all(), (layout, v)
        d = tp.dense(layout)
        assert tp.escaped_blocks(d.planes) == sum(p.shape[0] * p.shape[1] for p in d.planes)
        # the triangle: no MCU-order difference is large, the first blocks of consecutive MCU rows differ by 2200, and the block above
        # (which is block L - bw) is 2047 away and more somewhere
        t = tp.triangle(layout)
        g = tp.Geom(t.w, t.h, t.hv)
        for c, p in enumerate(t.planes):
            dc = p[:, :, 0].astype(np.int64)
            seq = tp.mcu_order(g, c)
            order = np.array([dc[by, bx] for by, bx in seq])
            assert np.abs(np.diff(np.concatenate([[0], order]))).max() <= 1100
            v = g.comp[c].v
            assert abs(int(dc[v, 0]) - int(dc[0, 0])) == 2200
            assert np.abs(np.diff(dc, axis=0)).max() > 2047
        assert not any(p[:, :, 1:].any() for p in t.planes)
    # the pairs: every branch a layout has, in every component; the predecessor in an earlier tile wherever a block index can cross one
    for layout, hv in tp.LAYOUTS.items():
        for comp, (a, v) in enumerate(hv):
            for branch in tp.BRANCHES:
                exists = {"a": a > 1, "b": v > 1}.get(branch, True)
                same, cross = tp.pair_site(layout, comp, branch, True), tp.pair_site(layout, comp, branch, False)
                assert (same is not None) == exists, (layout, comp, branch)
                assert (cross is not None) == (exists and branch in "bcd"), (layout, comp, branch)
                for site in (same, cross):
                    if site is not None:
                        assert site[0][0] * site[0][1] <= 70
    assert len(tp.dc_pairs("420")) == 4 * (8 + 5 + 5)  # luma: a, b twice, c twice, d twice, e; chroma: c twice, d twice, e
    assert len(tp.ac_limits("420")) == 2 + 2 * 4 * 3 * 2 and len(tp.ac_limits("grey")) == 2 + 4 * 3 * 2  # components, blocks, positions, signs
    for layout in tp.LAYOUTS:  # two DCs and nothing else: whatever other block a rule takes for the predecessor, it sees 1024 at the most
        for src, ok in tp.dc_pairs(layout):
            assert sum(int(np.count_nonzero(p)) for p in src.planes) == (1 if "branch e" in src.name else 2), src.name
            assert max(int(np.abs(p[:, :, 0].astype(np.int64)).max()) for p in src.planes) <= (2048 if "branch e" in src.name else 1024)
    pair = tp.dc_pair("420", 0, "d", False, -2048)
    dcs = pair.planes[0][:, :, 0]
    assert sorted(dcs[dcs != 0].tolist()) == [-1024, 1024] and not any(p[:, :, 0].any() for p in pair.planes[1:])


@pytest.mark.parametrize("layout", list(tp.LAYOUTS))
def test_chosen_planes_units_and_verdicts(ica, layout):
    """every source made from chosen planes, on both plane formats: the units the host reads equal the model's of the decoded planes and
    of the planes handed to the writer, and the model's verdict is the host's, at the unit check and through the whole path"""
    cases = tp.all_sources(layout)
    refused = 0
    for src, ok in cases:
        want = tp.expected_units(src)
        verdict = model.codable(tp.Geom(src.w, src.h, src.hv), want)
        assert verdict == ok, src.name
        refused += not verdict
        for compact in (False, True):
            desc, region = ica.host_decode_staged(src.data, 0, want_compact=compact)
            is_compact = bool(desc.flags & 4)
            assert is_compact == compact, src.name
            arena = ica.expand_compact_region(desc, region) if is_compact else region.view(np.int16)[:desc.coef_elems()]
            assert np.array_equal(model.units_from_planes(desc, ica.detile_coefficients(desc, arena)), want), (src.name, compact)
            got = ica.units_from_region(desc, region, is_compact)
            assert got is not None and np.array_equal(got, want), (src.name, compact)
            if is_compact:
                offs, _ = ica.compact_offsets(desc)
                flagged = 0
                for c, (lo, _, _) in enumerate(offs):
                    L = np.arange(desc.comp[c].bw * desc.comp[c].bh)
                    flagged += int((region[lo + ((L >> 6) << 12) + ((L & 63) << 3)] & 1).sum())
                assert flagged == tp.escaped_blocks(src.planes), src.name
        t, _ = ica.transcode_plan(desc)
        assert ica.units_codable(t, want)[0] == verdict, src.name
        for optimize in (False, True):
            out, why = ica.transcode_memory(src.data, optimize=optimize)
            assert (out is not None) == verdict, (src.name, optimize, why)
            if not verdict:
                assert ("DC" in why) if src.name.startswith("dc pair") else ("AC" in why), (src.name, why)
    assert refused == sum(1 for _, ok in cases if not ok) >= 10 + 24


def test_longest_units_fit_the_hosts_buffer(ica):
    """dense noise in every layout and the longest codable units under the Annex-K tables: some 200 to 250 bytes per unit, which
    mjh_transcode_memory's buffer has to hold (it was sized at 128 per unit and answered "emission failed")"""
    srcs = [tp.dense(layout) for layout in tp.LAYOUTS] + [tp.longest()]
    for src in srcs:
        want = tp.expected_units(src)
        assert model.codable(tp.Geom(src.w, src.h, src.hv), want)
        out, why = ica.transcode_memory(src.data, optimize=False)
        assert out is not None, (src.name, why)
        assert len(out) > 607 + 128 * len(want), src.name  # the case the old bound missed
        d2, r2 = ica.host_decode_staged(out, 0, want_compact=False)
        assert np.array_equal(ica.units_from_region(d2, r2, False), want), src.name
    assert len(ica.transcode_memory(tp.longest().data)[0]) > 240 * 387


@pytest.mark.parametrize("layout", list(tp.LAYOUTS))
def test_emission_model_equals_the_host_for_every_layout(ica, layout):
    """the emission model generalised to (dpm, ny) against mjw_temit / mjw_temit_optimized byte for byte, at eleven tiles and more, with
    a seam that shares a 0xFF byte and a seam on a byte boundary under the plain tables"""
    src = tp.emission(layout)
    du, want, stats, _ = tp.emission_model(layout)
    g = tp.Geom(src.w, src.h, src.hv)
    assert len(du) >= 1300 and stats["tiles"] == (len(du) + 127) // 128 >= 11
    assert stats.get("shared_ff", 0) >= 1 and stats.get("aligned", 0) >= 1, stats
    assert np.array_equal(du, em.adversarial_units(np.random.default_rng(tp.EMISSION[layout][1]), g.mcu_x * g.mcu_y, g.dpm, ny=g.ny))
    assert np.abs(em.dc_diffs(du, g.dpm, g.ny)).max() == 2047
    desc, region = ica.host_decode_staged(src.data, 0, want_compact=True)
    assert np.array_equal(ica.units_from_region(desc, region, bool(desc.flags & 4)), du)
    t, _ = ica.transcode_plan(desc)
    assert (t.plan.du_per_mcu, t.lh * t.lv if t.ncomp == 3 else 1) == (g.dpm, g.ny)
    for optimize in (False, True):
        got = ica.emit_transcoded(t, du, optimize)
        assert got == want[optimize], (layout, optimize)
        assert ica.transcode_memory(src.data, optimize=optimize)[0] == got, (layout, optimize)
    assert len(want[True]) < len(want[False])
    # the histogram the optimised tables come from, against the library's for the two layouts the writer's own plans have
    if layout in ("444", "420"):
        assert np.array_equal(hm.histogram(du, g.dpm, g.ny), ica.write_histogram(t.plan, du))
