"""Progressive streams in the written contract (include/mij_host.h, PROGRESSIVE STREAMS; csrc/jpeg_write_host.c, transcode_host.c), on the
CPU: libjpeg's own progressive files as the judge of the bytes, every stream decoded back by the host walk, the oracle, the live reference
and Pillow, hand-made units at the edges of the end-of-band-run and correction-bit rules, composition with the other transcode steps, the
argument errors, and the calls under AddressSanitizer + UBSan."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import progressive_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "progressive_libjpeg.npz")
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_progressive as mg  # noqa: E402  (its segment walk and the script it asserts; Pillow is only needed to regenerate)


@pytest.fixture(scope="module")
def pairs():
    z = np.load(FIXTURE)
    return [(str(n), z["plain_" + str(n)].tobytes(), z["progressive_" + str(n)].tobytes()) for n in z["names"]]


def prog(ica, data, **kw):
    got, why = ica.transcode_memory(data, progressive=True, **kw)
    assert got is not None, why
    return got


def _pixels_pillow(data):
    try:
        from PIL import Image
    except ImportError:
        return None
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def test_fixture_holds_what_it_is_for(pairs):
    """the scan scripts of the contract, every sampling, a luma grid narrower than the MCU grid, and EOBn symbols with n >= 1"""
    assert os.path.getsize(FIXTURE) < 100 * 1024
    assert [n for n, _, _ in pairs] == ["444", "422", "420", "grey", "smooth"]
    for n, plain, pg in pairs:
        assert mg.scan_script(pg) == (mg.SCRIPT_GREY if n == "grey" else mg.SCRIPT_COLOUR), n
        assert len(mg.scan_script(plain)) == 1
    assert any(v & 15 == 0 and 1 <= v >> 4 <= 14 for _, _, pg in pairs for v in mg.ac_symbols(pg))


def test_against_libjpeg(ica, pairs):
    """1: the transcode of libjpeg's plain file with the request is libjpeg's progressive file from SOF2 to EOI, byte for byte; so is the
    transcode of the progressive file; without the request nothing changed"""
    for n, plain, pg in pairs:
        got = prog(ica, plain)
        assert got[got.index(b"\xff\xc2"):] == pg[pg.index(b"\xff\xc2"):], n
        assert prog(ica, pg) == got, n
        assert prog(ica, plain, optimize=True) == got, n  # the tables are the optimal ones either way
        base = ica.transcode_memory(plain, optimize=True)[0]
        assert ica.transcode_memory(plain, optimize=True, progressive=False)[0] == base and b"\xff\xc0" in base[:700] and b"\xff\xc2" not in base[:700]
        # DHT segments: two in front of the first scan, one per AC scan, none in front of the DC refinement; one table each
        seg = [m for m, _, _ in mg.segments(got) if m in (0xC4, 0xDA)]
        want = [0xC4, 0xC4, 0xDA] if n != "grey" else [0xC4, 0xDA]
        nscan = len(mg.scan_script(got))
        for k in range(1, nscan):
            want += [0xDA] if mg.scan_script(got)[k][1] == 0 else [0xC4, 0xDA]
        assert seg == want, n


def test_decode_back(ica, oracle, pairs):
    """2: every output decodes, through the host walk, the oracle and (where built) the live reference, to the source's coefficient planes
    and pixels"""
    ref = helpers.Reference() if helpers.Reference.available() else None
    for n, plain, pg in pairs:
        got = prog(ica, plain)
        assert np.array_equal(ica.HostDecoder.decode(got, 0)[1], ica.HostDecoder.decode(plain, 0)[1]), n
        # the oracle captures blocks in the order it decodes them, which differs between a one-scan and a progressive file: libjpeg's own
        # progressive file of the picture is the like-for-like reference, the source's pixels the common one
        assert oracle.coef(got).size > 0 and np.array_equal(oracle.coef(got), oracle.coef(pg)), n
        assert np.array_equal(oracle.load(got, 3)[1], oracle.load(plain, 3)[1]), n
        if ref:
            assert np.array_equal(ref.load(got, 3)[1], ref.load(plain, 3)[1]), n
        if _pixels_pillow(plain) is not None:
            assert np.array_equal(_pixels_pillow(got), _pixels_pillow(plain)), n


def test_hand_made_units(ica):
    """3: runs across tile seams, ending at unit 128 and at the scan's end, the early flush at more than 937 pending correction bits, the
    flush at 0x7FFF blocks, single magnitudes of both signs, ZRLs in first and refinement scans: each stream decodes back to its units, and
    the writer's counters say the case met what it was made for"""
    seen = {}
    for name, t, du, forced in pc.cases(ica, huge=True):
        s = ica.emit_jpeg(t, du, progressive=True)
        assert s is not None and ica.binding.emit_transcoded(t, du, progressive=True) == s, name
        assert mg.scan_script(s) == (mg.SCRIPT_GREY if t.ncomp == 1 else mg.SCRIPT_COLOUR), name
        assert np.array_equal(pc.units_of(ica, s), du), name
        assert len(s) <= 6144 + 1024 * len(du), name  # MJW_PROGRESSIVE_STREAM_CAP
        st = ica.binding.progressive_stats(t, du)
        seen[name] = st
        assert (st.forced_bit_flushes > 0) == (forced == "bits") and (st.forced_run_flushes > 0) == (forced == "run"), name
    assert seen["run_across_two_seams"].longest_run >= 299  # blocks 1..299 are empty in every band
    assert seen["pending_bits_945"].most_pending_bits == 945
    assert seen["flat_33124_blocks"].longest_run == 32767 and seen["flat_33124_blocks"].forced_run_flushes >= 1
    # a ZRL in a first scan and in a refinement scan: symbol 0xF0 in the tables of scans of both kinds
    name, t, du, _ = [c for c in pc.cases(ica) if c[0] == "zrl_first_and_refinement"][0]
    s = ica.emit_jpeg(t, du, progressive=True)
    kinds, scan = set(), mg.scan_script(s)
    dht = [p for m, p, _ in mg.segments(s) if m == 0xC4]
    ac_scans = [k for k in range(len(scan)) if scan[k][1] > 0]
    for k, p in zip(ac_scans, dht[1:]):
        if 0xF0 in p[17:17 + sum(p[1:17])]:
            kinds.add(scan[k][3] > 0)
    assert kinds == {False, True}


def test_composition(ica, pairs):
    """4: orientation 6, a crop, quality 75 and grey with the request == the progressive emit of the baseline call's units"""
    smooth = [p for n, p, _ in pairs if n == "smooth"][0]
    kw = dict(orientation=6, trim=True, crop=(8, 0, 100, 150), tables=tuple(t.tobytes() for t in ica.binding.quality_tables(75)), grey=True)
    base, why = ica.transcode_memory(smooth, optimize=True, **kw)
    assert base is not None, why
    t = ica.binding.transcode_plan(ica.HostDecoder.probe(base, 0))[0]
    assert t.ncomp == 1 and (t.plan.width, t.plan.height) == (100, 150)
    assert prog(ica, smooth, **kw) == ica.binding.emit_transcoded(t, pc.units_of(ica, base), progressive=True)
    # markers are copied into a progressive stream as into any other
    with_markers = prog(ica, smooth, copy_markers=True)
    assert with_markers[with_markers.index(b"\xff\xc2"):] == prog(ica, smooth)[prog(ica, smooth).index(b"\xff\xc2"):]


def test_argument_errors(ica, pairs):
    """5: a non-bool request and the request with a restart interval are ValueErrors, in every host entry; the library refuses both too"""
    import ctypes as C
    plain = pairs[0][1]
    t = ica.binding.transcode_plan(ica.HostDecoder.probe(plain, 0))[0]
    du = pc.units_of(ica, plain)
    for bad in (1, 0, None, "yes", [True]):
        with pytest.raises(ValueError):
            ica.transcode_memory(plain, progressive=bad)
        with pytest.raises(ValueError):
            ica.emit_jpeg(t, du, progressive=bad)
        with pytest.raises(ValueError):
            ica.binding.emit_transcoded(t, du, progressive=bad)
    for kw in ({"restart_rows": 1}, {"restart_mcus": 3}):
        with pytest.raises(ValueError):
            ica.transcode_memory(plain, progressive=True, **kw)
    with pytest.raises(ValueError):
        ica.emit_jpeg(t, du, progressive=True, restart_mcus=2)
    with pytest.raises(ValueError):
        ica.binding.emit_transcoded(t, du, progressive=True, restart_mcus=2)
    assert ica.transcode_memory(plain, progressive=True, restart_mcus=0)[0] == prog(ica, plain)
    L = ica.lib()
    L.mjw_transcode_memory_progressive_at.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int,
                                                       C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_char_p)]
    out, n, why = C.c_void_p(), C.c_size_t(), C.c_char_p()
    assert not L.mjw_transcode_memory_progressive_at(plain, len(plain), 0, 1, 0, None, 0, None, None, 0, 2, C.byref(out), C.byref(n), None, C.byref(why))
    assert not out.value and b"progressive" in why.value
    du_bad = du.copy()
    du_bad[0, 5] = 2000  # outside the codable range: refused as the baseline emit refuses it
    assert ica.binding.emit_transcoded(t, du_bad, progressive=True) is None and ica.binding.progressive_stats(t, du_bad) is None


def test_host_calls_under_sanitizers(tmp_path):
    """6: tests/support/san_progressive.c -- every MCU shape, sizes that are no MCU multiple, every emitter, the early flush, every prefix
    of a stream -- as a stand-alone program built with -fsanitize=address,undefined"""
    root = os.path.dirname(HERE)
    csrc = root + "/image-codecs_amd/csrc/"
    exe = str(tmp_path / "san_progressive")
    cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-I" + root + "/include", "-I" + root + "/image-codecs_amd/csrc", "-o", exe, root + "/tests/support/san_progressive.c",
           csrc + "jpeg_write_host.c", csrc + "transcode_host.c", csrc + "transcode_orient.c", csrc + "exif.c", csrc + "jpeg_entropy.c", "-lm", "-lpthread"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
