"""Restart intervals in the written contract (include/mij_host.h, RESTART INTERVALS; csrc/jpeg_write_host.c, transcode_host.c), on the CPU:
libjpeg's own restart files as the judge of the bytes, every interval tied to the emitter that the other tests pin, the streams decoded
back by the host walk, the oracle, the live reference and Pillow, and the edges of the interval's range."""
import copy
import ctypes as C
import io
import os

import numpy as np
import pytest

import emit_model as em
import helpers
import hufopt_model as hm
import orient_coef_model as om

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "restart_libjpeg.npz")
LAYOUTS = {"grey": [(1, 1)], "444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)]}  # 1, 3, 4, 6 units per MCU


def split(stream):
    """(header, [interval bytes], [marker numbers]) of a one-scan stream: the entropy-coded segment cut at its RSTn markers"""
    i = stream.index(b"\xff\xda")
    start = i + 2 + (stream[i + 2] << 8 | stream[i + 3])
    body, parts, nums, a = stream[start:-2], [], [], 0
    assert stream[-2:] == b"\xff\xd9"
    for k in range(len(body) - 1):
        if body[k] == 0xFF and 0xD0 <= body[k + 1] <= 0xD7:
            parts.append(body[a:k])
            nums.append(body[k + 1] - 0xD0)
            a = k + 2
    return stream[:start], parts + [body[a:]], nums


def dri(stream):
    """the interval the stream's DRI segment declares, 0 without one; the segment must stand directly in front of SOS"""
    i = stream.find(b"\xff\xdd\x00\x04")
    if i < 0:
        return 0
    assert stream[i + 6:i + 8] == b"\xff\xda", "DRI is not directly in front of SOS"
    return stream[i + 4] << 8 | stream[i + 5]


def source(ica, layout, w, h, seed=1):
    plan, du = ica.host_transform(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8), 95)
    return helpers.baseline_layout_from_444(plan, du, LAYOUTS[layout])


def tplan_of(ica, data):
    t, why = ica.binding.transcode_plan(ica.HostDecoder.probe(data, 0))
    assert t is not None, why
    return t


def one_row(t, n):
    """the plan of n MCUs of t's kind in one row"""
    r = copy.deepcopy(t)
    r.plan.mcu_x, r.plan.mcu_y = n, 1
    r.plan.width, r.plan.height = n * 8 * (t.lh if t.ncomp == 3 else 1), 8 * (t.lv if t.ncomp == 3 else 1)
    return r


@pytest.fixture(scope="module")
def pairs():
    z = np.load(FIXTURE)
    return [(str(n), int(r), z["plain_" + str(n).split("_")[0]].tobytes(), z["restart_" + str(n)].tobytes()) for n, r in zip(z["names"], z["ri"])]


def test_fixture_holds_what_it_is_for(ica, pairs):
    """an interval whose padded last byte is 0xFF, nine intervals or more, an MCU count that is a multiple of Ri and one that is not"""
    assert os.path.getsize(FIXTURE) < 100 * 1024
    assert sum(any(b"\xff\x00\xff" + bytes([0xD0 + k]) in r for k in range(8)) for _, _, _, r in pairs) >= 1
    counts = [tplan_of(ica, p).plan.mcu_x * tplan_of(ica, p).plan.mcu_y for _, _, p, _ in pairs]
    assert max(-(-n // ri) for n, (_, ri, _, _) in zip(counts, pairs)) >= 9
    assert any(n % ri == 0 for n, (_, ri, _, _) in zip(counts, pairs)) and any(n % ri for n, (_, ri, _, _) in zip(counts, pairs))
    assert {n.split("_")[0] for n, _, _, _ in pairs} == {"444", "422", "420", "grey"}
    for _, ri, p, r in pairs:
        assert dri(r) == ri and dri(p) == 0


def test_against_libjpeg(ica, pairs):
    """1: the transcode of libjpeg's plain file at the pair's interval is libjpeg's restart file from its DRI segment to EOI, and
    transcoding the restart file with the same interval gives the same stream"""
    for name, ri, plain, rst in pairs:
        assert ica.transcode_memory(plain, optimize=False)[0][-len(split(plain)[1][0]) - 2:] == plain[-len(split(plain)[1][0]) - 2:], name
        got, why = ica.transcode_memory(plain, optimize=False, restart_mcus=ri)
        assert got is not None, (name, why)
        assert got[got.index(b"\xff\xdd"):] == rst[rst.index(b"\xff\xdd"):], name
        assert ica.transcode_memory(rst, optimize=False, restart_mcus=ri)[0] == got, name
        assert ica.transcode_memory(rst, optimize=False)[0] == ica.transcode_memory(plain, optimize=False)[0], name  # a source's DRI is not copied


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("optimize", [False, True])
def test_interval_decomposition(ica, layout, optimize):
    """2: interval k of a restart stream is the entropy-coded segment today's emitter writes for those MCUs alone as a one-row picture
    (under the stream's own tables where they are optimised: the model of emit_model.py, which the emission tests hold against mjw_emit),
    its marker is RST(k mod 8), and the restarted histogram is the sum of the intervals' own"""
    t = tplan_of(ica, source(ica, layout, 56, 40))
    dpm, ny, nm = t.plan.du_per_mcu, (t.lh * t.lv if t.ncomp == 3 else 1), t.plan.mcu_x * t.plan.mcu_y
    assert dpm == {"grey": 1, "444": 3, "422": 4, "420": 6}[layout] and nm >= 12
    du = em.adversarial_units(np.random.default_rng(dpm), nm, dpm, ny=ny)
    for ri in (1, 3, 5, nm - 1):
        s = ica.binding.emit_transcoded(t, du, optimize, restart_mcus=ri)
        assert s is not None and dri(s) == ri
        hdr, parts, nums = split(s)
        n_int = -(-nm // ri)
        assert len(parts) == n_int and nums == [k & 7 for k in range(n_int - 1)], (layout, ri)
        T, hlen = em.tables_from_stream(s)
        assert hlen == len(hdr)
        total = np.zeros((4, 256), np.int64)
        for k, part in enumerate(parts):
            m0, m1 = k * ri, min(nm, (k + 1) * ri)
            units = du[m0 * dpm:m1 * dpm]
            assert part == em.emit_entropy(T, units, dpm, ny=ny), (layout, ri, k)
            if not optimize:
                alone = ica.binding.emit_transcoded(one_row(t, m1 - m0), units, False)
                assert split(alone)[1] == [part], (layout, ri, k)
            total += hm.histogram(units, dpm, ny)
            if dpm in (3, 6):  # the writer's own two layouts: mjw_histogram itself
                p = copy.deepcopy(one_row(t, m1 - m0).plan)
                p.subsample = 1 if dpm == 6 else 0
                assert np.array_equal(ica.binding.write_histogram(p, units), hm.histogram(units, dpm, ny))
        got = ica.binding.restart_histogram(t, du, ri)
        assert np.array_equal(got, total), (layout, ri)
        if dpm in (3, 6):
            p = copy.deepcopy(t.plan)
            p.subsample = 1 if dpm == 6 else 0
            assert np.array_equal(ica.binding.restart_histogram(p, du, ri), total)
            assert ica.emit_jpeg(p, du, optimize, restart_mcus=ri)[-(len(s) - len(hdr)):] == s[len(hdr):]
        if optimize:  # the header's tables are those of the restarted counts
            tabs = hm.tables(total)
            assert tabs is not None
            want = ica.binding.transcode_header(t, (np.array([b for b, _ in tabs], np.uint8), np.array([np.pad(np.asarray(v, np.uint8), (0, 256 - len(v))) for _, v in tabs])))
            assert hdr == want[:-(10 if dpm == 1 else 14)] + bytes([0xFF, 0xDD, 0, 4, ri >> 8, ri & 255]) + want[-(10 if dpm == 1 else 14):]


def _pixels_pillow(data):
    try:
        from PIL import Image
    except ImportError:
        return None
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_decode_back(ica, oracle, layout):
    """3: for Ri in {1, 2, count - 1, count, count + 1, one row} the host walk and the oracle give the coefficients of the Ri = 0 stream, the
    live reference (where it is built) and Pillow (where importable) its pixels"""
    src = source(ica, layout, 72, 40, seed=7)
    t = tplan_of(ica, src)
    count = t.plan.mcu_x * t.plan.mcu_y
    base = ica.transcode_memory(src, optimize=True)[0]
    want_host, want_orc = ica.HostDecoder.decode(base, 0)[1], oracle.coef(base)
    ref = helpers.Reference() if helpers.Reference.available() else None
    want_ref = ref.load(base, 3)[1] if ref else None
    want_pil = _pixels_pillow(base)
    assert want_orc.size > 0
    for ri in (1, 2, count - 1, count, count + 1, t.plan.mcu_x):
        for optimize in (False, True):
            s = ica.transcode_memory(src, optimize=optimize, restart_mcus=ri)[0]
            assert dri(s) == ri
            assert np.array_equal(ica.HostDecoder.decode(s, 0)[1], want_host), (layout, ri)
            assert np.array_equal(oracle.coef(s), want_orc), (layout, ri)
            if ref:
                assert np.array_equal(ref.load(s, 3)[1], want_ref), (layout, ri)
            if want_pil is not None:
                assert np.array_equal(_pixels_pillow(s), want_pil), (layout, ri)
    assert ica.transcode_memory(src, optimize=True, restart_rows=1)[0] == ica.transcode_memory(src, optimize=True, restart_mcus=t.plan.mcu_x)[0]


def test_edges(ica):
    """4: Ri = 0 is today's call; Ri >= count differs by the DRI segment only; no trailing marker when Ri divides the count; 65535 is accepted
    and 65536, rows x mcu_x above 65535, a negative value and both at once are refused; the +-1500 DC pair is codable only with restarts; a
    worst-case unit at Ri = 1 fits MJW_STREAM_CAP"""
    B = ica.binding
    src = source(ica, "420", 64, 48)  # 4 x 3 MCUs
    t = tplan_of(ica, src)
    du = np.zeros((12 * 6, 64), np.int16)
    for opt in (False, True):
        today = ica.transcode_memory(src, optimize=opt)[0]
        assert ica.transcode_memory(src, optimize=opt, restart_mcus=0)[0] == today and ica.transcode_memory(src, optimize=opt, restart_rows=0)[0] == today
        assert B.emit_transcoded(t, du, opt, restart_mcus=0) == B.emit_transcoded(t, du, opt)
        for ri in (12, 13, 65535):
            s = ica.transcode_memory(src, optimize=opt, restart_mcus=ri)[0]
            i = s.index(b"\xff\xdd")
            assert s[:i] + s[i + 6:] == today and s[i:i + 6] == bytes([0xFF, 0xDD, 0, 4, ri >> 8, ri & 255]), ri
        for ri in (1, 2, 3, 4, 6):  # each divides 12
            hdr, parts, nums = split(ica.transcode_memory(src, optimize=opt, restart_mcus=ri)[0])
            assert len(parts) == 12 // ri and len(nums) == 12 // ri - 1 and all(parts)
    plan, pdu = ica.host_transform(np.random.default_rng(3).integers(0, 256, (40, 50, 3), dtype=np.uint8), 90)
    assert ica.emit_jpeg(plan, pdu, restart_mcus=0) == ica.emit_jpeg(plan, pdu) and ica.emit_jpeg(plan, pdu, True, restart_mcus=None) == ica.emit_jpeg(plan, pdu, True)
    assert ica.emit_jpeg(plan, pdu, restart_mcus=65536) is None and B.emit_transcoded(t, du, restart_mcus=65536) is None
    # the range, on a header alone: 300 MCUs a row
    wide = copy.deepcopy(t)
    wide.plan.mcu_x, wide.plan.mcu_y, wide.plan.width, wide.plan.height = 300, 400, 4800, 6400
    assert B.restart_interval(wide, None, 65535) == (65535, None) and B.restart_interval(wide, 218, None) == (65400, None)
    assert B.restart_interval(wide, 0, 0) == (0, None) and B.restart_interval(wide) == (0, None)
    for rows, mcus, word in ((None, 65536, "65535"), (219, None, "65535"), (1, 1, "both"), (-1, None, "negative"), (None, -5, "negative")):
        ri, why = B.restart_interval(wide, rows, mcus)
        assert ri is None and word in why, (rows, mcus, why)
    for kw in ({"restart_mcus": 65536}, {"restart_rows": 1, "restart_mcus": 1}, {"restart_mcus": -1}, {"restart_rows": 20000}):
        got, why = ica.transcode_memory(src, **kw)
        assert got is None and why, kw
    # DC +1500 then -1500: one segment cannot code the step of 3000, Ri = 1 predicts both from 0
    for layout in ("grey", "444"):
        pair = om.dc_grid(layout, (1500, -1500, 1500, -1500))[1]
        assert ica.transcode_memory(pair)[0] is None and ica.transcode_memory(pair, restart_mcus=2)[0] is None
        s = ica.transcode_memory(pair, restart_mcus=1)[0]
        assert s is not None
        tp = tplan_of(ica, s)
        u = B.units_from_region(*_region(ica, s))
        assert np.array_equal(u[:, 0].reshape(4, -1)[:, 0], [1500, -1500, 1500, -1500]) and not u[:, 1:].any()
        assert B.units_codable(tp, u) == (False, "a DC difference outside -2047..2047") and B.units_codable(tp, u, restart_mcus=1) == (True, None)
        climb = om.dc_grid(layout, (1000, 2000, 3000, 2000))[1]  # and the reverse: codable unbroken, 3000 against 0 is not
        assert ica.transcode_memory(climb)[0] is not None and ica.transcode_memory(climb, restart_mcus=1)[0] is None
    # the longest unit the ranges allow, every interval one grey unit: DC category 11 and 63 ACs of category 10 under the Annex-K tables
    g = one_row(tplan_of(ica, source(ica, "grey", 16, 8)), 40)
    worst = np.full((40, 64), -1023, np.int16)
    worst[:, 0] = np.where(np.arange(40) & 1, -2047, 2047)
    s = B.emit_transcoded(g, worst, False, restart_mcus=1)
    cap = 2048 + 40 * 64 * 7  # MJW_STREAM_CAP(40)
    L = ica.lib()
    L.mjw_temit_restart_to_memory.restype = C.c_size_t
    L.mjw_temit_restart_to_memory.argtypes = [C.POINTER(B.TranscodePlan), C.c_void_p, C.c_uint, C.c_int, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(cap)
    n = L.mjw_temit_restart_to_memory(C.byref(g), worst.ctypes.data_as(C.c_void_p), 0, 1, buf, cap)
    assert n == len(s) <= cap and buf.raw[:n] == s
    assert max(len(p) for p in split(s)[1]) + 2 <= 64 * 7, "an interval of one worst-case unit and its marker outgrow the 448 bytes a unit is given"
    assert L.mjw_temit_restart_to_memory(C.byref(g), worst.ctypes.data_as(C.c_void_p), 0, 1, buf, n - 1) == 0


def _region(ica, data):
    desc, region = ica.binding.host_decode_staged(data, 0, False)[:2]
    return desc, region, False


def test_the_transcode_header_of_a_default_plan_is_the_writers(ica):
    """the GPU encoder keeps one mjw_tplan per slot and writes every baseline header with mjw_theader_restart: for the writer's own
    4:2:0 / 4:4:4 plan (three components, lh = lv = subsample ? 2 : 1) that is mjw_header_restart byte for byte, over every comp,
    both samplings, tiny and padded sizes and the ends of the interval's range"""
    ica.lib()
    B, L = ica.binding, C.CDLL(ica.binding.LIB_PATH)  # a handle of its own: the prototypes set here stay off the one the other tests share
    L.mjw_plan_init.argtypes = [C.POINTER(B.WritePlan), C.c_int, C.c_int, C.c_int, C.c_int]
    L.mjw_header_restart.restype = L.mjw_theader_restart.restype = C.c_size_t
    L.mjw_header_restart.argtypes = [C.POINTER(B.WritePlan), C.c_int, C.c_char_p]
    L.mjw_theader_restart.argtypes = [C.POINTER(B.TranscodePlan), C.c_int, C.c_char_p]
    widths = (1, 7, 8, 16, 17, 200)
    cap = 607 + 6  # MJW_HEADER_RESTART_BYTES
    cases = 0
    for comp in (1, 2, 3, 4):
        for q in (1, 50, 90, 91, 100):
            for w, h in zip(widths, widths[::-1]):
                plan = B.WritePlan()
                assert L.mjw_plan_init(C.byref(plan), w, h, comp, q)
                t = B.TranscodePlan(copy.deepcopy(plan), 3, 2 if plan.subsample else 1, 2 if plan.subsample else 1)
                assert plan.subsample == (q <= 90)
                for ri in (0, 1, 5, 65535):
                    a, b = C.create_string_buffer(b"\xaa" * (cap + 8), cap + 8), C.create_string_buffer(b"\x55" * (cap + 8), cap + 8)
                    na, nb = L.mjw_header_restart(C.byref(plan), ri, a), L.mjw_theader_restart(C.byref(t), ri, b)
                    assert 0 < na == nb <= cap and a.raw[:na] == b.raw[:nb], (comp, q, w, h, ri)
                    assert a.raw[na:] == b"\xaa" * (cap + 8 - na) and b.raw[nb:] == b"\x55" * (cap + 8 - nb)
                    cases += 1
    assert cases == 480
