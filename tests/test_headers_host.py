"""The layer in front of the entropy data, on the CPU: the marker parser, the frame and scan headers and the Huffman table builders of the
host stage (jpeg_entropy.c) against the restatement (oracle_jpeg.c) and the reference (live where it is built, always against what it
answered, stored), over the families of header_cases.py -- segment arrangements, frame layouts, scan structures, table shapes, and one
minimal edit per failure reason.

Per case: verdict and reason three ways; for accepted streams the oracle's pixels against the reference's digest (3 and 4 channels), the
host walk's coefficients against the oracle's in the order and with the quantisation tables the reference de-quantises them in -- both
staging formats -- stbi_info_from_memory, and the gate in front of the GPU walk (mjh_extract_scan) against the status tabulated per kind;
what the gate hands out walks, sequentially, to the host walk's coefficients."""
import ctypes as C

import numpy as np
import pytest

import coef_cases as cc
import header_cases as hc
import helpers
from helpers import _dequantised_in_call_order

ZIG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50,
                43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def scan_structure(data):
    """-> (progressive, [[component index, ...] per scan]) of a stream, from its SOF and SOS segments alone"""
    ids, prog, groups, i = [], False, [], 2
    while i + 4 <= len(data):
        if data[i] != 0xFF or data[i + 1] == 0xFF:
            i += 1
            continue
        m = data[i + 1]
        if m == 0xD9:
            break
        if m in (0x00, 0x01) or 0xD0 <= m <= 0xD8:
            i += 2
            continue
        n = (data[i + 2] << 8) | data[i + 3]
        p = data[i + 4:i + 2 + n]
        if m in (0xC0, 0xC1, 0xC2):
            prog = m == 0xC2
            ids = [p[6 + 3 * c] for c in range(p[5])]
        elif m == 0xDA:
            groups.append([ids.index(p[1 + 2 * k]) for k in range(p[0])])
        i += 2 + n
    return prog, groups


def dequantised_in_scan_order(ica, desc, arena, data):
    """The host walk's planes in the order the reference transforms them, de-quantised with the descriptor's tables: a baseline file scan
    by scan (a scan of one component over that component's own block grid, a scan of several over the MCUs), a progressive file plane by
    plane when all scans are in."""
    prog, groups = scan_structure(data)
    if prog:
        return _dequantised_in_call_order(ica, desc, arena, progressive_order=True)
    planes = ica.detile_coefficients(desc, arena)
    dq = [np.array(desc.dequant[desc.comp[i].tq][:], dtype=np.int32).reshape(8, 8) for i in range(desc.ncomp)]
    blocks = []
    for g in groups:
        if len(g) == 1:
            cp = desc.comp[g[0]]
            for j in range((cp.y + 7) >> 3):
                for i in range((cp.x + 7) >> 3):
                    blocks.append((planes[g[0]][j, i].astype(np.int32) * dq[g[0]]).astype(np.int16))
            continue
        for my in range(desc.mcu_y):
            for mx in range(desc.mcu_x):
                for ci in g:
                    cp = desc.comp[ci]
                    for y in range(cp.v):
                        for x in range(cp.h):
                            blocks.append((planes[ci][my * cp.v + y, mx * cp.h + x].astype(np.int32) * dq[ci]).astype(np.int16))
    return np.stack(blocks).reshape(-1) if blocks else np.zeros(0, np.int16)


def extract(ica, data, req=3):
    """mjh_extract_scan with room for every restart interval's padding: -> (status, scan, stream bytes)"""
    from image_codecs_amd.binding import GpuScan
    L = ica.lib()
    L.mjh_extract_scan.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(GpuScan), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)]
    buf = np.zeros(len(data) + 48 * (data.count(b"\xff") + 1) + 4096, np.uint8)
    scan, n, why = GpuScan(), C.c_size_t(), C.c_char_p()
    st = L.mjh_extract_scan(bytes(data), len(data), req, C.byref(scan), C.c_void_p(buf.ctypes.data), buf.size, C.byref(n), C.byref(why))
    return st, scan, bytes(buf[:n.value])


def _product(ica, data, req):
    try:
        desc, arena = ica.HostDecoder.decode(data, req)
        return "ok", desc, arena
    except ica.MijError as e:
        return "fail", str(e), None


def check_case(ica, oracle, c, req=3):
    """product == oracle for one case: verdict, reason, coefficients in both staging formats.  -> the oracle's load result"""
    o = oracle.load(c.data, req)
    p = _product(ica, c.data, req)
    if o[0] == "fail":
        assert p[0] == "fail" and p[1] == (o[1] if o[1] is not None else "decode failed"), \
            "%s: oracle fail:%s, host walk %s" % (c.name, o[1], "accepts" if p[0] == "ok" else "fail:" + p[1])
        with pytest.raises(ica.MijError) as e:
            ica.host_decode_staged(c.data, req, True)
        assert str(e.value) == p[1], (c.name, str(e.value), p[1])
        return o
    assert p[0] == "ok", "%s: oracle accepts, host walk fail:%s" % (c.name, p[1])
    desc, arena = p[1], p[2]
    got = dequantised_in_scan_order(ica, desc, arena, c.data)
    want = oracle.coef(c.data, req)
    assert got.shape == want.shape and np.array_equal(got, want), "%s: coefficients differ (%s, %s)" % (c.name, got.shape, want.shape)
    dc, region = ica.host_decode_staged(c.data, req, True)
    assert (dc.flags & 1) == (desc.flags & 1) and dc.color == desc.color, c.name
    assert bytes(dc.dequant) == bytes(desc.dequant) and [dc.comp[i].tq for i in range(dc.ncomp)] == [desc.comp[i].tq for i in range(desc.ncomp)], c.name
    if dc.flags & 4:
        assert not scan_structure(c.data)[0], c.name
        staged = ica.expand_compact_region(dc, region)
        assert np.array_equal(staged, arena[:staged.size]), "%s: compact staging differs from int16 staging" % c.name
    else:
        n = desc.coef_elems()
        assert np.array_equal(region[:2 * n].view(np.int16), arena[:n]), c.name
    return o


@pytest.mark.parametrize("family", list(hc.FAMILIES))
def test_family_host(ica, oracle, family):
    ref = helpers.Reference() if helpers.Reference.available() else None
    stored = helpers.StoredReference()
    cases = hc.family(family)
    want = stored.verdicts("headers/" + family, [c.data for c in cases], 3)
    n_ok = 0
    status = {0: 0, 1: 0, 2: 0}
    for c, stored_v in zip(cases, want):
        o = check_case(ica, oracle, c)
        ov = helpers.verdict_of(o)
        assert ov == stored_v, "%s: oracle %s, the reference answered %s" % (c.name, ov, stored_v)
        if ref is not None:
            rv = helpers.verdict_of(helpers.primed_load(ref, c.data, 3))
            assert ov == rv, "%s: oracle %s, live reference %s" % (c.name, ov, rv)
        if o[0] == "ok":
            n_ok += 1
            for req in (3, 4):
                oo = o if req == 3 else oracle.load(c.data, req)
                assert helpers.digest_load(oo) == stored.load(c.data, req), "%s: the oracle's pixels (%d channels) are not the reference's" % (c.name, req)
                if ref is not None:
                    assert np.array_equal(ref.load(c.data, req)[1], oo[1]), (c.name, req)
        # stbi_info_from_memory
        ok, x, y, comp = ica.stbi_info_from_memory(c.data)
        mine = "%d %d %d %d" % (ok, x, y, comp) if ok else "0"
        assert mine == stored.info(c.data), "%s: info %s, the reference %s" % (c.name, mine, stored.info(c.data))
        oi = oracle.info(c.data)
        assert ("%d %d %d %d" % tuple(oi) if oi[0] else "0") == mine, (c.name, oi, mine)
        # the gate in front of the GPU walk
        assert c.status == hc.KIND_STATUS[c.kind]
        st, scan, stream = extract(ica, c.data)
        assert st == c.status, "%s: mjh_extract_scan says %d, kind '%s' is tabulated as %d" % (c.name, st, c.kind, c.status)
        status[st] += 1
        if st == 0:
            assert o[0] == "fail", c.name
        if st == 1 and o[0] == "ok":
            got, slack = helpers._walk_extracted_scan(scan, stream)
            assert 0 <= slack < 8, (c.name, slack)
            desc, arena = ica.HostDecoder.decode(c.data, 3)
            assert bytes(scan.desc.dequant) == bytes(desc.dequant), "%s: the gate hands out other quantisation tables than the host walk ends with" % c.name
            planes = ica.detile_coefficients(desc, arena)
            bpm, mcu_x = scan.blocks_per_mcu, desc.mcu_x
            for b in range(scan.nblocks):
                m, k = divmod(b, bpm)
                ci = scan.blk_comp[k]
                bx = (m % mcu_x) * desc.comp[ci].h + scan.blk_dx[k]
                by = (m // mcu_x) * desc.comp[ci].v + scan.blk_dy[k]
                assert np.array_equal(got[b], planes[ci][by, bx].reshape(64)[ZIG]), (c.name, b, ci, bx, by)
    print("%s: %d cases, %d accepted, extraction status %s" % (family, len(cases), n_ok, status))
    if family == "reasons":
        seen = {v[5:] for v in want if v != "ok"}
        missing = [r for r in hc.REASONS + ("None",) if r not in seen]
        assert not missing and n_ok == 0, (missing, n_ok)
    elif family == "tables":
        assert n_ok == len(cases) and status[1] >= len(cases) - 2
    else:
        assert n_ok >= len(cases) - 1 and status[1] >= 5 and status[2] >= 3, (n_ok, status)


def test_product_only_host_stage_equals_the_restatement(ica, oracle):
    """Streams the reference does not define an answer for: the host stage and the restatement, which both start from cleared tables,
    still agree on verdict, reason and coefficients -- and the gate neither takes a stream the host walk rejects nor faults on one."""
    for c in hc.family("product_only"):
        o = check_case(ica, oracle, c)
        st, _, _ = extract(ica, c.data)
        assert st in (0, 1, 2) and (st != 0 or o[0] == "fail"), (c.name, st)


def test_builder_reproduces_the_test_side_writer(ica):
    """With the tables and the arrangement parsed out of a pw_write_baseline_ex stream, the Writer gives that stream byte for byte:
    4:2:0, grey and CMYK, with and without a restart interval -- its coder, stuffing, padding and restart numbering are the C writer's,
    and optimal_table is its gen_table."""
    for layout, (w, h) in (("420", (72, 40)), ("grey", (41, 23)), ("cmyk", (40, 24)), ("411", (70, 9))):
        for restart in (0, 1, 3, 11):
            planes = cc._tame(cc.blank(layout, w, h), seed=restart)
            planes[0][0, 0, 5] = -300   # beyond a byte, and a long run in front of a last coefficient
            planes[-1][-1, -1, 63] = 77
            case = cc.Case("w", "w", layout, w, h, planes, restart=restart)
            data = case.stream()
            assert hc.rewrite(data, case.planes) == data, (layout, restart)
            # ... and with tables of its own making
            a = hc.parse_arrangement(data)
            hv = [(c[1], c[2]) for c in a["comps"]]
            assert hc.plain(w, h, hv, case.planes, restart, a["app14"], qt=a["qt"]).bytes() == data, (layout, restart)


def test_table_shapes():
    """shape_table: canonical codes over a given profile, pins honoured, refusals; the Kraft sum of every table of every family's
    streams is at most one."""
    bits, vals = hc.shape_table([5, 6, 7], [0, 1, 2] + [0] * 13, {7: 2})
    assert bits == tuple([0, 1, 2] + [0] * 13) and vals == (7, 5, 6)
    assert hc.canonical(bits, vals) == {7: (0, 2), 5: (2, 3), 6: (3, 3)}
    assert hc.canonical((0, 2) + (0,) * 14, (9, 9), "last") == {9: (1, 2)} and hc.canonical((0, 2) + (0,) * 14, (9, 9)) == {9: (0, 2)}
    bits, vals = hc.shape_table([1, 2], [1] * 15 + [2], {1: 16}, last=(1,))
    assert vals[-1] == 1 and hc.canonical(bits, vals)[1] == (0xFFFF, 16) and hc.kraft(bits) == 65536
    for bad in (lambda: hc.shape_table([1, 2, 3], [1, 1] + [0] * 14), lambda: hc.shape_table([1], [3] + [0] * 15),
                lambda: hc.shape_table([1, 2], [0, 1, 1] + [0] * 13, {1: 2, 2: 2}), lambda: hc.shape_table([1], [0] * 8 + [257] + [0] * 7)):
        with pytest.raises(ValueError):
            bad()
    n = 0
    for fam in list(hc.FAMILIES) + ["product_only"]:
        for c in hc.family(fam):
            for t in c.meta.get("tables", ()):
                assert hc.kraft(t[2]) <= 65536 and sum(t[2]) == len(t[3]) <= 256, (c.name, t[:3])
                n += 1
    assert n > 400


def test_every_table_shape_reaches_the_branch_it_names():
    """A plain sequential walk of each `tables` stream counts what it makes a decoder do (header_cases.walk_events); every event a shape
    names must occur (a minimum of 0 means: must NOT occur), and the stream must decode at all under its own tables."""
    for c in hc.family("tables"):
        if c.status != 1:
            continue
        ev = hc.walk_events(c.data)
        for name, least in c.meta["events"].items():
            assert (ev[name] >= least) if least else ev[name] == 0, "%s: '%s' occurs %d times" % (c.name, name, ev[name])
