"""Where the entropy data ENDS -- a cut, a marker, padding, a restart boundary -- both Huffman walks carry hand-written rules that restate
the reference's bit reader (code_bits, nomore, the refill to 24 bits, the skip to the next 0xff after the last block).  These tests aim
at those rules on the CPU: the host walk against the oracle (verdict, reason, every de-quantised coefficient), the oracle against the
reference (live where it is built, always against what it answered, stored), and the gate in front of the GPU walk (mjh_extract_scan)
against the table of what it must keep and what it must leave to the host walk.

Bit-exact throughout.  For damaged streams the reference is compared on verdict and reason only: where it stops early at a missing RSTn
(codec/jpeg.c:1183) it leaves the blocks it never reached uninitialised; the oracle defines them as zero coefficients.

Measured on the build machine (one core): the progressive test 26 s (18772 streams), its MIJ_NO_PDEP twin 26 s, the baseline test 6 s
(2767 streams)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import helpers
import stream_cases as sc
from helpers import _dequantised_in_call_order


def _references():
    return (helpers.Reference() if helpers.Reference.available() else None), helpers.StoredReference()


def _product(ica, data, req):
    """-> ("ok", desc, arena) or ("fail", reason, None)"""
    try:
        desc, arena = ica.HostDecoder.decode(data, req)
        return "ok", desc, arena
    except ica.MijError as e:
        return "fail", str(e), None


def _check_group(ica, oracle, ref, stored, group, cases, req, progressive):
    """Every case of one base: product == oracle (verdict, reason, coefficients), oracle == reference (verdict, reason; live and stored).
    -> (accepted, {reason: rejected})"""
    want_ref = stored.verdicts(group, [c.data for c in cases], req)
    n_ok, fails = 0, {}
    for c, stored_v in zip(cases, want_ref):
        o = oracle.load(c.data, req)
        ov = helpers.verdict_of(o)
        assert ov == stored_v, "%s %s: oracle %s, the reference answered %s" % (group, c.name, ov, stored_v)
        if ref is not None:
            rv = helpers.verdict_of(helpers.primed_load(ref, c.data, req))
            assert ov == rv, "%s %s: oracle %s, live reference %s" % (group, c.name, ov, rv)
        p = _product(ica, c.data, req)
        if o[0] == "fail":
            assert p[0] == "fail" and p[1] == (o[1] if o[1] is not None else "decode failed"), \
                "%s %s: oracle fail:%s, host walk %s" % (group, c.name, o[1], "accepts" if p[0] == "ok" else "fail:" + p[1])
            fails[o[1]] = fails.get(o[1], 0) + 1
        else:
            assert p[0] == "ok", "%s %s: oracle accepts, host walk fail:%s" % (group, c.name, p[1])
            got = _dequantised_in_call_order(ica, p[1], p[2], progressive_order=progressive)
            want = oracle.coef(c.data, req)
            # a baseline scan that stops early at a missing RSTn (codec/jpeg.c:1183) transforms only the blocks it reached: the capture ends
            # there, and the blocks behind it are zero coefficients by the oracle's definition
            assert len(want) <= len(got) and np.array_equal(got[:len(want)], want) and not got[len(want):].any(), "%s %s: coefficients differ" % (group, c.name)
            n_ok += 1
    return n_ok, fails


def _progressive_bases(golden, ica):
    """the six reference-made progressive goldens (0.6-3.5 KB: every byte is cut) and the five writer-made bases of
    test_progressive_host_walk_vs_oracle_fuzz (up to 32 KB: seeded cuts)"""
    small = [(n, golden.jpg(n)) for n in golden.names if n.startswith("prog")]
    assert len(small) == 6
    rng = np.random.default_rng(23)
    large = []
    for (w, h, q, script, kind) in ((97, 51, 95, 1, "noise"), (64, 64, 92, 2, "noise"), (120, 88, 100, 1, "noise"), (200, 120, 95, 2, "synth"), (33, 17, 91, 1, "synth")):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8) if kind == "noise" else ica.synth_rgb(w, h, w)
        plan, du = ica.host_transform(img, q)
        large.append(("writer_%dx%d_s%d" % (w, h, script), helpers.progressive_from_du(plan, du, script)))
    return small, large


def test_progressive_cuts_host_walk_vs_oracle(golden, ica, oracle):
    """Progressive streams cut inside their entropy data, each cut followed by a marker or by nothing.  The goldens are cut at EVERY byte
    of every scan, once with an EOI behind the cut and once with the other tails in rotation (nothing, RST0..7, DHT, SOS); the writer-made
    bases at 400 seeded offsets plus every byte of the last 64 of each refinement scan, in the same two passes.

    About one cut in a thousand lands where the reference's refill meets the marker with few bits left and a later symbol fails its
    `size > code_bits` test ("bad huffman code"), while a reader that refills once too often, or at another moment, zero-fills and decodes
    on.  Those rejections must be in the set -- an all-accept set would prove nothing: the oracle and the reference make 6 of them on the
    goldens' EOI pass (prog_444_64x64 cut@3396, prog_420_64x64 cut@2034, prog_422_50x30 cut@863 and cut@1470, prog_grey_40x40 cut@558
    and cut@824)."""
    ref, stored = _references()
    small, large = _progressive_bases(golden, ica)
    t0 = time.time()
    n_cases = n_ok = 0
    bad_code_eoi_small = bad_code_large = 0
    for name, base in small:
        for tag, tails in (("eoi", (sc.EOI,)), ("tails", sc.OTHER_TAILS)):
            cases = sc.cut_cases(base, None, 0, tails)
            ok, fails = _check_group(ica, oracle, ref, stored, "%s/%s" % (name, tag), cases, 0, True)
            n_cases += len(cases)
            n_ok += ok
            if tag == "eoi":
                bad_code_eoi_small += fails.get("bad huffman code", 0)
    for bi, (name, base) in enumerate(large):
        extra = sc.refinement_tail_offsets(base, 64)
        assert extra
        for tag, tails in (("eoi", (sc.EOI,)), ("tails", sc.OTHER_TAILS)):
            cases = sc.cut_cases(base, 400, 100 + bi, tails, extra)
            assert len(cases) >= min(400, len(sc.cut_offsets(base)))
            ok, fails = _check_group(ica, oracle, ref, stored, "%s/%s" % (name, tag), cases, 0, True)
            n_cases += len(cases)
            n_ok += ok
            bad_code_large += fails.get("bad huffman code", 0)
    print("progressive cuts: %d streams, %d accepted, 'bad huffman code' on the goldens' EOI pass %d, on the writer-made bases %d, %.1f s"
          % (n_cases, n_ok, bad_code_eoi_small, bad_code_large, time.time() - t0))
    assert bad_code_eoi_small >= 6, bad_code_eoi_small
    assert bad_code_large >= 1, bad_code_large
    assert n_ok > 9000 and n_cases > 18000, (n_ok, n_cases)


def test_progressive_cuts_without_pdep():
    """The same cuts where the refinement scans read their correction bits one by one (MIJ_NO_PDEP=1, read once when the library
    initialises its tables): a process of its own, as test_progressive_refinement_without_pdep does."""
    env = dict(os.environ, MIJ_NO_PDEP="1")
    env.pop("REF_DIGESTS_RECORD", None)
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
                        os.path.join(here, "test_stream_ends_host.py") + "::test_progressive_cuts_host_walk_vs_oracle"],
                       env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def baseline_bases(ica):
    """the six layouts the extract gate was tabulated on (plain, DRI 1 / 4 / 2 / 3 / 2, grey, 4:2:2) plus 4:4:4 and 4:4:0"""
    out = []
    for i, (w, h, q, dri, lay) in enumerate(((64, 48, 90, 0, "native"), (64, 48, 90, 1, "native"), (200, 133, 90, 4, "native"), (97, 51, 95, 2, "grey"),
                                             (250, 131, 95, 3, "422"), (33, 17, 100, 2, "native"))):
        plan, du = ica.host_transform(ica.synth_rgb(w, h, 60 + i), q)
        out.append(("%dx%d_dri%d_%s" % (w, h, dri, lay), helpers.baseline_from_du(plan, du, dri, lay)))
    plan, du = ica.host_transform(ica.synth_rgb(120, 80, 70), 95)
    assert plan.du_per_mcu == 3
    out.append(("120x80_dri0_444", helpers.baseline_from_du(plan, du, 0, "native")))
    out.append(("120x80_dri5_440", helpers.baseline_layout_from_444(plan, du, [(1, 2), (1, 1), (1, 1)], restart_mcus=5)))
    return out


def boundary_inputs(ica):
    """-> (bases, small) for stream_cases.boundary_cases: two pictures of a few subsequences (4:2:0 and 4:4:4), an 8x8 picture (shorter than
    one subsequence of either length), a flat picture with a restart interval of one MCU (segments of a few bits)"""
    bases = []
    for i, (w, h, q) in enumerate(((200, 133, 90), (120, 80, 95))):
        plan, du = ica.host_transform(ica.synth_rgb(w, h, 80 + i), q)
        bases.append(helpers.baseline_from_du(plan, du, 0, "native"))
    plan, du = ica.host_transform(ica.synth_rgb(8, 8, 82), 90)
    tiny = helpers.baseline_from_du(plan, du, 0, "native")
    plan, du = ica.host_transform(np.full((48, 64, 3), 117, np.uint8), 90)
    flat = helpers.baseline_from_du(plan, du, 1, "native")
    return bases, [tiny, flat]


def baseline_groups(ica):
    """-> [(group, base, [Case])]: per base tail_cases + 150 seeded cuts (tails in rotation); then the boundary cases (base None)"""
    groups = []
    for bi, (name, base) in enumerate(baseline_bases(ica)):
        groups.append((name + "/tail", base, sc.tail_cases(base)))
        groups.append((name + "/cut", base, sc.cut_cases(base, 150, 200 + bi, sc.TAILS)))
    bases, small = boundary_inputs(ica)
    groups.append(("boundary", None, sc.boundary_cases(bases, small)))
    return groups


def extract_status(ica, data, req=3):
    from image_codecs_amd.binding import GpuScan
    L = ica.lib()
    L.mjh_extract_scan.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(GpuScan), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)]
    buf = np.zeros(len(data) + 4096, np.uint8)
    scan, n, why = GpuScan(), C.c_size_t(), C.c_char_p()
    return L.mjh_extract_scan(bytes(data), len(data), req, C.byref(scan), C.c_void_p(buf.ctypes.data), buf.size, C.byref(n), C.byref(why))


def test_baseline_stream_ends_host_walk_and_extract_gate(ica, oracle):
    """Baseline streams in eight layouts: the structural variants (stream_cases.tail_cases), 150 cuts per base with every tail, and streams
    that end on and around subsequence boundaries.  Host walk == oracle == reference as above, and the verdict of mjh_extract_scan -- which
    needs no device -- is the one its own rule gives: per kind from the table (stream_cases.KIND_STATUS), and for every case from the marker
    structure (stream_cases.expected_extract_status).  The GPU walk must be offered everything it can keep and nothing it cannot see whole."""
    ref, stored = _references()
    t0 = time.time()
    n_cases = n_ok = 0
    status = {1: 0, 2: 0}
    for group, _, cases in baseline_groups(ica):
        ok, fails = _check_group(ica, oracle, ref, stored, group, cases, 3, False)
        n_cases += len(cases)
        n_ok += ok
        for c in cases:
            st = extract_status(ica, c.data)
            want = sc.expected_extract_status(c.data)
            assert st == want, "%s %s: mjh_extract_scan says %d, the marker structure %d" % (group, c.name, st, want)
            if c.kind in sc.KIND_STATUS:
                assert st == sc.KIND_STATUS[c.kind], "%s %s: mjh_extract_scan says %d, kind '%s' is tabulated as %d" % (group, c.name, st, c.kind, sc.KIND_STATUS[c.kind])
            status[st] += 1
    print("baseline stream ends: %d streams, %d accepted, to the GPU walk %d, to the host walk by extraction %d, %.1f s"
          % (n_cases, n_ok, status[1], status[2], time.time() - t0))
    assert n_cases > 2000 and status[1] > 800 and status[2] > 300, (n_cases, status)
    assert 100 < n_ok < n_cases - 100, n_ok


def test_case_generators_are_deterministic_and_stay_inside_the_entropy_data(golden, ica):
    """cut_cases never touches a header or a table, takes the first and the last allowed offset when asked for every byte, and gives the
    same list for the same seed; block_ends (what the GPU tests predict completion rules from) ends every interval inside its last byte."""
    base = golden.jpg("prog_420_64x64")
    ranges = helpers.entropy_ranges(base)
    assert len(ranges) > 3
    every = sc.cut_cases(base, None)
    assert len(every) == sum(b - a for a, b in ranges)
    assert every[0].data == base[:ranges[0][0] + 1] + sc.EOI and every[-1].data == base[:ranges[-1][1]] + sc.EOI
    a = sc.cut_cases(base, 50, 7, sc.TAILS)
    b = sc.cut_cases(base, 50, 7, sc.TAILS)
    assert [c.name for c in a] == [c.name for c in b] and [c.data for c in a] == [c.data for c in b] and len({c.name for c in a}) == 50
    for c in a:
        cut = int(c.name[4:c.name.index("+")])
        assert any(lo < cut <= hi for lo, hi in ranges), c.name
    for name, data in baseline_bases(ica)[:4]:
        for nbits, ends in sc.block_ends(data):
            assert ends and 0 <= nbits - ends[-1] < 8, name
    assert oracle_accepts_run_past_63(sc.run_past_63_stream())


def oracle_accepts_run_past_63(data):
    o = helpers.Oracle().load(data, 1)
    return o[0] == "ok" and o[1].shape == (8, 8, 1)
