"""Optimised Huffman tables on the host (include/mij_host.h: mjw_histogram, mjw_optimal_table, mjw_header_optimized,
mjw_emit_optimized): the Python model (hufopt_model) against files libjpeg wrote, the C pieces against the model, and the optimised
stream against the plain one -- same coefficients, same pixels, fewer bytes on the benchmark's pictures."""
import ctypes as C
import io

import numpy as np
import pytest

import emit_model as em
import helpers
import hufopt_model as hm


def plan_for(ica, w, h, c, q):
    p = ica.binding.WritePlan()
    L = ica.lib()
    L.mjw_plan_init.argtypes = [C.POINTER(ica.binding.WritePlan), C.c_int, C.c_int, C.c_int, C.c_int]
    assert L.mjw_plan_init(C.byref(p), w, h, c, q)
    return p


def plain_header(ica, plan):
    L = ica.lib()
    L.mjw_header.restype = C.c_size_t
    L.mjw_header.argtypes = [C.POINTER(ica.binding.WritePlan), C.c_void_p]
    buf = np.zeros(em.HDR, np.uint8)
    assert L.mjw_header(C.byref(plan), buf.ctypes.data_as(C.c_void_p)) == em.HDR
    return bytes(buf)


def _pillow():
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


def test_fast_code_sizes_equal_the_literal_procedure():
    """the heap form of K.2's loop used below gives the code sizes of the loop as the contract spells it, ties included"""
    rng = np.random.default_rng(1)
    for i in range(40):
        f = rng.integers(0, [3, 10, 1000, 1 << 31][i % 4], size=256)
        f[rng.random(256) < (i % 5) * 0.2] = 0
        assert hm.code_sizes(f) == hm.code_sizes_literal(f), i
    for f in ([1] * 256, [0] * 255 + [1], [7, 7] + [0] * 254, hm.deep_counts(33) + [0] * 223):
        assert hm.code_sizes(f) == hm.code_sizes_literal(f)


def test_model_equals_libjpeg_tables():
    """1: 24 seeded baseline files written by Pillow with optimize=True (noise, ramps, flat; quality 5-100; subsampling 0, 1, 2;
    sizes 8-200; RGB and grey): every DHT table of the file equals the model's table for the file's own symbol counts"""
    Image = _pillow()
    if Image is None:
        pytest.skip("Pillow is not installed")
    rng = np.random.default_rng(24)
    tables = 0
    for i in range(24):
        w, h = int(rng.integers(8, 201)), int(rng.integers(8, 201))
        kind, q, sub = i % 3, [5, 20, 50, 75, 90, 95, 100, 35][i % 8], (i // 3) % 3
        grey = i % 6 == 5
        if kind == 0:
            a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        elif kind == 1:
            yy, xx = np.mgrid[0:h, 0:w]
            a = np.stack([(xx * 255 // max(1, w - 1)), (yy * 255 // max(1, h - 1)), ((xx + yy) * 3 % 256)], axis=2).astype(np.uint8)
        else:
            a = np.full((h, w, 3), [int(v) for v in rng.integers(0, 256, 3)], dtype=np.uint8)
        buf = io.BytesIO()
        if grey:
            Image.fromarray(a[:, :, 0], "L").save(buf, "JPEG", quality=q, optimize=True)
        else:
            Image.fromarray(a, "RGB").save(buf, "JPEG", quality=q, optimize=True, subsampling=sub)
        for bits, vals, counts in hm.scan_symbol_counts(buf.getvalue()):
            assert hm.optimal_table(counts) == (bits, vals), (i, w, h, q, sub, grey)
            tables += 1
    assert tables >= 80


def _histograms():
    rng = np.random.default_rng(1000)
    out = []
    for i in range(1000):
        hi = [2, 4, 100, 1 << 16, 1 << 31, (1 << 31) + 1][i % 6]
        f = rng.integers(0, hi, size=256, dtype=np.int64)
        f[rng.random(256) < (i % 7) / 7.0] = 0  # from all 256 symbols down to a few
        out.append(f)
    one = np.zeros(256, np.int64)
    one[0x21] = 5
    two = np.zeros(256, np.int64)
    two[[3, 200]] = 9
    out += [one, two, np.ones(256, np.int64)]
    return out


def _deep(depth, rng=None):
    """Fibonacci-like counts on `depth` scattered symbols"""
    f = np.zeros(256, np.int64)
    idx = np.arange(0, 256, 7)[:depth] if rng is None else rng.permutation(256)[:depth]
    f[idx] = hm.deep_counts(depth)
    return f


def test_optimal_table_equals_model(ica):
    """2: mjw_optimal_table on 1000 seeded histograms with counts from 0 up to 2^31, one symbol, two equal symbols, 256 symbols of
    count 1, chains of unlimited depth 17, 24 and 32 (K.3's shortening), and depth 33, which returns 0"""
    for i, f in enumerate(_histograms()):
        assert ica.optimal_huffman_table(f) == hm.optimal_table(f), i
    assert ica.optimal_huffman_table(_histograms()[1000]) == ([1] + [0] * 15, [0x21])
    rng = np.random.default_rng(2)
    for depth in (17, 24, 32):
        for f in (_deep(depth), _deep(depth, rng)):
            assert hm.unlimited_depth(f) == depth
            got = ica.optimal_huffman_table(f)
            assert got == hm.optimal_table(f), depth
            assert sum(got[0]) == depth and max(l + 1 for l, n in enumerate(got[0]) if n) == 16
    f = _deep(33)
    assert hm.unlimited_depth(f) == 33 and hm.optimal_table(f) is None
    assert ica.optimal_huffman_table(f) is None


def _writer_units(ica, kind, w, h, q):
    rng = np.random.default_rng(w * 1000 + h)
    if kind == "noise":
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == "ramp":
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([xx * 255 // (w - 1), yy * 255 // (h - 1), (xx + 2 * yy) % 256], axis=2).astype(np.uint8)
    else:
        img = np.full((h, w, 3), (200, 40, 90), np.uint8)
    return ica.host_transform(img, q)


def _unit_cases(ica):
    """(name, plan, units): the model's adversarial units and the writer's own for a noise picture, a ramp and a flat picture, at
    quality 90 (4:2:0) and 95 (4:4:4)"""
    out = []
    for q in (90, 95):
        rng = np.random.default_rng(q)
        p = plan_for(ica, 72, 40, 3, q)
        out.append(("adversarial q%d" % q, p, em.adversarial_units(rng, p.mcu_x * p.mcu_y, p.du_per_mcu)))
        for kind, (w, h) in (("noise", (57, 33)), ("ramp", (64, 48)), ("flat", (40, 40))):
            p, du = _writer_units(ica, kind, w, h, q)
            out.append(("%s q%d" % (kind, q), p, du))
    return out


def test_histogram_equals_numpy_count(ica):
    """3: mjw_histogram against the model's numpy count"""
    for name, p, du in _unit_cases(ica):
        got = ica.write_histogram(p, du)
        assert got is not None and np.array_equal(got.astype(np.int64), hm.histogram(du, p.du_per_mcu)), name
        assert got[0].sum() + got[1].sum() == du.shape[0], name  # one DC category per unit


def test_emit_optimized_equals_model(ica):
    """4: mjw_emit_optimized = the model header + emit_model.emit_entropy under the header's tables + EOI, on the same units at quality
    90 and 95; mjw_header_optimized alone gives the model header"""
    L = ica.lib()
    L.mjw_header_optimized.restype = C.c_size_t
    L.mjw_header_optimized.argtypes = [C.POINTER(ica.binding.WritePlan), C.c_void_p, C.c_void_p, C.c_void_p]
    for name, p, du in _unit_cases(ica):
        plain = plain_header(ica, p)
        want = hm.emit_optimized(plain, du, p.du_per_mcu)
        got = ica.emit_jpeg(p, du, optimize=True)
        assert got == want, name
        tabs = hm.tables(hm.histogram(du, p.du_per_mcu))
        bits = np.array([t[0] for t in tabs], np.uint8)
        vals = np.zeros((4, 256), np.uint8)
        for k, t in enumerate(tabs):
            vals[k, :len(t[1])] = t[1]
        buf = np.zeros(em.HDR, np.uint8)
        n = L.mjw_header_optimized(C.byref(p), bits.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p))
        assert n <= em.HDR and bytes(buf[:n]) == hm.header(plain, tabs) == got[:n], name
        assert ica.emit_jpeg(p, du) == plain + em.emit_entropy(em.tables_from_header(plain), du, p.du_per_mcu) + b"\xff\xd9", name


def test_flat_picture_gets_one_bit_chroma_codes(ica):
    """a flat grey picture's chroma tables hold one symbol each, coded in one bit"""
    p, du = ica.host_transform(np.full((64, 64, 3), 128, np.uint8), 90)
    got = ica.emit_jpeg(p, du, optimize=True)
    t = hm.tables_from_header(got[:got.index(b"\xff\xda") + 14])
    assert t[1] == {0: (0, 1)} and t[3] == {0: (0, 1)}


def test_over_32_falls_back_to_the_plain_stream(ica):
    """units whose luma AC counts form a chain of depth 33 (the counts scaled down would not: only the real counts reach it) are
    written with the plain tables: mjw_emit_optimized == mjw_emit; mjw_optimized_tables says 0"""
    import deep_units
    p, du = deep_units.deep_chain_units(ica, 33)
    f = hm.histogram(du, p.du_per_mcu)
    assert hm.unlimited_depth(f[2]) == 33
    L = ica.lib()
    L.mjw_optimized_tables.argtypes = [C.POINTER(ica.binding.WritePlan), C.c_void_p, C.c_void_p, C.c_void_p]
    bits, vals = np.zeros((4, 16), np.uint8), np.zeros((4, 256), np.uint8)
    assert L.mjw_optimized_tables(C.byref(p), du.ctypes.data_as(C.c_void_p), bits.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p)) == 0
    assert ica.emit_jpeg(p, du, optimize=True) == ica.emit_jpeg(p, du)
    p, du = deep_units.deep_chain_units(ica, 20)
    assert hm.unlimited_depth(hm.histogram(du, p.du_per_mcu)[2]) == 20
    assert ica.emit_jpeg(p, du, optimize=True) == hm.emit_optimized(plain_header(ica, p), du, p.du_per_mcu)


def test_same_coefficients_and_pixels(ica, oracle):
    """5: the optimised stream decodes to the plain stream's coefficients and pixels: the oracle, the product's host decoder and,
    where it was built, the reference"""
    ref = helpers.Reference() if helpers.Reference.available() else None
    for name, p, du in _unit_cases(ica):
        if name.startswith("adversarial"):
            continue  # not a picture's units: values no decoder's output range was made for
        plain, opt = ica.emit_jpeg(p, du), ica.emit_jpeg(p, du, optimize=True)
        assert opt != plain
        assert np.array_equal(oracle.coef(opt), oracle.coef(plain)), name
        a, b = oracle.load(opt), oracle.load(plain)
        assert a[0] == b[0] == "ok" and np.array_equal(a[1], b[1]), name
        (_, ca), (_, cb) = ica.HostDecoder.decode(opt), ica.HostDecoder.decode(plain)
        assert np.array_equal(ca, cb), name
        if ref is not None:
            r = ref.load(opt)
            assert r[0] == "ok" and np.array_equal(r[1], b[1]), name


@pytest.mark.parametrize("q", [90, 95])
def test_optimised_stream_is_shorter_on_the_bench_pictures(ica, q):
    """6: synth_rgb seeds 0-3 at 512 x 384: the optimised stream is shorter than the plain one (a condition on these inputs;
    observed ratios 0.904-0.906 at quality 90 and 0.946-0.947 at quality 95)"""
    for seed in range(4):
        p, du = ica.host_transform(ica.synth_rgb(512, 384, seed), q)
        plain, opt = ica.emit_jpeg(p, du), ica.emit_jpeg(p, du, optimize=True)
        print("q%d seed %d: %d -> %d bytes, ratio %.4f" % (q, seed, len(plain), len(opt), len(opt) / len(plain)))
        assert len(opt) < len(plain), (seed, len(opt), len(plain))


def test_histogram_refuses_counts_beyond_32_bits(ica):
    """a plan of more than 2^32 / 64 units is refused before any unit is read"""
    p = plan_for(ica, 65535, 65535, 3, 95)
    assert p.mcu_x * p.mcu_y * p.du_per_mcu * 64 >= 1 << 32
    L = ica.lib()
    L.mjw_histogram.argtypes = [C.POINTER(ica.binding.WritePlan), C.c_void_p, C.c_void_p]
    freq = np.zeros((4, 256), np.uint32)
    assert L.mjw_histogram(C.byref(p), np.zeros(64, np.int16).ctypes.data_as(C.c_void_p), freq.ctypes.data_as(C.c_void_p)) == 0


def test_tensor_encoder_refuses_non_bool_optimize(ica):
    """7: TensorEncoder.encode(optimize=...) takes a bool only, checked before any device call (no GPU here)"""
    enc = ica.TensorEncoder()
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="optimize"):
            enc.encode([], optimize=bad)
    assert enc.encode([], optimize=True) == []


def test_host_pieces_under_sanitizers(tmp_path):
    """tests/support/san_hufopt.c: histogram, table build, optimised emission (to a callback and to memory) on exact-size heap blocks
    under ASan + UBSan, as a stand-alone CPU program"""
    import os
    import subprocess
    root = helpers.ROOT
    exe = str(tmp_path / "san_hufopt")
    cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-I" + root + "/include", "-I" + root + "/image-codecs_amd/csrc", "-o", exe,
           root + "/tests/support/san_hufopt.c", root + "/image-codecs_amd/csrc/jpeg_write_host.c"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("no address sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-2000:]
    assert "hufopt harness: 0 failures" in run.stdout
