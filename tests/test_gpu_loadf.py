"""The float loaders and the batch's float output on the GPU (k_out_f32), bit for bit against stbi__ldr_to_hdr applied with
libm's pow to the uint8 pixels the reference (golden vectors) or the oracle made."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import helpers
import loadf_expect as fx

pytestmark = pytest.mark.gpu

MIJ_E_ARG, MIJ_E_STATE = -2, -5
UNINIT_IN_REFERENCE = {"dri_without_rst"}  # the reference reads uninitialised planes here (test_gpu_parity.py)


def _expect(pixels, gamma=2.2, scale=1.0):
    return fx.apply(fx.lut(pixels.shape[-1], gamma, scale), pixels)


def test_loadf_golden_every_req_comp(ica, gpu_ctx, golden):
    checked = failed = 0
    for name in golden.names:
        data = golden.jpg(name)
        for req in range(5):
            kind, want = golden.expect(name, req)
            if kind == "skip":
                continue
            got = ica.stbi_loadf_from_memory(data, req)
            if kind == "fail":
                assert got is None, (name, req)
                assert ica.stbi_failure_reason() == "unknown image type", (name, req)
                failed += 1
                continue
            assert got is not None, (name, req, ica.stbi_failure_reason())
            px, x, y, comp = got
            u8 = ica.stbi_load_from_memory(data, req)
            assert (x, y, comp) == u8[1:], (name, req)
            if name in UNINIT_IN_REFERENCE:
                want = u8[0]
            assert px.shape == want.shape, (name, req)
            assert fx.same_bits(px, _expect(want)), (name, req)
            checked += 1
    assert checked >= 250 and failed >= 20


@pytest.mark.parametrize("w,h", [(200, 120), (33, 17), (1920, 1080)])
def test_loadf_both_front_ends(ica, oracle, gpu_ctx, w, h):
    """below MIJ_GPU_WALK_MIN_PIXELS the host walk, at 1080p the GPU walk"""
    data = ica.synth_jpeg(w, h, seed=w + h, quality=90)
    for req in (0, 1, 2, 3, 4):
        got = ica.stbi_loadf_from_memory(data, req)
        assert got is not None, ica.stbi_failure_reason()
        assert fx.same_bits(got[0], _expect(oracle.load(data, req)[1])), (w, h, req)


def test_loadf_gamma_scale_and_flip(ica, oracle, gpu_ctx):
    data = ica.synth_jpeg(96, 71, seed=5, quality=95)
    want4 = oracle.load(data, 4)[1]
    try:
        for gamma, scale in ((1.0, 2.5), (0.5, 1.0), (3.7, 0.25)):
            ica.stbi_ldr_to_hdr_gamma(gamma)
            ica.stbi_ldr_to_hdr_scale(scale)
            assert fx.same_bits(ica.stbi_loadf_from_memory(data, 4)[0], _expect(want4, gamma, scale)), (gamma, scale)
            ica.stbi_hdr_to_ldr_gamma(gamma)  # never read for JPEG
            ica.stbi_hdr_to_ldr_scale(scale)
    finally:
        ica.stbi_ldr_to_hdr_gamma(2.2)
        ica.stbi_ldr_to_hdr_scale(1.0)
    assert fx.same_bits(ica.stbi_loadf_from_memory(data, 4)[0], _expect(want4))
    try:
        ica.stbi_set_flip_vertically_on_load(1)
        for req in (0, 2, 3):
            assert fx.same_bits(ica.stbi_loadf_from_memory(data, req)[0], _expect(oracle.load(data, req)[1])[::-1]), req
        big = ica.synth_jpeg(1920, 1080, seed=2)
        assert fx.same_bits(ica.stbi_loadf_from_memory(big, 3)[0], _expect(oracle.load(big, 3)[1])[::-1])
    finally:
        ica.stbi_set_flip_vertically_on_load(0)


def test_loadf_file_callbacks_and_name(ica, oracle, gpu_ctx, tmp_path):
    data = ica.synth_jpeg(130, 67, seed=8)
    want = _expect(oracle.load(data, 3)[1])
    path = tmp_path / "p.jpg"
    path.write_bytes(b"\0" * 10 + data + b"tail")
    (res, pos) = ica.stbi_loadf_from_file(str(path), 3, offset=10)
    assert res is not None and fx.same_bits(res[0], want)
    (res8, pos8) = ica.stbi_load_from_file(str(path), 3, offset=10)
    assert res8 is not None
    # the 8-bit loader seeks back over what its 128-byte reads took beyond the end of the stream (convert.c:208); the float loader
    # does not (convert.c:331-336).  The stream does not end on a read boundary, so the last read took bytes beyond it.
    assert len(data) % 128 != 0
    assert pos8 <= 10 + len(data) < pos <= 10 + len(data) + 4, (pos, pos8)
    path.write_bytes(data)
    res = ica.stbi_loadf(str(path), 3)
    assert res is not None and fx.same_bits(res[0], want) and res[3] == 3
    for chunk in (None, helpers.CB_PATTERNS[2]):
        res = ica.stbi_loadf_from_callbacks(data, 3, chunk=chunk)
        assert res is not None and fx.same_bits(res[0], want)
    # a one-byte first read: the reference's rewind after its type test loses bytes (the 8-bit loader says "no SOI")
    assert ica.stbi_load_from_callbacks(data, 3, chunk=lambda k: 1 + (k * 7) % 50) is None
    assert ica.stbi_loadf_from_callbacks(data, 3, chunk=lambda k: 1 + (k * 7) % 50) is None
    assert ica.stbi_failure_reason() == "unknown image type"
    assert ica.stbi_loadf_from_callbacks(data[:40], 3) is None
    assert ica.stbi_failure_reason() == "unknown image type"


def test_loadf_eight_threads(ica, oracle, gpu_ctx):
    datas = [ica.synth_jpeg(w, h, seed=i) for i, (w, h) in enumerate([(640, 480), (1920, 1080), (33, 17), (512, 512)] * 2)]
    wants = [_expect(oracle.load(d, 3)[1]) for d in datas]
    errors = []

    def run(i):
        for _ in range(3):
            got = ica.stbi_loadf_from_memory(datas[i], 3)
            if got is None or not fx.same_bits(got[0], wants[i]):
                errors.append(i)

    ts = [threading.Thread(target=run, args=(i,)) for i in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors


def _mixed_inputs(ica, golden):
    datas = [ica.synth_jpeg(1920, 1080, 1, 90), ica.synth_jpeg(640, 360, 2, 90), ica.synth_jpeg(333, 211, 3, 95), ica.synth_jpeg(1, 1, 4, 90),
             ica.synth_jpeg(33, 17, 5, 90), ica.synth_jpeg(1000, 700, 6, 75)]
    for name in ("b422_37x21", "b422_256x64", "b444_40x24_q95", "grey_33x20", "grey_1x1", "cmyk_40x30", "cmyk_transform2_40x30",
                 "prog_420_23x41", "big_prog_420_320x200", "b420_33x17_q50"):
        datas.append(golden.jpg(name))
    return datas


def _decode(ica, ctx, datas, req, f32=None):
    """one batch of datas; f32: {index: lut or None (stb table)} asked before submit"""
    cb = 64 << 20
    b = ica.Batch(ctx, len(datas), cb, cb, 64 << 20)
    ok, slots, reasons = b.decode_jpegs(datas, req, threads=4)
    assert ok == len(datas), reasons
    if f32:
        b.reserve_out_f32(256 << 20)
        for i, t in f32.items():
            b.set_out_f32(slots[i], t)
    b.submit()
    b.wait()
    return b, slots


def test_mixed_batch_float_slots(ica, oracle, gpu_ctx, golden):
    datas = _mixed_inputs(ica, golden)
    assert len(datas) == 16
    rng = np.random.default_rng(7)
    for req in (0, 4, 2):
        wants = [oracle.load(d, req)[1] for d in datas]
        rand_idx = 2
        rand_t = rng.random((wants[rand_idx].shape[-1], 256), dtype=np.float32) * np.float32(100) - np.float32(50)
        f32 = {i: None for i in (0, 1, 3, 4, 5, 7, 9, 10, 11, 13, 15)}
        f32[rand_idx] = rand_t
        plain, pslots = _decode(ica, gpu_ctx, datas, req)
        b, slots = _decode(ica, gpu_ctx, datas, req, f32)
        for i in range(len(datas)):
            u8 = b.fetch(slots[i])
            assert np.array_equal(u8, wants[i]), (req, i)
            assert b.hash_out(slots[i]) == plain.hash_out(pslots[i]), (req, i)
            if i in f32:
                t = rand_t if i == rand_idx else fx.lut(u8.shape[-1])
                got = b.fetch_f32(slots[i])
                assert fx.same_bits(got, fx.apply(t, u8)), (req, i)
                assert fx.same_bits(got, fx.apply(t, wants[i])), (req, i)
                assert b.device_out_f32(slots[i])
            else:
                assert b.device_out_f32(slots[i]) is None
        b.close()
        plain.close()


def test_mixed_batch_gpu_walk_front_end(ica, oracle, gpu_ctx):
    datas = [ica.synth_jpeg(1920, 1080, s, 90) for s in range(3)] + [ica.synth_jpeg(800, 600, 9, 95)]
    cb = 64 << 20
    b = ica.Batch(gpu_ctx, len(datas), cb, cb, 64 << 20)
    b.entropy_reserve(sum(len(d) for d in datas) * 2 + (1 << 20))
    ok, slots, reasons = b.decode_jpegs(datas, 3, threads=2, gpu_entropy=True)
    assert ok == len(datas), reasons
    b.reserve_out_f32(128 << 20)
    for s in slots[:3]:
        b.set_out_f32(s)
    b.submit()
    b.wait()
    for i, s in enumerate(slots):
        want = oracle.load(datas[i], 3)[1]
        assert np.array_equal(b.fetch(s), want)
        if i < 3:
            assert fx.same_bits(b.fetch_f32(s), _expect(want)), i
    b.close()


def test_batch_f32_errors(ica, gpu_ctx):
    L = ica.lib()
    L.mij_batch_set_out_f32.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mij_batch_out_f32_reserve.argtypes = [C.c_void_p, C.c_size_t]
    L.mij_batch_fetch_f32.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    lut = np.zeros(1024, dtype=np.float32)
    lp = lut.ctypes.data_as(C.c_void_p)
    dst = np.zeros(64 * 48 * 4, dtype=np.float32)
    dp = dst.ctypes.data_as(C.c_void_p)
    datas = [ica.synth_jpeg(64, 48, 1), ica.synth_jpeg(64, 48, 2)]
    b = ica.Batch(gpu_ctx, 4, 8 << 20, 8 << 20, 8 << 20)
    b.decode_jpegs(datas, 3, threads=1, gpu_entropy=False)
    h = b._h
    assert L.mij_batch_set_out_f32(h, 0, lp) == MIJ_E_ARG          # no float arena yet
    assert L.mij_batch_out_f32_reserve(h, 0) == MIJ_E_ARG
    assert L.mij_batch_out_f32_reserve(h, 1024) == 0
    assert L.mij_batch_set_out_f32(h, 0, lp) == MIJ_E_ARG          # arena too small for 64 x 48 x 3 floats
    assert L.mij_batch_out_f32_reserve(h, 1 << 20) == 0
    assert L.mij_batch_set_out_f32(h, 7, lp) == MIJ_E_ARG          # no such slot
    assert L.mij_batch_set_out_f32(h, 0, None) == MIJ_E_ARG
    assert L.mij_batch_set_out_f32(h, 0, lp) == 0
    assert L.mij_batch_out_f32_reserve(h, 4 << 20) == MIJ_E_STATE  # cannot move the arena under a request
    assert L.mij_batch_fetch_f32(h, 0, dp, dst.size) == MIJ_E_STATE  # before launch
    flags = b.slot_flags(1)
    b.set_flags(1, flags | 2)  # MIJ_FLAG_SKIP
    assert L.mij_batch_set_out_f32(h, 1, lp) == MIJ_E_STATE
    b.set_flags(1, flags)
    b.submit()
    b.wait()
    assert L.mij_batch_set_out_f32(h, 1, lp) == MIJ_E_STATE        # after upload
    assert L.mij_batch_fetch_f32(h, 1, dp, dst.size) == MIJ_E_STATE  # slot without float output
    assert L.mij_batch_fetch_f32(h, 0, dp, 10) == MIJ_E_ARG          # destination too small
    assert L.mij_batch_fetch_f32(h, 0, dp, dst.size) == 0
    assert not dst[:64 * 48 * 3].any()  # the all-zero table
    # reset forgets the request; the same slot number is a plain slot again
    b.reset()
    b.decode_jpegs(datas[:1], 3, threads=1, gpu_entropy=False)
    b.submit()
    b.wait()
    assert L.mij_batch_fetch_f32(h, 0, dp, dst.size) == MIJ_E_STATE
    assert b.device_out_f32(0) is None
    b.close()


def test_batch_f32_reserve_recovers_after_failure(ica, oracle, gpu_ctx):
    """A reserve the device cannot satisfy fails with MIJ_E_NOMEM and leaves a usable batch: float requests are refused while it has
    no arena, and the next reserve of a normal size works."""
    L = ica.lib()
    L.mij_batch_out_f32_reserve.argtypes = [C.c_void_p, C.c_size_t]
    L.mij_batch_set_out_f32.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    data = ica.synth_jpeg(64, 48, 3)
    b = ica.Batch(gpu_ctx, 2, 8 << 20, 8 << 20, 8 << 20)
    b.decode_jpegs([data], 3, threads=1, gpu_entropy=False)
    lut = np.ascontiguousarray(ica.ldr_to_hdr_lut(3))
    assert L.mij_batch_out_f32_reserve(b._h, 1 << 20) == 0
    assert L.mij_batch_out_f32_reserve(b._h, 1 << 52) == -3  # MIJ_E_NOMEM
    rc = L.mij_batch_set_out_f32(b._h, 0, lut.ctypes.data_as(C.c_void_p))
    assert rc in (0, MIJ_E_ARG)  # the old arena survives when there was room to try beside it
    if rc == MIJ_E_ARG:
        assert L.mij_batch_out_f32_reserve(b._h, 1 << 20) == 0
        b.set_out_f32(0)
    b.submit()
    b.wait()
    assert fx.same_bits(b.fetch_f32(0), _expect(oracle.load(data, 3)[1]))
    b.close()


@pytest.mark.spawns_gpu_children
def test_c_caller_runs(ica, tmp_path):
    exe = fx.build_caller(tmp_path)
    data = ica.synth_jpeg(97, 45, seed=11)
    path = tmp_path / "in.jpg"
    path.write_bytes(data)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[:4] == ["ok", "97", "45", "3"], r.stdout
    want = _expect(helpers.Oracle().load(data, 0)[1])
    assert abs(float(words[4]) - float(want.astype(np.float64).sum())) < 1e-3 * max(1.0, float(want.sum()))
