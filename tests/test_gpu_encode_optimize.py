"""Optimised Huffman tables built and used on the GPU (mij_enc_set_optimize / mij_enc_slot_optimized, k_emit_hist and k_emit_build in
csrc/mij_emit_kernels.h; TensorEncoder.encode(optimize=True)): every optimised stream byte for byte what mjw_emit_optimized writes
for the same data units on the host, every plain stream still mjw_emit's."""
import ctypes as C

import numpy as np
import pytest
import torch

import deep_units
import emit_model as em
import hufopt_model as hm

pytestmark = pytest.mark.gpu

MIJ_E_ARG, MIJ_E_STATE = -2, -5
ARENA = 16 << 20


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def plan_for(ica, w, h, c, q):
    p = ica.binding.WritePlan()
    L = ica.lib()
    L.mjw_plan_init.argtypes = [C.POINTER(ica.binding.WritePlan), C.c_int, C.c_int, C.c_int, C.c_int]
    assert L.mjw_plan_init(C.byref(p), w, h, c, q)
    return p


def in_tensor(ica, t):
    """an InTensor for an HWC (or 2-D grey) uint8 torch tensor"""
    if t.dim() == 2:
        return ica.InTensor(t.data_ptr(), ica.MIJ_LAYOUT_HWC, t.shape[1], t.shape[0], 1, t.stride(0), 0)
    h, w, c = t.shape
    return ica.InTensor(t.data_ptr(), ica.MIJ_LAYOUT_HWC, w, h, c, t.stride(0), 0)


def expect(ica, img, q, optimize, flip=False):
    plan, du = ica.host_transform(img, q, flip)
    return ica.emit_jpeg(plan, du, optimize)


def pictures():
    """the smallest pictures at which each piece can go wrong (HWC; one 2-D grey, one RGBA)"""
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:9, 0:17]
    return [
        rng.integers(0, 256, (1, 1, 3), dtype=np.uint8),
        rng.integers(0, 256, (8, 8, 3), dtype=np.uint8),
        rng.integers(0, 256, (16, 16, 3), dtype=np.uint8),
        np.stack([xx * 15, yy * 28, xx + yy], axis=2).astype(np.uint8),  # 17 x 9
        np.full((64, 64, 3), 128, np.uint8),                             # flat: one symbol per chroma table, 1-bit codes
        rng.integers(0, 256, (120, 200, 3), dtype=np.uint8),             # five tiles at 4:2:0: the histogram spans tiles
        rng.integers(0, 256, (8, 344, 3), dtype=np.uint8),               # quality 95: 129 units, a full tile and a tile of one unit
        rng.integers(0, 256, (31, 33), dtype=np.uint8),                  # 2-D grey
        rng.integers(0, 256, (20, 24, 4), dtype=np.uint8),               # RGBA
    ]


_cache = {}


def optimised_streams(ica, q):
    """TensorEncoder.encode(optimize=True) of pictures() in ONE call, computed once per quality and shared"""
    if q not in _cache:
        enc = ica.TensorEncoder()
        try:
            _cache[q] = enc.encode([dev(a) for a in pictures()], quality=q, layout="HWC", optimize=True), enc.last_host_emitted
        finally:
            enc.close()
    return _cache[q]


@pytest.mark.parametrize("q", [90, 95])
def test_tensor_encoder_equals_host_optimised_emission(ica, gpu_ctx, q):
    """1: one encode(optimize=True) call over every picture == mjw_emit_optimized of the host transform; the plain call is unchanged"""
    got, host = optimised_streams(ica, q)
    assert host == 0
    pics = pictures()
    assert len(got) == len(pics)
    for i, a in enumerate(pics):
        want = expect(ica, a, q, True)
        assert want != expect(ica, a, q, False), i
        assert got[i] == want, (i, a.shape, len(got[i]), len(want))
    t = hm.tables_from_header(got[4][:got[4].index(b"\xff\xda") + 14])
    assert t[1] == {0: (0, 1)} and t[3] == {0: (0, 1)}
    if q == 95:
        assert plan_for(ica, 344, 8, 3, q).du_elems() == 129 * 64
    enc = ica.TensorEncoder()
    plain = enc.encode([dev(a) for a in pics], quality=q, layout="HWC")
    enc.close()
    assert plain == [expect(ica, a, q, False) for a in pics]


def test_one_launch_mixes_plain_and_optimised_slots_of_every_kind(ica, gpu_ctx):
    """2: host pixels, device pixels, given units and clones, each plain and optimised, in one launch: plain slots are mjw_emit's
    bytes, optimised slots mjw_emit_optimized's, slot_optimized says which; the request is refused after the upload and forgotten
    by reset"""
    rng = np.random.default_rng(2)
    enc = ica.Encoder(gpu_ctx, 32, 8 << 20, 8 << 20)
    enc.stream_reserve(ARENA)
    want = []  # (slot, bytes, optimised)
    keep = []
    for i, (w, h, c, q) in enumerate([(50, 37, 3, 90), (23, 40, 1, 95), (64, 24, 4, 75), (200, 90, 3, 100)]):
        a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        flip = bool(i & 1)
        for opt in (False, True):
            s = enc.add(a, q, flip=flip)
            t = dev(a)
            keep.append(t)
            d = enc.add_device(in_tensor(ica, t), q, flip)
            for slot in (s, d):
                if opt:
                    enc.set_optimize(slot)
                want.append((slot, expect(ica, a, q, opt, flip), opt))
            cl = enc.add_clone(s if i & 1 else d)  # a clone inherits the request of the slot it is made from
            want.append((cl, expect(ica, a, q, opt, flip), opt))
            if opt and i == 0:  # and can drop it again
                cl2 = enc.add_clone(cl)
                enc.set_optimize(cl2, False)
                want.append((cl2, expect(ica, a, q, False, flip), False))
    for q in (90, 95):
        p = plan_for(ica, 48, 32, 3, q)
        du = em.adversarial_units(rng, p.mcu_x * p.mcu_y, p.du_per_mcu)
        want.append((enc.add_units(48, 32, 3, q, du), ica.emit_jpeg(p, du), False))
        s = enc.add_units(48, 32, 3, q, du)
        enc.set_optimize(s)
        want.append((s, ica.emit_jpeg(p, du, True), True))
    L = ica.lib()
    L.mij_enc_set_optimize.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.mij_enc_slot_optimized.argtypes = [C.c_void_p, C.c_int]
    assert L.mij_enc_set_optimize(enc._h, len(want), 1) == MIJ_E_ARG
    enc.upload()
    assert L.mij_enc_set_optimize(enc._h, 0, 1) == MIJ_E_STATE
    enc.launch()
    assert L.mij_enc_slot_optimized(enc._h, 0) == MIJ_E_STATE  # before fetch_streams
    assert enc.fetch_streams() == len(want)
    for slot, w, opt in want:
        data, n = enc.stream(slot)
        assert data == w and n == len(w), (slot, opt)
        assert enc.slot_optimized(slot) == opt, slot
    # reset forgets the requests: the same slots again, nothing asked
    enc.reset()
    a = rng.integers(0, 256, (30, 30, 3), dtype=np.uint8)
    s = enc.add(a, 90)
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == 1 and enc.stream(s)[0] == expect(ica, a, 90, False) and not enc.slot_optimized(s)
    enc.close()


def test_given_units(ica, gpu_ctx):
    """3: given units with optimisation: the model's adversarial units (zero runs of 15-48, coefficient 63 set, all-zero units, DC
    +-2047, AC +-1023) at 4:2:0 and 4:4:4 across several tiles; a luma AC chain of unlimited depth 20, so that K.3's shortening runs on
    the device; and one of depth 33, which falls back: slot_optimized 0 and mjw_emit's bytes"""
    rng = np.random.default_rng(3)
    cases = []
    for (w, h, q) in ((64, 48, 90), (40, 24, 95), (16, 16, 30), (8, 8, 100), (300, 200, 90), (200, 96, 91)):
        p = plan_for(ica, w, h, 3, q)
        cases.append((p, em.adversarial_units(rng, p.mcu_x * p.mcu_y, p.du_per_mcu), True, q))
    p20, du20 = deep_units.deep_chain_units(ica, 20)
    assert hm.unlimited_depth(hm.histogram(du20, 6)[2]) == 20
    cases.append((p20, du20, True, 90))
    p33, du33 = deep_units.deep_chain_units(ica, 33)
    assert hm.unlimited_depth(ica.write_histogram(p33, du33)[2]) == 33
    cases.append((p33, du33, False, 90))
    enc = ica.Encoder(gpu_ctx, 16, 1 << 20, sum(du.size * 2 + 512 for _, du, _, _ in cases), stage_bytes=0)
    enc.stream_reserve(64 << 20)
    slots = []
    for p, du, _, q in cases:
        s = enc.add_units(p.width, p.height, 3, q, du)
        enc.set_optimize(s)
        slots.append(s)
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == len(cases)
    for s, (p, du, opt, _) in zip(slots, cases):
        data, _ = enc.stream(s)
        want = ica.emit_jpeg(p, du, True)
        assert (want != ica.emit_jpeg(p, du)) == opt, s
        assert data == want, (s, len(data), len(want))
        assert enc.slot_optimized(s) == opt, s
    enc.close()


def test_small_arena(ica, gpu_ctx):
    """4: optimised slots past the arena report the exact optimised length and are not written; TensorEncoder returns the same bytes
    as with a large arena and says how many it finished on the host"""
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, size=(64, 96, 3), dtype=np.uint8) for _ in range(6)]
    want = [expect(ica, a, 90, True) for a in imgs]
    ts = [dev(a) for a in imgs]
    enc = ica.Encoder(gpu_ctx, 8, 8 << 20, 8 << 20, stage_bytes=0)
    enc.stream_reserve(len(want[0]) + len(want[1]) + len(want[2]) // 2)
    for t in ts:
        enc.set_optimize(enc.add_device(in_tensor(ica, t), 90))
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == 2
    for s in range(6):
        data, n = enc.stream(s)
        assert n == len(want[s]), s
        assert (data == want[s]) if s < 2 else data is None, s
        assert enc.slot_optimized(s), s
        if s >= 2:
            assert ica.emit_jpeg(enc.plan(s), enc.fetch(s), True) == want[s]
    enc.close()
    tenc = ica.TensorEncoder()
    tenc.reserve_arena(len(want[0]) + 100)
    batch = torch.stack(ts)
    assert tenc.encode(batch, quality=90, layout="HWC", optimize=True) == want
    assert tenc.last_host_emitted == 5
    assert tenc.encode(batch, quality=90, layout="HWC", optimize=True) == want
    assert tenc.last_host_emitted == 0
    tenc.close()


@pytest.mark.parametrize("gpu_walk", [True, False])
def test_round_trip_through_the_decoder(ica, oracle, gpu_ctx, gpu_walk):
    """5: the optimised streams of test 1 through Batch.decode_jpegs, with the GPU walk and with the host walk: the pixels of the plain
    streams under the oracle"""
    for q in (90, 95):
        got, _ = optimised_streams(ica, q)
        pics = pictures()
        b = ica.Batch(gpu_ctx, len(got), ARENA, ARENA, ARENA)
        if gpu_walk:
            b.entropy_reserve(8 << 20)
        ok, slots, reasons = b.decode_jpegs(got, 3, threads=2, gpu_entropy=gpu_walk)
        assert ok == len(got), reasons
        b.submit()
        b.wait()
        for i, (s, a) in enumerate(zip(slots, pics)):
            verdict, want, _ = oracle.load(expect(ica, a, q, False), 3)
            assert verdict == "ok" and np.array_equal(b.fetch(s), want), (q, i)
        b.close()


def test_launch_without_optimised_slots(ica, gpu_ctx):
    """6: with no request the launch writes the plain bytes and reports slot_optimized == 0 everywhere"""
    pics = pictures()
    enc = ica.Encoder(gpu_ctx, 16, 8 << 20, 8 << 20)
    enc.stream_reserve(ARENA)
    slots = [enc.add(a if a.ndim == 3 else a[:, :, None], 90) for a in pics]
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == len(pics)
    for s, a in zip(slots, pics):
        assert enc.stream(s)[0] == expect(ica, a, 90, False), s
        assert enc.slot_optimized(s) is False, s
    enc.close()


def test_write_jpg_calls_take_the_request(ica, gpu_ctx):
    """mij_write_jpg_to_memory and mij_write_jpg_batch with optimize=True (the _ex calls with MJW_OPTIMIZE_HUFFMAN) finish their
    streams with mjw_emit_optimized; without it they are unchanged; unknown flags are refused"""
    pics = [a for a in pictures() if a.ndim == 3]
    for q in (90, 95):
        want = [expect(ica, a, q, True) for a in pics]
        assert ica.mij_write_jpg_batch(pics, q, threads=4, optimize=True) == want
        assert ica.mij_write_jpg_batch(pics, q, threads=4) == [expect(ica, a, q, False) for a in pics]
        assert ica.mij_write_jpg_to_memory(pics[5], q, optimize=True) == want[5]
        assert ica.mij_write_jpg_to_memory(pics[5], q) == expect(ica, pics[5], q, False)
    L = ica.lib()
    cb = ica.binding._WRITE_CB(lambda _c, data, size: None)
    a = pics[1]
    L.mij_write_jpg_to_func_ex.argtypes = [ica.binding._WRITE_CB, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_uint]
    assert L.mij_write_jpg_to_func_ex(cb, None, 8, 8, 3, a.ctypes.data_as(C.c_void_p), 90, 2) == 0
