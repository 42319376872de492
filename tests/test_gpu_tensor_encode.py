"""JPEG streams from device tensors with the Huffman stage on the GPU (mij_enc_add_device, mij_enc_add_units,
mij_enc_stream_reserve / fetch_streams / stream; TensorEncoder): every stream byte for byte what the host writer gives for the
same picture -- the reference-made goldens, the benchmark pictures' stored digests, and mjw_emit over the host transform."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

import emit_model as em
import helpers

pytestmark = pytest.mark.gpu

MIJ_E_ARG, MIJ_E_STATE = -2, -5
WG = os.path.join(helpers.ROOT, "tests", "golden", "writer_golden_r3.npz")


def expect(ica, img, q, flip=False):
    plan, du = ica.host_transform(img, q, flip)
    return ica.emit_jpeg(plan, du)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def plan_for(ica, w, h, c, q):
    p = ica.binding.WritePlan()
    L = ica.lib()
    L.mjw_plan_init.argtypes = [C.POINTER(ica.binding.WritePlan), C.c_int, C.c_int, C.c_int, C.c_int]
    assert L.mjw_plan_init(C.byref(p), w, h, c, q)
    return p


def in_tensor(ica, t, layout):
    """an InTensor for a 3-D (or 2-D grey) uint8 torch view"""
    if t.dim() == 2:
        return ica.InTensor(t.data_ptr(), ica.MIJ_LAYOUT_HWC, t.shape[1], t.shape[0], 1, t.stride(0), 0)
    if layout == "CHW":
        c, h, w = t.shape
        return ica.InTensor(t.data_ptr(), ica.MIJ_LAYOUT_CHW, w, h, c, t.stride(1), t.stride(0))
    h, w, c = t.shape
    return ica.InTensor(t.data_ptr(), ica.MIJ_LAYOUT_HWC, w, h, c, t.stride(0), 0)


@pytest.fixture(scope="module")
def tenc(ica, gpu_ctx):
    e = ica.TensorEncoder()
    yield e
    e.close()


def test_small_writer_goldens_from_device_tensors(ica, golden, tenc):
    """1: the reference-made small goldens, uploaded as HWC and as CHW tensors, come back as their golden bytes"""
    for nm in golden.enc_names:
        img, q = golden[nm + "/rgb"], int(golden[nm + "/q"][0])
        want = bytes(golden[nm + "/jpg"])
        t = dev(img)
        if t.dim() == 2:
            assert tenc.encode([t], quality=q) == [want], nm
            continue
        assert tenc.encode([t], quality=q, layout="HWC") == [want], nm
        assert tenc.encode([t.permute(2, 0, 1).contiguous()], quality=q, layout="CHW") == [want], nm


@pytest.mark.parametrize("q,count", [(90, 16), (95, 4)])
def test_bench_pictures_equal_the_reference_digests(ica, tenc, q, count):
    """2: synth_rgb(1920, 1080, seed) through TensorEncoder: the length and SHA-256 the reference's writer gave"""
    wg = np.load(WG, allow_pickle=False)
    lens, shas = wg["bench/q%d/len" % q], wg["bench/q%d/sha256" % q]
    batch = dev(np.stack([ica.synth_rgb(1920, 1080, s) for s in range(count)])).permute(0, 3, 1, 2)  # [N, 3, H, W] view, strided
    got = tenc.encode(batch.contiguous(), quality=q)
    got_hwc = tenc.encode(batch.permute(0, 2, 3, 1), quality=q, layout="HWC")
    for seed in range(count):
        for g in (got[seed], got_hwc[seed]):
            assert len(g) == int(lens[seed]), (seed, len(g))
            assert hashlib.sha256(g).digest() == bytes(shas[seed]), seed


def test_seeded_pictures_equal_host_writer(ica, tenc):
    """3: 48 seeded pictures, 1x1 to 300x200 with widths at every residue around 8 and 16, comp 1-4, q in {1, 30, 75, 90, 91, 100},
    flip on and off, both layouts, as strided views cut from larger tensors"""
    rng = np.random.default_rng(2024)
    widths = [1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 300]
    qs = [1, 30, 75, 90, 91, 100]
    for i in range(48):
        w = widths[i % len(widths)] if i < 30 else int(rng.integers(1, 301))
        h = int(rng.integers(1, 201)) if i % 4 else [1, 8, 16, 17][i // 4 % 4]
        c, q, flip, layout = 1 + i % 4, qs[i % len(qs)], bool(i & 1), ("CHW", "HWC")[(i >> 1) & 1]
        base = rng.integers(0, 256, size=(h + 5, w + 7, c + 1), dtype=np.uint8)
        smooth = (np.add.outer(np.arange(h + 5), np.arange(w + 7)) * (i + 1) % 256).astype(np.uint8)
        base = np.where(rng.random(base.shape) < 0.7, smooth[:, :, None], base).astype(np.uint8)
        big = dev(base)
        if layout == "HWC":
            view = dev(base[:, :, :c])[2:2 + h, 3:3 + w, :]  # strides (row, C, 1): rows of a wider picture
            img = view.cpu().numpy()
        else:
            view = big.permute(2, 0, 1)[:c].contiguous()[:, 2:2 + h, 3:3 + w]  # planes and rows of a larger CHW tensor
            img = view.permute(1, 2, 0).cpu().numpy()
        if c == 1 and i % 8 == 0:  # a 2-D grey picture
            view, img = dev(img[:, :, 0]), img[:, :, 0]
        got = tenc.encode([view], quality=q, layout=layout, flip_vertically=flip)
        assert got == [expect(ica, img, q, flip)], (i, w, h, c, q, flip, layout)


def test_host_slots_with_gpu_emission(ica, gpu_ctx):
    """4: host-pixel slots (mij_enc_add) with GPU emission give emit_jpeg(plan, fetch(slot)); the units stay fetchable and equal the
    host transform"""
    rng = np.random.default_rng(4)
    enc = ica.Encoder(gpu_ctx, 16, 16 << 20, 16 << 20)
    enc.stream_reserve(8 << 20)
    imgs = []
    for i in range(12):
        w, h, c, q = int(rng.integers(1, 250)), int(rng.integers(1, 180)), 1 + i % 4, [50, 90, 95, 100][i % 4]
        img = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
        imgs.append((img, q, bool(i % 3 == 0)))
        enc.add(img, q, flip=i % 3 == 0)
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == len(imgs)
    for s, (img, q, flip) in enumerate(imgs):
        data, n = enc.stream(s)
        units = enc.fetch(s)
        assert np.array_equal(units, ica.host_transform(img, q, flip)[1]), s
        assert data == ica.emit_jpeg(enc.plan(s), units) and n == len(data), s
    enc.close()


def test_given_units_and_their_range_checks(ica, gpu_ctx):
    """5: add_units with the model's adversarial units gives emit_jpeg; units outside the writer's tables are refused"""
    rng = np.random.default_rng(5)
    enc = ica.Encoder(gpu_ctx, 16, 1 << 20, 64 << 20, stage_bytes=0)
    enc.stream_reserve(32 << 20)
    cases = []
    for (w, h, q) in ((64, 48, 90), (40, 24, 95), (16, 16, 30), (8, 8, 100), (300, 200, 90), (200, 96, 91)):
        p = plan_for(ica, w, h, 3, q)
        du = em.adversarial_units(rng, p.mcu_x * p.mcu_y, p.du_per_mcu)
        cases.append((enc.add_units(w, h, 3, q, du), p, du))
    ff = np.stack([em._unit(rng, "ff") for _ in range(6 * 16)])  # 0xFF-dense
    p = plan_for(ica, 64, 64, 3, 90)
    cases.append((enc.add_units(64, 64, 3, 90, ff), p, ff))
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == len(cases)
    for s, p, du in cases:
        data, _ = enc.stream(s)
        assert data == ica.emit_jpeg(p, du), s
        assert np.array_equal(enc.fetch(s), du.reshape(-1, 64)), s
    p = plan_for(ica, 16, 16, 3, 90)
    bad = np.zeros((6, 64), np.int16)
    bad[0, 0] = 2048  # DC difference 2048 from 0
    with pytest.raises(ica.MijError, match="DC"):
        enc.add_units(16, 16, 3, 90, bad)
    bad[0, 0] = 1000
    bad[4, 0] = -1000
    bad[5, 0] = 1000
    bad[1, 0] = -1048  # Y: 1000 -> -1048 = -2048
    with pytest.raises(ica.MijError, match="DC"):
        enc.add_units(16, 16, 3, 90, bad)
    bad[:] = 0
    bad[3, 17] = -1024
    with pytest.raises(ica.MijError, match="AC"):
        enc.add_units(16, 16, 3, 90, bad)
    bad[3, 17] = -1023
    s = enc.add_units(16, 16, 3, 90, bad)
    with pytest.raises(ica.MijError):
        enc.add_clone(s)  # given units have no pixels to clone
    enc.close()


def test_one_launch_mixes_every_slot_kind(ica, gpu_ctx):
    """6: device, host, clone and units slots in one launch -- over 1000 small clones and one 4096 x 4096 q=95 picture"""
    rng = np.random.default_rng(6)
    small = [rng.integers(0, 256, size=(int(rng.integers(1, 40)), int(rng.integers(1, 40)), 3), dtype=np.uint8) for _ in range(4)]
    bigimg = ica.synth_rgb(4096, 4096, 3)
    big_t = dev(bigimg).permute(2, 0, 1).contiguous()
    small_t = [dev(a) for a in small]
    enc = ica.Encoder(gpu_ctx, 1200, 128 << 20, 256 << 20)
    enc.stream_reserve(64 << 20)
    want = []
    s_big = enc.add_device(in_tensor(ica, big_t, "CHW"), 95)
    want.append((s_big, expect(ica, bigimg, 95)))
    roots = []
    for k, (a, t) in enumerate(zip(small, small_t)):
        q, flip = [90, 95, 20, 100][k], k % 2 == 1
        if k % 2:
            s = enc.add_device(in_tensor(ica, t, "HWC"), q, flip)
        else:
            s = enc.add(a, q, flip=flip)
        roots.append((s, expect(ica, a, q, flip)))
        want.append(roots[-1])
    p = plan_for(ica, 48, 32, 3, 90)
    du = em.adversarial_units(rng, p.mcu_x * p.mcu_y, p.du_per_mcu)
    want.append((enc.add_units(48, 32, 3, 90, du), ica.emit_jpeg(p, du)))
    for i in range(1100):
        s, w = roots[i % len(roots)]
        want.append((enc.add_clone(s), w))
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == len(want)
    for s, w in want:
        data, n = enc.stream(s)
        assert data == w and n == len(w), s
    enc.close()


def test_small_arena(ica, gpu_ctx, tenc):
    """7: slots past the arena report NULL with the length they need, the ones before are exact; TensorEncoder finishes the others on
    the host, says how many, and needs none on the next call"""
    rng = np.random.default_rng(7)
    imgs = [rng.integers(0, 256, size=(64, 96, 3), dtype=np.uint8) for _ in range(6)]
    want = [expect(ica, a, 90) for a in imgs]
    ts = [dev(a) for a in imgs]
    enc = ica.Encoder(gpu_ctx, 8, 8 << 20, 8 << 20, stage_bytes=0)
    enc.stream_reserve(len(want[0]) + len(want[1]) + len(want[2]) // 2)
    for t in ts:
        enc.add_device(in_tensor(ica, t, "HWC"), 90)
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == 2
    for s in range(6):
        data, n = enc.stream(s)
        assert n == len(want[s]), s
        assert (data == want[s]) if s < 2 else data is None, s
        if s >= 2:
            assert "did not fit" in ica.lib().mij_last_error().decode()
            assert ica.emit_jpeg(enc.plan(s), enc.fetch(s)) == want[s]
    enc.close()
    tenc.reserve_arena(len(want[0]) + 100)
    batch = torch.stack(ts).permute(0, 3, 1, 2).contiguous()
    assert tenc.encode(batch, quality=90) == want
    assert tenc.last_host_emitted == 5
    assert tenc.encode(batch, quality=90) == want
    assert tenc.last_host_emitted == 0


def test_encode_sees_the_torch_write_just_before_it(ica, tenc):
    """8: a torch op writes the tensor on the current stream right before encode: the streams encode the new contents"""
    g = torch.Generator(device="cuda").manual_seed(8)
    src = torch.randint(0, 256, (8, 3, 720, 1280), dtype=torch.uint8, device="cuda", generator=g)
    t = torch.zeros_like(src)
    for _ in range(2):
        x = src.float()
        for _ in range(8):
            x = (x * 1.0001).clamp_(0, 255)
        t.copy_(x.to(torch.uint8))  # queued on the current stream, not waited for
        got = tenc.encode(t, quality=75)
        host = t.permute(0, 2, 3, 1).cpu().numpy()
        assert got == [expect(ica, host[i], 75) for i in range(8)]
        src = 255 - src


def test_without_an_arena_nothing_changes(ica, gpu_ctx):
    """9: an encoder without an arena behaves as before: fetch_streams is MIJ_E_STATE, the units are fetched as ever"""
    img = ica.synth_rgb(100, 60, 1)
    enc = ica.Encoder(gpu_ctx, 2, 1 << 20, 1 << 20)
    s = enc.add(img, 90)
    enc.upload()
    enc.launch()
    L = ica.lib()
    L.mij_enc_fetch_streams.argtypes = [C.c_void_p]
    assert L.mij_enc_fetch_streams(enc._h) == MIJ_E_STATE
    assert ica.emit_jpeg(enc.plan(s), enc.fetch(s)) == expect(ica, img, 90)
    enc.stream_reserve(1 << 20)  # reserving after the upload asks for a new upload
    with pytest.raises(ica.MijError):
        enc.launch()
    enc.upload()
    assert L.mij_enc_fetch_streams(enc._h) == MIJ_E_STATE  # before launch
    enc.launch()
    assert enc.fetch_streams() == 1 and enc.stream(s)[0] == expect(ica, img, 90)
    enc.close()


def test_bad_tensors_are_refused(ica, gpu_ctx):
    """10: a host pointer, an extent past the allocation and overlapping pitches are MIJ_E_ARG"""
    enc = ica.Encoder(gpu_ctx, 8, 1 << 20, 1 << 20, stage_bytes=0)
    L = ica.lib()
    L.mij_enc_add_device.argtypes = [C.c_void_p, C.POINTER(ica.InTensor), C.c_int, C.c_int]
    paths = {ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    dp = C.c_void_p()
    assert hip.hipMalloc(C.byref(dp), 3 * 48 * 64) == 0  # exactly one CHW picture: torch's allocator would hand out a larger block
    p = dp.value
    host = np.zeros((3, 48, 64), np.uint8)

    def add(ptr, layout, w, h, c, rp, pp):
        return L.mij_enc_add_device(enc._h, C.byref(ica.InTensor(ptr, layout, w, h, c, rp, pp)), 90, 0)

    CHW, HWC = ica.MIJ_LAYOUT_CHW, ica.MIJ_LAYOUT_HWC
    t = torch.zeros((3, 48, 64), dtype=torch.uint8, device="cuda")
    assert add(p, CHW, 64, 48, 3, 64, 64 * 48) >= 0                      # ends exactly at the end of the allocation
    assert add(host.ctypes.data, CHW, 64, 48, 3, 64, 64 * 48) == MIJ_E_ARG      # host memory
    assert add(p + 1, CHW, 64, 48, 3, 64, 64 * 48) == MIJ_E_ARG                 # one byte past the allocation
    assert add(p, CHW, 64, 48, 3, 65, 65 * 48) == MIJ_E_ARG                     # rows past the allocation
    assert add(t.data_ptr(), CHW, 64, 48, 3, 63, 64 * 48) == MIJ_E_ARG         # CHW rows overlap
    assert add(t.data_ptr(), CHW, 64, 48, 3, 64, 64 * 47) == MIJ_E_ARG         # CHW planes overlap
    assert add(t.data_ptr(), HWC, 32, 48, 3, 32 * 3 - 1, 0) == MIJ_E_ARG       # HWC rows overlap
    assert add(t.data_ptr(), HWC, 32, 48, 3, 32 * 3, 0) >= 0
    assert add(t.data_ptr(), 7, 32, 48, 3, 32 * 3, 0) == MIJ_E_ARG             # unknown layout
    assert add(t.data_ptr(), HWC, 32, 48, 5, 32 * 5, 0) == MIJ_E_ARG           # comp the writer refuses
    assert add(0, HWC, 32, 48, 3, 32 * 3, 0) == MIJ_E_ARG
    enc.close()
    assert hip.hipFree(dp) == 0
