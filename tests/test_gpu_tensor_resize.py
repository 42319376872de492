"""Resized tensor output on the GPU (k_out_resize through mij_batch_set_out_tensor_resized and TensorDecoder.decode(size=...)), bit for
bit against resize_model applied to the reference's pixels (golden vectors or the oracle): every filter, dtype, layout, channel count
and flip, down and up; 1080p to 224 x 224 and random-resized crops; identity sizes; extreme ratios; guard bytes; mixed pictures; plain
and resized requests in one batch; rejected pictures, reset and every new refusal of the C-ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

import resize_model as rm
import tensor_model as tm

pytestmark = pytest.mark.gpu

MIJ_E_ARG, MIJ_E_STATE = -2, -5
DTYPES = (torch.uint8, torch.float16, torch.bfloat16, torch.float32)
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
SENTINEL = 0xA5


def _norm(dtype, n):
    return (None, None) if dtype == torch.uint8 else (MEAN[:n], STD[:n])


@pytest.fixture(scope="module")
def dec(ica, gpu_ctx):
    d = ica.TensorDecoder("cuda:0")
    yield d
    d.close()


def _check(got, pxs, wins, size, name, fxs, fys, layout, dtype, mean=None, std=None):
    n = pxs[0].shape[-1] if pxs[0].ndim == 3 else 1
    t = None if dtype == torch.uint8 else tm.tables(n, dtype, mean, std)
    cache = {}
    for i, px in enumerate(pxs):
        key = (id(px), wins[i], fxs[i], fys[i])
        if key not in cache:
            cache[key] = rm.window(px, wins[i], size, name, fxs[i], fys[i], layout, t, dtype)
        assert tm.same_bits(got[i], cache[key]), (i, wins[i], size, name, fxs[i], fys[i], layout, dtype)


def test_filters_dtypes_layouts_channels_flips(ica, oracle, golden, dec):
    """every filter x dtype x layout x req_comp 0..4 x the four flip combinations, on odd windows of a colour and a grey file, down
    (27 x 15 -> 11 x 7) and up (-> 40 x 23)"""
    flips = [(False, False), (True, False), (False, True), (True, True)]
    fx, fy = [f[0] for f in flips], [f[1] for f in flips]
    win = (3, 1, 27, 15)
    for data in (ica.synth_jpeg(33, 17, seed=3, quality=90), golden.jpg("grey_33x20")):
        for req in range(5):
            px = oracle.load(data, req)[1]
            for k, name in enumerate(rm.FILTERS):
                for size in ((7, 11), (23, 40)):
                    for dtype in DTYPES:
                        mean, std = _norm(dtype, px.shape[-1])
                        layout = ("CHW", "HWC")[(k + DTYPES.index(dtype) + req) % 2]
                        got, reasons = dec.decode([data] * 4, req_comp=req, crops=[win] * 4, flip_x=fx, flip_y=fy, layout=layout, dtype=dtype,
                                                  mean=mean, std=std, size=size, filter=name)
                        assert reasons == [None] * 4
                        C_ = px.shape[-1]
                        shape = (4, C_) + size if layout == "CHW" else (4,) + size + (C_,)
                        assert tuple(got.shape) == shape and got.dtype == dtype
                        _check(got, [px] * 4, [win] * 4, size, name, fx, fy, layout, dtype, mean, std)


def test_1080p_whole_and_random_resized_crops(ica, oracle, dec):
    """whole 1080p pictures -> 224 x 224 (f16 CHW normalised), and 300 seeded random-resized crops of 1080p pictures -> 224 x 224 with
    random flips in one bf16 batch"""
    srcs = [ica.synth_jpeg(1920, 1080, seed=s, quality=90) for s in range(3)]
    pxs = [oracle.load(d, 3)[1] for d in srcs]
    got, reasons = dec.decode(srcs, size=(224, 224), dtype=torch.float16, mean=MEAN[:3], std=STD[:3])
    assert reasons == [None] * 3
    _check(got, pxs, [(0, 0, 1920, 1080)] * 3, (224, 224), "bilinear", [False] * 3, [False] * 3, "CHW", torch.float16, MEAN[:3], STD[:3])
    rng = np.random.default_rng(17)
    pick = rng.integers(0, 3, 300)
    crops = []
    for _ in range(300):  # RandomResizedCrop's sampler: scale 0.08..1 of the area, ratio 3/4..4/3 (log-uniform)
        while True:
            area = 1920 * 1080 * rng.uniform(0.08, 1.0)
            ratio = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
            w, h = int(round(np.sqrt(area * ratio))), int(round(np.sqrt(area / ratio)))
            if 0 < w <= 1920 and 0 < h <= 1080:
                break
        crops.append((int(rng.integers(0, 1920 - w + 1)), int(rng.integers(0, 1080 - h + 1)), w, h))
    fx, fy = [bool(v) for v in rng.integers(0, 2, 300)], [bool(v) for v in rng.integers(0, 2, 300)]
    got, reasons = dec.decode([srcs[k] for k in pick], crops=crops, flip_x=fx, flip_y=fy, dtype=torch.bfloat16, mean=MEAN[:3], std=STD[:3],
                              size=(224, 224))
    assert reasons == [None] * 300
    _check(got, [pxs[k] for k in pick], crops, (224, 224), "bilinear", fx, fy, "CHW", torch.bfloat16, MEAN[:3], STD[:3])


def test_identity_size_equals_plain_request(ica, dec):
    data = ica.synth_jpeg(203, 97, seed=12, quality=92)
    win = (5, 3, 131, 61)
    for name in rm.FILTERS:
        for dtype, layout in ((torch.uint8, "HWC"), (torch.float16, "CHW")):
            mean, std = _norm(dtype, 3)
            plain, _ = dec.decode([data, data], crops=[win] * 2, flip_x=[False, True], flip_y=[True, False], layout=layout, dtype=dtype, mean=mean,
                                  std=std)
            rsz, _ = dec.decode([data, data], crops=[win] * 2, flip_x=[False, True], flip_y=[True, False], layout=layout, dtype=dtype, mean=mean,
                                std=std, size=(61, 131), filter=name)
            assert tm.same_bits(plain, rsz), (name, dtype)


def test_extreme_ratios(ica, oracle, dec):
    """a 1 x 1 window up to 512 x 512, a full-width strip down to 1 x 1, and an 8192-wide window, down and up"""
    data = ica.synth_jpeg(640, 480, seed=5, quality=90)
    px = oracle.load(data, 3)[1]
    for name in ("bilinear", "lanczos"):
        for win, size in (((17, 9, 1, 1), (512, 512)), ((0, 200, 640, 4), (1, 1)), ((0, 0, 640, 480), (1, 1)), ((0, 7, 640, 1), (3, 1000))):
            got, reasons = dec.decode([data], crops=[win], size=size, filter=name, dtype=torch.uint8, layout="HWC")
            assert reasons == [None]
            _check(got, [px], [win], size, name, [False], [False], "HWC", torch.uint8)
    wide = ica.synth_jpeg(8192, 24, seed=6, quality=90)
    px = oracle.load(wide, 3)[1]
    for name, size in (("lanczos", (1, 1)), ("bicubic", (5, 37)), ("box", (24, 8192)), ("hamming", (48, 9000))):
        got, reasons = dec.decode([wide], size=size, filter=name, dtype=torch.float32, flip_x=True)
        assert reasons == [None]
        _check(got, [px], [(0, 0, 8192, 24)], size, name, [True], [False], "CHW", torch.float32)


def _guarded(ica, oracle, gpu_ctx, data, req, r):
    """r: (dtype, layout, offset_elems, win, size, row_pitch, plane_pitch, fx, fy, filter) into a sentinel-filled buffer; every byte is
    compared with the model: the written elements and the untouched rest"""
    dtype, layout, off, win, size, rp, pp, fx, fy, name = r
    px = oracle.load(data, req)[1]
    n = px.shape[-1]
    b = ica.Batch(gpu_ctx, 1, 8 << 20, 8 << 20, 8 << 20)
    ok, slots, why = b.decode_jpegs([data], req, threads=1)
    assert ok == 1, why
    es = tm.ESIZE[dtype]
    oh, ow = size
    last = (oh - 1) * rp + ((n - 1) * pp + ow - 1 if layout == "CHW" else ow * n - 1)
    buf = torch.full(((off + last + 1) * es + 64,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    t = tm.tables(n, dtype, *_norm(dtype, n)) if dtype != torch.uint8 else None
    tb = None if t is None else t.view(tm.BITS[dtype]).numpy()
    b.set_out_tensor_resized(slots[0], buf.data_ptr() + off * es, tm.CODE[dtype], layout, *win, ow, oh, rp, pp, fx, fy, tb, name)
    torch.cuda.synchronize()
    b.submit()
    b.wait()
    want = torch.full((buf.numel(),), SENTINEL, dtype=torch.uint8)
    vals = rm.window(px, win, size, name, fx, fy, layout, t, dtype).view(tm.BITS[dtype]).contiguous().view(torch.uint8).view(-1, es)
    if layout == "CHW":
        c, y, x = torch.meshgrid(torch.arange(n), torch.arange(oh), torch.arange(ow), indexing="ij")
        el = off + c * pp + y * rp + x
    else:
        y, x, c = torch.meshgrid(torch.arange(oh), torch.arange(ow), torch.arange(n), indexing="ij")
        el = off + y * rp + x * n + c
    idx = (el.reshape(-1, 1) * es + torch.arange(es)).reshape(-1)
    want[idx] = vals.reshape(-1)
    got = buf.cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (r, bad[:8].tolist())
    b.close()


def test_guard_bytes_unaligned_padded(ica, oracle, gpu_ctx):
    data = ica.synth_jpeg(203, 97, seed=12, quality=92)
    for req in (3, 1, 4):
        for k, dtype in enumerate(DTYPES):
            es = tm.ESIZE[dtype]
            for layout in ("HWC", "CHW"):
                win = (17 + k, 5, 61 + 2 * k, 23) if layout == "HWC" else (2 * k + 1, 9, 129, 31 - k)
                size = (37 - k, 45 + 3 * k) if layout == "HWC" else (13, 200 + k)
                oh, ow = size
                rp = (ow * req if layout == "HWC" else ow) + 3 + 2 * k
                pp = (oh - 1) * rp + ow + 5 if layout == "CHW" else 0
                off = (1, 3, 5, 7, 9, 11, 13, 15)[(k * 2 + (layout == "CHW")) % 8] % (16 // es) or 1
                _guarded(ica, oracle, gpu_ctx, data, req, (dtype, layout, off, win, size, rp, pp, bool(k & 1), layout == "CHW", rm.FILTERS[k]))
    big = ica.synth_jpeg(1920, 1080, seed=4)
    _guarded(ica, oracle, gpu_ctx, big, 3, (torch.float16, "CHW", 3, (0, 0, 1920, 1080), (224, 224), 231, 231 * 224 + 7, True, False, "bilinear"))


@pytest.mark.parametrize("name", ["b422_37x21", "cmyk_40x30", "prog_420_23x41", "grey_1x1", "big_prog_420_320x200"])
def test_mixed_sizes_and_families(ica, oracle, golden, dec, name):
    """golden 4:2:2, CMYK, progressive and grey pictures next to a synthetic one of another size, whole pictures resized into one
    tensor"""
    data = golden.jpg(name)
    other = ica.synth_jpeg(61, 45, seed=9, quality=90)
    for req in (3, 4, 1):
        kind, px = golden.expect(name, req)
        if kind != "ok":
            continue
        po = oracle.load(other, req)[1]
        H, W = px.shape[:2]
        for size, filt in (((19, 23), "bicubic"), ((50, 70), "lanczos")):
            got, reasons = dec.decode([data, other, data], req_comp=req, size=size, filter=filt, dtype=torch.float32, mean=MEAN[:req], std=STD[:req],
                                      flip_x=[False, True, True])
            assert reasons == [None] * 3
            _check(got, [px, po, px], [(0, 0, W, H), (0, 0, 61, 45), (0, 0, W, H)], size, filt, [False, True, True], [False] * 3, "CHW",
                   torch.float32, MEAN[:req], STD[:req])


def test_plain_and_resized_in_one_batch(ica, oracle, gpu_ctx):
    datas = [ica.synth_jpeg(301, 77, seed=21), ica.synth_jpeg(120, 200, seed=22), ica.synth_jpeg(64, 48, seed=23)]
    pxs = [oracle.load(d, 3)[1] for d in datas]
    b = ica.Batch(gpu_ctx, 4, 8 << 20, 8 << 20, 8 << 20)
    ok, slots, _ = b.decode_jpegs(datas, 3, threads=1)
    assert ok == 3
    plain = torch.full((3, 40, 50), -1.0, dtype=torch.float32, device="cuda:0")
    r1 = torch.full((3, 32, 32), -1.0, dtype=torch.float32, device="cuda:0")
    r2 = torch.full((32, 32, 3), 7, dtype=torch.uint8, device="cuda:0")
    t = tm.tables(3, torch.float32, MEAN[:3], STD[:3])
    b.set_out_tensor(slots[0], plain.data_ptr(), 3, "CHW", 10, 20, 50, 40, 50, 2000, False, True, t.numpy())
    b.set_out_tensor_resized(slots[1], r1.data_ptr(), 3, "CHW", 0, 0, 120, 200, 32, 32, 32, 1024, True, False, t.numpy(), "hamming")
    b.set_out_tensor_resized(slots[2], r2.data_ptr(), 0, "HWC", 3, 2, 50, 40, 32, 32, 96, 0, False, False, None, "box")
    torch.cuda.synchronize()
    b.submit()
    b.wait()
    assert tm.same_bits(plain, tm.window(pxs[0], (10, 20, 50, 40), False, True, "CHW", t, torch.float32))
    assert tm.same_bits(r1, rm.window(pxs[1], (0, 0, 120, 200), (32, 32), "hamming", True, False, "CHW", t, torch.float32))
    assert tm.same_bits(r2, rm.window(pxs[2], (3, 2, 50, 40), (32, 32), "box", False, False, "HWC"))
    assert np.array_equal(b.fetch(slots[0]), pxs[0])
    b.close()


def test_rejected_picture_keeps_its_slice(ica, oracle, golden, dec):
    good = [ica.synth_jpeg(640, 480, seed=s) for s in range(2)] + [ica.synth_jpeg(333, 211, seed=7)]
    datas = good[:2] + [golden.jpg("trunc_noeoi"), golden.jpg("garbage"), good[2]]
    out = torch.full((5, 3, 30, 40), 3.5, dtype=torch.float32, device="cuda:0")
    got, reasons = dec.decode(datas, size=(30, 40), filter="bicubic", dtype=torch.float32, out=out)
    assert reasons[2] == "expected marker" and reasons[3] == "unknown image type"
    assert reasons[:2] == [None, None] and reasons[4] is None
    assert bool((got[2:4] == 3.5).all())
    pxs = [oracle.load(d, 3)[1] for d in good]
    wins = [(0, 0, 640, 480)] * 2 + [(0, 0, 333, 211)]
    _check(got[[0, 1, 4]], pxs, wins, (30, 40), "bicubic", [False] * 3, [False] * 3, "CHW", torch.float32)


def test_reset_and_refusals(ica, gpu_ctx):
    L = ica.lib()
    L.mij_batch_set_out_tensor_resized.argtypes = [C.c_void_p, C.c_int, C.POINTER(ica.OutTensor), C.POINTER(ica.OutResize), C.c_void_p]
    data = ica.synth_jpeg(64, 48, 1)
    b = ica.Batch(gpu_ctx, 2, 8 << 20, 8 << 20, 8 << 20)
    b.decode_jpegs([data, data], 3, threads=1, gpu_entropy=False)
    buf = torch.full((32 * 32 * 3 + 64,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()

    def req(out_w=32, out_h=32, filt=1, reserved=0, rp=32 * 3, w=64, h=48, slot=0, resize=True):
        t = ica.OutTensor(C.c_void_p(p), 0, 0, 0, 0, w, h, 0, 0, rp, 0)
        r = ica.OutResize(out_w, out_h, filt, reserved)
        return L.mij_batch_set_out_tensor_resized(b._h, slot, C.byref(t), C.byref(r) if resize else None, None)

    assert req(filt=5) == MIJ_E_ARG and req(filt=-1) == MIJ_E_ARG       # unknown filter
    assert req(out_w=0) == MIJ_E_ARG and req(out_h=0) == MIJ_E_ARG
    assert req(out_w=16385) == MIJ_E_ARG and req(out_h=16385) == MIJ_E_ARG
    assert req(reserved=1) == MIJ_E_ARG
    assert req(resize=False) == MIJ_E_ARG                              # no mij_out_resize
    assert req(w=65) == MIJ_E_ARG                                      # the source window leaves the picture
    assert req(rp=32 * 3 - 1) == MIJ_E_ARG                             # pitches apply to the resized extent
    assert req(out_w=33) == MIJ_E_ARG                                  # (32 * 3 per row is too short for 33 pixels)
    flags = b.slot_flags(1)
    b.set_flags(1, flags | 2)  # MIJ_FLAG_SKIP
    assert req(slot=1) == MIJ_E_STATE
    b.set_flags(1, flags)
    assert req(rp=32 * 3) == 0
    b.submit()
    b.wait()
    assert req(slot=1) == MIJ_E_STATE                                  # after upload
    px = b.fetch(0)
    assert tm.same_bits(buf[:32 * 32 * 3].view(32, 32, 3), rm.window(px, (0, 0, 64, 48), (32, 32), "bilinear", layout="HWC"))
    assert bool((buf[32 * 32 * 3:] == SENTINEL).all())
    # reset forgets the request: the next launch leaves buf untouched
    buf.fill_(SENTINEL)
    torch.cuda.synchronize()
    b.reset()
    b.decode_jpegs([data], 3, threads=1)
    b.submit()
    b.wait()
    assert bool((buf == SENTINEL).all())
    b.close()
