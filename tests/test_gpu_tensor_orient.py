"""Oriented tensor output on the GPU (mij_batch_set_out_tensor_oriented, k_out_tensor_t / k_out_resize_t for orientations 5..8, the
existing passes with mirrored windows and coefficients for 2..4, and TensorDecoder.decode(orientation=...)), bit for bit against
tensor_model / resize_model applied to orient_model's displayed picture of the reference's pixels (golden vectors or the oracle)."""
import ctypes as C

import numpy as np
import pytest
import torch

import exif_build as eb
import orient_model as om
import resize_model as rm
import tensor_model as tm

pytestmark = pytest.mark.gpu

MIJ_E_ARG, MIJ_E_STATE = -2, -5
DTYPES = (torch.uint8, torch.float16, torch.bfloat16, torch.float32)
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
SENTINEL = 0xA5
FLIPS = [(False, False), (True, False), (False, True), (True, True)]


def _norm(dtype, n):
    return (None, None) if dtype == torch.uint8 else (MEAN[:n], STD[:n])


def _want(px, o, win, size, name, fx, fy, layout, dtype, mean=None, std=None):
    d = om.orient(px, o)
    n = d.shape[-1] if d.ndim == 3 else 1
    t = None if dtype == torch.uint8 else tm.tables(n, dtype, mean, std)
    if size is None:
        return tm.window(d, win, fx, fy, layout, t, dtype)
    return rm.window(d, win, size, name, fx, fy, layout, t, dtype)


@pytest.fixture(scope="module")
def dec(ica, gpu_ctx):
    d = ica.TensorDecoder("cuda:0")
    yield d
    d.close()


def test_every_orientation_dtype_layout_channels_flips(ica, oracle, golden, dec):
    """o 1..8 x dtype x layout x req_comp 0..4 x the four flips, on odd windows of a colour and a grey file, plain and resized
    (down and up, the filter cycling)"""
    fx, fy = [f[0] for f in FLIPS], [f[1] for f in FLIPS]
    for data in (ica.synth_jpeg(33, 17, seed=3, quality=90), golden.jpg("grey_33x20")):
        for req in range(5):
            px = oracle.load(data, req)[1]
            H, W = px.shape[:2]
            for o in range(1, 9):
                dw, dh = om.displayed_size(W, H, o)
                win = (1, 2, dw - 4, dh - 3)
                for k, dtype in enumerate(DTYPES):
                    mean, std = _norm(dtype, px.shape[-1] if px.ndim == 3 else 1)
                    layout = ("CHW", "HWC")[(k + o + req) % 2]
                    name = rm.FILTERS[(k + o) % len(rm.FILTERS)]
                    for size in (None, (7, 11), (23, 40)):
                        got, reasons = dec.decode([data] * 4, req_comp=req, crops=[win] * 4, flip_x=fx, flip_y=fy, layout=layout, dtype=dtype,
                                                  mean=mean, std=std, size=size, filter=name, orientation=o)
                        assert reasons == [None] * 4
                        for i in range(4):
                            want = _want(px, o, win, size, name, fx[i], fy[i], layout, dtype, mean, std)
                            assert tm.same_bits(got[i], want), (o, req, dtype, layout, size, name, FLIPS[i])


@pytest.mark.parametrize("name", rm.FILTERS)
def test_every_filter_down_and_up(ica, oracle, dec, name):
    data = ica.synth_jpeg(61, 43, seed=8, quality=92)
    px = oracle.load(data, 3)[1]
    for o in range(2, 9):
        dw, dh = om.displayed_size(61, 43, o)
        for size in ((13, 19), (50, 71), (dh, 9), (5, dw)):
            win = (2, 1, dw - 3, dh - 2)
            got, reasons = dec.decode([data, data], crops=[win] * 2, flip_x=[False, True], flip_y=[True, False], size=size, filter=name,
                                      dtype=torch.float32, mean=MEAN[:3], std=STD[:3], orientation=o)
            assert reasons == [None] * 2
            for i, (fx, fy) in enumerate(((False, True), (True, False))):
                assert tm.same_bits(got[i], _want(px, o, win, size, name, fx, fy, "CHW", torch.float32, MEAN[:3], STD[:3])), (o, size)


def test_mirror_comes_before_the_resize(ica, oracle, dec):
    """box 12 -> 8 (scale 1.5: every even output's bounds fall on a half) differs mirrored first and mirrored last; the GPU mirrors
    first, for every orientation that mirrors the resized axis"""
    for (W, H), size, cases in (((12, 5), (5, 8), (2, 3)), ((5, 12), (8, 5), (3, 4)), ((5, 12), (5, 8), (6, 7)), ((12, 5), (8, 5), (7, 8))):
        data = ica.synth_jpeg(W, H, seed=W * H, quality=95)
        px = oracle.load(data, 3)[1]
        for o in cases:
            out_h, out_w = size
            first = rm.resize(om.orient(px, o), out_w, out_h, "box")
            # resized in D's frame without the mirror, then mirrored: what a flip after the resize would give
            r = rm.resize(om.orient(px, 5) if o >= 5 else px, out_w, out_h, "box")
            mirrored_last = {2: r[:, ::-1], 3: r[::-1, ::-1], 4: r[::-1], 6: r[:, ::-1], 7: r[::-1, ::-1], 8: r[::-1]}[o]
            assert not np.array_equal(first, mirrored_last), (o, W, H)  # the case keeps its force
            got, reasons = dec.decode([data], size=size, filter="box", dtype=torch.uint8, layout="HWC", orientation=o)
            assert reasons == [None]
            assert np.array_equal(got[0].cpu().numpy(), first), (o, W, H)


def test_transpose_comes_before_the_resize(ica, oracle, dec):
    """37 x 53 -> 23 x 19 in D's frame differs from the same resize in the stored frame transposed afterwards, for every filter"""
    data = ica.synth_jpeg(53, 37, seed=2, quality=95)
    px = oracle.load(data, 3)[1]
    for name in rm.FILTERS:
        for o in (5, 6, 7, 8):
            d = om.orient(px, o)  # 37 wide, 53 tall
            right = rm.resize(d, 23, 19, name)
            s = om.ORIENT[o](np.ascontiguousarray(rm.resize(px, 19, 23, name)))  # resize in S, then orient
            assert not np.array_equal(right, np.ascontiguousarray(s)), (name, o)
            got, reasons = dec.decode([data], size=(19, 23), filter=name, dtype=torch.uint8, layout="HWC", orientation=o)
            assert reasons == [None]
            assert np.array_equal(got[0].cpu().numpy(), right), (name, o)


def test_identity_sizes_and_thin_windows(ica, oracle, dec):
    data = ica.synth_jpeg(29, 18, seed=6, quality=90)
    px = oracle.load(data, 3)[1]
    for o in range(1, 9):
        dw, dh = om.displayed_size(29, 18, o)
        plain, _ = dec.decode([data], orientation=o, dtype=torch.float16)
        same, _ = dec.decode([data], orientation=o, dtype=torch.float16, size=(dh, dw), filter="lanczos")
        assert tm.same_bits(plain, same) and tm.same_bits(plain[0], _want(px, o, (0, 0, dw, dh), None, None, False, False, "CHW", torch.float16))
        for win in ((0, 0, 1, 1), (dw - 1, dh - 1, 1, 1), (3, 0, 1, dh), (0, 5, dw, 1), (dw - 2, 1, 1, dh - 2)):
            for size in (None, (3, 4)):
                for fx, fy in FLIPS:
                    got, reasons = dec.decode([data], crops=[win], orientation=o, flip_x=fx, flip_y=fy, size=size, dtype=torch.uint8, layout="HWC")
                    assert reasons == [None]
                    assert tm.same_bits(got[0], _want(px, o, win, size, "bilinear", fx, fy, "HWC", torch.uint8)), (o, win, size, fx, fy)


def test_tiles_both_ways_and_big_pictures(ica, oracle, dec):
    """9000 x 24 and 24 x 9000 RGB (past the 8192-pixel segment of RGB output before and after the transpose), and a 4000 x 3000 4:2:0
    picture at o = 6 to 224 x 224"""
    for W, H in ((9000, 24), (24, 9000)):
        data = ica.synth_jpeg(W, H, seed=W, quality=90)
        px = oracle.load(data, 3)[1]
        for o in (1, 2, 5, 6, 7, 8):
            dw, dh = om.displayed_size(W, H, o)
            for layout, dtype in (("CHW", torch.float16), ("HWC", torch.uint8)):
                mean, std = _norm(dtype, 3)
                got, reasons = dec.decode([data, data], orientation=o, layout=layout, dtype=dtype, mean=mean, std=std, flip_x=[False, True],
                                          flip_y=[True, False])
                assert reasons == [None] * 2
                for i, (fx, fy) in enumerate(((False, True), (True, False))):
                    assert tm.same_bits(got[i], _want(px, o, (0, 0, dw, dh), None, None, fx, fy, layout, dtype, mean, std)), (W, H, o, layout)
            got, _ = dec.decode([data], orientation=o, size=(31, 29), filter="hamming", dtype=torch.uint8, layout="HWC")
            assert tm.same_bits(got[0], _want(px, o, (0, 0, dw, dh), (31, 29), "hamming", False, False, "HWC", torch.uint8)), (W, H, o)
    data = ica.synth_jpeg(4000, 3000, seed=40, quality=85)
    px = oracle.load(data, 3)[1]
    got, reasons = dec.decode([data], orientation=6, size=(224, 224), dtype=torch.float16, mean=MEAN[:3], std=STD[:3])
    assert reasons == [None]
    assert tm.same_bits(got[0], _want(px, 6, (0, 0, 3000, 4000), (224, 224), "bilinear", False, False, "CHW", torch.float16, MEAN[:3], STD[:3]))


def test_long_spans_transposed(ica, oracle, dec):
    """the transposed resize where its taps outgrow LDS: a 180 x 4200 stored picture is 4200 x 180 displayed.  Lanczos to 1 x 2 reads
    4200 stored rows per output column (more than the stage's 4096: the span is walked in chunks) with 12601 horizontal taps (read from
    the plan) and 1081 vertical ones (read from the plan); a 700-wide window to 1 x 1 has the same taps with the span in one chunk"""
    data = ica.synth_jpeg(180, 4200, seed=18, quality=90)
    px = oracle.load(data, 3)[1]
    for o in (5, 6, 7, 8):
        for win, size in (((0, 0, 4200, 180), (1, 2)), ((100, 0, 700, 180), (1, 1))):
            got, reasons = dec.decode([data], crops=[win], orientation=o, size=size, filter="lanczos", dtype=torch.uint8, layout="HWC")
            assert reasons == [None]
            assert tm.same_bits(got[0], _want(px, o, win, size, "lanczos", False, False, "HWC", torch.uint8)), (o, win, size)


def test_random_resized_crops_in_displayed_frame(ica, oracle, dec):
    data = ica.synth_jpeg(640, 360, seed=31, quality=90)
    px = oracle.load(data, 3)[1]
    rng = np.random.default_rng(23)
    n = 96
    os_ = [int(v) for v in rng.integers(1, 9, n)]
    crops, fxs = [], [bool(v) for v in rng.integers(0, 2, n)]
    for o in os_:
        dw, dh = om.displayed_size(640, 360, o)
        while True:
            area = dw * dh * rng.uniform(0.08, 1.0)
            ratio = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
            w, h = int(round(np.sqrt(area * ratio))), int(round(np.sqrt(area / ratio)))
            if 0 < w <= dw and 0 < h <= dh:
                break
        crops.append((int(rng.integers(0, dw - w + 1)), int(rng.integers(0, dh - h + 1)), w, h))
    got, reasons = dec.decode([data] * n, crops=crops, flip_x=fxs, size=(64, 64), dtype=torch.bfloat16, mean=MEAN[:3], std=STD[:3], orientation=os_)
    assert reasons == [None] * n
    for i in range(n):
        assert tm.same_bits(got[i], _want(px, os_[i], crops[i], (64, 64), "bilinear", fxs[i], False, "CHW", torch.bfloat16, MEAN[:3], STD[:3])), i


def _guarded(ica, oracle, gpu_ctx, data, req, r):
    """r: (dtype, layout, offset_elems, win, size or None, row_pitch, plane_pitch, fx, fy, filter, o) into a sentinel-filled buffer;
    every byte is compared with the model: the written elements and the untouched rest"""
    dtype, layout, off, win, size, rp, pp, fx, fy, name, o = r
    px = oracle.load(data, req)[1]
    n = px.shape[-1] if px.ndim == 3 else 1
    b = ica.Batch(gpu_ctx, 1, 8 << 20, 8 << 20, 8 << 20)
    ok, slots, why = b.decode_jpegs([data], req, threads=1)
    assert ok == 1, why
    es = tm.ESIZE[dtype]
    oh, ow = size if size is not None else (win[3], win[2])
    last = (oh - 1) * rp + ((n - 1) * pp + ow - 1 if layout == "CHW" else ow * n - 1)
    buf = torch.full(((off + last + 1) * es + 64,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    t = tm.tables(n, dtype, *_norm(dtype, n)) if dtype != torch.uint8 else None
    tb = None if t is None else t.view(tm.BITS[dtype]).numpy()
    if size is None:
        b.set_out_tensor(slots[0], buf.data_ptr() + off * es, tm.CODE[dtype], layout, *win, rp, pp, fx, fy, tb, orientation=o)
    else:
        b.set_out_tensor_resized(slots[0], buf.data_ptr() + off * es, tm.CODE[dtype], layout, *win, ow, oh, rp, pp, fx, fy, tb, name, orientation=o)
    torch.cuda.synchronize()
    b.submit()
    b.wait()
    want = torch.full((buf.numel(),), SENTINEL, dtype=torch.uint8)
    vals = _want(px, o, win, size, name, fx, fy, layout, dtype, *_norm(dtype, n)).view(tm.BITS[dtype]).contiguous().view(torch.uint8).view(-1, es)
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
            for o in (2, 5, 6, 7, 8):
                dw, dh = om.displayed_size(203, 97, o)
                for layout in ("HWC", "CHW"):
                    for size in (None, (37 - k, 45 + 3 * k)):
                        win = (3 + k, 5, min(61 + 2 * k, dw - 4 - k), min(83, dh - 6))
                        oh, ow = size if size is not None else (win[3], win[2])
                        rp = (ow * req if layout == "HWC" else ow) + 3 + 2 * k
                        pp = (oh - 1) * rp + ow + 5 if layout == "CHW" else 0
                        off = (1, 3, 5, 7, 9, 11, 13, 15)[(k * 2 + o + (layout == "CHW")) % 8] % (16 // tm.ESIZE[dtype]) or 1
                        _guarded(ica, oracle, gpu_ctx, data, req,
                                 (dtype, layout, off, win, size, rp, pp, bool(k & 1), layout == "CHW", rm.FILTERS[(k + o) % 5], o))


def test_orientation_1_equals_existing_calls(ica, gpu_ctx):
    L = ica.lib()
    L.mij_batch_set_out_tensor_oriented.argtypes = [C.c_void_p, C.c_int, C.POINTER(ica.OutTensor), C.POINTER(ica.OutResize), C.c_int32, C.c_void_p]
    data = ica.synth_jpeg(301, 77, seed=5)
    b = ica.Batch(gpu_ctx, 4, 8 << 20, 8 << 20, 8 << 20)
    ok, slots, _ = b.decode_jpegs([data] * 4, 3, threads=1)
    assert ok == 4
    outs = [torch.full((3, 40, 61), -7.0, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    routs = [torch.full((3, 24, 32), -7.0, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    t = tm.tables(3, torch.float32, MEAN[:3], STD[:3]).numpy()
    b.set_out_tensor(slots[0], outs[0].data_ptr(), 3, "CHW", 11, 20, 61, 40, 61, 61 * 40, True, False, t)
    b.set_out_tensor_resized(slots[2], routs[0].data_ptr(), 3, "CHW", 11, 20, 200, 50, 32, 24, 32, 32 * 24, False, True, t, "bicubic")
    tp = t.ctypes.data_as(C.c_void_p)
    tt = ica.OutTensor(C.c_void_p(outs[1].data_ptr()), 3, 1, 11, 20, 61, 40, 1, 0, 61, 61 * 40)
    assert L.mij_batch_set_out_tensor_oriented(b._h, slots[1], C.byref(tt), None, 1, tp) == 0
    tr = ica.OutTensor(C.c_void_p(routs[1].data_ptr()), 3, 1, 11, 20, 200, 50, 0, 1, 32, 32 * 24)
    r = ica.OutResize(32, 24, ica.MIJ_FILTER_BICUBIC, 0)
    assert L.mij_batch_set_out_tensor_oriented(b._h, slots[3], C.byref(tr), C.byref(r), 1, tp) == 0
    torch.cuda.synchronize()
    b.submit()
    b.wait()
    assert tm.same_bits(outs[0], outs[1]) and tm.same_bits(routs[0], routs[1])
    assert not bool((outs[0] == -7.0).any()) and not bool((routs[0] == -7.0).any())
    b.close()


@pytest.mark.parametrize("front", ["gpu_walk", "host_walk"])
def test_exif_end_to_end_mixed_batch(ica, oracle, golden, dec, monkeypatch, front):
    """files tagged 1..8 (both byte orders) and one untagged, of different sizes, larger than the GPU walk's batch threshold, to
    224 x 224, with one rejected file; through the default front end and the host walk"""
    if front == "host_walk":
        monkeypatch.setenv("MIJ_ENTROPY", "host")
    srcs = [ica.synth_jpeg(400 + 16 * o, 300 - 8 * o, seed=o, quality=90) for o in range(1, 9)] + [ica.synth_jpeg(350, 260, seed=99)]
    datas = [eb.tagged(d, o, o % 2 == 0) for o, d in zip(range(1, 9), srcs[:8])] + [srcs[8]]
    datas.insert(3, golden.jpg("trunc_noeoi"))
    got, reasons = dec.decode(datas, size=(224, 224), orientation="exif", dtype=torch.float16, mean=MEAN[:3], std=STD[:3], threads=16)
    assert reasons[3] == "expected marker" and bool((got[3] == 0).all())
    k = 0
    for i, d in enumerate(datas):
        if i == 3:
            continue
        o = ica.exif_orientation(d)
        assert o == (k + 1 if k < 8 else 1)
        px = oracle.load(srcs[k], 3)[1]
        H, W = px.shape[:2]
        dw, dh = om.displayed_size(W, H, o)
        assert reasons[i] is None
        assert tm.same_bits(got[i], _want(px, o, (0, 0, dw, dh), (224, 224), "bilinear", False, False, "CHW", torch.float16, MEAN[:3], STD[:3])), i
        k += 1


def test_all_request_kinds_in_one_batch(ica, oracle, gpu_ctx):
    import loadf_expect as fx
    datas = [ica.synth_jpeg(301, 77, seed=21), ica.synth_jpeg(120, 200, seed=22), ica.synth_jpeg(64, 48, seed=23), ica.synth_jpeg(97, 131, seed=24)]
    pxs = [oracle.load(d, 3)[1] for d in datas]
    b = ica.Batch(gpu_ctx, 5, 8 << 20, 8 << 20, 8 << 20)
    ok, slots, _ = b.decode_jpegs(datas, 3, threads=1)
    assert ok == 4
    b.reserve_out_f32(1 << 20)
    b.set_out_f32(slots[2])
    plain = torch.full((3, 40, 50), -1.0, dtype=torch.float32, device="cuda:0")
    rsz = torch.full((3, 32, 32), -1.0, dtype=torch.float32, device="cuda:0")
    ori = torch.full((60, 45, 3), 7, dtype=torch.uint8, device="cuda:0")
    orr = torch.full((3, 30, 20), -1.0, dtype=torch.float32, device="cuda:0")
    t = tm.tables(3, torch.float32, MEAN[:3], STD[:3])
    b.set_out_tensor(slots[0], plain.data_ptr(), 3, "CHW", 10, 20, 50, 40, 50, 2000, False, True, t.numpy())
    b.set_out_tensor_resized(slots[1], rsz.data_ptr(), 3, "CHW", 0, 0, 120, 200, 32, 32, 32, 1024, True, False, t.numpy(), "hamming")
    b.set_out_tensor(slots[2], ori.data_ptr(), 0, "HWC", 1, 2, 45, 60, 45 * 3, 0, True, False, None, orientation=6)
    b.set_out_tensor_resized(slots[3], orr.data_ptr(), 3, "CHW", 5, 3, 120, 90, 20, 30, 20, 600, False, True, t.numpy(), "lanczos", orientation=7)
    torch.cuda.synchronize()
    b.submit()
    b.wait()
    assert tm.same_bits(plain, tm.window(pxs[0], (10, 20, 50, 40), False, True, "CHW", t, torch.float32))
    assert tm.same_bits(rsz, rm.window(pxs[1], (0, 0, 120, 200), (32, 32), "hamming", True, False, "CHW", t, torch.float32))
    assert tm.same_bits(ori, _want(pxs[2], 6, (1, 2, 45, 60), None, None, True, False, "HWC", torch.uint8))
    assert tm.same_bits(orr, _want(pxs[3], 7, (5, 3, 120, 90), (30, 20), "lanczos", False, True, "CHW", torch.float32, MEAN[:3], STD[:3]))
    assert fx.same_bits(b.fetch_f32(slots[2]), fx.apply(fx.lut(3), pxs[2]))
    assert np.array_equal(b.fetch(slots[2]), pxs[2])
    b.close()


def test_reset_and_refusals(ica, gpu_ctx):
    L = ica.lib()
    L.mij_batch_set_out_tensor_oriented.argtypes = [C.c_void_p, C.c_int, C.POINTER(ica.OutTensor), C.POINTER(ica.OutResize), C.c_int32, C.c_void_p]
    data = ica.synth_jpeg(64, 48, 1)
    b = ica.Batch(gpu_ctx, 2, 8 << 20, 8 << 20, 8 << 20)
    b.decode_jpegs([data, data], 3, threads=1, gpu_entropy=False)
    buf = torch.full((64 * 64 * 3 + 64,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()

    def req(o=6, x0=0, y0=0, w=48, h=64, rp=48 * 3, slot=0, resize=None, filt=1):
        t = ica.OutTensor(C.c_void_p(p), 0, 0, x0, y0, w, h, 0, 0, rp, 0)
        r = None if resize is None else ica.OutResize(resize[0], resize[1], filt, 0)
        return L.mij_batch_set_out_tensor_oriented(b._h, slot, C.byref(t), C.byref(r) if r is not None else None, o, None)

    for o in (0, 9, -1, 65542):
        assert req(o=o) == MIJ_E_ARG
    assert req(o=6, w=64, h=48, rp=64 * 3) == MIJ_E_ARG          # fits the stored 64 x 48, not the displayed 48 x 64
    assert req(o=2, w=48, h=64) == MIJ_E_ARG                     # fits the displayed 48 x 64 of o >= 5 only
    assert req(o=5, x0=1) == MIJ_E_ARG and req(o=8, y0=1) == MIJ_E_ARG
    assert req(o=7, resize=(16, 16), filt=5) == MIJ_E_ARG        # the resize's own refusals
    assert req(o=6, resize=(16, 16), rp=16 * 3 - 1) == MIJ_E_ARG  # pitches apply to the output extent
    flags = b.slot_flags(1)
    b.set_flags(1, flags | 2)  # MIJ_FLAG_SKIP
    assert req(slot=1) == MIJ_E_STATE
    b.set_flags(1, flags)
    assert req(o=6) == 0
    assert req(o=9) == MIJ_E_ARG  # refused: the o = 6 request stays
    b.submit()
    b.wait()
    assert req(slot=1) == MIJ_E_STATE                                  # after upload
    px = b.fetch(0)
    assert tm.same_bits(buf[:64 * 48 * 3].view(64, 48, 3), tm.window(om.orient(px, 6), (0, 0, 48, 64), layout="HWC"))
    assert bool((buf[64 * 48 * 3:] == SENTINEL).all())
    # reset forgets the request: the next launch leaves buf untouched
    buf.fill_(SENTINEL)
    torch.cuda.synchronize()
    b.reset()
    b.decode_jpegs([data], 3, threads=1)
    b.submit()
    b.wait()
    assert bool((buf == SENTINEL).all())
    b.close()
