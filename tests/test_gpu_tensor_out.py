"""Tensor output on the GPU (k_out_tensor through mij_batch_set_out_tensor and TensorDecoder), bit for bit against tensor_model applied
to the reference's pixels (golden vectors or the oracle): every dtype, layout, channel count and flip, edge windows, both front ends,
guard bytes around unaligned and padded destinations, many slots, rejected pictures and every refusal of the C-ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

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


def _check(got, pxs, wins, fxs, fys, layout, dtype, mean=None, std=None):
    n = pxs[0].shape[-1] if pxs[0].ndim == 3 else 1
    t = None if dtype == torch.uint8 else tm.tables(n, dtype, mean, std)
    for i, px in enumerate(pxs):
        want = tm.window(px, wins[i], fxs[i], fys[i], layout, t, dtype)
        assert tm.same_bits(got[i], want), (i, wins[i], fxs[i], fys[i], layout, dtype)


def test_dtypes_layouts_channels_flips(ica, oracle, golden, dec):
    """every dtype x both layouts x req_comp 0..4 on a colour and a grey file x the four flip combinations, at an odd window"""
    flips = [(False, False), (True, False), (False, True), (True, True)]
    for data in (ica.synth_jpeg(33, 17, seed=3, quality=90), golden.jpg("grey_33x20")):
        for req in range(5):
            px = oracle.load(data, req)[1]
            win = (3, 1, 27, 15)
            for dtype in DTYPES:
                mean, std = _norm(dtype, px.shape[-1])
                for layout in ("CHW", "HWC"):
                    got, reasons = dec.decode([data] * 4, req_comp=req, crops=[win] * 4, flip_x=[f[0] for f in flips], flip_y=[f[1] for f in flips],
                                              layout=layout, dtype=dtype, mean=mean, std=std)
                    assert reasons == [None] * 4
                    shape = (4, px.shape[-1], 15, 27) if layout == "CHW" else (4, 15, 27, px.shape[-1])
                    assert tuple(got.shape) == shape and got.dtype == dtype and got.device.type == "cuda"
                    _check(got, [px] * 4, [win] * 4, [f[0] for f in flips], [f[1] for f in flips], layout, dtype, mean, std)


@pytest.mark.parametrize("w,h", [(1, 1), (33, 17), (1920, 1080)])
def test_edge_windows(ica, oracle, dec, w, h):
    """odd x0, width 1, height 1, the whole picture, windows on the right and bottom edges; 1080p takes the GPU walk"""
    data = ica.synth_jpeg(w, h, seed=w + h, quality=90)
    px = oracle.load(data, 3)[1]
    wins = [(0, 0, w, h), (w - 1, h - 1, 1, 1), (0, h - 1, w, 1), (w - 1, 0, 1, h)]
    if w > 8:
        wins += [(3, 2, 1, h - 5), (5, 3, w - 9, 1), (w - 11, h - 7, 11, 7), (1, 1, w - 1, h - 1), (7, 0, w - 7, h)]
    for k, win in enumerate(wins):
        dtype = DTYPES[k % 4]
        layout = ("CHW", "HWC")[k % 2]
        fx, fy = bool(k & 2), bool(k & 4)
        mean, std = _norm(dtype, 3)
        got, reasons = dec.decode([data, data], crops=[win, win], flip_x=[fx, not fx], flip_y=[fy, fy], layout=layout, dtype=dtype, mean=mean, std=std)
        assert reasons == [None, None]
        _check(got, [px, px], [win, win], [fx, not fx], [fy, fy], layout, dtype, mean, std)


@pytest.mark.parametrize("name", ["b422_37x21", "cmyk_40x30", "prog_420_23x41", "grey_1x1", "big_prog_420_320x200"])
def test_golden_families(golden, dec, name):
    """4:2:2, CMYK, progressive (host front end, int16 staging) and grey golden files feed the pass"""
    data = golden.jpg(name)
    for req in (0, 3, 4, 1):
        kind, px = golden.expect(name, req)
        if kind != "ok":
            continue
        H, W = px.shape[:2]
        win = (W // 3, H // 4, W - W // 3, H - H // 4)
        for dtype, layout in ((torch.float16, "CHW"), (torch.uint8, "HWC"), (torch.bfloat16, "HWC"), (torch.float32, "CHW")):
            mean, std = _norm(dtype, px.shape[-1])
            got, reasons = dec.decode([data, data], req_comp=req, crops=[win, (0, 0, win[2], win[3])], flip_x=[True, False], flip_y=[False, True],
                                      layout=layout, dtype=dtype, mean=mean, std=std)
            assert reasons == [None, None]
            _check(got, [px, px], [win, (0, 0, win[2], win[3])], [True, False], [False, True], layout, dtype, mean, std)


def _guarded(ica, oracle, gpu_ctx, data, req, reqs):
    """reqs: (dtype, layout, offset_elems, win, row_pitch, plane_pitch, fx, fy) into one sentinel-filled buffer each; every byte is
    compared with the model: the written elements and the untouched rest"""
    px = oracle.load(data, req)[1]
    n = px.shape[-1]
    b = ica.Batch(gpu_ctx, 1, 8 << 20, 8 << 20, 8 << 20)
    ok, slots, why = b.decode_jpegs([data], req, threads=1)
    assert ok == 1, why
    bufs = []
    for (dtype, layout, off, win, rp, pp, fx, fy) in reqs:
        es = tm.ESIZE[dtype]
        x0, y0, w, h = win
        last = (h - 1) * rp + ((n - 1) * pp + w - 1 if layout == "CHW" else w * n - 1)
        nbytes = (off + last + 1) * es + 64
        buf = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        t = tm.tables(n, dtype, *_norm(dtype, n)) if dtype != torch.uint8 or fx else None  # one u8 request through a table
        tb = None if t is None else t.view(tm.BITS[dtype]).numpy()
        b.set_out_tensor(slots[0], buf.data_ptr() + off * es, tm.CODE[dtype], layout, x0, y0, w, h, rp, pp, fx, fy, tb)
        bufs.append((buf, dtype, layout, off, win, rp, pp, fx, fy, t))
    torch.cuda.synchronize()
    b.submit()
    b.wait()
    for (buf, dtype, layout, off, win, rp, pp, fx, fy, t) in bufs:
        es = tm.ESIZE[dtype]
        want = torch.full((buf.numel(),), SENTINEL, dtype=torch.uint8)
        vals = tm.window(px, win, fx, fy, layout, t, dtype).view(tm.BITS[dtype]).contiguous().view(torch.uint8).view(-1, es)
        x0, y0, w, h = win
        if layout == "CHW":
            c, y, x = torch.meshgrid(torch.arange(n), torch.arange(h), torch.arange(w), indexing="ij")
            el = off + c * pp + y * rp + x
        else:
            y, x, c = torch.meshgrid(torch.arange(h), torch.arange(w), torch.arange(n), indexing="ij")
            el = off + y * rp + x * n + c
        idx = (el.reshape(-1, 1) * es + torch.arange(es)).reshape(-1)
        want[idx] = vals.reshape(-1)
        got = buf.cpu()
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (dtype, layout, off, win, rp, pp, fx, fy, bad[:8].tolist())
    b.close()


def test_guard_bytes_unaligned_padded(ica, oracle, gpu_ctx):
    data = ica.synth_jpeg(203, 97, seed=12, quality=92)
    for req in (3, 1, 4, 2):
        reqs = []
        for k, dtype in enumerate(DTYPES):
            es = tm.ESIZE[dtype]
            for layout in ("HWC", "CHW"):
                win = (17 + k, 5, 61 + 2 * k, 23) if layout == "HWC" else (2 * k + 1, 9, 129, 31 - k)
                w, h = win[2], win[3]
                rp = (w * req if layout == "HWC" else w) + 3 + 2 * k  # odd, padded
                pp = (h - 1) * rp + w + 5 if layout == "CHW" else 0
                off = (1, 3, 5, 7, 9, 11, 13, 15)[(k * 2 + (layout == "CHW")) % 8] % (16 // es) or 1
                reqs.append((dtype, layout, off, win, rp, pp, bool(k & 1), layout == "CHW"))
        # several requests may not share a slot (asking again replaces): one batch per request
        for r in reqs:
            _guarded(ica, oracle, gpu_ctx, data, req, [r])
    # a whole 1080p picture into a padded, unaligned destination
    big = ica.synth_jpeg(1920, 1080, seed=4)
    _guarded(ica, oracle, gpu_ctx, big, 3, [(torch.float16, "CHW", 3, (0, 0, 1920, 1080), 1931, 1931 * 1080 + 7, True, False)])
    _guarded(ica, oracle, gpu_ctx, big, 3, [(torch.uint8, "HWC", 5, (1, 3, 1919, 1077), 1919 * 3 + 9, 0, False, True)])


def _crops(rng, sizes, n, cw=224, ch=224):
    out = []
    for i in range(n):
        W, H = sizes[i]
        out.append((int(rng.integers(0, W - cw + 1)), int(rng.integers(0, H - ch + 1)), cw, ch))
    return out


def test_many_slots_random_crops(ica, oracle, dec):
    """300 random 224 x 224 crops with random flips from mixed 1080p / 640 x 480 pictures, one bf16 CHW tensor and one channels-last
    (HWC) tensor; the CHW one is a slice of a larger, padded tensor"""
    srcs = [ica.synth_jpeg(1920, 1080, seed=s, quality=90) for s in range(3)] + [ica.synth_jpeg(640, 480, seed=10 + s, quality=85) for s in range(3)]
    pxs = [oracle.load(d, 3)[1] for d in srcs]
    rng = np.random.default_rng(5)
    pick = rng.integers(0, len(srcs), 300)
    datas = [srcs[k] for k in pick]
    crops = _crops(rng, [(pxs[k].shape[1], pxs[k].shape[0]) for k in pick], 300)
    fx, fy = [bool(v) for v in rng.integers(0, 2, 300)], [bool(v) for v in rng.integers(0, 2, 300)]
    big = torch.full((300, 4, 230, 240), -7.0, dtype=torch.bfloat16, device="cuda:0")
    out = big[:, 1:, 3:227, 5:229]
    got, reasons = dec.decode(datas, crops=crops, flip_x=fx, flip_y=fy, dtype=torch.bfloat16, mean=MEAN[:3], std=STD[:3], out=out)
    assert got.data_ptr() == out.data_ptr() and reasons == [None] * 300
    _check(got, [pxs[k] for k in pick], crops, fx, fy, "CHW", torch.bfloat16, MEAN[:3], STD[:3])
    pad = big.clone()
    pad[:, 1:, 3:227, 5:229] = -7.0
    assert bool((pad.float() == -7.0).all())  # nothing outside the slice was written
    got, reasons = dec.decode(datas, crops=crops, flip_x=fx, flip_y=fy, layout="HWC", dtype=torch.bfloat16, mean=MEAN[:3], std=STD[:3])
    assert tuple(got.shape) == (300, 224, 224, 3) and reasons == [None] * 300
    _check(got, [pxs[k] for k in pick], crops, fx, fy, "HWC", torch.bfloat16, MEAN[:3], STD[:3])
    cl = got.permute(0, 3, 1, 2)  # the same memory seen as a channels-last [N, C, h, w] tensor
    assert cl.is_contiguous(memory_format=torch.channels_last)


def test_rejected_picture_keeps_its_slice(ica, oracle, golden, dec):
    good = [ica.synth_jpeg(640, 480, seed=s) for s in range(4)]
    bad = golden.jpg("trunc_noeoi")  # header fine, stream rejected
    datas = good[:2] + [bad, golden.jpg("garbage")] + good[2:]
    crops = [(7, 5, 40, 30)] * 2 + [(0, 0, 40, 30), (0, 0, 40, 30)] + [(100, 50, 40, 30)] * 2
    out = torch.full((6, 3, 30, 40), 3.5, dtype=torch.float32, device="cuda:0")
    got, reasons = dec.decode(datas, crops=crops, dtype=torch.float32, out=out)
    assert reasons[2] == "expected marker" and reasons[3] == "unknown image type"
    assert reasons[:2] == [None, None] and reasons[4:] == [None, None]
    assert bool((got[2:4] == 3.5).all())
    pxs = [oracle.load(d, 3)[1] for d in good]
    _check(got[[0, 1, 4, 5]], pxs, [crops[i] for i in (0, 1, 4, 5)], [False] * 4, [False] * 4, "CHW", torch.float32)
    fresh, reasons = dec.decode(datas, crops=crops, dtype=torch.float16)
    assert bool((fresh[2:4] == 0).all())  # a tensor the decoder allocated: zero there


def test_float_tensor_and_fetch_agree_then_reset(ica, oracle, gpu_ctx):
    import loadf_expect as fx
    data = ica.synth_jpeg(301, 77, seed=21)
    px = oracle.load(data, 3)[1]
    b = ica.Batch(gpu_ctx, 2, 8 << 20, 8 << 20, 8 << 20)
    ok, slots, _ = b.decode_jpegs([data], 3, threads=1)
    b.reserve_out_f32(1 << 20)
    b.set_out_f32(slots[0])
    dst = torch.full((3, 77, 301), -1.0, dtype=torch.float32, device="cuda:0")
    t = tm.tables(3, torch.float32, MEAN[:3], STD[:3])
    b.set_out_tensor(slots[0], dst.data_ptr(), 3, "CHW", 0, 0, 301, 77, 301, 301 * 77, False, False, t.numpy())
    torch.cuda.synchronize()
    b.submit()
    b.wait()
    assert np.array_equal(b.fetch(slots[0]), px)
    assert fx.same_bits(b.fetch_f32(slots[0]), fx.apply(fx.lut(3), px))
    assert tm.same_bits(dst, tm.window(px, (0, 0, 301, 77), layout="CHW", table=t, dtype=torch.float32))
    # reset forgets the request: the next launch leaves dst untouched
    dst.fill_(-1.0)
    torch.cuda.synchronize()
    b.reset()
    ok, slots, _ = b.decode_jpegs([data], 3, threads=1)
    b.submit()
    b.wait()
    assert np.array_equal(b.fetch(slots[0]), px)
    assert bool((dst == -1.0).all())
    b.close()


def _hip():
    """the HIP runtime this process already uses (torch's and the library's)"""
    paths = {ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


def test_refusals_leave_the_sentinel(ica, gpu_ctx):
    L = ica.lib()
    L.mij_batch_set_out_tensor.argtypes = [C.c_void_p, C.c_int, C.POINTER(ica.OutTensor), C.c_void_p]
    datas = [ica.synth_jpeg(64, 48, 1), ica.synth_jpeg(64, 48, 2)]
    b = ica.Batch(gpu_ctx, 4, 8 << 20, 8 << 20, 8 << 20)
    b.decode_jpegs(datas, 3, threads=1, gpu_entropy=False)
    buf = torch.full((64 * 48 * 3 * 2 + 64,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()

    def req(dst, dtype=0, layout=0, x0=0, y0=0, w=64, h=48, rp=64 * 3, pp=0, slot=0, table=None):
        t = ica.OutTensor(C.c_void_p(dst), dtype, layout, x0, y0, w, h, 0, 0, rp, pp)
        return L.mij_batch_set_out_tensor(b._h, slot, C.byref(t), table)

    assert req(p, x0=1) == MIJ_E_ARG                          # window leaves the picture on the right
    assert req(p, y0=1) == MIJ_E_ARG                          # ... at the bottom
    assert req(p, w=0) == MIJ_E_ARG and req(p, h=0) == MIJ_E_ARG and req(p, x0=-1, w=10) == MIJ_E_ARG
    assert req(p, rp=64 * 3 - 1) == MIJ_E_ARG                 # HWC rows overlap
    assert req(p, layout=1, rp=63, pp=64 * 48) == MIJ_E_ARG   # CHW rows overlap
    assert req(p, layout=1, rp=64, pp=64 * 47) == MIJ_E_ARG   # CHW planes overlap
    lut = tm.tables(3, torch.float16).view(torch.int16).numpy()
    lp = lut.ctypes.data_as(C.c_void_p)
    assert req(p + 1, dtype=1, rp=64 * 3, table=lp) == MIJ_E_ARG  # misaligned for 2-byte elements
    assert req(p, dtype=1, table=None) == MIJ_E_ARG           # a float type needs its table
    assert req(p, dtype=7) == MIJ_E_ARG and req(p, layout=2) == MIJ_E_ARG
    host = np.full(64 * 48 * 3, SENTINEL, np.uint8)
    assert req(host.ctypes.data) == MIJ_E_ARG                 # host (numpy) memory
    # hipMalloc'd memory: an extent that ends exactly at the end is accepted, one element further is not
    hip = _hip()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    n = 64 * 48 * 3
    dp = C.c_void_p()
    assert hip.hipMalloc(C.byref(dp), n * 2 + 2) == 0
    try:
        assert hip.hipMemset(dp, SENTINEL, n * 2 + 2) == 0
        assert req(dp.value + 4, dtype=1, table=lp) == MIJ_E_ARG  # 2 bytes past the end
        assert req(dp.value + 2, dtype=1, table=lp) == 0
        assert req(1 << 47, dtype=0) == MIJ_E_ARG                 # no allocation at all; the accepted request stays
        flags = b.slot_flags(1)
        b.set_flags(1, flags | 2)  # MIJ_FLAG_SKIP
        assert req(p, slot=1) == MIJ_E_STATE                      # skipped slot
        b.set_flags(1, flags)
        assert req(p, slot=5) == MIJ_E_ARG                        # no such slot
        b.submit()
        b.wait()
        assert req(p, slot=1) == MIJ_E_STATE                      # after upload
        got = np.empty(n * 2 + 2, np.uint8)
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), dp, got.size, 2) == 0  # hipMemcpyDeviceToHost
        want = tm.window(b.fetch(0), (0, 0, 64, 48), layout="HWC", table=tm.tables(3, torch.float16), dtype=torch.float16)
        assert got[:2].tolist() == [SENTINEL, SENTINEL]
        assert np.array_equal(got[2:], want.view(torch.int16).numpy().view(np.uint8).reshape(-1))
    finally:
        hip.hipFree(dp)
    assert bool((buf == SENTINEL).all()) and bool((torch.from_numpy(host) == SENTINEL).all())
    b.close()


def test_extent_past_a_torch_allocation(ica, gpu_ctx):
    """a torch tensor that fills its allocator segment: an extent one element past the segment's end is refused"""
    L = ica.lib()
    L.mij_batch_set_out_tensor.argtypes = [C.c_void_p, C.c_int, C.POINTER(ica.OutTensor), C.c_void_p]
    b = ica.Batch(gpu_ctx, 1, 8 << 20, 8 << 20, 8 << 20)
    b.decode_jpegs([ica.synth_jpeg(64, 48, 1)], 3, threads=1, gpu_entropy=False)
    buf = torch.full((4 << 20,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= buf.data_ptr() < s["address"] + s["total_size"]]
    assert len(seg) == 1
    end = seg[0]["address"] + seg[0]["total_size"]
    n = 64 * 48 * 3
    for off, rc in ((1, MIJ_E_ARG), (0, 0)):
        t = ica.OutTensor(C.c_void_p(end - n + off), 0, 0, 0, 0, 64, 48, 0, 0, 64 * 3, 0)
        assert L.mij_batch_set_out_tensor(b._h, 0, C.byref(t), None) == rc
    b.close()
    assert bool((buf == SENTINEL).all())
