"""Float pictures into the encoder on the GPU (mij_enc_add_device_float, k_enc_gather_float, TensorEncoder.encode_normalized).

Expected bytes never come from the code under test: they are emit_jpeg(*host_transform(model(x), q, flip)) -- the numpy model of the
contract (tests/denorm_model.py), then the host writer that the reference goldens pin.  Wherever the C-level Encoder is used the
slot's data units are compared as well as its stream.

Which load path a group of 4 pixels takes is the kernel's own rule (mij_emit_kernels.h), restated in path_groups(): a run of 4
elements is one vector load when the group lies inside the picture (x0 + 4 <= width) and the run's address is a multiple of 4
elements; the right-edge group, the padding groups and misaligned runs take element loads.  torch allocations start on at least 256
bytes, so a contiguous picture whose width is a multiple of 4 is all vector loads up to its edge, the same picture one element into
its allocation is all element loads, and an odd row pitch alternates between the two from row to row."""
import ctypes as C

import numpy as np
import pytest
import torch

import denorm_model as dm

pytestmark = pytest.mark.gpu

MIJ_E_ARG = -2
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
MEAN4, STD4 = dm.IM_MEAN + (0.5,), dm.IM_STD + (0.25,)
WIDTHS, HEIGHTS = (1, 3, 4, 5, 8, 15, 16, 17, 33), (1, 3, 4, 5, 9)


def code(ica, dtype):
    return {torch.float16: ica.MIJ_DT_F16, torch.bfloat16: ica.MIJ_DT_BF16, torch.float32: ica.MIJ_DT_F32}[dtype]


def normalised(rng, shape, c, dtype, mean=MEAN4, std=STD4):
    """seeded floats spread over about [-0.3, 1.3] in normalised units, channels last in `shape`, as a CPU tensor of dtype"""
    v = rng.uniform(-0.3, 1.3, size=shape)
    x = (v - np.array(mean[:c])) / np.array(std[:c])
    return torch.from_numpy(x.astype(np.float32)).to(dtype)


def hwc(t, layout):
    """a 2-D / 3-D torch view -> float32 numpy, channels last"""
    a = dm.widen(t)
    return a if a.ndim == 2 or layout == "HWC" else np.ascontiguousarray(a.transpose(1, 2, 0))


def in_tensor(ica, t, layout):
    if t.dim() == 2:
        return ica.InTensor(t.data_ptr(), ica.MIJ_LAYOUT_HWC, t.shape[1], t.shape[0], 1, t.stride(0), 0)
    if layout == "CHW":
        c, h, w = t.shape
        return ica.InTensor(t.data_ptr(), ica.MIJ_LAYOUT_CHW, w, h, c, t.stride(1), t.stride(0))
    h, w, c = t.shape
    return ica.InTensor(t.data_ptr(), ica.MIJ_LAYOUT_HWC, w, h, c, t.stride(0), 0)


def path_groups(t, layout):
    """(vector loads, groups on element loads) the kernel's rule gives for a view on the GPU"""
    es = t.element_size()
    if t.dim() == 2:
        planes, (h, w), rp, pp, sx = 1, t.shape, t.stride(0), 0, 1
    elif layout == "CHW":
        c, h, w = t.shape
        planes, rp, pp, sx = (3 if c > 2 else 1), t.stride(1), t.stride(0), 1
    else:
        h, w, c = t.shape
        planes, rp, pp, sx = 1, t.stride(0), 0, c
        if c == 1:
            sx = 1
    vec = el = 0
    for p in range(planes):
        for y in range(h):
            addr = t.data_ptr() + (y * rp + p * pp) * es
            inside = w // 4
            if addr % (4 * es) == 0:
                vec += inside * sx
            else:
                el += inside
            el += 1  # the group that holds or follows the right edge: every padded row has one
    return vec, el


def expect(ica, pic, q, flip, optimize=False):
    plan, du = ica.host_transform(pic, q, flip)
    return du, ica.emit_jpeg(plan, du, optimize)


def run_slots(ica, ctx, items):
    """items: (view on the GPU, layout, InConvert, q, flip, expected uint8 picture).  One encoder, one launch; every slot's units and
    stream against the host writer's for the expected picture."""
    enc = ica.Encoder(ctx, len(items), 64 << 20, 64 << 20, stage_bytes=0)
    enc.stream_reserve(16 << 20)
    for (t, layout, cv, q, flip, _) in items:
        enc.add_device_float(in_tensor(ica, t, layout), cv, q, flip)
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == len(items)
    for s, (t, layout, cv, q, flip, pic) in enumerate(items):
        du, jpg = expect(ica, pic, q, flip)
        what = (s, tuple(t.shape), layout, q, flip)
        assert np.array_equal(enc.fetch(s), du), what
        assert enc.stream(s)[0] == jpg, what
    enc.close()


def convert(ica, dtype, c, mean=MEAN4, std=STD4):
    scale, bias = dm.scale_bias(c, mean[:c], std[:c])
    return ica.InConvert(code(ica, dtype), scale, bias), scale, bias


@pytest.fixture(scope="module")
def tenc(ica, gpu_ctx):
    e = ica.TensorEncoder()
    yield e
    e.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_every_shape_layout_quality_and_flip(ica, gpu_ctx, dtype):
    """widths 1..33 x heights 1..9 (partial row groups, the edge clamp, padding to 8 and 16), comp 1..4, both layouts and 2-D grey,
    q 90 (4:2:0) and 95 (4:4:4), flipped and not: one launch of contiguous pictures, both clamps firing"""
    rng = np.random.default_rng(100 + DTYPES.index(dtype))
    items, lo, hi, vec, el = [], 0, 0, 0, 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for c in (1, 2, 3, 4):
                cv, scale, bias = convert(ica, dtype, c)
                for layout in ("CHW", "HWC"):
                    x = normalised(rng, (h, w, c), c, dtype)
                    pic = dm.picture(dm.widen(x), scale, bias)
                    lo, hi = lo + int((pic == 0).sum()), hi + int((pic == 255).sum())
                    if c == 1 and layout == "HWC":
                        t, pic = x[:, :, 0].contiguous().cuda(), pic[:, :, 0]  # 2-D grey
                    else:
                        t = (x.permute(2, 0, 1) if layout == "CHW" else x).contiguous().cuda()
                    v, e = path_groups(t, layout)
                    vec, el = vec + v, el + e
                    for (q, flip) in ((90, False), (95, True), (90, True), (95, False)):
                        items.append((t, layout, cv, q, flip, pic))
    assert lo > 1000 and hi > 1000 and vec > 1000 and el > 1000, (lo, hi, vec, el)
    run_slots(ica, gpu_ctx, items)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_views_alignment_and_strides(ica, gpu_ctx, dtype):
    """the same kind of pictures as views: one element into the allocation, an odd row pitch, the channels of a wider tensor, a
    slice of a larger 4-D batch -- with the load path of each counted by the kernel's rule.  (A channel slice of an HWC tensor has
    a pixel stride above C, which the layout cannot say and encode() refuses; the channel slice is CHW alone.)"""
    rng = np.random.default_rng(200 + DTYPES.index(dtype))
    items, seen = [], {}

    def add(kind, view, layout, c):
        cv, scale, bias = convert(ica, dtype, c)
        pic = dm.picture(hwc(view, layout), scale, bias)
        v, e = path_groups(view, layout)
        seen.setdefault((kind, layout), []).append((v, e))
        for q, flip in ((90, False), (95, True)):
            items.append((view, layout, cv, q, flip, pic))

    for (w, h, c) in ((4, 3, 3), (16, 5, 1), (17, 4, 3), (33, 9, 4), (8, 5, 2), (15, 1, 3), (32, 8, 3)):
        pitch = (w + 8) // 4 * 4  # rows of a multiple of 4 elements: the base pointer alone decides
        big = normalised(rng, (h, pitch, c), c, dtype)
        chw = big.permute(2, 0, 1).contiguous().cuda()
        add("aligned", chw[:, :, 0:w], "CHW", c)
        add("offset", chw[:, :, 1:1 + w], "CHW", c)
        hw = big.cuda()
        add("aligned", hw[:, 0:w, :], "HWC", c)
        add("offset", hw[:, 1:1 + w, :], "HWC", c)
        odd = w + 1 if w % 2 == 0 else w + 2  # an odd row pitch: a row is aligned where y * pitch is a multiple of 4 (CHW)
        big = normalised(rng, (h, odd, c), c, dtype)
        add("odd", big.permute(2, 0, 1).contiguous().cuda()[:, :, 0:w], "CHW", c)
        add("odd", big.cuda()[:, 0:w, :], "HWC", c)
        wide = normalised(rng, (h, w, c + 1), c + 1, dtype, MEAN4[:c] + (0.3,), STD4[:c] + (0.4,)).permute(2, 0, 1).contiguous().cuda()
        add("channels", wide[:c], "CHW", c)
        if c > 1:
            wide1 = normalised(rng, (h, w, c), c, dtype, (0.3,) + MEAN4[:c - 1], (0.4,) + STD4[:c - 1]).permute(2, 0, 1).contiguous().cuda()
            add("channels", wide1[1:], "CHW", c - 1)  # begins one plane in: h * w elements from the allocation's start
        batch = normalised(rng, (4, h + 2, w + 3, c), c, dtype)
        b_chw = batch.permute(0, 3, 1, 2).contiguous().cuda()[1:3, :, 1:1 + h, 2:2 + w]
        b_hwc = batch.cuda()[1:3, 1:1 + h, 2:2 + w, :]
        for i in range(2):
            add("batch", b_chw[i], "CHW", c)
            add("batch", b_hwc[i], "HWC", c)
    # the paths, by the rule: aligned rows of 4 and more pixels load vectors; one element further in none do (CHW: always; HWC: the
    # offset is C elements, a multiple of 4 for C = 4 alone); odd pitches and batch slices mix both
    assert all(v > 0 for (v, e) in seen[("aligned", "CHW")]) and all(v > 0 for (v, e) in seen[("aligned", "HWC")])
    assert all(v == 0 and e > 0 for (v, e) in seen[("offset", "CHW")])
    assert sum(v == 0 for (v, e) in seen[("offset", "HWC")]) >= 5 and any(v > 0 for (v, e) in seen[("offset", "HWC")])
    for key in (("odd", "CHW"), ("odd", "HWC"), ("batch", "CHW"), ("batch", "HWC"), ("channels", "CHW")):
        assert sum(v for (v, e) in seen[key]) > 0 and sum(e for (v, e) in seen[key]) > 0, key
    run_slots(ica, gpu_ctx, items)


def special_values(dtype):
    """k + 0.5 for every k the type can say it for (k < 300), the neighbours of those, -0.0, negatives, values above 255, +-Inf,
    NaN, the type's subnormals -> a 1-D CPU tensor of dtype"""
    ks = torch.arange(0, 300, dtype=torch.float64) + 0.5
    ties = ks.to(dtype)
    ties = ties[ties.to(torch.float64) == ks]
    ity = torch.int32 if dtype == torch.float32 else torch.int16
    bits = ties.view(ity)
    other = torch.tensor([-0.0, 0.0, -0.25, -0.5, -1.0, -255.5, -1e4, 0.25, 0.75, 1.0, 127.0, 254.0, 254.75, 255.0, 255.25, 255.5, 256.0, 300.0, 1e4, 65504.0,
                          float("inf"), -float("inf"), float("nan"), -float("nan")], dtype=torch.float32).to(dtype)
    mant = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23}[dtype]
    sign = 1 << (31 if dtype == torch.float32 else 15)
    sub = [1, 2, 3, 1 << (mant - 1), (1 << mant) - 1]
    sub = np.array(sub + [b | sign for b in sub], dtype=np.uint32 if dtype == torch.float32 else np.uint16)
    sub = torch.from_numpy(sub.view(np.int32 if dtype == torch.float32 else np.int16).copy()).view(dtype)
    assert float(sub.to(torch.float64).abs().max()) < {torch.float16: 2.0 ** -14, torch.bfloat16: 2.0 ** -126, torch.float32: 2.0 ** -126}[dtype]
    return torch.cat([ties, (bits - 1).view(dtype), (bits + 1).view(dtype), other, sub])


def blocks(vals, cols=32):
    """every value as an 8 x 8 block of a grey picture: one level of one value moves its block's DC by 8 quantiser steps at q = 100"""
    n = -(-vals.numel() // cols) * cols
    v = torch.cat([vals, torch.zeros(n - vals.numel(), dtype=vals.dtype)]).reshape(-1, cols)
    return v.repeat_interleave(8, 0).repeat_interleave(8, 1).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_special_values(ica, gpu_ctx, dtype):
    """scale 1, bias 0: ties to even, their neighbours, -0.0, both clamps, +-Inf, NaN and the subnormals, each filling a block"""
    vals = special_values(dtype)
    assert vals.numel() > {torch.float16: 900, torch.bfloat16: 400, torch.float32: 900}[dtype]
    one, zero = np.ones(1, np.float32), np.zeros(1, np.float32)
    want = dm.denorm(dm.widen(vals), one[0], zero[0])
    assert {0, 1, 2, 127, 128, 254, 255} <= set(want.tolist())
    x = blocks(vals)
    pic = dm.picture(dm.widen(x), one, zero)
    cv = ica.InConvert(code(ica, dtype), [1.0], [0.0])
    items = [(x.cuda(), "HWC", cv, 100, False, pic)]
    if dtype == torch.float16:  # its subnormals widen exactly: k * 2^-24 times 2^24 is k
        sub = torch.arange(1, 256, dtype=torch.int16).view(torch.float16)
        xs = blocks(sub)
        pics = dm.picture(dm.widen(xs), np.array([2.0 ** 24], np.float32), zero)
        assert np.array_equal(pics[::8, ::8].reshape(-1)[:255], np.arange(1, 256))
        items.append((xs.cuda(), "HWC", ica.InConvert(code(ica, dtype), [2.0 ** 24], [0.0]), 100, False, pics))
    run_slots(ica, gpu_ctx, items)


def test_no_fused_multiply_add(ica, gpu_ctx):
    """the host test's triples, three to a 1 x 1 float32 RGB picture (the pixel fills its block): the bytes exact arithmetic gives
    for two roundings, where a fused multiply-add would give another"""
    triples = dm.no_fma_triples()
    assert len(triples) >= 64
    triples = triples + triples[:(-len(triples)) % 3]
    items = []
    for i in range(0, len(triples), 3):
        tr = triples[i:i + 3]
        x = torch.tensor([[[float(t[0]) for t in tr]]], dtype=torch.float32)
        scale, bias = np.array([t[1] for t in tr], np.float32), np.array([t[2] for t in tr], np.float32)
        pic = np.array([[[t[3] for t in tr]]], np.uint8)
        fused = np.array([[[t[4] for t in tr]]], np.uint8)
        assert np.array_equal(dm.picture(dm.widen(x), scale, bias), pic)
        assert not np.array_equal(expect(ica, fused, 100, False)[0], expect(ica, pic, 100, False)[0])  # the units tell them apart
        cv = ica.InConvert(ica.MIJ_DT_F32, scale, bias)
        items.append((x.cuda(), "HWC", cv, 100, False, pic))
        items.append((x.permute(2, 0, 1).contiguous().cuda(), "CHW", cv, 100, False, pic))
    run_slots(ica, gpu_ctx, items)


@pytest.mark.parametrize("layout", ["CHW", "HWC"])
def test_round_trip_with_the_decoder(ica, golden, tenc, layout):
    """two small goldens decoded as normalised float16 / bfloat16 / float32 and encoded back equal encode() of their uint8 decode"""
    dec = ica.TensorDecoder()
    done = 0
    for name in golden.names[:24]:
        if golden.expect(name, 3)[0] != "ok":
            continue
        jpg = golden.jpg(name)
        u8, reasons = dec.decode([jpg], dtype=torch.uint8, layout=layout)
        if reasons[0] is not None:
            continue
        want = tenc.encode(u8, quality=90, layout=layout)
        for dtype in DTYPES:
            x, reasons = dec.decode([jpg], dtype=dtype, mean=dm.IM_MEAN, std=dm.IM_STD, layout=layout)
            assert reasons[0] is None
            assert tenc.encode_normalized(x, mean=dm.IM_MEAN, std=dm.IM_STD, quality=90, layout=layout) == want, (name, dtype)
        done += 1
        if done == 2:
            break
    dec.close()
    assert done == 2


def test_encode_normalized_front_end(ica, tenc):
    """TensorEncoder.encode_normalized: a slice of a larger [N, C, H, W] batch, a list of pictures of different sizes with a 2-D grey
    one, HWC with flip and optimised tables, 0..255 values under std = 1/255, and no mean / std (v / 255)"""
    rng = np.random.default_rng(300)
    batch = normalised(rng, (5, 40, 52, 3), 3, torch.float16, dm.IM_MEAN, dm.IM_STD)
    scale, bias = dm.scale_bias(3, dm.IM_MEAN, dm.IM_STD)
    view = batch.permute(0, 3, 1, 2).contiguous().cuda()[1:4, :, 3:36, 2:51]
    got = tenc.encode_normalized(view, mean=dm.IM_MEAN, std=dm.IM_STD, quality=90)
    host = batch[1:4, 3:36, 2:51, :]
    assert got == [expect(ica, dm.picture(dm.widen(host[i]), scale, bias), 90, False)[1] for i in range(3)]
    # no mean / std: the pictures hold v / 255; different sizes, a grey 2-D picture among them
    plain = [normalised(rng, s, 1, torch.bfloat16, (0.0,) * 4, (1.0,) * 4) for s in ((3, 9, 17), (24, 31), (1, 5, 5), (4, 8, 8))]
    s1, b1 = dm.scale_bias(4)
    want = [expect(ica, dm.picture(hwc(t, "CHW"), s1, b1), 95, False)[1] for t in plain]
    assert tenc.encode_normalized([t.cuda() for t in plain], quality=95) == want
    # HWC, flipped, optimised tables, 0..255 values
    raw = torch.from_numpy(rng.uniform(-20.0, 280.0, size=(2, 23, 37, 4)).astype(np.float32))
    s255, b255 = dm.scale_bias(4, None, [1 / 255] * 4)
    assert np.array_equal(s255, np.ones(4, np.float32))
    want = [expect(ica, dm.picture(raw[i].numpy(), s255, b255), 75, True, True)[1] for i in range(2)]
    assert tenc.encode_normalized(raw.cuda(), std=[1 / 255] * 4, quality=75, layout="HWC", flip_vertically=True, optimize=True) == want
    with pytest.raises(ValueError, match="uint8"):
        tenc.encode(raw.cuda(), layout="HWC")


def test_one_launch_mixes_every_slot_kind(ica, gpu_ctx):
    """host slots, uint8 device slots, float device slots of all three dtypes and the clone of a float slot in one launch"""
    rng = np.random.default_rng(400)
    enc = ica.Encoder(gpu_ctx, 16, 8 << 20, 8 << 20)
    enc.stream_reserve(4 << 20)
    keep, want = [], []
    for k in range(3):
        img = rng.integers(0, 256, size=(20 + k, 30 + k, 3), dtype=np.uint8)
        want.append((enc.add(img, 90, flip=k == 1), img, 90, k == 1))
        t = torch.from_numpy(img).cuda()
        keep.append(t)
        want.append((enc.add_device(in_tensor(ica, t, "HWC"), 95, k == 2), img, 95, k == 2))
        dtype = DTYPES[k]
        x = normalised(rng, (19 + k, 33 + k, 3), 3, dtype)
        cv, scale, bias = convert(ica, dtype, 3)
        pic = dm.picture(dm.widen(x), scale, bias)
        t = x.permute(2, 0, 1).contiguous().cuda()
        keep.append(t)
        s = enc.add_device_float(in_tensor(ica, t, "CHW"), cv, 90, k == 0)
        want.append((s, pic, 90, k == 0))
        if k == 1:
            want.append((enc.add_clone(s), pic, 90, False))
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == len(want)
    for (s, pic, q, flip) in want:
        du, jpg = expect(ica, pic, q, flip)
        assert np.array_equal(enc.fetch(s), du), s
        assert enc.stream(s)[0] == jpg, s
    enc.close()


def test_optimised_tables_on_a_float_slot(ica, gpu_ctx):
    rng = np.random.default_rng(500)
    x = normalised(rng, (48, 64, 3), 3, torch.float32)
    cv, scale, bias = convert(ica, torch.float32, 3)
    pic = dm.picture(dm.widen(x), scale, bias)
    t = x.cuda()
    enc = ica.Encoder(gpu_ctx, 2, 1 << 20, 1 << 20, stage_bytes=0)
    enc.stream_reserve(1 << 20)
    s = enc.add_device_float(in_tensor(ica, t, "HWC"), cv, 90)
    enc.set_optimize(s)
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == 1
    plan, du = ica.host_transform(pic, 90, False)
    assert np.array_equal(enc.fetch(s), du)
    assert enc.stream(s)[0] == ica.emit_jpeg(plan, du, True)
    enc.close()


def test_small_arena_falls_back_to_the_host(ica):
    """an arena that holds one stream: the others are finished on the host, the bytes are the same, the next call needs none"""
    rng = np.random.default_rng(600)
    x = normalised(rng, (6, 64, 96, 3), 3, torch.bfloat16)
    scale, bias = dm.scale_bias(3, MEAN4[:3], STD4[:3])
    want = [expect(ica, dm.picture(dm.widen(x[i]), scale, bias), 90, False)[1] for i in range(6)]
    t = x.permute(0, 3, 1, 2).contiguous().cuda()
    te = ica.TensorEncoder()
    te.reserve_arena(len(want[0]) + 100)
    assert te.encode_normalized(t, mean=MEAN4[:3], std=STD4[:3], quality=90) == want
    assert te.last_host_emitted > 0
    assert te.encode_normalized(t, mean=MEAN4[:3], std=STD4[:3], quality=90) == want
    assert te.last_host_emitted == 0
    te.close()


def test_refusals_at_the_c_level(ica, gpu_ctx):
    """MIJ_DT_U8 and unknown dtypes, a misaligned src, a scale or bias that is not finite, an extent past the allocation counted in
    elements of the dtype: MIJ_E_ARG each, and the encoder goes on working"""
    enc = ica.Encoder(gpu_ctx, 16, 1 << 20, 1 << 20, stage_bytes=0)
    enc.stream_reserve(1 << 20)
    L = ica.lib()
    L.mij_enc_add_device_float.argtypes = [C.c_void_p, C.POINTER(ica.InTensor), C.POINTER(ica.InConvert), C.c_int, C.c_int]
    L.mij_last_error.restype = C.c_char_p
    paths = {ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    dp = C.c_void_p()
    nbytes = 3 * 48 * 64 * 2  # exactly one float16 CHW picture: torch's allocator would hand out a larger block
    assert hip.hipMalloc(C.byref(dp), nbytes) == 0 and hip.hipMemset(dp, 0, nbytes) == 0
    p = dp.value
    CHW, HWC = ica.MIJ_LAYOUT_CHW, ica.MIJ_LAYOUT_HWC
    F16, BF16, F32 = ica.MIJ_DT_F16, ica.MIJ_DT_BF16, ica.MIJ_DT_F32
    inf, nan = float("inf"), float("nan")

    def add(ptr, layout, w, h, c, rp, pp, dt, scale=(1.0, 1.0, 1.0, 1.0), bias=(7.0, 8.0, 9.0, 0.0)):
        cv = ica.InConvert(dt, scale, bias)
        return L.mij_enc_add_device_float(enc._h, C.byref(ica.InTensor(ptr, layout, w, h, c, rp, pp)), C.byref(cv), 100, 0)

    good = add(p, CHW, 64, 48, 3, 64, 64 * 48, F16)  # ends exactly at the end of the allocation
    assert good >= 0
    assert add(p, CHW, 64, 48, 3, 64, 64 * 48, BF16) >= 0
    assert add(p, CHW, 64, 48, 3, 64, 64 * 48, F32) == MIJ_E_ARG      # the same elements at 4 bytes each leave the allocation
    assert add(p, CHW, 64, 24, 3, 64, 64 * 24, F32) >= 0              # half the rows fit exactly
    assert add(p, CHW, 64, 24, 3, 64, 64 * 24 + 1, F32) == MIJ_E_ARG  # one element further per plane
    assert add(p + 2, CHW, 64, 48, 3, 64, 64 * 48, F16) == MIJ_E_ARG  # one element past the end
    assert add(p, CHW, 64, 48, 3, 65, 65 * 48, F16) == MIJ_E_ARG      # rows past the end
    assert add(p, HWC, 64, 48, 3, 64 * 3, 0, F16) >= 0
    assert add(p, CHW, 64, 48, 3, 64, 64 * 48, ica.MIJ_DT_U8) == MIJ_E_ARG and b"mij_enc_add_device" in L.mij_last_error()
    assert add(p, CHW, 64, 48, 3, 64, 64 * 48, 4) == MIJ_E_ARG and add(p, CHW, 64, 48, 3, 64, 64 * 48, -1) == MIJ_E_ARG
    assert add(p + 1, CHW, 32, 24, 3, 64, 64 * 48, F16) == MIJ_E_ARG and b"aligned" in L.mij_last_error()  # inside, but on an odd byte
    assert add(p + 2, CHW, 32, 24, 3, 64, 64 * 24, F32) == MIJ_E_ARG and b"aligned" in L.mij_last_error()
    assert add(p + 2, CHW, 32, 24, 3, 64, 64 * 48, F16) >= 0                                               # an element in: fine
    for bad in (inf, -inf, nan):
        assert add(p, CHW, 64, 48, 3, 64, 64 * 48, F16, scale=(1.0, bad, 1.0, 1.0)) == MIJ_E_ARG and b"finite" in L.mij_last_error()
        assert add(p, CHW, 64, 48, 3, 64, 64 * 48, F16, bias=(0.0, 0.0, bad, 0.0)) == MIJ_E_ARG
        assert add(p, CHW, 64, 48, 3, 64, 64 * 48, F16, scale=(1.0, 1.0, 1.0, bad)) >= 0  # beyond comp: never read
        assert add(p, HWC, 64, 48, 1, 64, 0, F16, bias=(0.0, bad, bad, bad)) >= 0
    assert add(p, 7, 64, 48, 3, 64, 64 * 48, F16) == MIJ_E_ARG        # the checks of mij_enc_add_device
    assert add(p, CHW, 64, 48, 3, 63, 64 * 48, F16) == MIJ_E_ARG
    assert add(0, CHW, 64, 48, 3, 64, 64 * 48, F16) == MIJ_E_ARG
    assert add(np.zeros(3 * 48 * 64, np.float16).ctypes.data, CHW, 64, 48, 3, 64, 64 * 48, F16) == MIJ_E_ARG  # host memory
    # the encoder is as usable as before: the zeros of the first slot are its biases
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() > good
    pic = np.broadcast_to(np.array([7, 8, 9], np.uint8), (48, 64, 3))
    du, jpg = expect(ica, pic, 100, False)
    assert np.array_equal(enc.fetch(good), du) and enc.stream(good)[0] == jpg
    enc.close()
    assert hip.hipFree(dp) == 0
