"""libjpeg's arithmetic in the GPU encoder (mij_enc_set_arith, k_lj_enc_color, k_lj_encode_planes; TensorEncoder's arithmetic=): Pillow's
files (tests/golden/libjpeg_pillow_enc.npz) byte for byte through host and device pixels, with and without an emission arena; the host
twin (include/mij_host.h, LIBJPEG ENCODING) at the strip seams; float and plane input; mixed batches; an encoder without a request;
the state and refusal codes."""
import ctypes as C

import numpy as np
import pytest
import torch

import libjpeg_enc_model as EM
from test_encode_libjpeg_host import KINDS, load_goldens, parse

pytestmark = pytest.mark.gpu

MIJ_E_ARG, MIJ_E_STATE = -2, -5
STB, LIBJPEG = 0, 1
STRIP = {"444": 64, "422": 64, "420": 32, "grey": 256}  # MCUs per work item of k_lj_encode_planes
MCU_W = {"444": 8, "422": 16, "420": 16, "grey": 8}
# the kernel table's groups (mij_enc_group_work)
G_420, G_444, G_422, G_GREY, G_P444 = 4, 5, 6, 8, 9
G_LJC = {"444": 14, "422": 15, "420": 16, "grey": 17}
G_LJ = {"444": 18, "422": 19, "420": 20, "grey": 21}


@pytest.fixture(scope="module")
def goldens():
    return load_goldens()


@pytest.fixture(scope="module")
def tenc(ica, gpu_ctx):
    e = ica.TensorEncoder()
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def options(enc, slot, kind, mcu_x):
    if kind == "o":
        enc.set_optimize(slot)
    elif kind == "p":
        enc.set_progressive(slot)
    elif kind == "r":
        enc.set_restart(slot, mcu_x)


def finish(ica, enc, slot, kind):
    """a slot's stream without an emission arena: the units through the host emission, in libjpeg's framing"""
    t = enc.tplan(slot)
    data = ica.emit_transcoded(t, enc.fetch(slot), kind == "o", restart_mcus=enc.slot_restart(slot), progressive=kind == "p")
    return ica.libjpeg_reframe(data)


def picture(w, h, seed, comp=3):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    base = np.stack([(x * 7 + y * 3) % 256, (x * 2 + y * 11) % 256, (x * y) % 256], -1)
    a = np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)
    return a if comp == 3 else np.ascontiguousarray(a[..., 0])


@pytest.mark.parametrize("arena", [True, False])
@pytest.mark.parametrize("where", ["host", "device"])
def test_every_golden_is_pillows_file(ica, gpu_ctx, goldens, where, arena):
    """every golden through Encoder: host and device pixels, with and without an emission arena"""
    cases = [g for g in goldens if not parse(g[0])[3]]
    enc = ica.Encoder(gpu_ctx, len(cases), 8 << 20, 16 << 20)
    if arena:
        enc.stream_reserve(8 << 20)
    slots, keep = [], []
    for name, src, jpg in cases:
        sampling, quality, kind, _ = parse(name)
        h, w = src.shape[:2]
        if where == "host":
            slot = enc.add(src, quality, sampling=sampling)
        else:
            d = dev(src)
            keep.append(d)
            comp = 1 if src.ndim == 2 else 3
            slot = enc.add_device(ica.InTensor(d.data_ptr(), ica.MIJ_LAYOUT_HWC, w, h, comp, w * comp, 0), quality, sampling=sampling)
        enc.set_arith(slot, "libjpeg")
        assert enc.slot_arith(slot) == LIBJPEG
        options(enc, slot, kind, enc.tplan(slot).plan.mcu_x)
        slots.append((slot, name, jpg, kind))
    torch.cuda.synchronize()
    enc.upload()
    enc.launch()
    if arena:
        assert enc.fetch_streams() == len(slots)
    else:
        enc.wait()
    bad = []
    for slot, name, jpg, kind in slots:
        data = bytes(enc.stream(slot)[0]) if arena else finish(ica, enc, slot, kind)
        if data != jpg:
            bad.append(name)
    enc.close()
    assert not bad, "%d of %d differ from Pillow's files: %s" % (len(bad), len(slots), bad[:8])


@pytest.mark.parametrize("sampling", ["444", "422", "420", "grey"])
def test_strip_seams_equal_the_host_twin(ica, gpu_ctx, sampling):
    """widths of STRIP MCUs - 1, + 0 and + 1 pixels: the last work item full, and one MCU into the next; units and bytes"""
    enc = ica.Encoder(gpu_ctx, 8, 8 << 20, 8 << 20)
    enc.stream_reserve(4 << 20)
    want = []
    for k, dw in enumerate((-1, 0, 1)):
        w, h = STRIP[sampling] * MCU_W[sampling] + dw, 11
        img = picture(w, h, 31 * k + w, 1 if sampling == "grey" else 3)
        slot = enc.add(img, 85, sampling=sampling)
        enc.set_arith(slot, LIBJPEG)
        t, du = ica.host_transform_libjpeg(img, 85, sampling)
        want.append((slot, du, ica.write_jpg_libjpeg_to_memory(img, 85, sampling), w))
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == len(want)
    for slot, du, data, w in want:
        assert np.array_equal(enc.fetch(slot), du), (sampling, w)
        assert bytes(enc.stream(slot)[0]) == data, (sampling, w)
    enc.close()


def test_strips_cross_row_ends_next_to_dummies(ica, gpu_ctx):
    """a 3-MCU-wide, many-row 4:2:0 picture with a dummy column and a dummy row: a strip of 32 MCUs runs over ten row ends"""
    enc = ica.Encoder(gpu_ctx, 4, 4 << 20, 4 << 20)
    want = []
    for (w, h) in ((40, 16 * 23 + 8), (33, 16 * 22 + 1), (48, 16 * 11 + 7)):
        assert -(-w // 16) == 3
        img = picture(w, h, w + h)
        slot = enc.add(img, 75, sampling="420")
        enc.set_arith(slot, LIBJPEG)
        want.append((slot, ica.host_transform_libjpeg(img, 75, "420")[1], EM.units(img, "420", 75), (w, h)))
    enc.upload()
    enc.launch()
    enc.wait()
    for slot, du, model, what in want:
        assert np.array_equal(du, model), what
        assert np.array_equal(enc.fetch(slot), du), what
    enc.close()


@pytest.mark.parametrize("layout", ["CHW", "HWC"])
def test_tensor_encoder_equals_pillow(ica, tenc, goldens, layout):
    """TensorEncoder.encode(arithmetic="libjpeg"): the plain goldens of every colour sampling in one call, the options per call"""
    plain = [g for g in goldens if parse(g[0])[2] == "b" and parse(g[0])[0] not in ("grey",) and not parse(g[0])[3]]
    imgs = [dev(src).permute(2, 0, 1).contiguous() if layout == "CHW" else dev(src) for _, src, _ in plain]
    by_q = {}
    for k, (name, _, _) in enumerate(plain):
        by_q.setdefault(parse(name)[1], []).append(k)
    for q, ks in by_q.items():
        got = tenc.encode([imgs[k] for k in ks], quality=q, layout=layout, subsampling=[parse(plain[k][0])[0] for k in ks], arithmetic="libjpeg")
        assert got == [plain[k][2] for k in ks], q
        assert tenc.last_arithmetic == ["libjpeg"] * len(ks)
    for name, src, jpg in goldens:
        sampling, q, kind, ycbcr = parse(name)
        if kind == "b" or ycbcr:
            continue
        t = dev(src) if src.ndim == 2 else (dev(src).permute(2, 0, 1).contiguous() if layout == "CHW" else dev(src))
        assert tenc.encode([t], quality=q, layout=layout, subsampling=sampling, arithmetic="libjpeg", **KINDS[kind]) == [jpg], name
    # no subsampling: libjpeg's "420", not the writer's choice for the quality
    name, src, jpg = next(g for g in goldens if g[0].startswith("420_24x24_"))
    q = parse(name)[1]
    t = dev(src).permute(2, 0, 1).contiguous() if layout == "CHW" else dev(src)
    assert tenc.encode([t], quality=q, layout=layout, arithmetic="libjpeg") == [jpg] and tenc.last_subsampling == ["420"]
    assert tenc.encode([t], quality=95, layout=layout, arithmetic="libjpeg") == [ica.write_jpg_libjpeg_to_memory(src, 95, "420")]


def test_small_arena_finishes_on_the_host(ica, goldens):
    """slots that do not fit the arena come back through the host emission in libjpeg's framing"""
    e = ica.TensorEncoder()
    cases = [g for g in goldens if g[0].startswith(("420_97x61_", "422_160x120_", "444_97x61_"))]
    for name, src, jpg in cases:
        sampling, q, kind, _ = parse(name)
        assert len(jpg) > 512  # even the header is longer
        e.reserve_arena(512)  # a miss grows it: set again for every call
        assert e.encode([dev(src)], quality=q, layout="HWC", subsampling=sampling, arithmetic="libjpeg", **KINDS[kind]) == [jpg], name
        assert e.last_host_emitted == 1, name
    assert len(cases) >= 9
    e.close()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_encode_normalized_equals_encode(ica, tenc, dtype):
    """a decoded float batch (v / 255) gives the bytes of its uint8 pictures"""
    imgs = [dev(picture(w, h, w)).permute(2, 0, 1).contiguous() for (w, h) in ((33, 31), (40, 24), (97, 61))]
    floats = [(t.to(torch.float32) / 255.0).to(dtype) for t in imgs]
    for kw in ({}, {"subsampling": "444", "optimize": True}, {"subsampling": "422", "restart_rows": 1}):
        want = tenc.encode(imgs, quality=75, arithmetic="libjpeg", **kw)
        assert tenc.encode_normalized(floats, quality=75, arithmetic="libjpeg", **kw) == want, kw
        assert want == [ica.write_jpg_libjpeg_to_memory(t.permute(1, 2, 0).cpu().numpy(), 75, kw.get("subsampling"), optimize=kw.get("optimize", False),
                                                        restart_rows=kw.get("restart_rows")) for t in imgs]


def test_encode_ycbcr_equals_the_ycbcr_and_grey_goldens(ica, tenc, goldens):
    seen = 0
    for name, src, jpg in goldens:
        sampling, q, kind, ycbcr = parse(name)
        if ycbcr:
            pic = tuple(dev(src[..., c]) for c in range(3))
        elif sampling == "grey":
            pic = dev(src)
        else:
            continue
        assert tenc.encode_ycbcr([pic], subsampling=sampling, quality=q, arithmetic="libjpeg", **KINDS[kind]) == [jpg], name
        seen += 1
    assert seen >= 14 and tenc.last_arithmetic == ["libjpeg"]


def test_encode_ycbcr_of_the_models_planes_equals_the_rgb_scan(ica, tenc, goldens):
    """4:2:0 planes made by the model's colour conversion and filter give the RGB golden's bytes: whole-MCU widths, where extending each
    plane by its last column is extending the pixels'"""
    seen = 0
    for name, src, jpg in goldens:
        if not name.startswith(("420_16x16_", "420_160x120_", "420_8x8_", "420_24x24_")):
            continue
        h, w = src.shape[:2]
        if w % 16:
            continue
        ycc = EM.rgb_to_ycc(src)
        rows = -(-h // 2) * 2
        planes = [ycc[0].astype(np.uint8)] + [EM.downsample(EM._extend(ycc[c], rows, w), 2, 2).astype(np.uint8) for c in (1, 2)]
        got = tenc.encode_ycbcr([tuple(dev(p) for p in planes)], subsampling="420", quality=parse(name)[1], arithmetic="libjpeg")
        sos = jpg.index(b"\xff\xda")
        assert got[0][got[0].index(b"\xff\xda"):] == jpg[sos:] and got == [jpg], name
        seen += 1
    assert seen == 2


def test_mixed_batches_each_by_its_own_judge(ica, tenc, gpu_ctx, goldens, oracle):
    plain = [g for g in goldens if g[0].startswith(("420_33x31_", "444_17x15_", "422_40x24_", "420_97x61_"))]
    plain = [g for g in plain if parse(g[0])[2] == "b"]
    assert len(plain) == 4
    enc = ica.Encoder(gpu_ctx, 16, 4 << 20, 8 << 20)
    enc.stream_reserve(4 << 20)
    slots = []
    for name, src, jpg in plain:
        sampling, q, _, _ = parse(name)
        a = enc.add(src, q, sampling=sampling)
        enc.set_arith(a, LIBJPEG)
        slots.append((a, jpg))
        slots.append((enc.add(src, q, sampling=sampling), ica.write_jpg_sampled_to_memory(src, q, sampling)))
        slots.append((enc.add(src, q), oracle.encode(src, q)))
        c = enc.add_clone(a)  # a clone inherits the request
        assert enc.slot_arith(c) == LIBJPEG
        slots.append((c, jpg))
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == len(slots)
    for slot, want in slots:
        assert bytes(enc.stream(slot)[0]) == want, slot
    enc.close()
    imgs = [dev(src).permute(2, 0, 1).contiguous() for _, src, _ in plain]
    ar = ["libjpeg", "stb", "libjpeg", "stb"]
    got = tenc.encode(imgs, quality=75, subsampling="420", arithmetic=ar)
    assert tenc.last_arithmetic == ar
    for k, (name, src, _) in enumerate(plain):
        want = ica.write_jpg_libjpeg_to_memory(src, 75, "420") if ar[k] == "libjpeg" else ica.write_jpg_sampled_to_memory(src, 75, "420")
        assert got[k] == want, name


def test_no_request_queues_what_it_queued_before(ica, gpu_ctx, oracle):
    """the kernels, work items and bytes of an encoder without a request; and of the stb slots beside a libjpeg slot"""
    imgs = [(picture(97, 61, 1), 90, None), (picture(97, 61, 2), 95, None), (picture(40, 24, 3), 75, "422"), (picture(33, 31, 4, 1), 75, "grey")]
    want_work = [0] * ica.ENC_GROUPS
    want_work[G_420], want_work[G_444], want_work[G_422], want_work[G_GREY] = 1, 2, 1, 1  # 28 MCUs of 32; 104 of 64; 9 of 32; 20 of 256
    for with_lj in (False, True):
        enc = ica.Encoder(gpu_ctx, 8, 4 << 20, 8 << 20)
        enc.stream_reserve(4 << 20)
        slots = [(enc.add(img, q, sampling=sm), oracle.encode(img, q) if sm is None else ica.write_jpg_sampled_to_memory(img, q, sm))
                 for img, q, sm in imgs]
        work = list(want_work)
        if with_lj:
            s = enc.add(imgs[0][0], 90, sampling="420")
            enc.set_arith(s, LIBJPEG)
            slots.append((s, ica.write_jpg_libjpeg_to_memory(imgs[0][0], 90, "420")))
            work[G_LJC["420"]], work[G_LJ["420"]] = 4 * 8, 1  # 32 rows of cells; 28 MCUs of 32
        enc.upload()
        assert enc.group_work() == work, with_lj
        enc.launch()
        assert enc.fetch_streams() == len(slots)
        for slot, want in slots:
            assert bytes(enc.stream(slot)[0]) == want, (with_lj, slot)
        enc.close()


def test_plane_slot_runs_pass_two_only(ica, gpu_ctx, goldens):
    name, src, jpg = next(g for g in goldens if g[0].startswith("ycc444_"))
    planes = tuple(np.ascontiguousarray(src[..., c]) for c in range(3))
    enc = ica.Encoder(gpu_ctx, 4, 1 << 20, 1 << 20)
    enc.stream_reserve(1 << 20)
    a = enc.add_planes(planes, "444", parse(name)[1])
    enc.set_arith(a, LIBJPEG)
    b = enc.add_planes(planes, "444", parse(name)[1])
    enc.upload()
    work = enc.group_work()
    assert work[G_LJ["444"]] == 1 and work[G_P444] == 1 and sum(work) == 2
    enc.launch()
    assert enc.fetch_streams() == 2
    assert bytes(enc.stream(a)[0]) == jpg
    assert bytes(enc.stream(b)[0]) == ica.write_jpg_planes_to_memory(planes, "444", parse(name)[1])
    enc.close()


def test_state_and_refusal_codes(ica, gpu_ctx):
    L = ica.lib()
    L.mij_enc_set_arith.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.mij_enc_slot_arith.argtypes = [C.c_void_p, C.c_int]
    enc = ica.Encoder(gpu_ctx, 16, 1 << 20, 1 << 20)
    rgb, grey = picture(16, 16, 1), picture(16, 16, 2, 1)
    s = enc.add(rgb, 90)
    assert L.mij_enc_slot_arith(enc._h, s) == STB
    assert L.mij_enc_set_arith(enc._h, s, 2) == MIJ_E_ARG and L.mij_enc_set_arith(enc._h, 99, LIBJPEG) == MIJ_E_ARG
    assert L.mij_enc_slot_arith(enc._h, 99) == MIJ_E_ARG
    assert L.mij_enc_set_arith(enc._h, s, LIBJPEG) == 0 and L.mij_enc_slot_arith(enc._h, s) == LIBJPEG
    assert L.mij_enc_set_arith(enc._h, s, STB) == 0 and L.mij_enc_slot_arith(enc._h, s) == STB
    assert L.mij_enc_set_arith(enc._h, enc.add(rgb, 90, sampling="440"), LIBJPEG) == MIJ_E_ARG
    for comp in (2, 4):
        px = np.zeros((16, 16, comp), np.uint8)
        assert L.mij_enc_set_arith(enc._h, enc.add(px, 90, sampling="444"), LIBJPEG) == MIJ_E_ARG, comp
        assert L.mij_enc_set_arith(enc._h, enc.add(px, 90, sampling="grey"), LIBJPEG) == MIJ_E_ARG, comp
    assert L.mij_enc_set_arith(enc._h, enc.add(grey, 90, sampling="grey"), LIBJPEG) == 0
    t, du = ica.host_transform_sampled(rgb, 90)
    u = enc.add_units(16, 16, 3, 90, du)
    assert L.mij_enc_set_arith(enc._h, u, LIBJPEG) == MIJ_E_ARG and L.mij_enc_set_arith(enc._h, u, STB) == 0
    y = np.zeros((16, 16), np.uint8)
    assert L.mij_enc_set_arith(enc._h, enc.add_planes((y, y[:8], y[:8]), "440"), LIBJPEG) == MIJ_E_ARG
    assert L.mij_enc_set_arith(enc._h, enc.add_planes((y, y[:8, :8], y[:8, :8]), "420"), LIBJPEG) == 0
    enc.upload()
    assert L.mij_enc_set_arith(enc._h, s, LIBJPEG) == MIJ_E_STATE and L.mij_enc_set_arith(enc._h, s, STB) == MIJ_E_STATE
    enc.reset()  # forgets every request
    s = enc.add(rgb, 90)
    assert L.mij_enc_slot_arith(enc._h, s) == STB
    enc.close()


def test_coefficient_slots_refuse(ica, gpu_ctx):
    L = ica.lib()
    L.mij_enc_set_arith.argtypes = [C.c_void_p, C.c_int, C.c_int]
    data = ica.synth_jpeg(32, 32, seed=3, quality=90)
    b = ica.Batch(gpu_ctx, 1, 1 << 20, 1 << 20, 1 << 20)
    ok, slots, _ = b.decode_jpegs([data], 3, threads=1)
    assert ok == 1
    b.upload()
    enc = ica.Encoder(gpu_ctx, 2, 1 << 20, 1 << 20)
    c = enc.add_coef(b, slots[0])
    assert L.mij_enc_set_arith(enc._h, c, LIBJPEG) == MIJ_E_ARG
    enc.close()
    b.close()


def test_argument_errors(ica, tenc):
    t = dev(picture(16, 16, 1)).permute(2, 0, 1).contiguous()
    for bad in ("turbo", None, 1, ["libjpeg", "stb"], ["libjpeg", 3]):
        with pytest.raises(ValueError):
            tenc.encode([t], arithmetic=bad)
    with pytest.raises(ValueError):
        tenc.encode([t], subsampling="440", arithmetic="libjpeg")
    with pytest.raises(ValueError):
        tenc.encode([torch.zeros((4, 16, 16), dtype=torch.uint8, device="cuda")], arithmetic="libjpeg")
    with pytest.raises(ValueError):
        tenc.encode_ycbcr([(t[0], t[1, :8], t[2, :8])], subsampling="440", arithmetic="libjpeg")
    assert tenc.encode([], arithmetic="libjpeg") == [] and tenc.last_arithmetic == []
