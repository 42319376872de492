"""Plane encoding on the GPU (mij_enc_add_planes, mij_enc_add_device_planes, k_enc_gather_planes, k_encode_planes<LH, LV>;
TensorEncoder.encode_ycbcr): the units and the streams of the host twin (include/mij_host.h, PLANE ENCODING) bit for bit, through
views, emission options, a small arena, the video-range conversion and a round trip through the decoder."""
import ctypes as C

import numpy as np
import pytest
import torch

import planes_cases as pc
import sampling_cases as sc

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def triples(planes):
    return [(t.data_ptr(), t.stride(0) if t.shape[0] > 1 else 0, t.stride(1) if t.shape[1] > 1 else 1) for t in planes]


def twin(ica, pl, name, q=90, **kw):
    data = ica.write_jpg_planes_to_memory(pc.arg(pl), name, q, **kw)
    assert data is not None
    return data


@pytest.fixture(scope="module")
def tenc(ica, gpu_ctx):
    e = ica.TensorEncoder()
    yield e
    e.close()


@pytest.mark.parametrize("name", pc.SAMPLINGS)
@pytest.mark.parametrize("q", [50, 95])
def test_units_equal_the_hosts(ica, gpu_ctx, name, q):
    """1: mij_enc_fetch of host-pointer slots and of device slots equals mjw_ptransform_host, at every size and at the strip seam, plain,
    flipped and range-converted"""
    enc = ica.Encoder(gpu_ctx, 64, 4 << 20, 8 << 20)
    want, keep = [], []
    for k, (w, h) in enumerate(pc.sizes(name)):
        pl = pc.planes(w, h, name, 13 * k + q)
        for flip, vr in ((False, False), (True, True)):
            t, du = ica.host_transform_planes(pc.arg(pl), name, q, flip=flip, video_range=vr)
            d = [dev(p) for p in pl]
            keep.append(d)
            a = enc.add_planes(pc.arg(pl), name, q, flip=flip, video_range=vr)
            b = enc.add_device_planes(triples(d), w, h, name, q, flip=flip, video_range=vr)
            want += [(a, du, (w, h, flip, "host")), (b, du, (w, h, flip, "device"))]
            assert enc.plane_bytes(w, h, name) == -(-t.du_elems() // 256) * 256
    torch.cuda.synchronize()
    enc.upload()
    enc.launch()
    enc.wait()
    for slot, du, what in want:
        got = enc.fetch(slot)
        assert got.shape == du.shape and np.array_equal(got, du), (name, q, what)
        t = enc.tplan(slot)
        assert (t.ncomp, t.lh, t.lv) == pc.FACTORS[name]
    enc.close()


def device_views(pl):
    """the views of planes_cases.views as device tensors, built on the device"""
    out = {}
    cut = []
    for p in pl:
        big = torch.randint(0, 256, (p.shape[0] + 5, p.shape[1] + 9), dtype=torch.uint8, device="cuda")
        big[2:2 + p.shape[0], 3:3 + p.shape[1]] = dev(p)
        cut.append(big[2:2 + p.shape[0], 3:3 + p.shape[1]])
    out["cut"] = cut
    out["flipped"] = [dev(p[::-1]) for p in pl]
    if len(pl) == 3:
        nv12 = torch.stack([dev(pl[1]), dev(pl[2])], dim=-1)
        out["nv12"] = (dev(pl[0]), nv12)
        nv21 = nv12.flip(-1).contiguous()
        out["nv21_flip"] = (dev(pl[0]), nv21.flip(-1))  # a copy in NV12 order
        out["nv21_slices"] = (dev(pl[0]), nv21[:, :, 1], nv21[:, :, 0])
        if pl[1].shape == pl[0].shape:
            hwc = torch.stack([dev(p) for p in pl], dim=-1)
            out["packed"] = tuple(hwc[:, :, k] for k in range(3))
    return out


@pytest.mark.parametrize("name", pc.SAMPLINGS)
def test_views_on_device_tensors(ica, tenc, name):
    """2: NV12, NV21, pitched rows, planes cut out of larger tensors, packed HWC and flip_vertically give the host twin's streams"""
    for (w, h) in ((17, 9), (33, 18)):
        pl = pc.planes(w, h, name, w)
        want = twin(ica, pl, name, 80)
        for what, pic in device_views(pl).items():
            pic = pic[0] if name == "grey" else pic
            got = tenc.encode_ycbcr([pic], subsampling=name, quality=80, flip_vertically=what == "flipped")
            assert got == [want], (name, what, w, h)
    if name == "444":
        batch = torch.stack([torch.stack([dev(p) for p in pc.planes(24, 16, "444", s)]) for s in range(3)])
        assert tenc.encode_ycbcr(batch, subsampling="444") == [twin(ica, pc.planes(24, 16, "444", s), "444") for s in range(3)]


def test_streams_equal_the_host_twin(ica, tenc, gpu_ctx, oracle):
    """3: encode_ycbcr against mjh_write_jpg_planes_to_memory byte for byte: every sampling at every size, one call of mixed samplings
    and sizes, and one upload that holds plane slots and RGB pixel slots, whose RGB streams are still the oracle's"""
    for name in pc.SAMPLINGS:
        pls = [pc.planes(w, h, name, 7 * k + 2) for k, (w, h) in enumerate(pc.sizes(name))]
        got = tenc.encode_ycbcr([pc.arg([dev(p) for p in pl]) for pl in pls], subsampling=name, quality=75)
        assert got == [twin(ica, pl, name, 75) for pl in pls], name
        assert tenc.last_subsampling == [name] * len(pls)
    mixed = [("420", 33, 17), ("grey", 9, 17), ("444", 40, 24), ("422", 17, 9), ("440", 7, 5), ("420", 1, 1)]
    pls = [pc.planes(w, h, name, k) for k, (name, w, h) in enumerate(mixed)]
    got = tenc.encode_ycbcr([pc.arg([dev(p) for p in pl]) for pl in pls], subsampling=[m[0] for m in mixed], qtables=sc.random_tables(8))
    assert got == [twin(ica, pl, m[0], qtables=sc.random_tables(8)) for pl, m in zip(pls, mixed)]
    assert tenc.last_subsampling == [m[0] for m in mixed]

    enc = ica.Encoder(gpu_ctx, 16, 4 << 20, 4 << 20)
    enc.stream_reserve(4 << 20)
    slots, keep = [], []
    for k, (name, w, h) in enumerate(mixed[:4]):
        img = sc.picture(w + 3, h + 2, 3, 50 + k)
        q = (50, 95)[k & 1]
        slots.append((enc.add(img, q), oracle.encode(img, q)))
        d = [dev(p) for p in pls[k]]
        keep.append(d)
        slots.append((enc.add_device_planes(triples(d), w, h, name, q), twin(ica, pls[k], name, q)))
        slots.append((enc.add_planes(pc.arg(pls[k]), name, q), twin(ica, pls[k], name, q)))
    torch.cuda.synchronize()
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == len(slots)
    for slot, want in slots:
        data, n = enc.stream(slot)
        assert data is not None and bytes(data) == want, slot
    enc.close()


@pytest.mark.parametrize("name", ["420", "422", "grey"])
def test_emission_composes(ica, tenc, name):
    """4: optimised tables, both restart forms and progressive scans equal the host twin's bytes"""
    pls = [pc.planes(w, h, name, 3 * k) for k, (w, h) in enumerate(((40, 24), pc.SEAM_SIZE[name]))]
    pics = [pc.arg([dev(p) for p in pl]) for pl in pls]
    for kw in ({"optimize": True}, {"restart_mcus": 1}, {"restart_rows": 1}, {"restart_mcus": 5, "optimize": True}, {"progressive": True}):
        got = tenc.encode_ycbcr(pics, subsampling=name, quality=75, **kw)
        assert got == [twin(ica, pl, name, 75, **kw) for pl in pls], (name, kw)
    tenc.encode_ycbcr(pics, subsampling=name, restart_rows=1)
    assert tenc.last_restarts == [ica.planes_plan(pl[0].shape[1], pl[0].shape[0], name).plan.mcu_x for pl in pls]
    with pytest.raises(ValueError):
        tenc.encode_ycbcr(pics, subsampling=name, restart_mcus=1, progressive=True)


def test_clone_of_a_plane_slot(ica, gpu_ctx):
    """mij_enc_add_clone of a device and of a host plane slot: the same units"""
    pl = pc.planes(33, 17, "420", 6)
    enc = ica.Encoder(gpu_ctx, 4, 1 << 20, 1 << 20)
    d = [dev(p) for p in pl]
    a = enc.add_device_planes(triples(d), 33, 17, "420", 80)
    b = enc.add_clone(a)
    c = enc.add_clone(enc.add_planes(pc.arg(pl), "420", 80))
    torch.cuda.synchronize()
    enc.upload()
    enc.launch()
    enc.wait()
    _, du = ica.host_transform_planes(pc.arg(pl), "420", 80)
    for slot in (a, b, c):
        assert np.array_equal(enc.fetch(slot), du), slot
    enc.close()


def test_small_arena_is_finished_on_the_host(ica, gpu_ctx):
    """5: an emission arena too small for one slot: the slot is finished on the host from its units, with the same bytes"""
    e = ica.TensorEncoder()
    pls = [pc.planes(200, 120, name, 5) for name in ("420", "grey", "444")]
    names = ["420", "grey", "444"]
    pics = [pc.arg([dev(p) for p in pl]) for pl in pls]
    want = [twin(ica, pl, name, 90) for pl, name in zip(pls, names)]
    e.reserve_arena(len(want[0]) + len(want[1]) + 64)
    assert e.encode_ycbcr(pics, subsampling=names) == want
    assert e.last_host_emitted == 1
    assert e.encode_ycbcr(pics, subsampling=names, progressive=True) == [twin(ica, pl, name, 90, progressive=True) for pl, name in zip(pls, names)]
    e.close()


@pytest.mark.parametrize("name", pc.SAMPLINGS)
def test_video_range_on_the_gpu(ica, tenc, name):
    """6: video_range=True equals the host twin, on planes that hold every value 0..255 and through strided views"""
    every = np.arange(256, dtype=np.uint8).reshape(16, 16)
    shapes = pc.shapes(32, 32, name)
    pl = [np.ascontiguousarray(np.tile(every.T if k else every, (2, 2))[:s[0], :s[1]]) for k, s in enumerate(shapes)]
    assert all(len(np.unique(p)) == 256 for p in pl)
    want = twin(ica, pl, name, 85, video_range=True)
    assert want != twin(ica, pl, name, 85)
    assert tenc.encode_ycbcr([pc.arg([dev(p) for p in pl])], subsampling=name, quality=85, video_range=True) == [want]
    views = device_views(pl)
    for what in ("cut",) + (("nv12",) if name != "grey" else ()):
        pic = views[what][0] if name == "grey" else views[what]
        assert tenc.encode_ycbcr([pic], subsampling=name, quality=85, video_range=True) == [want], what
    ly, lc = pc.video_range_luts()
    conv = [(lc if k else ly)[p] for k, p in enumerate(pl)]
    assert tenc.encode_ycbcr([pc.arg([dev(p) for p in conv])], subsampling=name, quality=85) == [want]


ROUND_TRIP_MAX = 5  # measured for the host twin on the CPU (oracle.load of both streams) on the picture below


def test_round_trip_inside_the_library(ica, tenc, oracle):
    """7: Y, Cb and Cr as the reference writer computes them from an RGB picture, rounded to uint8, encoded "444" under tables of ones and
    decoded by TensorDecoder, against the same picture decoded from the oracle's quality-100 stream.  The largest difference is 5, as
    measured for the host twin on the CPU; the GPU must match it exactly because its streams are the twin's."""
    f = np.float32
    rgb = sc.picture(64, 48, 3, 40)
    r, g, b = [rgb[..., k].astype(np.float32) for k in range(3)]
    y = f(0.299) * r + f(0.587) * g
    y = y + f(0.114) * b
    cb = f(-0.16874) * r - f(0.33126) * g
    cb = cb + f(0.5) * b + f(128)
    cr = f(0.5) * r - f(0.41869) * g
    cr = cr - f(0.08131) * b + f(128)
    pl = [np.clip(np.rint(p), 0, 255).astype(np.uint8) for p in (y, cb, cr)]
    ref = oracle.encode(rgb, 100)
    host = twin(ica, pl, "444", qtables=pc.ONES)
    cpu = int(np.abs(oracle.load(host, 3)[1].astype(int) - oracle.load(ref, 3)[1].astype(int)).max())
    assert cpu == ROUND_TRIP_MAX, "host twin: largest difference %d" % cpu
    ours = tenc.encode_ycbcr([tuple(dev(p) for p in pl)], subsampling="444", qtables=pc.ONES)
    assert ours == [host]
    dec = ica.TensorDecoder()
    out, reasons = dec.decode([ours[0], ref], layout="HWC", dtype=torch.uint8)
    assert reasons == [None, None]
    out = out.cpu().numpy().astype(int)
    got = int(np.abs(out[0] - out[1]).max())
    dec.close()
    assert got == ROUND_TRIP_MAX, "largest difference %d, the host twin's is %d" % (got, ROUND_TRIP_MAX)


def test_argument_errors(ica, tenc, gpu_ctx):
    """8: a tensor on the wrong device, a wrong dtype, wrong shapes, a missing sampling, and a plane whose extent leaves its allocation"""
    y, cb, cr = [dev(p) for p in pc.planes(17, 9, "420", 3)]
    for pic, kw in (((y.cpu(), cb, cr), {}), ((y, cb.cpu(), cr), {}), ((y, cb.to(torch.int16), cr), {}), ((y.float(), cb, cr), {}),
                    ((y, cb[:, :-1], cr), {}), ((y, cb, cr), {"subsampling": "444"}), ((y, cb, cr), {"subsampling": "grey"}),
                    ((y, cb, cr), {"subsampling": None}), ((y, cb, cr), {"subsampling": "411"}), ((y, cb), {}),
                    ((y, cb, cr), {"restart_mcus": 1, "progressive": True}), ((y, cb, cr), {"qtables": ([0] * 64, [1] * 64)}),
                    ((y, cb[:1].expand(cb.shape[0], -1), cr), {})):  # a stride of 0
        with pytest.raises(ValueError):
            tenc.encode_ycbcr([pic], **kw)
    with pytest.raises(ValueError):
        tenc.encode_ycbcr(torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device="cuda"), subsampling="444", video_range=1)
    enc = ica.Encoder(gpu_ctx, 8, 1 << 20, 1 << 20)
    good = triples([y, cb, cr])
    paths = {ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    dp = C.c_void_p()
    assert hip.hipMalloc(C.byref(dp), 9 * 17) == 0  # exactly one Y plane: torch's allocator would hand out a larger block
    p = dp.value
    host = np.zeros((9, 17), np.uint8)
    assert enc.add_device_planes([(p, 17, 1)] + good[1:], 17, 9, "420") == 0  # ends exactly at the end of the allocation
    for bad in ([(p + 1, 17, 1)] + good[1:],                              # one byte past the allocation
                [(p, 18, 1)] + good[1:],                                  # rows past the allocation
                [(p, 17, 2)] + good[1:],                                  # samples past the allocation
                [good[0], (good[1][0], good[1][1], 0), good[2]],          # a zero x_pitch
                [good[0], (good[1][0], 2, 1), good[2]],                   # rows that overlap
                [good[0], good[1], (0, 9, 1)],                            # a missing plane
                [(host.ctypes.data, 17, 1)] + good[1:]):                  # host memory
        with pytest.raises(ica.MijError):
            enc.add_device_planes(bad, 17, 9, "420")
    with pytest.raises(ica.MijError):
        L = ica.lib()
        q, keep = ica.binding.in_planes(good, 17, 9, "grey")  # chroma planes given for grey
        ica.binding._check(L.mij_enc_add_device_planes(enc._h, C.byref(q), 90), "mij_enc_add_device_planes")
    assert enc.add_device_planes(good, 17, 9, "420") == 1
    enc.close()
    assert hip.hipFree(dp) == 0
