"""The host contract of plane encoding (include/mij_host.h, PLANE ENCODING: mjw_pplan_init, mjw_ptransform_host,
mjh_write_jpg_planes_to_memory): luma anchored on the reference writer, chroma anchored on luma, flat planes that decode exactly, unit
order and headers, views, the video-range conversion, composition with optimised tables, restart intervals and progressive scans, and
the arguments that are refused.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import helpers
import planes_cases as pc
import sampling_cases as sc
import upsample_model as um


def enc(ica, pl, sampling, q=90, **kw):
    data = ica.write_jpg_planes_to_memory(pc.arg(pl) if isinstance(pl, list) else pl, sampling, q, **kw)
    assert data is not None
    return data


@pytest.fixture(scope="module")
def reference():
    return helpers.Reference() if helpers.Reference.available() else None


def test_exact_luma_values():
    """the set the luma anchor draws from, computed here with the writer's expression"""
    ex = pc.exact_luma_values()
    assert len(ex) == 227 and 255 in ex
    assert all(v in ex for v in range(40)) and min(set(range(256)) - set(ex)) > 39


@pytest.mark.parametrize("name", pc.SAMPLINGS)
@pytest.mark.parametrize("q", [50, 95])
def test_luma_anchored_on_the_reference(ica, oracle, reference, name, q):
    """1: a Y plane of values on which the writer's luma is exact carries the luma blocks of the writer's stream of the grey picture"""
    ex = pc.exact_luma_values()
    for k, (w, h) in enumerate(pc.sizes(name)):
        pl = pc.planes(w, h, name, 31 * k + q, values=ex)
        assert set(np.unique(pl[0])) <= set(ex)
        ours = sc.blocks(*sc.walk(ica, enc(ica, pl, name, q)))[0]
        grey = pl[0][:, :, None]
        want = oracle.encode(grey, q)
        if reference is not None:
            assert reference.encode(grey, q) == want, (name, w, h)
        theirs = sc.blocks(*sc.walk(ica, want))[0]
        bh, bw = min(ours.shape[0], theirs.shape[0]), min(ours.shape[1], theirs.shape[1])
        assert bh >= (h + 7) // 8 and bw >= (w + 7) // 8
        assert np.array_equal(ours[:bh, :bw], theirs[:bh, :bw]), (name, q, w, h)


@pytest.mark.parametrize("name", ["420", "422", "440"])
def test_chroma_anchored_on_luma(ica, name):
    """2: under one table for luma and chroma, Cb = Cr = P gives the Y blocks of a "444" encode whose Y is P: the same arithmetic and the
    same edge rule on the chroma plane's own size"""
    T = sc.random_tables(17)[0]
    for k, (w, h) in enumerate(pc.sizes(name)):
        pl = pc.planes(w, h, name, 5 * k + 1)
        P = pl[1]
        _, cb, cr = sc.blocks(*sc.walk(ica, enc(ica, [pl[0], P, P], name, qtables=(T, T))))
        ph, pw = P.shape
        other = pc.planes(pw, ph, "444", 99 + k)
        y = sc.blocks(*sc.walk(ica, enc(ica, [P, other[1], other[2]], "444", qtables=(T, T))))[0]
        assert cb.shape == y.shape, (name, w, h)
        assert np.array_equal(cb, y) and np.array_equal(cr, y), (name, w, h)


FLAT_VALUES = (0, 1, 16, 77, 128, 200, 235, 240, 254, 255)


@pytest.fixture(scope="module")
def flat_ok(oracle):
    """the values whose flat grey picture the reference writer's own stream (quality 100: tables of ones) gives back exactly"""
    ok = []
    for v in FLAT_VALUES:
        kind, px, _ = oracle.load(oracle.encode(np.full((8, 8, 1), v, np.uint8), 100), 1)
        if kind == "ok" and np.all(px == v):
            ok.append(v)
    return ok


@pytest.mark.parametrize("name", pc.SAMPLINGS)
def test_flat_planes_decode_exactly(ica, oracle, flat_ok, name):
    """3: under tables of ones a flat block is DC 8 * (v - 128) and no AC, so the decoder gets the samples back: every pixel is
    ycbcr_to_rgb(a, b, c)"""
    assert len(flat_ok) >= 6, flat_ok
    n = 0
    for i, a in enumerate(flat_ok):
        b, c = flat_ok[(i + 3) % len(flat_ok)], flat_ok[(2 * i + 1) % len(flat_ok)]
        for (w, h) in ((17, 9), (1, 1)):
            pl = [np.full(s, v, np.uint8) for s, v in zip(pc.shapes(w, h, name), (a, b, c))]
            t, du = ica.host_transform_planes(pc.arg(pl), name, qtables=pc.ONES)
            assert np.all(du[:, 1:] == 0)
            kind, px, comp = oracle.load(enc(ica, pl, name, qtables=pc.ONES))
            assert kind == "ok" and px.shape == (h, w, len(pl))
            want = np.uint8(a) if name == "grey" else um.ycbcr_to_rgb(np.uint8(a), np.uint8(b), np.uint8(c))
            assert np.all(px == want), (name, a, b, c, w, h)
            n += 1
    assert n >= 12


@pytest.mark.parametrize("name", pc.SAMPLINGS)
def test_unit_order_and_headers(ica, oracle, name):
    """4: the walked descriptor has the requested components and factors, the walked units are mjw_ptransform_host's in order, the DQT
    carries the quality's tables or the given ones"""
    pl = pc.planes(37, 21, name, 11)
    ncomp, lh, lv = pc.FACTORS[name]
    for q, tabs in ((75, None), (90, sc.random_tables(4))):
        data = enc(ica, pl, name, q, qtables=tabs)
        t, du = sc.walk(ica, data)
        assert t.ncomp == ncomp and (ncomp == 1 or (t.lh, t.lv) == (lh, lv))
        plan, want = ica.host_transform_planes(pc.arg(pl), name, q, qtables=tabs)
        assert plan.plan.comp == ncomp and plan.plan.du_per_mcu == (1 if ncomp == 1 else lh * lv + 2)
        assert (plan.plan.mcu_x, plan.plan.mcu_y) == ((37 + 8 * lh - 1) // (8 * lh), (21 + 8 * lv - 1) // (8 * lv))
        assert np.array_equal(du, want)
        luma, chroma = tabs if tabs else [list(x) for x in ica.quality_tables(q)]
        got = sc.stream_tables(data)
        assert got[0] == list(luma) and (ncomp == 1) == (1 not in got) and (ncomp == 1 or got[1] == list(chroma))
        kind, pixels, comp = oracle.load(data)
        assert kind == "ok" and pixels.shape == (21, 37, ncomp)
    try:
        from PIL import Image
    except ImportError:
        return  # Pillow is optional: everything above has been checked
    import io
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (37, 21) and im.mode == ("L" if ncomp == 1 else "RGB")


@pytest.mark.parametrize("name", pc.SAMPLINGS)
def test_views_give_the_bytes_of_their_copies(ica, name):
    """5: NV12, NV21, a wider row pitch, planes cut out of larger arrays, packed HWC and flip_vertically"""
    seen = set()
    for (w, h) in ((17, 9), (33, 18)):
        pl = pc.planes(w, h, name, w)
        want = enc(ica, pl, name, 80)
        for what, pic in pc.views(pl, seed=h).items():
            got = ica.write_jpg_planes_to_memory(pic, name, 80, flip=what == "flipped")
            assert got == want, (name, what, w, h)
            seen.add(what)
        assert enc(ica, pl, name, 80, flip=True) != want
    assert {"cut", "flipped"} <= seen and (name == "grey" or {"nv12", "nv21", "nv12_pitched"} <= seen) and (name != "444" or "packed" in seen)


def test_video_range(ica):
    """6: every sample value, on luma and on chroma, converts as the numpy float32 restatement of the contract says"""
    ly, lc = pc.video_range_luts()
    assert (ly[16], ly[235], lc[128], lc[240], lc[16]) == (0, 255, 128, 255, 0)
    assert np.all(ly[:16] == 0) and np.all(ly[235:] == 255) and np.all(lc[:16] == 0) and np.all(lc[240:] == 255)
    assert np.all(np.diff(ly.astype(int)) >= 0) and np.all(np.diff(lc.astype(int)) >= 0)
    cv = ica.video_range_convert()
    assert [cv.scale[0], cv.bias[0], cv.scale[1], cv.bias[1]] == [float(np.float32(255 / 219)), float(np.float32(-16 * 255 / 219)),
                                                                  float(np.float32(255 / 224)), float(np.float32(128 - 128 * 255 / 224))]
    assert (cv.scale[2], cv.bias[2]) == (cv.scale[1], cv.bias[1])
    # flat planes under tables of ones show the converted value itself: DC = 8 * (u - 128)
    for v in list(range(256)):
        for name, pl in (("grey", [np.full((8, 8), v, np.uint8)]), ("444", [np.full((8, 8), 128, np.uint8), np.full((8, 8), v, np.uint8), np.full((8, 8), 255 - v, np.uint8)])):
            _, du = ica.host_transform_planes(pc.arg(pl), name, qtables=pc.ONES, video_range=True)
            if name == "grey":
                assert du[0, 0] == 8 * (int(ly[v]) - 128), v
            else:
                assert (du[1, 0], du[2, 0]) == (8 * (int(lc[v]) - 128), 8 * (int(lc[255 - v]) - 128)), v
    every = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for name in pc.SAMPLINGS:
        pl = [np.ascontiguousarray((every.T if k else every)[:s[0], :s[1]]) for k, s in enumerate(pc.shapes(16, 16, name))]
        conv = [(lc if k else ly)[p] for k, p in enumerate(pl)]
        assert enc(ica, pl, name, 85, video_range=True) == enc(ica, conv, name, 85), name
        assert enc(ica, pl, name, 85, video_range=True) != enc(ica, pl, name, 85), name
        # the caller's own scale and bias go through the same arithmetic
        assert enc(ica, pl, name, 85, convert=((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))) == enc(ica, pl, name, 85), name


@pytest.mark.parametrize("name", ["420", "440", "grey"])
def test_composition_on_the_host(ica, name):
    """7: optimised tables, restart intervals and progressive scans carry the plain stream's units (progressive: as
    test_encode_sampling_host.py states it)"""
    pl = pc.planes(40, 24, name, 9)
    plain = enc(ica, pl, name, 75)
    t0, du0 = sc.walk(ica, plain)
    for kw in ({"optimize": True}, {"restart_mcus": 1}, {"restart_rows": 1}, {"progressive": True}):
        data = enc(ica, pl, name, 75, **kw)
        assert data != plain
        t, du = sc.walk(ica, data)
        assert (t.ncomp, t.lh, t.lv, t.plan.mcu_x, t.plan.mcu_y) == (t0.ncomp, t0.lh, t0.lv, t0.plan.mcu_x, t0.plan.mcu_y)
        if "progressive" not in kw:
            assert np.array_equal(du, du0), kw
            continue
        # AC scans of luma alone cover ceil(W / 8) x ceil(H / 8) blocks (T.81 A.2.3): blocks that only pad the last MCU keep their DC
        assert np.array_equal(du[:, 0], du0[:, 0]), kw
        for got, want in zip(sc.blocks(t, du), sc.blocks(t0, du0)):
            assert np.array_equal(got[:3, :5], want[:3, :5]), kw
    assert b"\xff\xdd\x00\x04\x00\x01" in enc(ica, pl, name, 75, restart_mcus=1)
    mcu_x = t0.plan.mcu_x
    assert b"\xff\xdd\x00\x04" + bytes([mcu_x >> 8, mcu_x & 255]) in enc(ica, pl, name, 75, restart_rows=1)
    with pytest.raises(ValueError):
        ica.write_jpg_planes_to_memory(pc.arg(pl), name, 75, restart_mcus=1, progressive=True)


def test_argument_errors(ica):
    """8: a missing or unknown sampling, wrong chroma shapes, chroma given for grey, bad tables, a conversion that is not finite"""
    y, cb, cr = pc.planes(17, 9, "420", 3)
    for bad in (None, "411", "4:2:0", 420, b"420", ""):
        with pytest.raises(ValueError):
            ica.write_jpg_planes_to_memory((y, cb, cr), bad)
    for pic, name in (((y, cb[:, :-1], cr), "420"), ((y, cb, cr), "422"), ((y, cb, cr), "444"), ((y, cb), "420"), ((y, cb, cr), "grey"), (y, "420"),
                      ((y, cb.astype(np.int16), cr), "420"), ((y[None], cb, cr), "420"), ((y, np.stack([cb, cr, cr], -1)), "420")):
        with pytest.raises(ValueError):
            ica.write_jpg_planes_to_memory(pic, name)
    for bad in (([0] * 64, [1] * 64), ([1] * 63, [1] * 64), ([256] * 64, [1] * 64), ([1] * 64,), 5):
        with pytest.raises(ValueError):
            ica.write_jpg_planes_to_memory((y, cb, cr), "420", qtables=bad)
    for bad in (((float("nan"), 1, 1), (0, 0, 0)), ((1, 1, 1), (0, float("inf"), 0))):
        with pytest.raises(ValueError):
            ica.write_jpg_planes_to_memory((y, cb, cr), "420", convert=bad)
    with pytest.raises(ValueError):
        ica.write_jpg_planes_to_memory((y, cb, cr), "420", video_range=True, convert=((1, 1, 1), (0, 0, 0)))
    assert ica.planes_plan(0, 8, "420") is None and ica.planes_plan(8, 8, "grey") is not None

    # the C calls themselves return 0
    L, B = ica.lib(), ica.binding
    L.mjw_pplan_init.argtypes = [C.POINTER(B.TranscodePlan), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p]
    t = B.TranscodePlan()
    for fac in ((0, 0, 0), (3, 4, 1), (1, 2, 2), (2, 1, 1)):
        assert L.mjw_pplan_init(C.byref(t), 17, 9, 90, *fac, None, None) == 0, fac
    assert L.mjw_pplan_init(C.byref(t), 17, 9, 90, 3, 2, 2, bytes([1] * 64), None) == 0
    assert L.mjw_pplan_init(C.byref(t), 17, 9, 90, 3, 2, 2, None, None) == 1
    L.mjw_ptransform_host.argtypes = [C.POINTER(B.TranscodePlan), C.POINTER(B.Plane), C.c_void_p, C.c_int, C.c_void_p]
    du = np.zeros(t.du_elems(), np.int16)
    good = [B.Plane(a.ctypes.data, a.strides[0], 1) for a in (y, cb, cr)]

    def run(planes, cv=None):
        arr = (B.Plane * 3)(*planes)
        return L.mjw_ptransform_host(C.byref(t), arr, C.byref(cv) if cv is not None else None, 0, du.ctypes.data_as(C.c_void_p))

    assert run(good) == 1
    assert run([good[0], B.Plane(None, 0, 1), good[2]]) == 0  # a missing chroma plane
    assert run([good[0], B.Plane(cb.ctypes.data, cb.strides[0], 0), good[2]]) == 0  # a zero x_pitch
    assert run(good, B.InConvert(B.MIJ_DT_U8, (1, float("nan"), 1), (0, 0, 0))) == 0
    assert run(good, B.InConvert(B.MIJ_DT_F32, (1, 1, 1), (0, 0, 0))) == 0
    g = B.TranscodePlan()
    assert L.mjw_pplan_init(C.byref(g), 17, 9, 90, 1, 1, 1, None, None) == 1
    arr = (B.Plane * 3)(*good)
    assert L.mjw_ptransform_host(C.byref(g), arr, None, 0, du.ctypes.data_as(C.c_void_p)) == 0  # chroma given for grey


def test_host_pieces_under_sanitizers(tmp_path):
    """tests/support/san_planes.c: the plane transform and writer on exact-size heap blocks (planar, pitched, NV12, flipped, range-
    converted) under ASan + UBSan, as a stand-alone CPU program: the edge rule reads nothing past a plane's last sample"""
    import os
    import subprocess
    root = helpers.ROOT
    exe = str(tmp_path / "san_planes")
    cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-I" + root + "/include", "-I" + root + "/image-codecs_amd/csrc", "-o", exe,
           root + "/tests/support/san_planes.c", root + "/image-codecs_amd/csrc/jpeg_write_host.c"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("no address sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-2000:]
    assert "planes harness: 90 cases, 0 failures" in run.stdout
