"""Decode with libjpeg's arithmetic on the GPU (mij_batch_set_arith, MIJ_ARITH_LIBJPEG; k_lj_idct and k_lj_color of
mij_libjpeg_kernels.h; TensorDecoder.decode(arithmetic="libjpeg")): byte for byte against Pillow's pixels of
tests/golden/libjpeg_pillow.npz and against tests/libjpeg_model.py, the numpy restatement of the contract in include/mij.h."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library is first loaded: torch and the library share one HIP runtime (tensor_out._one_hip_runtime)

import coef_cases as CC
import idct_model as M
import libjpeg_model as LM

pytestmark = pytest.mark.gpu

MIJ_E_ARG, MIJ_E_STATE = -2, -5
STB, LIBJPEG = 0, 1
MB = 1 << 20
ITEM_W, ITEM_H = 256, 16  # one pass-2 work item (MIJ_LJ_ITEM_W x MIJ_LJ_ITEM_H)
FACTORS = {"444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "440": [(1, 2), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)], "grey": [(1, 1)]}
LJ_KIND = {"444": "MK_LJ_COLOR+LJ_11", "422": "MK_LJ_COLOR+LJ_21", "440": "MK_LJ_COLOR+LJ_12", "420": "MK_LJ_COLOR+LJ_22", "grey": "MK_LJ_COLOR+LJ_11"}


@pytest.fixture(scope="module")
def goldens():
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "libjpeg_pillow.npz"))
    return [(str(n), z["jpg_" + str(n)].tobytes(), z["pix_" + str(n)]) for n in z["names"]]


_model = {}


def _want(name, data, n_out):
    if (name, n_out) not in _model:
        _model[(name, n_out)] = LM.decode(data, n_out)
    return _model[(name, n_out)]


def _set_arith(ica, b, slot, arith):
    L = ica.lib()
    L.mij_batch_set_arith.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.mij_batch_set_arith.restype = C.c_int
    return L.mij_batch_set_arith(b._h, int(slot), int(arith))


def _decode(ica, gpu_ctx, datas, n_out, fmt="compact", walk=False, arith=LIBJPEG):
    """every file through the C-ABI with `arith` -> (batch, slots); walk: the GPU Huffman walk where it takes the file (the batch's
    `walked` counts those)"""
    b = ica.Batch(gpu_ctx, len(datas), 64 * MB, 64 * MB, 64 * MB)
    b.set_coef_format(fmt)
    b.walked = 0
    if walk:
        b.entropy_reserve(8 * MB)
        slots, later = [None] * len(datas), []
        for i, d in enumerate(datas):
            st, slot = b.add_jpeg_stream(d, n_out)
            assert st in (1, 2), (i, st, b.last_reason)
            if st == 1:
                slots[i] = slot
            else:
                later.append(i)
        assert b.entropy_run() == []
        b.walked = len(datas) - len(later)
        for i in later:
            slots[i] = b.add_jpeg(datas[i], n_out)
    else:
        slots = [b.add_jpeg(d, n_out) for d in datas]
    arith = [arith] * len(datas) if isinstance(arith, int) else arith
    for s, a in zip(slots, arith):
        if a != STB:
            b.set_arith(s, a)
    b.submit()
    b.wait()
    return b, slots


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("walk", [False, True], ids=["host_walk", "gpu_walk"])
def test_goldens_equal_pillow(ica, gpu_ctx, goldens, fmt, walk):
    """every golden, n_out 3 and 4 against Pillow's pixels, n_out 1 against the model's Y (Pillow's "L" for a grey file)"""
    datas = [d for _, d, _ in goldens]
    walked = 0
    for n_out in (3, 4, 1):
        b, slots = _decode(ica, gpu_ctx, datas, n_out, fmt, walk)
        for (name, data, pix), s in zip(goldens, slots):
            got = b.fetch(s).reshape(pix.shape[0], pix.shape[1], n_out)
            sampling = name.split("_")[0]
            assert b.slot_path(s) == 10, name
            assert b.slot_kernel(s)[:2] == ("MK_LJ_COLOR+LJ_11" if n_out == 1 else LJ_KIND[sampling], n_out - 1), (name, b.slot_kernel(s))
            assert b.slot_coef_bytes(s) == (1 if fmt == "compact" else 0), name
            assert b.work_items(s) == -(-pix.shape[1] // ITEM_W) * -(-pix.shape[0] // ITEM_H), name
            if n_out == 1:
                want = pix if pix.ndim == 2 else _want(name, data, 1)[..., 0]
                assert np.array_equal(got[..., 0], want), (name, n_out, fmt, walk)
            else:
                want = pix if pix.ndim == 3 else np.repeat(pix[..., None], 3, axis=2)
                assert np.array_equal(got[..., :3], want), (name, n_out, fmt, walk, int((got[..., :3] != want).sum()))
                assert n_out == 3 or (got[..., 3] == 255).all(), name
        walked += b.walked
        b.close()
    assert (walked > 0) == walk


def test_walk_front_end_with_lowered_threshold(ica, gpu_ctx, goldens, monkeypatch):
    """the 160 x 120 4:2:0 golden through the default front end with the batch threshold of the GPU walk lowered, and through the host walk"""
    name, data, pix = next(g for g in goldens if g[0].startswith("420_160x120_"))
    for front in ("gpu", "host"):
        monkeypatch.setenv("MIJ_GPU_WALK_BATCH_MIN_PIXELS", "0")
        b = ica.Batch(gpu_ctx, 2, 8 * MB, 8 * MB, 8 * MB)
        ok, slots, reasons = b.decode_jpegs([data, data], 3, threads=2, gpu_entropy=None if front == "gpu" else False)
        assert ok == 2, reasons
        b.set_arith(slots[1], LIBJPEG)
        b.submit()
        b.wait()
        assert b.slot_path(slots[0]) == 1 and b.slot_path(slots[1]) == 10
        assert np.array_equal(b.fetch(slots[1]).reshape(pix.shape), pix), front
        b.close()


def _sampled(ica, w, h, sampling, seed):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    a = np.stack([x * 3 % 256, y * 5 % 256, (x + 2 * y) % 256], -1) + rng.integers(-20, 21, (h, w, 3))
    return ica.write_jpg_sampled_to_memory(np.clip(a, 0, 255).astype(np.uint8), quality=92, sampling=sampling)


def test_seams_between_work_items(ica, gpu_ctx):
    """pictures that span two pass-2 items each way, and widths of 8k +- 1 and 16k +- 1 around one item's width, against the model"""
    cases = [("420", 2 * ITEM_W + 37, 2 * ITEM_H + 5), ("422", 2 * ITEM_W + 11, 2 * ITEM_H + 3)]
    for k, w in enumerate((ITEM_W - 9, ITEM_W - 7, ITEM_W - 1, ITEM_W + 1, ITEM_W + 7, ITEM_W + 9, ITEM_W + 15, ITEM_W + 17)):
        cases.append((("420", "422")[k % 2], w, 19 - k % 2))
    datas = [_sampled(ica, w, h, s, i) for i, (s, w, h) in enumerate(cases)]
    for n_out in (3, 4):
        b, slots = _decode(ica, gpu_ctx, datas, n_out)
        for i, ((s, w, h), sl) in enumerate(zip(cases, slots)):
            assert b.slot_path(sl) == 10 and b.slot_kernel(sl)[0] == LJ_KIND[s]
            assert b.work_items(sl) == -(-w // ITEM_W) * -(-h // ITEM_H)
            got, want = b.fetch(sl).reshape(h, w, n_out), _want("seam%d" % i, datas[i], n_out)
            assert np.array_equal(got, want), (s, w, h, n_out, int((got != want).sum()))
        b.close()


def _extreme_cases():
    """synthetic coefficient planes (coef_cases.py): single coefficients at each of the 64 positions at +-1 and at the largest codable
    value (1023; 2047 for DC) with tables of ones and of 255, which also gives escaped blocks and samples that clamp at 0 and at 255;
    and pictures of DC-only blocks over the whole codable range, where every wavefront takes the DC-only class"""
    out = []
    for layout, w, h in (("grey", 192, 96), ("420", 384, 192), ("444", 192, 96), ("422", 384, 96), ("440", 192, 192)):
        for qv in (1, 255):
            planes = CC.blank(layout, w, h)
            for c, p in enumerate(planes):
                flat = p.reshape(-1, 64)
                for i in range(min(len(flat), 256 + 16)):
                    pos, form = i % 64, (i // 64) % 4
                    big = 2047 if pos == 0 else 1023
                    flat[i, pos] = (1, -1, big, -big)[(form + c) % 4]
                    if i >= 256:  # dense escaped blocks next to plain ones
                        flat[i, :8] = (900, -700, 300, -200, 129, -129, 128, -128) if i % 2 else (100, -100, 50, 0, 0, 3, 0, -1)
            out.append(CC.Case("lj_single_%s_q%d" % (layout, qv), "lj", layout, w, h, planes, qt=np.full(128, qv, np.int64)))
        planes = CC.blank(layout, w, h)
        for c, p in enumerate(planes):
            flat = p.reshape(-1, 64)
            flat[:, 0] = np.linspace(-1024, 1023, len(flat)).astype(np.int16) * (1 if c != 1 else -1)
        out.append(CC.Case("lj_dc_%s" % layout, "lj", layout, w, h, planes, qt=np.full(128, 8, np.int64)))
    return out


def test_extreme_coefficients(ica, gpu_ctx):
    cases = _extreme_cases()
    datas = [c.stream() for c in cases]
    want = [LM.picture(c.quantised(), [M.zz_to_nat(c.q_of(k)) for k in range(len(c.planes))], FACTORS[c.layout], (c.w, c.h), 3) for c in cases]
    assert any((w == 0).any() and (w == 255).any() for w in want)
    for fmt in ("compact", "int16"):
        b, slots = _decode(ica, gpu_ctx, datas, 3, fmt)
        for c, s, w in zip(cases, slots, want):
            assert b.slot_path(s) == 10
            if fmt == "compact" and "single" in c.name:
                assert b.slot_escapes(s) > 0, c.name
            got = b.fetch(s).reshape(c.h, c.w, 3)
            assert np.array_equal(got, w), (c.name, fmt, int((got != w).sum()))
        b.close()


def test_mixed_batch_and_untouched_default(ica, oracle, gpu_ctx, goldens):
    """STB and LIBJPEG slots interleaved, each right by its own checker; a batch without a request keeps its paths, kernels and pixels"""
    pick = [g for g in goldens if g[0].split("_")[1] in ("33x31", "17x15", "97x61", "17x17")]
    datas = [d for _, d, _ in pick]
    arith = [(LIBJPEG, STB)[i % 2] for i in range(len(pick))]
    plain, pslots = _decode(ica, gpu_ctx, datas, 3, arith=STB)
    mixed, mslots = _decode(ica, gpu_ctx, datas, 3, arith=arith)
    for (name, data, pix), a, ps, ms in zip(pick, arith, pslots, mslots):
        stb = oracle.load(data, 3)
        assert stb[0] == "ok"
        assert plain.slot_path(ps) in (1, 3, 4, 5, 6) and np.array_equal(plain.fetch(ps).reshape(stb[1].shape), stb[1]), name
        if a == STB:
            assert mixed.slot_path(ms) == plain.slot_path(ps) and mixed.slot_kernel(ms) == plain.slot_kernel(ps), name
            assert np.array_equal(mixed.fetch(ms).reshape(stb[1].shape), stb[1]), name
        else:
            want = pix if pix.ndim == 3 else np.repeat(pix[..., None], 3, axis=2)
            assert mixed.slot_path(ms) == 10 and np.array_equal(mixed.fetch(ms).reshape(want.shape), want), name
    plain.close()
    mixed.close()


def test_state_and_refusals(ica, gpu_ctx, goldens):
    name, data, pix = next(g for g in goldens if g[0].startswith("420_33x31_") and g[0].endswith("_b"))
    b = ica.Batch(gpu_ctx, 8, 8 * MB, 8 * MB, 8 * MB)
    s = b.add_jpeg(data, 3)
    assert _set_arith(ica, b, s, 2) == MIJ_E_ARG and _set_arith(ica, b, 99, LIBJPEG) == MIJ_E_ARG
    # a scaled slot, in both orders
    b.set_scale(s, 2)
    assert _set_arith(ica, b, s, LIBJPEG) == MIJ_E_ARG
    b.set_scale(s, 1)
    assert _set_arith(ica, b, s, LIBJPEG) == 0
    L = ica.lib()
    L.mij_batch_set_scale.argtypes = [C.c_void_p, C.c_int, C.c_int]
    assert L.mij_batch_set_scale(b._h, s, 2) == MIJ_E_ARG and L.mij_batch_set_scale(b._h, s, 1) == 0
    # asking again replaces the request
    assert _set_arith(ica, b, s, STB) == 0 and _set_arith(ica, b, s, LIBJPEG) == 0
    # layouts that are refused, not approximated
    for layout in ("cmyk", "411", "rgb", "ycck"):
        r = b.add_jpeg(CC.Case("lj_" + layout, "lj", layout, 32, 16, CC.blank(layout, 32, 16)).stream(), 3)
        assert _set_arith(ica, b, r, LIBJPEG) == MIJ_E_ARG, layout
        assert _set_arith(ica, b, r, STB) == 0
    clone = b.add_clone(s)  # clones start at STB
    b.set_roi(s, 8, 8, 9, 9)  # a region is accepted; the picture is decoded whole
    b.upload()
    assert _set_arith(ica, b, s, STB) == MIJ_E_STATE  # after upload
    b.launch()
    b.wait()
    assert b.slot_path(s) == 10 and b.slot_path(clone) == 1
    assert b.roi_rect(s) == (0, 0, 33, 31)
    assert np.array_equal(b.fetch(s).reshape(pix.shape), pix)
    assert not np.array_equal(b.fetch(clone).reshape(pix.shape), pix)
    b.reset()  # forgets the request
    s = b.add_jpeg(data, 3)
    b.submit()
    b.wait()
    assert b.slot_path(s) == 1
    b.close()


def test_tensor_path(ica, gpu_ctx, goldens):
    """TensorDecoder.decode(arithmetic="libjpeg") with crops, a bicubic resize and EXIF orientation 6: resize_model on Pillow's pixels"""
    import exif_build as eb
    import orient_model as om
    import resize_model as rm
    import tensor_model as tm

    pick = [g for g in goldens if g[0].split("_")[1] == "97x61" and g[0].split("_")[0] != "grey"]
    assert len(pick) >= 6
    datas = [d for _, d, _ in pick]
    datas[1] = eb.tagged(datas[1], 6, False)
    orients = [6 if i == 1 else 1 for i in range(len(pick))]
    crops = [(3, 2, 50, 41) if o == 6 else (5, 3, 80, 50) for o in orients]
    dec = ica.TensorDecoder("cuda:0")
    got, reasons = dec.decode(datas, crops=crops, size=(24, 24), filter="bicubic", dtype=torch.uint8, orientation="exif", arithmetic="libjpeg")
    assert reasons == [None] * len(pick) and dec.last_arithmetic == ["libjpeg"] * len(pick)
    for i, ((name, _, pix), o, win) in enumerate(zip(pick, orients, crops)):
        want = rm.window(om.orient(pix, o), win, (24, 24), "bicubic")
        assert tm.same_bits(got[i], want), name
    stb, _ = dec.decode(datas, crops=crops, size=(24, 24), filter="bicubic", dtype=torch.uint8, orientation="exif")
    assert dec.last_arithmetic == ["stb"] * len(pick) and not torch.equal(stb, got)
    with pytest.raises(ValueError):
        dec.decode(datas, crops=crops, size=(24, 24), arithmetic="libjpeg", reduce=2)
    with pytest.raises(ValueError):
        dec.decode(datas, arithmetic="turbo")
    bad = CC.Case("lj_411_t", "lj", "411", 97, 61, CC.blank("411", 97, 61)).stream()
    got2, reasons2 = dec.decode([datas[0], bad], crops=[(0, 0, 40, 40)] * 2, dtype=torch.uint8, arithmetic="libjpeg")
    assert reasons2[0] is None and "libjpeg" in reasons2[1] and dec.last_arithmetic == ["libjpeg", None] and bool((got2[1] == 0).all())
    dec.close()
