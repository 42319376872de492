"""Region-of-interest decode on the GPU (mij_batch_set_roi / _roi_auto / mij_batch_slot_roi_rect): inside the region the
bytes of the whole-picture decode (the oracle at full size, tests/scaled_model.py at reduced size), outside the decoded rectangle the
bytes the slot's output region held before the launch, and the decoded rectangle within the contract's bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import coef_cases as CC
from roi_cases import MB, MCU, bound, dense, paint, rounded_out, run_windows, stored_window, want  # noqa: F401  (shared with test_gpu_roi_seams.py)

pytestmark = pytest.mark.gpu

MIJ_E_ARG, MIJ_E_STATE = -2, -5
REDUCIBLE = ("420", "422", "444", "grey")
SIZES = ((77, 45), (80, 48))

_cache = {}


def wide_case(layout):
    """one stream of the layout that needs MIJ_FLAG_WIDE_IDCT"""
    k = ("wide", layout)
    if k not in _cache:
        _cache[k] = next(c for c in CC.l1_family(layout) if c.needs_wide())
    return _cache[k]


def windows(W, H, mw, mh):
    """centre pixel, one interior MCU, a 2 x 2 window across an MCU corner, the four corners, last column, last row, the whole picture"""
    assert W > 2 * mw and H > 2 * mh
    return [(W // 2, H // 2, 1, 1), (mw, mh, mw, mh), (mw - 1, mh - 1, 2, 2), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1),
            (W - 1, 0, 1, H), (0, H - 1, W, 1), (0, 0, W, H)]


# ------------------------------------------------------------------ 1. exactness inside, silence outside

@pytest.mark.parametrize("layout", ("grey", "444", "420", "422", "440", "cmyk", "411"))
def test_inside_exact_outside_untouched(ica, gpu_ctx, oracle, layout):
    scales = (1, 2, 4, 8) if layout in REDUCIBLE else (1,)
    reqs = (1, 3, 4)
    n = 0
    for size in SIZES:
        case = dense(layout, size)
        for s in scales:
            W, H = -(-case.w // s), -(-case.h // s)
            wins = windows(W, H, MCU[layout][0] // s, MCU[layout][1] // s)
            for req in reqs:
                for fmt in ("compact", "int16"):
                    n += len(run_windows(ica, gpu_ctx, oracle, case, req, fmt, s, wins))
    assert n == len(SIZES) * len(scales) * len(reqs) * 2 * 10
    # one stream that needs the wide transform, in both plane formats
    wc = wide_case(layout)
    mw, mh = MCU[layout]
    wins = [(wc.w // 2, wc.h // 2, 1, 1), (mw, 0, mw, mh), (mw - 1, mh - 1, 2, 2), (wc.w - 1, wc.h - 1, 1, 1), (0, 0, wc.w, wc.h)]
    strong = wc.strong  # (component, block row, block column): a window on the strong block itself
    hv = CC.LAYOUTS[layout][0]
    hmax, vmax = max(a for a, _ in hv), max(v for _, v in hv)
    sx, sy = strong[2] * 8 * hmax // hv[strong[0]][0], strong[1] * 8 * vmax // hv[strong[0]][1]
    wins.append((min(sx, wc.w - 1), min(sy, wc.h - 1), 1, 1))
    for fmt in ("compact", "int16"):
        run_windows(ica, gpu_ctx, oracle, wc, 3, fmt, 1, wins, tag=("wide",))


def test_a_region_really_takes_the_windowed_path(ica, gpu_ctx, oracle):
    """the decoded rectangles of the families with column support are the region rounded out to MCUs (blocks for the 1 x 1 families),
    so a one-pixel window decodes one unit -- far less than the picture"""
    for layout, s, unit in (("420", 1, (16, 16)), ("440", 1, (8, 16)), ("444", 1, (8, 8)), ("grey", 1, (8, 8)), ("cmyk", 1, (8, 8)), ("420", 2, (8, 8)),
                            ("422", 4, (4, 2)), ("grey", 8, (1, 1))):
        case = dense(layout, (80, 48))
        W, H = 80 // s, 48 // s
        (win, rect, _), = run_windows(ica, gpu_ctx, oracle, case, 3, "compact", s, [(W // 2 + 1, H // 2 + 1, 1, 1)])
        ux, uy = unit
        assert rect == (win[0] // ux * ux, win[1] // uy * uy, ux, uy), (layout, s, rect)
    case = dense("422", (80, 48))
    (win, rect, _), = run_windows(ica, gpu_ctx, oracle, case, 3, "compact", 1, [(41, 25, 1, 1)])
    assert rect == (0, 24, 80, 8)


# ------------------------------------------------------------------ 2. row stores of the windowed 1 x 1 kernels

@pytest.mark.parametrize("layout", ("444", "grey"))
@pytest.mark.parametrize("width", (1024, 1022))
def test_row_stores(ica, gpu_ctx, oracle, layout, width):
    """windows of 70 blocks from an odd block column on a picture of two block rows: the window's first wave lies in one block row and
    takes the LDS-transposed stores (where the pitch allows: four channels, or a width that is a multiple of four), the second spans both
    rows and the last is partial"""
    case = dense(layout, (width, 16))
    wins = [(8 * 3, 0, 8 * 70, 16), (8 * 3 + 1, 1, 8 * 70 - 2, 14), (8 * 57, 0, width - 8 * 57, 16), (8 * 5, 8, 8 * 70, 8)]
    for req in (3, 4, 1):
        for fmt in ("compact", "int16"):
            for win, rect, _ in run_windows(ica, gpu_ctx, oracle, case, req, fmt, 1, wins):
                assert rect == (win[0] // 8 * 8, win[1] // 8 * 8, min(width, -(-(win[0] + win[2]) // 8) * 8) - win[0] // 8 * 8, 16 - win[1] // 8 * 8), (win, rect)


# ------------------------------------------------------------------ 3. column segments

def test_segments(ica, gpu_ctx, oracle):
    """5904 x 32 4:2:0 is cut into segments without any region (369 MCU columns; 365 fit the LDS): a window across the seam of that plan
    at MCU column 123, one across both seams, and one wider than a segment's LDS budget (180 columns), which the planner has to cut"""
    case = dense("420", (5904, 32))
    wins = [(16 * 120, 0, 16 * 6, 32), (16 * 100 + 5, 3, 16 * 160, 20), (16 * 10 + 5, 0, 16 * 290 - 10, 32), (16 * 200, 16, 5904 - 16 * 200, 16)]
    for req, fmt in ((3, "compact"), (4, "int16")):
        for win, rect, got in run_windows(ica, gpu_ctx, oracle, case, req, fmt, 1, wins):
            px = want(oracle, case, req)
            rx, ry, rw, rh = rect
            assert rect == (win[0] // 16 * 16, win[1] // 16 * 16, min(5904, -(-(win[0] + win[2]) // 16) * 16) - win[0] // 16 * 16,
                            -(-(win[1] + win[3]) // 16) * 16 - win[1] // 16 * 16), (win, rect)
            # every seam inside the decoded rectangle is exact: the whole rectangle is the plain decode
            assert np.array_equal(got[ry:ry + rh, rx:rx + rw], px[ry:ry + rh, rx:rx + rw]), (win, rect)


# ------------------------------------------------------------------ 4. both producers

@pytest.mark.parametrize("layout", ("420", "444"))
def test_both_producers(ica, gpu_ctx, oracle, layout):
    case = dense(layout, (77, 45), seed=2)
    wins = windows(77, 45, *MCU[layout])
    for fmt in ("compact", "int16"):
        host = run_windows(ica, gpu_ctx, oracle, case, 3, fmt, 1, wins, producer="host")
        walk = run_windows(ica, gpu_ctx, oracle, case, 3, fmt, 1, wins, producer="walk")
        for (win, r0, g0), (_, r1, g1) in zip(host, walk):
            assert r0 == r1
            x0, y0, w, h = win
            assert np.array_equal(g0[y0:y0 + h, x0:x0 + w], g1[y0:y0 + h, x0:x0 + w]), win
    case2 = dense(layout, (77, 45), seed=2)
    for s in (2,):
        W, H = -(-77 // s), -(-45 // s)
        run_windows(ica, gpu_ctx, oracle, case2, 3, "compact", s, windows(W, H, MCU[layout][0] // s, MCU[layout][1] // s), producer="walk")


# ------------------------------------------------------------------ 5. tensor path

@pytest.fixture(scope="module")
def dec(ica, gpu_ctx):
    d = ica.TensorDecoder("cuda:0")
    yield d
    d.close()


def test_tensor_path(ica, dec):
    """decode(crops=..., roi=True) equals roi=False bit for bit.  Between the two, the same decoder decodes OTHER pictures of the same
    layouts and sizes whole, so the slots' output regions hold foreign pixels when the automatic regions are decoded: a region that is
    misplaced or too small shows in the tensor.  The decoded rectangle is the stored-frame window of the request, found independently
    (stored_window), rounded out to the family's unit; outside it the foreign pixels are still there."""
    shapes = (("420", (203, 77)), ("444", (120, 90)), ("422", (64, 300)))
    cases = [dense(lay, size, seed=3) for lay, size in shapes]
    others = [dense(lay, size, seed=4) for lay, size in shapes]
    datas, paint_datas = [c.stream() for c in cases], [c.stream() for c in others]
    n = 0
    for reduce in (None, 2):
        s = reduce or 1
        for o in (1, 3, 6, 5, 8):
            for size in (None, (9, 11)):
                crops = []
                for c in cases:
                    sw, sh = -(-c.w // s), -(-c.h // s)
                    dw, dh = (sh, sw) if o >= 5 else (sw, sh)
                    crops.append((dw // 3, dh // 4 + 1, 13, 10) if size is None else (dw // 3, dh // 4 + 1, min(17, dw - dw // 3), min(21, dh - dh // 4 - 1)))
                kw = dict(crops=crops, size=size, orientation=o, reduce=reduce, dtype=torch.uint8, layout="HWC")
                tag = (reduce, o, size)
                plain, r0 = dec.decode(datas, roi=False, **kw)
                plain = plain.clone()
                b = dec._batch
                plain_px = [b.fetch(i) for i in range(3)]
                for i in range(3):
                    assert b.roi_rect(i) == (0, 0) + b.out_size(i), tag
                dec.decode(paint_datas, roi=False, **kw)
                assert dec._batch is b  # the same arena, the same slots
                paint_px = [b.fetch(i) for i in range(3)]
                got, r1 = dec.decode(datas, roi=True, **kw)
                assert dec._batch is b and r0 == r1 == [None] * 3, tag
                assert torch.equal(got, plain), tag
                for i, c in enumerate(cases):
                    sw, sh = b.out_size(i)
                    assert (sw, sh) == (-(-c.w // s), -(-c.h // s)), tag
                    win = stored_window(sw, sh, o, crops[i])
                    mw, mh = MCU[c.layout][0] // s, MCU[c.layout][1] // s
                    rect = b.roi_rect(i)
                    assert rect == rounded_out(win, sw, sh, mw, mh, c.layout == "422" and s == 1), tag + (i, win, rect)
                    rx, ry, rw, rh = rect
                    assert rw * rh < sw * sh and rh < sh, tag + (i, rect)
                    x0, y0, w, h = win
                    after = b.fetch(i)
                    assert not np.array_equal(paint_px[i][y0:y0 + h, x0:x0 + w], plain_px[i][y0:y0 + h, x0:x0 + w]), tag + (i,)  # the paint is foreign
                    assert np.array_equal(after[y0:y0 + h, x0:x0 + w], plain_px[i][y0:y0 + h, x0:x0 + w]), tag + (i, win, rect)
                    outside = np.ones((sh, sw), bool)
                    outside[ry:ry + rh, rx:rx + rw] = False
                    assert np.array_equal(after[outside], paint_px[i][outside]), tag + (i, win, rect)
                n += 1
    assert n == 20
    # without crops roi=True is accepted and changes nothing
    one, _ = dec.decode(datas[:1], roi=True, dtype=torch.uint8, layout="HWC")
    assert dec._batch.roi_rect(0) == (0, 0, 203, 77)
    two, _ = dec.decode(datas[:1], dtype=torch.uint8, layout="HWC")
    assert torch.equal(one, two)


# ------------------------------------------------------------------ 6. rules

def _set(ica, b, slot, *r):
    L = ica.lib()
    L.mij_batch_set_roi.argtypes = [C.c_void_p] + [C.c_int] * 5
    return L.mij_batch_set_roi(b._h, int(slot), *[int(v) for v in r])


def _rect(ica, b, slot):
    L = ica.lib()
    L.mij_batch_slot_roi_rect.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int * 4)]
    r = (C.c_int * 4)()
    return L.mij_batch_slot_roi_rect(b._h, int(slot), C.byref(r)), tuple(r)


def test_rules(ica, gpu_ctx, oracle):
    case = dense("420", (80, 48))
    px = want(oracle, case, 3)
    b = ica.Batch(gpu_ctx, 8, 16 * MB, 16 * MB, 16 * MB)
    try:
        s0, s1 = b.add_jpeg(case.stream(), 3), b.add_jpeg(case.stream(), 3)
        for r in ((-1, 0, 4, 4), (0, -1, 4, 4), (77, 0, 4, 4), (0, 45, 4, 4), (0, 0, 81, 1), (0, 0, 1, 49), (80, 0, 1, 1), (3, 3, 0, 5), (3, 3, 5, 0), (3, 3, -2, 4),
                  (0, 0, 2 ** 31 - 1, 1)):
            assert _set(ica, b, s0, *r) == MIJ_E_ARG, r
        assert _set(ica, b, 9, 0, 0, 4, 4) == MIJ_E_ARG
        assert _rect(ica, b, s0)[0] == MIJ_E_STATE  # valid after upload only
        # a region on slot 0 only leaves slot 1 whole and exact; a later call replaces the region
        assert _set(ica, b, s0, 0, 0, 4, 4) == 0 and _set(ica, b, s0, 40, 20, 9, 9) == 0
        b.upload()
        assert _set(ica, b, s0, 0, 0, 4, 4) == MIJ_E_STATE
        L = ica.lib()
        L.mij_batch_set_roi_auto.argtypes = [C.c_void_p, C.c_int, C.c_int]
        assert L.mij_batch_set_roi_auto(b._h, s0, 1) == MIJ_E_STATE
        b.launch()
        b.wait()
        assert b.roi_rect(s0) == (32, 16, 32, 16) and b.roi_rect(s1) == (0, 0, 80, 48)
        assert np.array_equal(b.fetch(s1), px)
        assert np.array_equal(b.fetch(s0)[20:29, 40:49], px[20:29, 40:49])
        assert b.slot_path(s0) == b.slot_path(s1) == 1
        # hash_out and diff_slots refuse the slot with a region, and serve the other
        with pytest.raises(ica.MijError, match="region"):
            b.hash_out(s0)
        with pytest.raises(ica.MijError, match="region"):
            b.diff_slots([(s0, s1)])
        assert b.diff_slots([(s1, s1)]) == 0 and b.hash_out(s1)
        # reset forgets the region; a clone has none; w == h == 0 takes a region back
        b.reset()
        s0 = b.add_jpeg(case.stream(), 3)
        s1 = b.add_jpeg(case.stream(), 3)
        b.set_roi(s1, 0, 0, 8, 8)
        s2 = b.add_clone(s1)
        s3 = b.add_jpeg(case.stream(), 3)
        b.set_roi(s3, 0, 0, 8, 8)
        b.set_roi(s3, 0, 0, 0, 0)
        b.submit()
        b.wait()
        assert b.roi_rect(s0) == b.roi_rect(s2) == b.roi_rect(s3) == (0, 0, 80, 48) and b.roi_rect(s1) == (0, 0, 16, 16)
        assert b.hash_out(s0) == b.hash_out(s2) == b.hash_out(s3)
        # float output and a region refuse each other, in either order
        b.reset()
        b.reserve_out_f32(4 * MB)
        f, g, a = b.add_jpeg(case.stream(), 3), b.add_jpeg(case.stream(), 3), b.add_jpeg(case.stream(), 3)
        b.set_out_f32(f)
        assert _set(ica, b, f, 0, 0, 8, 8) == MIJ_E_ARG and b"float" in L.mij_last_error()
        assert L.mij_batch_set_roi_auto(b._h, f, 1) == MIJ_E_ARG and b"float" in L.mij_last_error()
        b.set_roi(g, 0, 0, 8, 8)
        with pytest.raises(ica.MijError, match="region"):
            b.set_out_f32(g)
        # an automatic region without a request is refused at upload
        b.set_roi_auto(a)
        with pytest.raises(ica.MijError, match="no tensor request"):
            b.upload()
        assert L.mij_batch_upload(b._h) == MIJ_E_STATE
        b.set_roi_auto(a, False)
        b.upload()
        # a request whose window leaves an explicit region is refused at upload; inside it, it is served
        b.reset()
        t = b.add_jpeg(case.stream(), 3)
        out = torch.zeros((10, 12, 3), dtype=torch.uint8, device="cuda:0")
        b.set_out_tensor(t, out.data_ptr(), 0, 0, 30, 20, 12, 10, 36)
        b.set_roi(t, 31, 20, 20, 20)
        assert L.mij_batch_upload(b._h) == MIJ_E_ARG and b"outside the slot's region" in L.mij_last_error()
        b.set_roi(t, 30, 20, 12, 10)
        torch.cuda.synchronize()
        b.submit()
        b.wait()
        assert np.array_equal(out.cpu().numpy(), px[20:30, 30:42])
        # the region is validated again against the scale in force
        b.reset()
        t = b.add_jpeg(case.stream(), 3)
        b.set_roi(t, 40, 24, 40, 24)
        b.set_scale(t, 2)
        assert L.mij_batch_upload(b._h) == MIJ_E_ARG and b"stored picture" in L.mij_last_error()
        b.set_roi(t, 20, 12, 20, 12)
        b.upload()
        assert b.roi_rect(t) == (16, 8, 24, 16)
    finally:
        b.close()
