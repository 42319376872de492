"""Region-of-interest decode across the seams its planner makes ("What the tests cover"): between two bands of a region,
between bands and column segments, between the 256-unit work items of the windowed kernels, and between slots of every kind in one launch.
Every slot is painted first; the whole decoded rectangle -- seams lie inside the rectangle, not necessarily inside the region -- has to be
the whole-picture decode (the oracle at full size, tests/scaled_model.py at reduced size), everything else the paint; and every slot has to
have been cut into the number of work items that tests/roi_cases.py derives from the planner's rules (mij_batch_slot_work_items), so that a
planner which stops cutting a region fails here instead of passing on one item."""
import ctypes as C

import numpy as np
import pytest
import torch

import roi_cases as RC
from roi_cases import MB, check_slot, dense, expected_items, paint, read_back, rounded_out, run_windows, stored_window, unit_px, want

pytestmark = pytest.mark.gpu

MIJ_FLAG_SKIP = 2
MIJ_E_ARG, MIJ_E_STATE = -2, -5


def _run(ica, ctx, oracle, case, wins, fmt, band_rows=0, producer="host"):
    """one batch of windows that share channels and scale: exact rectangle, exact item count"""
    req, s = wins[0].req, wins[0].s
    assert all(w.req == req and w.s == s for w in wins)
    items = [expected_items(case.layout, req, s, (case.w, case.h), w.win, band_rows) for w in wins]
    run_windows(ica, ctx, oracle, case, req, fmt, s, [w.win for w in wins], producer=producer, tag=("band rows %d" % band_rows,), whole_rect=True, items=items)
    return items


# ------------------------------------------------------------------ A. band seams

@pytest.mark.parametrize("layout", ("420", "440", "422"))
def test_band_seams(ica, gpu_ctx, oracle, layout, monkeypatch):
    """regions of every first and last MCU row on a picture of 11 MCU rows (4:2:2: 21, the lengths around its band height of eight): every
    band count from one to the picture's, seams next to MCU row 0 and next to the partial last MCU row, at the default band height (both
    plane formats, three and four channels, both producers) and at MIJ_BAND_ROWS 1, 2, 3 and 5 -- at 1 every MCU-row boundary inside a region
    is a seam.  4:2:2 has no halo and a band height of its own, which the variable must not change."""
    case = dense(layout, RC.BAND_PICTURES[layout])
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    wins = RC.band_windows(layout)
    assert len(wins) == (75 if layout == "422" else 66)
    seen = set()
    for fmt in ("compact", "int16"):
        for req in (3, 4):
            seen |= set(_run(ica, gpu_ctx, oracle, case, [RC.Win(w.name, w.win, req=req) for w in wins], fmt))
    seen |= set(_run(ica, gpu_ctx, oracle, case, wins, "compact", producer="walk"))
    assert seen == {1, 2, 3}  # 11 MCU rows in bands of four; 21 in bands of eight
    for env in RC.BAND_ROWS_ENV[1:]:
        monkeypatch.setenv("MIJ_BAND_ROWS", env)  # read when the batch is created
        got = _run(ica, gpu_ctx, oracle, case, wins, "compact", band_rows=int(env))
        assert max(got) == (3 if layout == "422" else -(-11 // int(env))), (env, max(got))


# ------------------------------------------------------------------ B. bands x segments

@pytest.mark.parametrize("layout", ("420", "440"))
def test_bands_and_segments(ica, gpu_ctx, oracle, layout):
    """two bands (MCU rows 1 to 6) of windows on either side of one column segment's LDS budget.  A segment and its two halo columns take
    (columns + 2) x 448 bytes of LDS for 4:2:0 and (columns + 2) x 304 bytes for 4:4:0, and two workgroups share a CU's 160 KiB: 180 columns
    of 4:2:0 (182 x 448 = 81536 <= 81920 < 183 x 448), 267 of 4:4:0 (269 x 304 = 81776 <= 81920 < 270 x 304).  Within the budget: 2 items;
    above it: 4.  The pictures themselves (200 and 300 MCU columns) are one workgroup wide without a region."""
    assert RC.FIT == {"420": 180, "440": 267}
    size, widths = RC.SEGMENT_PICTURES[layout]
    case = dense(layout, size)
    wins = RC.segment_windows(layout)
    for req, fmt in ((3, "compact"), (4, "int16")):
        items = _run(ica, gpu_ctx, oracle, case, [RC.Win(w.name, w.win, req=req) for w in wins], fmt)
        assert items == [2 if n <= RC.FIT[layout] else 4 for n in widths], items


# ------------------------------------------------------------------ C. the windowed 1 x 1 kernels past 256 units

@pytest.mark.parametrize("name", tuple(RC.BLOCK_PICTURES))
def test_block_windows_past_one_item(ica, gpu_ctx, oracle, name):
    """windows of 260 to 762 blocks from an odd block column: second and third work items that begin in the middle of a window row, a last
    item of four lanes, waves of a later item that lie in one window row (the LDS-transposed stores, where the pitch allows) and waves that
    span two; a width that is no multiple of four, a partial last block column and row (grey); the grey kernel over the luma plane of a
    4:2:0 picture; CMYK (with one channel: two-pass, the region dropped)"""
    layout, size, reqs, _ = RC.BLOCK_PICTURES[name]
    case = dense(layout, size)
    for req in reqs:
        wins = RC.block_windows(name, req)
        for fmt in ("compact", "int16"):
            items = _run(ica, gpu_ctx, oracle, case, wins, fmt)
            if name != "cmyk":
                assert items == [2, 2, 2, 3, 3]
            else:
                assert items == ([2] if req >= 3 else [10])


# ------------------------------------------------------------------ D. the windowed reduced-size kernels past 256 units

@pytest.mark.parametrize("layout", tuple(RC.SCALED_PICTURES))
def test_scaled_windows_past_one_item(ica, gpu_ctx, oracle, layout):
    """40 x 30 MCUs with a partial last column and row, at 1/2, 1/4 and 1/8 size: three items that each begin in the middle of a window row, a
    last item of three lanes, thirty runs of one MCU, a window into the partial last column and the last row; odd pixel offsets and odd
    reduced widths, so that with three channels the runs begin at every byte alignment.  4:2:0 also with one channel: luma blocks."""
    case = dense(layout, RC.SCALED_PICTURES[layout])
    for s in (2, 4, 8):
        for fmt in ("compact", "int16"):
            for req in (3, 4):
                assert _run(ica, gpu_ctx, oracle, case, RC.scaled_windows(layout, s, req), fmt) == [3, 2, 1, 2]
            if layout == "420":
                assert _run(ica, gpu_ctx, oracle, case, RC.scaled_windows(layout, s, 1), fmt) == [3]


# ------------------------------------------------------------------ E. one launch, many kinds

@pytest.mark.parametrize("fmt", ("compact", "int16"))
def test_one_launch_many_kinds(ica, gpu_ctx, oracle, fmt, monkeypatch):
    """a skipped slot 0, slots with regions of every family, slots without, a clone, reduced slots and a two-pass slot in one launch; then
    the same batch again after reset with the slots in another order, so that a window table (or a work list) left over from the first
    upload shows.  MIJ_BAND_ROWS = 4 (the regions' own default) fixes the band count of the 4:2:0 slots without a region."""
    monkeypatch.setenv("MIJ_BAND_ROWS", "4")
    spec = RC.mixed_slots()
    assert len(spec) == 13 and len({e[4] for e in spec if e[4]}) == sum(1 for e in spec if e[4])
    # second order: back to front, the clone still behind its source; the skipped slot comes last
    second = [e for e in reversed(spec) if e[5] != "clone"]
    k = next(i for i, e in enumerate(second) if e[0] == "420 two bands")
    second.insert(k + 1, spec[3])
    b = ica.Batch(gpu_ctx, len(spec), 64 * MB, 64 * MB, 64 * MB)
    try:
        b.set_coef_format(fmt)
        for rnd, order in enumerate((spec, second)):
            if rnd:
                b.reset()
            slots = []
            for name, layout, size, s, win, kind in order:
                case = dense(layout, size)
                if kind == "clone":
                    sl = b.add_clone(slots[-1])
                elif kind == "skip":
                    sl = b.add(ica.HostDecoder.probe(case.stream(), 3))
                    b.set_flags(sl, MIJ_FLAG_SKIP)
                else:
                    sl = b.add_jpeg(case.stream(), 3)
                    if s > 1:
                        b.set_scale(sl, s)
                    if win:
                        b.set_roi(sl, *win)
                slots.append(sl)
            assert slots == list(range(len(order)))
            # the getter speaks of the last upload: MIJ_E_STATE before it (also after reset, when an earlier upload's counts are stale)
            L = ica.lib()
            L.mij_batch_slot_work_items.argtypes = [C.c_void_p, C.c_int]
            assert L.mij_batch_slot_work_items(b._h, 1) == MIJ_E_STATE and b"before mij_batch_upload" in L.mij_last_error()
            with pytest.raises(ica.MijError, match="before mij_batch_upload"):
                b.work_items(1)
            b.upload()
            assert L.mij_batch_slot_work_items(b._h, len(order)) == MIJ_E_ARG and L.mij_batch_slot_work_items(b._h, -1) == MIJ_E_ARG
            b.wait()
            pxs = [want(oracle, dense(e[1], e[2]), 3, e[3]) for e in order]
            pats = [paint(ica, b, sl, px.size, 91 + 13 * rnd + sl).reshape(px.shape) for sl, px in zip(slots, pxs)]
            b.launch()
            b.wait()
            for sl, (name, layout, size, s, win, kind), px, pat in zip(slots, order, pxs, pats):
                t = (fmt, "round %d" % rnd, "slot %d" % sl, name)
                if kind == "skip":
                    assert b.slot_path(sl) == 0 and b.work_items(sl) == 0, t
                    assert np.array_equal(read_back(ica, b, sl, pat.shape), pat), t + ("a skipped slot was written",)
                    continue
                # a clone has no region; neither has a two-pass slot once planned, but it was asked for one and is checked as such
                items = expected_items(layout, 3, s, size, None if kind == "clone" else win, band_rows=4)
                check_slot(b, sl, dense(layout, size), 3, s, None if kind == "clone" else win, pat, px, t, whole_rect=True, items=items)
            by_name = {e[0]: b.work_items(sl) for sl, e in zip(slots, order)}
            assert by_name == {"skipped": 0, "420 whole": 3, "420 two bands": 2, "420 clone": 3, "444 two items": 2, "444 whole": 3, "grey window": 2,
                               "cmyk window": 2, "422 region": 2, "440 region": 3, "420 half size window": 3, "444 quarter size whole": 5, "411 region": 12}, by_name
    finally:
        b.close()


# ------------------------------------------------------------------ F. tensor path with tall crops

@pytest.fixture(scope="module")
def dec(ica, gpu_ctx):
    d = ica.TensorDecoder("cuda:0")
    yield d
    d.close()


def test_tensor_path_tall_crops(ica, dec):
    """decode(crops=..., roi=True) equals roi=False bit for bit on random-resized-crop windows, which are tall enough to be cut into several
    bands (test_gpu_roi.py's crops are at most 21 rows).  As there: between the two calls the decoder decodes OTHER pictures of the same
    sizes whole, so that the output regions hold foreign pixels; the decoded rectangle is the stored-frame window, found independently,
    rounded out; outside it the foreign pixels are still there.  The count at the end keeps the test from going vacuous: at least half of
    the slots that a band kernel decodes with a region in force were cut into two or more work items."""
    cases = [dense(lay, size, seed=3) for lay, size in RC.TENSOR_PICTURES]
    others = [dense(lay, size, seed=4) for lay, size in RC.TENSOR_PICTURES]
    n_each = 12
    datas = [c.stream() for c in cases for _ in range(n_each)]
    paint_datas = [c.stream() for c in others for _ in range(n_each)]
    owner = [c for c in cases for _ in range(n_each)]
    band_slots = band_cut = n = 0
    for reduce in (None, 2):
        s = reduce or 1
        for o in (1, 6, 8):
            for size in ((32, 32), None):
                crops = [c for per in RC.tensor_crops(o, s, size is not None, n_each) for c in per]
                kw = dict(crops=crops, size=size, orientation=o, reduce=reduce, dtype=torch.uint8, layout="HWC")
                tag = (reduce, o, size)
                plain, r0 = dec.decode(datas, roi=False, **kw)
                plain = plain.clone()
                b = dec._batch
                plain_px = [b.fetch(i) for i in range(len(datas))]
                dec.decode(paint_datas, roi=False, **kw)
                assert dec._batch is b  # the same arena, the same slots
                paint_px = [b.fetch(i) for i in range(len(datas))]
                got, r1 = dec.decode(datas, roi=True, **kw)
                assert dec._batch is b and r0 == r1 == [None] * len(datas), tag
                assert torch.equal(got, plain), tag
                for i, c in enumerate(owner):
                    sw, sh = b.out_size(i)
                    assert (sw, sh) == (-(-c.w // s), -(-c.h // s)), tag
                    win = stored_window(sw, sh, o, crops[i])
                    rx, ry, rw, rh = rect = b.roi_rect(i)
                    assert rect == rounded_out(win, sw, sh, *unit_px(c.layout, 3, s)), tag + (i, win, rect)
                    after = b.fetch(i)
                    assert not np.array_equal(paint_px[i][ry:ry + rh, rx:rx + rw], plain_px[i][ry:ry + rh, rx:rx + rw]), tag + (i,)  # the paint is foreign
                    assert np.array_equal(after[ry:ry + rh, rx:rx + rw], plain_px[i][ry:ry + rh, rx:rx + rw]), tag + (i, win, rect)
                    outside = np.ones((sh, sw), bool)
                    outside[ry:ry + rh, rx:rx + rw] = False
                    assert np.array_equal(after[outside], paint_px[i][outside]), tag + (i, win, rect)
                    whole = rect == (0, 0, sw, sh)  # a region that needs every unit is dropped
                    if not (whole and c.layout == "420" and s == 1):  # (left to itself, the band count of a whole 4:2:0 picture follows the device)
                        assert b.work_items(i) == expected_items(c.layout, 3, s, (c.w, c.h), win), tag + (i, win, b.work_items(i))
                    if b.slot_path(i) in (1, 4) and not whole:
                        band_slots += 1
                        band_cut += b.work_items(i) >= 2
                n += 1
    assert n == 12
    assert band_slots >= 100 and 2 * band_cut >= band_slots, (band_cut, band_slots)
