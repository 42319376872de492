"""Region-of-interest decode, the part that needs no GPU: the argument check of TensorDecoder.decode(roi=...), the C surface, and the
generators of tests/roi_cases.py -- that the windows test_gpu_roi_seams.py sends really cross the seams their names speak of."""
import os
import re

import numpy as np
import pytest

import helpers
import roi_cases as RC

NEW = ("mij_batch_set_roi", "mij_batch_set_roi_auto", "mij_batch_slot_roi_rect", "mij_batch_slot_work_items")


@pytest.mark.parametrize("bad", (1, 0, None, "yes", [True], (0, 0, 8, 8)))
def test_decode_refuses_a_roi_that_is_no_bool(ica, bad):
    """before any device call: the decoder has no context, no batch and no device index afterwards, and the streams were not even parsed"""
    import torch  # noqa: F401  (the decoder module needs it)
    dec = ica.TensorDecoder("cuda")
    with pytest.raises(ValueError, match="roi"):
        dec.decode([b"not a jpeg"], crops=[(0, 0, 8, 8)], roi=bad)
    assert dec._ctx is None and dec._batch is None and dec._dev.index is None


def test_new_symbols_are_declared_and_exported(ica):
    src = open(os.path.join(helpers.ROOT, "include", "mij.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(mij_\w+)\s*\(", src, flags=re.M))
    L = ica.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name


def test_work_items_needs_a_batch_and_a_slot(ica):
    L = ica.lib()
    assert L.mij_batch_slot_work_items(None, 0) == -2  # MIJ_E_ARG


# ------------------------------------------------------------------ the generators of roi_cases.py

def _describe():
    return [(g, name, lay, size, w.name, w.win, w.req, w.s, w.seam, per, n) for g, name, lay, size, w, per, n in RC.every_seam_case()]


def test_window_lists_are_deterministic_and_inside_their_pictures():
    first, again = _describe(), _describe()
    assert first == again and len(first) > 1000
    assert {e[0] for e in first} == {"A", "B", "C", "D"}
    for g, name, lay, (W, H), wname, (x0, y0, w, h), req, s, seam, per, n in first:
        sw, sh = -(-W // s), -(-H // s)
        assert 0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= sw and y0 + h <= sh, (g, name, wname)
    for o in (1, 6, 8):
        for s in (1, 2):
            for sized in (True, False):
                a, b = RC.tensor_crops(o, s, sized), RC.tensor_crops(o, s, sized)
                assert a == b and [len(v) for v in a] == [12] * 3
                for (lay, (W, H)), crops in zip(RC.TENSOR_PICTURES, a):
                    sw, sh = -(-W // s), -(-H // s)
                    dw, dh = (sh, sw) if o >= 5 else (sw, sh)
                    assert all(0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= dw and y + h <= dh for x, y, w, h in crops)
                    assert sized or len({c[2:] for c in crops}) == 1


def test_no_window_needs_every_unit_and_first_columns_are_odd():
    for g, name, lay, size, w, per, n in RC.every_seam_case():
        need, have = RC.units_needed(lay, w.req, w.s, size, w.win)
        assert 0 < need < have, (g, name, w)
    for lay, size, _, wins in RC.BLOCK_PICTURES.values():
        assert all(x & 1 and x + w <= -(-size[0] // 8) and y + h <= -(-size[1] // 8) for w, h, x, y in wins), lay
    assert all(x & 1 for _, _, x, _ in RC.SCALED_WINDOWS + (RC.SCALED_LUMA_WINDOW,))
    for e in RC.mixed_slots():
        if e[4]:
            need, have = RC.units_needed(e[1], 3, e[3], e[2], e[4])
            assert 0 < need < have, e[0]


def test_seam_windows_have_more_than_one_item():
    """the counts by the rules of roi_cases.py, worked out here once more for the simple shapes"""
    cases = RC.every_seam_case()
    for g, name, lay, size, w, per, n in cases:
        assert n >= 1 and (n > 1 or not w.seam), (g, name, w, n)
    count = lambda g: [n for gg, *_, n in cases if gg == g]
    # A: with bands of one MCU row every pair a < b is cut; at the default height the 11-row pictures see 1, 2 and 3 bands
    for lay in ("420", "440"):
        for env in RC.BAND_ROWS_ENV:
            per = int(env or 4)
            got = [n for g, name, l, size, w, p, n in cases if g == "A" and l == lay and p == int(env or 0)]
            assert got == [-(-(b - a + 1) // per) for a in range(11) for b in range(a, 11)], (lay, env)
    got = {(w.name, p): n for g, name, l, size, w, p, n in cases if g == "A" and l == "422"}
    assert len(got) == 75 * 5 and all(n == -(-(int(k[0][4:].split("-")[1]) - int(k[0][4:].split("-")[0]) + 1) // 8) for k, n in got.items())
    assert {n for n in got.values()} == {1, 2, 3}
    # B: 2 bands x 1 or 2 segments, on either side of the budgets
    assert RC.FIT == {"420": 163840 // 896 - 2, "440": 163840 // 608 - 2} == {"420": 180, "440": 267}
    assert count("B") == [2, 4, 4, 2, 2, 4, 4]
    # C, D: ceil(units / 256); every picture has windows of two and of three items
    assert sorted(set(count("C"))) == [2, 3, 10] and sorted(set(count("D"))) == [1, 2, 3]
    seams = sum(1 for *_, w, _, _ in cases if w.seam)
    assert seams > len(cases) // 2, (seams, len(cases))


def test_mixed_slots_cover_every_kind():
    spec = RC.mixed_slots()
    assert [e[5] for e in spec] == ["skip", "plain", "plain", "clone"] + ["plain"] * 9 and spec[3][1:3] == spec[2][1:3]
    wins = [e[4] for e in spec if e[4]]
    assert len(wins) == 8 and len(set(wins)) == 8
    assert [RC.expected_items(e[1], 3, e[3], e[2], None if e[5] == "clone" else e[4], band_rows=4) for e in spec[1:]] == [3, 2, 3, 2, 3, 2, 2, 2, 3, 3, 5, 12]


def test_tensor_crops_are_mostly_cut_into_several_bands():
    """at full size, of the 4:2:0 and 4:2:2 slots whose region is in force (it is dropped when it needs every MCU row -- every MCU for 4:2:0)
    at least half are taller than one band"""
    slots = cut = 0
    for o in (1, 6, 8):
        for sized in (True, False):
            for (lay, (W, H)), crops in zip(RC.TENSOR_PICTURES, RC.tensor_crops(o, 1, sized)):
                if lay == "444":
                    continue
                for crop in crops:
                    win = RC.stored_window(W, H, o, crop)
                    if RC.rounded_out(win, W, H, *RC.unit_px(lay, 3, 1)) == (0, 0, W, H):
                        continue
                    slots += 1
                    cut += RC.expected_items(lay, 3, 1, (W, H), win) >= 2
    assert slots >= 100 and 2 * cut >= slots, (cut, slots)


def test_oracle_decodes_every_seam_picture(oracle):
    pics = RC.every_picture()
    assert len(pics) >= 18
    for lay, size, seed in pics:
        case = RC.dense(lay, size, seed)
        kind, px, _ = oracle.load(case.stream(), 3)
        assert kind == "ok" and px.shape == (size[1], size[0], 3), (lay, size)
        if lay in RC.SCALED_PICTURES and size == RC.SCALED_PICTURES[lay]:
            for s in (2, 4, 8):
                assert RC.want(oracle, case, 3, s).shape == (-(-size[1] // s), -(-size[0] // s), 3)
