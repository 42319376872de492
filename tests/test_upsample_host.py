"""The output-stage model (upsample_model.py) and the sample-level pictures (sample_cases.py) on the CPU: the model equals the oracle --
and the reference itself where it is built -- on every layout, size kind and channel count, and the pictures can tell a kernel that reads
the MCU padding, or the wrong neighbour, from one that does not, where an encoder-made picture of the same size cannot.

The GPU module (test_gpu_upsample.py) compares the kernels with the model alone; that the model is the reference's answer is shown here."""
import numpy as np
import pytest

import helpers
import sample_cases as S
import upsample_model as U

INTERPOLATING = [l for l in S.LAYOUTS if set(S.kinds(l)) & {"v_2", "h_2", "hv_2"}]
AIMS = {"noise": U.BLUNDERS, "stripes_h": (U.WRONG_SIDE, U.NO_RIGHT_CLAMP), "stripes_v": (U.NEAR_FAR_SWAPPED, U.NO_BOTTOM_CLAMP),
        "poison": (U.NO_RIGHT_CLAMP, U.NO_BOTTOM_CLAMP)}


@pytest.fixture(scope="module")
def reference():
    return helpers.Reference() if helpers.Reference.available() else None


def _agree(oracle, reference, case, reqs=(1, 2, 3, 4)):
    data = case.stream()
    for req in reqs:
        want = U.picture(case, req)
        kind, px, _ = oracle.load(data, req)
        assert kind == "ok" and px.shape == want.shape and np.array_equal(px, want), (case.name, req, "oracle")
        if reference is not None:
            kind, px, _ = reference.load(data, req)
            assert kind == "ok" and np.array_equal(px, want), (case.name, req, "reference")


def test_layout_table():
    """the additions are the upsampling layouts of make_golden_r2b.py that coef_cases lacks (and four-component YCbCr), and coef_cases' own
    table, families and everything() do not see them"""
    import coef_cases as CC
    from test_oracle_golden import LAYOUTS_R2
    have = {(tuple(hv), a) for hv, a in S.LAYOUTS.values()}
    for hv, a in LAYOUTS_R2:
        assert (tuple(hv), a) in have, (hv, a)
    assert not set(CC.EXTRA_LAYOUTS) & set(CC.LAYOUTS) and len(S.LAYOUTS) == len(CC.LAYOUTS) + 9
    assert {k for l in S.LAYOUTS for k in S.kinds(l)} == {"row_1", "v_2", "h_2", "hv_2", "generic"}


@pytest.mark.parametrize("layout", list(S.LAYOUTS))
def test_model_is_the_reference_noise_sweep(oracle, reference, layout):
    """every W in 1 .. 2 mw + 3 at nine heights and every H in 1 .. 2 mh + 3 at nine widths, nothing thinned: independent noise in every
    sample, padding included, so a model that read one sample from the wrong place would differ"""
    sizes = S.sweep_sizes(layout)
    mw, mh = S.mcu_px(layout)
    assert len(sizes) == (2 * mw + 3) * 9 + (2 * mh + 3) * 9 - 81
    for w, h in sizes:
        _agree(oracle, reference, S.make("noise", layout, w, h))


@pytest.mark.parametrize("layout", list(S.LAYOUTS))
def test_model_is_the_reference_stripes_poison_wide(oracle, reference, layout):
    """the other families at the nine-by-nine corner sizes, and every family once with the strong block that makes the picture WIDE"""
    for w, h in S.corner_sizes(layout):
        for family in ("stripes_h", "stripes_v", "poison"):
            _agree(oracle, reference, S.make(family, layout, w, h))
    mw, mh = S.mcu_px(layout)
    for family in S.FAMILIES:
        plain, wide = S.make(family, layout, 2 * mw + 3, mh + 1), S.make(family, layout, 2 * mw + 3, mh + 1, wide=True)
        assert wide.needs_wide() and not plain.needs_wide(), (family, plain.max_l1(), wide.max_l1())
        _agree(oracle, reference, wide)


def test_which_cases_are_wide():
    """no family passes MIJ_BLOCK_L1_LIMIT by itself at any sweep or corner size (noise comes closest, about 4600 of 5903), so the non-WIDE
    kernels get every family as it is and the WIDE ones get each through make(..., wide=True)"""
    worst = {f: 0 for f in S.FAMILIES}
    for layout in ("420", "422", "440", "ycck_k", "lumasub"):
        for w, h in S.corner_sizes(layout):
            for f in S.FAMILIES:
                worst[f] = max(worst[f], S.make(f, layout, w, h).max_l1())
    assert max(worst.values()) <= 5903, worst


# ------------------------------------------------------------------ the discriminating power of the inputs

def can_show(layout, size, blunder):
    """Whether the blunder changes the FORMULA of some pixel at this size, for some component the three-channel decode resamples -- from the
    reference's code alone, not from any picture:
      near / far swapped   v_2, hv_2: some output row has two different rows to mix: comp.y >= 2
      wrong side           h_2, hv_2: a sample has a neighbour: w_lores >= 2
      no right clamp       hv_2: the last pixel is the last form (t[w - 1] alone) only when W is even, and column w_lores must exist;
                           h_2: the same for even W; for odd W the last pixel is the last-but-one form, which becomes the interior form
                           (w_lores >= 2; no padding is read)
      no bottom clamp      v_2, hv_2: the last row mixes row comp.y - 1 with itself only when H is even, and row comp.y must exist"""
    W, H = size
    hv, hmax, vmax = S.factors(layout)
    import coef_cases as CC
    for (h, v), kind, (bh, bw) in zip(hv, S.kinds(layout), CC.geometry(layout, W, H)[2]):
        w, cy = -(-W // (hmax // h)), -(-H * v // vmax)
        if blunder == U.NEAR_FAR_SWAPPED and kind in ("v_2", "hv_2") and cy >= 2:
            return True
        if blunder == U.WRONG_SIDE and kind in ("h_2", "hv_2") and w >= 2:
            return True
        if blunder == U.NO_RIGHT_CLAMP and kind in ("h_2", "hv_2") and W % 2 == 0 and w < bw * 8:
            return True
        if blunder == U.NO_RIGHT_CLAMP and kind == "h_2" and W % 2 == 1 and w >= 2:
            return True
        if blunder == U.NO_BOTTOM_CLAMP and kind in ("v_2", "hv_2") and H % 2 == 0 and cy < bh * 8:
            return True
    return False


@pytest.mark.parametrize("layout", INTERPOLATING)
def test_every_family_shows_the_blunders_it_aims_at(layout):
    """at every corner size at which a blunder can change a pixel at all, each family that aims at it changes one; where it cannot (an odd
    width under hv_2, one chroma row, ...) the blundering model equals the reference -- on any input"""
    shown = {b: 0 for b in U.BLUNDERS}
    for size in S.corner_sizes(layout):
        for family, aims in AIMS.items():
            case = S.make(family, layout, *size)
            good = U.picture(case, 3)
            for b in U.BLUNDERS:
                changed = not np.array_equal(U.picture(case, 3, blunder=b), good)
                if not can_show(layout, size, b):
                    assert not changed, (case.name, b, "a blunder with no formula to change changed a pixel")
                elif b in aims:
                    assert changed, (case.name, b, "not shown")
                    shown[b] += 1
    kinds = set(S.kinds(layout))
    assert all(shown[b] >= 20 for b in (U.WRONG_SIDE, U.NO_RIGHT_CLAMP) if kinds & {"h_2", "hv_2"}), shown
    assert all(shown[b] >= 20 for b in (U.NEAR_FAR_SWAPPED, U.NO_BOTTOM_CLAMP) if kinds & {"v_2", "hv_2"}), shown


def _stream_planes(ica, data):
    """the sample planes a stream's own coefficients give (host walk, de-quantised, idct_model)"""
    import idct_model as M
    desc, arena = ica.HostDecoder.decode(data, 3)
    out = []
    for c, q in enumerate(ica.detile_coefficients(desc, arena)):
        dq = np.array(desc.dequant[desc.comp[c].tq][:], np.int64).reshape(8, 8)
        s = M.idct_exact(M.dequant(q.astype(np.int64), dq))
        out.append(np.ascontiguousarray(s.transpose(0, 2, 1, 3).reshape(q.shape[0] * 8, q.shape[1] * 8)))
    return out


@pytest.mark.parametrize("size", ((33, 17), (34, 18), (50, 38)))
def test_the_blind_spot_of_encoder_made_pictures(ica, oracle, size):
    """a 4:2:0 picture from the writer, whose padding repeats the edge: the model without the right-edge clamp and the model without the
    bottom clamp give the reference's pixels, bit for bit -- at 33 x 17 because no formula changes (odd W under hv_2, odd H), at the even
    sizes, where a sample-level picture shows both (above), because column wc and row comp.y hold what the clamp gives.  A flat picture
    makes that exact: replicated padding keeps every block flat, and a flat block survives quantisation as a flat block."""
    hv = [(2, 2), (1, 1), (1, 1)]
    W, H = size
    flat = np.empty((H, W, 3), np.uint8)
    flat[:] = (200, 40, 90)
    shown = 0
    for name, data in (("synth", ica.synth_jpeg(W, H, 3, 90)), ("flat", ica.stbi_write_jpg_to_memory(flat, 90))):
        planes = _stream_planes(ica, data)
        good = U.stage(planes, hv, "ycc", size, 3)
        assert np.array_equal(good, oracle.load(data, 3)[1]), name
        for b in (U.NO_RIGHT_CLAMP, U.NO_BOTTOM_CLAMP):
            diff = int((U.stage(planes, hv, "ycc", size, 3, blunder=b) != good).sum())
            if name == "flat" or not can_show("420", size, b):
                assert diff == 0, (name, size, b, diff)
            # (the noisy picture at an even size: quantisation moves its padding samples by a level or two, and a few bytes follow, off by one)
    for b in (U.NO_RIGHT_CLAMP, U.NO_BOTTOM_CLAMP):
        if can_show("420", size, b):
            case = S.make("poison", "420", W, H)
            shown += int(not np.array_equal(U.picture(case, 3, blunder=b), U.picture(case, 3)))
    assert shown == sum(can_show("420", size, b) for b in (U.NO_RIGHT_CLAMP, U.NO_BOTTOM_CLAMP))


# ------------------------------------------------------------------ the band forms

def test_band_form_switches():
    """the restated rules put the switches where the LDS arithmetic puts them: 448 / 304 / 256 + 16 bytes per MCU column against 160 KiB"""
    assert S.form_ranges("420") == [("MK_420T", 1, 24), ("MK_420S", 25, 56), ("MK_420", 57, 121), ("MK_420W", 122, 182), ("MK_420X", 183, 365)]
    assert S.form_ranges("422") == [("MK_422T", 1, 24), ("MK_422S", 25, 56), ("MK_422", 57, 213), ("MK_422W", 214, 319), ("MK_422X", 320, 639)]
    assert S.form_ranges("440") == [("MK_440", 1, 179), ("MK_440W", 180, 538)]
    assert [S.band_form("420", c) for c in (366, 367, 368, 540, 541)] == [("MK_420C", 3)] * 4 + [("MK_420C", 4)]
    assert [S.band_form("440", c) for c in (539, 801, 802)] == [("MK_440C", 3), ("MK_440C", 3), ("MK_440C", 4)]
    assert S.band_form("422", 640) == ("MK_RS_FAST+RS_H2", 1)
    import roi_cases
    assert roi_cases.FIT == {"420": 180, "440": 267}
