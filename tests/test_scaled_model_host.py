"""The reduced-size decode contract on the CPU: identities of tests/scaled_model.py (the K tables against their formula, the full lengths
against idct_model, N = 1 against the DC shortcut, coefficients outside the kept rectangle), its anchor on the reference for DC-only
pictures, its closeness to Pillow's Image.reduce of the full-size decode (gain, offset and siting blunders), and the argument checks of
TensorDecoder.decode(reduce=...) that need no device."""
import numpy as np
import pytest

import coef_cases as CC
import idct_model as M
import scaled_model as SM

# mean absolute difference between the model at scale s and Image.reduce(s) of the reference's full-size pixels, measured with the
# pictures of test_close_to_full_size_decoding (DESIGN.md 4g has the table); the test asserts 1.5 x these: the margin covers other
# seeds, not other arithmetic
MEASURED_MAD = {("420", 2): 0.982, ("420", 4): 0.587, ("420", 8): 0.442, ("444", 2): 1.011, ("444", 4): 0.587, ("444", 8): 0.437}


def test_k_tables_are_the_formula():
    for n in (1, 2, 4):
        assert np.array_equal(SM.K[n], SM.k_formula(n)), n
        assert (SM.K[n][:, 0] == 4096).all()
    # the length-8 weights are the reference's own, which differ from the formula by its float rounding: only their DC weight is pinned
    assert (M.first_pass_weights()[:, 0] == 4096).all()


def _random_blocks(seed, n=400, big=False):
    r = np.random.default_rng(seed)
    b = r.integers(-60, 61, (n, 8, 8))
    b[:, 0, 0] = r.integers(-1040, 1041, n)
    if big:  # first-pass outputs beyond int16, products that wrap
        b[::3] = r.integers(-32768, 32768, (len(b[::3]), 8, 8))
    return b


def test_full_lengths_are_idct_exact():
    for big in (False, True):
        b = _random_blocks(1 + big, big=big)
        assert np.array_equal(SM.block_transform(b, 8, 8), M.idct_exact(b))


def test_n1_is_the_dc_shortcut():
    """sample = clamp(((short)(dc * q0) * 16384 + 65536 + (128 << 17)) >> 17): the class-0 formula of the sparse kernels"""
    d = np.arange(-1040, 1041)
    blocks = np.zeros((d.size, 8, 8), np.int64)
    blocks[:, 0, 0] = d
    blocks[:, 1:, 1:] = 77  # never read
    want = np.clip((d * 16384 + 65536 + (128 << 17)) >> 17, 0, 255)
    assert np.array_equal(SM.block_transform(blocks, 1, 1)[:, 0, 0], want)
    # and a DC-only block is flat, with the same value, at every length
    blocks[:, 1:, 1:] = 0
    for nv, nh in ((2, 2), (4, 4), (8, 8), (4, 8), (1, 2), (2, 4), (8, 4)):
        s = SM.block_transform(blocks, nv, nh)
        assert (s == want[:, None, None]).all(), (nv, nh)


def test_coefficients_outside_the_kept_rectangle_change_nothing():
    b = _random_blocks(5, big=True)
    for nv, nh in ((1, 1), (2, 2), (4, 4), (1, 2), (2, 4), (4, 8), (2, 1)):
        cut = np.zeros_like(b)
        cut[:, :nv, :nh] = b[:, :nv, :nh]
        assert np.array_equal(SM.block_transform(b, nv, nh), SM.block_transform(cut, nv, nh)), (nv, nh)


def test_colour_row_is_the_oracles(oracle):
    g = np.array(CC.GRID)
    y, cb, cr = [a.reshape(-1).astype(np.uint8) for a in np.meshgrid(g, g, g, indexing="ij")]
    assert np.array_equal(SM.ycbcr_to_rgb(y, cb, cr), oracle.ycc(y, cb, cr, 3))


@pytest.mark.parametrize("layout", ["444", "grey"])
def test_dc_only_pictures_are_the_reference_sampled(oracle, layout):
    """DC-only blocks are flat at full size and hold the same value at every scale: the model equals the oracle's decode[::s, ::s]"""
    cases = [CC.dc_sweep(layout, 0)] + ([CC.colour_grid("444")] if layout == "444" else [])
    for case in cases:
        for req in ((1, 2, 3, 4) if layout == "grey" else (3, 4, 1)):
            kind, full, _ = oracle.load(case.stream(), req)
            assert kind == "ok"
            for s in (2, 4, 8):
                got = SM.scaled_picture(case.dequantised(), layout, (case.w, case.h), s, req)
                assert np.array_equal(got, full[::s, ::s]), (case.name, req, s)


def _planes_of(ica, data):
    desc, arena = ica.HostDecoder.decode(data, 0)
    nat = ica.detile_coefficients(desc, arena)
    return [M.dequant(nat[c].astype(np.int64), np.array(desc.dequant[desc.comp[c].tq], np.int64).reshape(8, 8)) for c in range(desc.ncomp)]


def _mad(a, b):
    return float(np.abs(a.astype(np.int64) - b.astype(np.int64)).mean())


@pytest.mark.parametrize("layout", ["420", "444"])
def test_close_to_full_size_decoding(ica, oracle, layout):
    """The model against Pillow's Image.reduce(s) of the reference's full-size pixels, on the project's synthetic pictures; a one-sample
    shift of the model's output and a gain of 0.9 must both leave the bound"""
    from PIL import Image
    w, h = 256, 192
    data = ica.synth_jpeg(w, h, seed=11, quality=90) if layout == "420" else ica.synth_jpeg(w, h, seed=12, quality=95)
    planes = _planes_of(ica, data)
    hv = [(2, 2), (1, 1), (1, 1)] if layout == "420" else [(1, 1)] * 3
    assert [tuple(p.shape[:2]) for p in planes] == [(h // 8 * v // (2 if layout == "420" else 1), w // 8 * hh // (2 if layout == "420" else 1)) for hh, v in hv]
    full = oracle.load(data, 3)[1]
    for s in (2, 4, 8):
        want = np.asarray(Image.fromarray(full).reduce(s))
        got = SM.scaled_picture(planes, layout, (w, h), s, 3)
        assert got.shape == want.shape
        mad, bound = _mad(got, want), 1.5 * MEASURED_MAD[(layout, s)]
        shifted = min(_mad(got[:, 1:], want[:, :-1]), _mad(got[1:], want[:-1]))
        gain = _mad(np.rint(got * 0.9), want)
        print("layout %s s %d: mad %.3f (bound %.3f), shifted %.3f, gain 0.9 %.3f" % (layout, s, mad, bound, shifted, gain))
        assert mad <= bound, (layout, s, mad)
        assert shifted > bound and gain > bound, (layout, s, shifted, gain, bound)


# ---------------------------------------------------------------- binding: argument errors before any device call

def _decoder(ica):
    import torch
    return ica.TensorDecoder("cuda:0"), torch


@pytest.mark.parametrize("bad", [3, 0, 16, -2, True, 2.0, "half", [2], [2, 3], [2, None]])
def test_bad_reduce_values(ica, bad):
    dec, _ = _decoder(ica)
    data = ica.synth_jpeg(32, 32, seed=1, quality=90)
    with pytest.raises(ValueError):
        dec.decode([data, data], reduce=bad)


def test_auto_needs_size_and_no_crops(ica):
    dec, _ = _decoder(ica)
    data = ica.synth_jpeg(32, 32, seed=1, quality=90)
    with pytest.raises(ValueError, match="auto"):
        dec.decode([data], reduce="auto")
    with pytest.raises(ValueError, match="auto"):
        dec.decode([data], reduce="auto", size=(8, 8), crops=[(0, 0, 16, 16)])


def test_auto_rule_and_supported_layouts(ica):
    from image_codecs_amd import tensor_out as T
    assert T.auto_reduce(1920, 1080, 224, 224) == 4
    assert T.auto_reduce(1792, 1792, 224, 224) == 8
    assert T.auto_reduce(1791, 1792, 224, 224) == 8  # ceil(1791 / 8) = 224
    assert T.auto_reduce(1784, 1792, 224, 224) == 4
    assert T.auto_reduce(447, 448, 224, 224) == 2 and T.auto_reduce(446, 448, 224, 224) == 1
    assert T.auto_reduce(100, 100, 224, 224) == 1
    for layout, ok in (("420", True), ("422", True), ("444", True), ("grey", True), ("440", False), ("411", False), ("rgb", False), ("cmyk", False), ("ycck", False)):
        d = ica.HostDecoder.probe(CC.edge_pairs(layout, (40, 24)).stream(), 3)
        assert T.reducible(d) == ok, layout
