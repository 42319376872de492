"""The host side of plane output (include/mij.h, PLANE OUTPUT): the model of the contract (planes_out_model.py) tied to the reference's
pixels, the shapes the binding reports, and the arguments TensorDecoder.decode_ycbcr refuses before it touches a device.  No GPU."""
import numpy as np
import pytest

import coef_cases as CC
import helpers
import planes_cases as pc
import planes_out_cases as POC
import planes_out_model as PM


@pytest.fixture(scope="module")
def reference():
    return helpers.Reference() if helpers.Reference.available() else None


def _loaders(oracle, reference):
    return [oracle] + ([reference] if reference is not None else [])


@pytest.mark.parametrize("layout", ("420", "422", "440", "444", "411"))
def test_luma_plane_is_the_reference_luma(oracle, reference, layout):
    """one requested channel of a YCbCr file is its luma untouched: the model's Y plane, byte for byte"""
    for size in ((33, 17), (17, 9), (8, 8), (1, 1)):
        case = POC.picture(layout, size)
        y = POC.planes_of(oracle, case)[0]
        assert y.shape == (size[1], size[0])
        for ld in _loaders(oracle, reference):
            kind, px, _ = ld.load(case.stream(), 1)
            assert kind == "ok"
            assert np.array_equal(px[:, :, 0], y), (layout, size, type(ld).__name__)


def test_luma_plane_of_real_files(ica, oracle, reference, golden):
    """the same through Oracle.coef's call order: a progressive file and a baseline file of the product's own writer"""
    for data in (golden.jpg("prog_420_23x41"), ica.synth_jpeg(77, 45, seed=3, quality=90), golden.jpg("grey_1x1")):
        pl, (w, h, hv, _) = POC.stream_planes(oracle, data)
        assert [p.shape for p in pl] == PM.shapes(w, h, hv)
        for ld in _loaders(oracle, reference):
            kind, px, _ = ld.load(data, 1)
            assert kind == "ok"
            assert np.array_equal(px[:, :, 0], pl[0])


def test_444_planes_give_the_reference_pixels(oracle, reference):
    """4:4:4 has no upsampling: the colour row over the model's three planes is the decoded picture"""
    for size in ((33, 17), (17, 9), (1, 1)):
        case = POC.picture("444", size)
        y, cb, cr = POC.planes_of(oracle, case)
        rgb = oracle.ycc(y.reshape(-1), cb.reshape(-1), cr.reshape(-1), 3).reshape(size[1], size[0], 3)
        for ld in _loaders(oracle, reference):
            kind, px, _ = ld.load(case.stream(), 3)
            assert kind == "ok"
            assert np.array_equal(px, rgb), (size, type(ld).__name__)


def test_call_order_agrees_with_the_planes(oracle):
    """the two sources of blocks agree: Oracle.coef of a synthetic case's stream gives the planes Case.dequantised gives"""
    for layout in ("420", "411", "grey", "cmyk"):
        case = POC.picture(layout, (33, 17))
        pl, (w, h, hv, prog) = POC.stream_planes(oracle, case.stream())
        assert (w, h, hv, prog) == (33, 17, POC.hv_of(layout), False)
        for a, b in zip(pl, POC.planes_of(oracle, case)):
            assert np.array_equal(a, b), layout


@pytest.mark.parametrize("layout", sorted(CC.LAYOUTS))
def test_plane_shapes(ica, layout):
    hv = CC.LAYOUTS[layout][0]
    for w, h in ((1, 1), (8, 8), (17, 9), (33, 17)):
        case = CC.Case("shape_%s_%dx%d" % (layout, w, h), "shape", layout, w, h, CC._tame(CC.blank(layout, w, h)))
        d = ica.HostDecoder.probe(case.stream())
        got = ica.HostDecoder.plane_shapes(d)
        hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
        assert got == [(-(-h * b // vmax), -(-w * a // hmax)) for a, b in hv] == PM.shapes(w, h, hv), (layout, w, h)
        if layout in pc.SAMPLINGS:
            assert got == pc.shapes(w, h, layout)


def test_rect_of_a_window():
    hv = CC.LAYOUTS["420"][0]
    assert PM.rect(267, 69, hv, 0, (6, 10, 101, 37)) == (6, 10, 101, 37)
    assert PM.rect(267, 69, hv, 1, (6, 10, 101, 37)) == (3, 5, 51, 19)
    assert PM.rect(267, 69, hv, 2, (266, 68, 1, 1)) == (133, 34, 1, 1)
    assert PM.rect(267, 69, hv, 1) == (0, 0, 134, 35)
    assert not PM.on_grid(267, 69, hv, (5, 10, 8, 8), (0, 1, 2)) and PM.on_grid(267, 69, hv, (5, 11, 8, 8), (0,))


def test_subsampling_names(ica):
    for layout, name in (("420", "420"), ("422", "422"), ("440", "440"), ("444", "444"), ("grey", "grey"), ("411", "h4v1")):
        case = POC.picture(layout, (17, 9))
        assert ica.ycbcr_subsampling(ica.HostDecoder.probe(case.stream())) == name


def test_decode_ycbcr_refuses_before_any_device_call(ica):
    """every ValueError of decode_ycbcr, on a machine that may have no GPU: none of them reaches a device call"""
    import torch
    dec = ica.TensorDecoder("cuda:0")
    a = POC.picture("420", (33, 17)).stream()
    g = POC.picture("grey", (33, 17)).stream()
    y, c = torch.zeros((17, 33), dtype=torch.uint8), torch.zeros((9, 17), dtype=torch.uint8)
    bad = [
        dict(format="i420"), dict(format=None), dict(luma_only=1),
        dict(crops=[(0, 0, 8, 8)]),                                    # one window for two pictures
        dict(crops=[(0, 0, 8), None]),                                 # not (x0, y0, w, h)
        dict(crops=[(0, 0, 34, 8), None]), dict(crops=[None, (0, 10, 8, 8)]), dict(crops=[(0, 0, 0, 8), None]), dict(crops=[(-2, 0, 8, 8), None]),
        dict(crops=[(1, 0, 8, 8), None]), dict(crops=[(0, 3, 8, 8), None]),  # off the chroma grid of a 4:2:0 file
        dict(out=[None]),                                              # one entry for two pictures
        dict(out=[(y, c), None]),                                      # two planes, three expected
        dict(out=[(y, c, torch.zeros((9, 16), dtype=torch.uint8)), None]),
        dict(out=[(y, c, c.to(torch.int16)), None]),
        dict(out=[(y, c, c), None]),                                   # right shapes, not on the GPU
        dict(out=[(y, c, torch.zeros((1, 17), dtype=torch.uint8).expand(9, 17)), None]),  # rows that share memory
        dict(out=[None, (y, c, c)]),                                   # a grey file is its Y plane alone
        dict(format="nv12", out=[(y, torch.zeros((9, 17, 3), dtype=torch.uint8)), None]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            dec.decode_ycbcr([a, g], **kw)
    # an off-grid window is fine where only luma is wanted
    with pytest.raises(ValueError):
        dec.decode_ycbcr([a], crops=[(1, 3, 8, 8)], luma_only=True, out=[torch.zeros((8, 9), dtype=torch.uint8)])  # on the grid: the shape is what is wrong
    # rejected pictures need no device either: nothing is left to decode
    pics, why = dec.decode_ycbcr([a[:40], POC.picture("cmyk", (17, 9)).stream()])
    assert pics == [None, None] and why[0] and "mij_batch_set_out_planes" in why[1]
    assert dec.last_subsampling == [None, None]
