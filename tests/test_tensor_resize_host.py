"""Resized tensor output without a GPU: the library's host coefficients (mjh_resize_coeffs) against resize_model, resize_model against
Pillow (when it is installed), and TensorDecoder.decode's size / filter errors, raised before any device call."""
import numpy as np
import pytest
import torch

import resize_model as rm

PAIRS = [(1, 1), (1, 2), (2, 1), (1, 16384), (8192, 1), (7, 7), (224, 224), (1920, 224), (1080, 224), (224, 1920), (3, 5), (5, 3),
         (300, 299), (299, 300), (37, 13), (13, 37), (1000, 3), (3, 1000), (16384, 16384), (65535, 16384), (4000, 7)]


@pytest.mark.parametrize("name", rm.FILTERS)
def test_host_coeffs_equal_model(ica, name):
    rng = np.random.default_rng(7)
    pairs = PAIRS + [(int(a), int(b)) for a, b in rng.integers(1, 3000, (40, 2))]
    for n_in, n_out in pairs:
        lo, n, k = ica.resize_coeffs(n_in, n_out, name)
        mlo, mn, mk, ks = rm.coeffs(n_in, n_out, name)
        assert k.shape == (n_out, ks), (n_in, n_out)
        assert np.array_equal(lo, mlo) and np.array_equal(n, mn) and np.array_equal(k, mk), (name, n_in, n_out)
        assert (lo >= 0).all() and (n >= 1).all() and (lo + n <= n_in).all()  # taps never leave the input


def test_host_coeffs_refusals(ica):
    for args in ((0, 5, "bilinear"), (5, 0, "bilinear"), (5, 5, 5), (5, 5, -1)):
        with pytest.raises(ValueError):
            ica.resize_coeffs(*args)


def test_identity_axis_is_skipped(ica):
    """out == in: the contract skips the pass; the model returns the input"""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    for name in rm.FILTERS:
        assert np.array_equal(rm.resize(a, 11, 9, name), a)


def _pillow():
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


def test_model_equals_pillow():
    """the model equals Pillow's Image.resize of one "L" channel on seeded cases; only windows with h <= 50 * w, because Pillow
    runs the vertical pass first on some tall, narrow sources"""
    Image = _pillow()
    if Image is None:
        pytest.skip("Pillow is not installed")
    R = Image.Resampling
    pf = {"box": R.BOX, "bilinear": R.BILINEAR, "hamming": R.HAMMING, "bicubic": R.BICUBIC, "lanczos": R.LANCZOS}
    rng = np.random.default_rng(11)
    cases = 0
    while cases < 300:
        w, h = int(rng.integers(1, 260)), int(rng.integers(1, 260))
        if h > 50 * w:
            continue
        ow, oh = int(rng.integers(1, 260)), int(rng.integers(1, 260))
        name = rm.FILTERS[cases % 5]
        if cases % 2:
            a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        else:
            yy, xx = np.mgrid[0:h, 0:w]
            a = ((np.sin(xx / 7.0) + np.cos(yy / 5.0)) * 60 + 128).astype(np.uint8)
        want = np.asarray(Image.fromarray(a, "L").resize((ow, oh), pf[name]))
        assert np.array_equal(rm.resize(a, ow, oh, name), want), (w, h, ow, oh, name)
        cases += 1
    # every channel on its own: an RGB picture equals its three channels resized as "L"
    a = rng.integers(0, 256, (41, 67, 3), dtype=np.uint8)
    got = rm.resize(a, 29, 53, "bicubic")
    for c in range(3):
        assert np.array_equal(got[:, :, c], np.asarray(Image.fromarray(np.ascontiguousarray(a[:, :, c]), "L").resize((29, 53), R.BICUBIC)))


@pytest.fixture(scope="module")
def dec(ica):
    return ica.TensorDecoder("cuda:0")  # no device is touched before the arguments pass


def test_decode_resize_argument_errors_before_any_device_call(ica, dec):
    a, b = ica.synth_jpeg(64, 48, 1), ica.synth_jpeg(80, 40, 2)
    with pytest.raises(ValueError, match="filter"):
        dec.decode([a, b], size=(32, 32), filter="nearest")
    with pytest.raises(ValueError, match="filter"):
        dec.decode([a], size=(32, 32), filter=1)
    for bad in ((0, 32), (32, 0), (16385, 32), (32, 16385), (32,), (1, 2, 3), 32, (-1, 5)):
        with pytest.raises(ValueError, match="size"):
            dec.decode([a, b], size=bad)
    with pytest.raises(ValueError, match="outside"):  # windows are still checked against their pictures
        dec.decode([a, b], crops=[(0, 0, 20, 10), (61, 0, 20, 10)], size=(16, 16))
    with pytest.raises(ValueError, match="differ from out"):
        dec.decode([a, b], size=(16, 16), out=torch.empty((2, 3, 16, 17), dtype=torch.float16))
    with pytest.raises(ValueError, match="out is on"):  # sizes and windows pass: the next check is the device of out
        dec.decode([a, b], crops=[(0, 0, 20, 10), (3, 1, 21, 11)], size=(16, 16), out=torch.empty((2, 3, 16, 16), dtype=torch.float16))
    with pytest.raises(ValueError, match="out is on"):  # whole pictures of different sizes
        dec.decode([a, b], size=(16, 24), out=torch.empty((2, 3, 16, 24), dtype=torch.float16))
