"""Tensor output without a GPU: the normalisation tables against torch's own CPU arithmetic, TensorDecoder's argument errors (found
from headers before any device call) and the lazy torch import."""
import os
import subprocess
import sys

import pytest
import torch

import tensor_model as tm

MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_tables_match_torch_normalise_then_cast(ica, dtype, n):
    v = torch.arange(256, dtype=torch.float32)
    got = ica.tensor_tables(n, dtype)
    assert got.shape == (n, 256) and got.dtype == dtype
    for c in range(n):
        assert torch.equal(got[c].view(tm.BITS[dtype]), (v / 255).to(dtype).view(tm.BITS[dtype]))
    got = ica.tensor_tables(n, dtype, MEAN[:n], STD[:n])
    x = (v / 255).repeat(n, 1)
    want = ((x - torch.tensor(MEAN[:n])[:, None]) / torch.tensor(STD[:n])[:, None]).to(dtype)  # torch's broadcast normalise
    assert torch.equal(got.view(tm.BITS[dtype]), want.view(tm.BITS[dtype]))
    assert tm.same_bits(got, tm.tables(n, dtype, MEAN[:n], STD[:n]))


def test_tables_uint8_identity(ica):
    t = ica.tensor_tables(3, torch.uint8)
    assert t.dtype == torch.uint8 and t.shape == (3, 256)
    assert all(torch.equal(t[c], torch.arange(256).to(torch.uint8)) for c in range(3))
    with pytest.raises(ValueError):
        ica.tensor_tables(3, torch.uint8, MEAN[:3], STD[:3])
    with pytest.raises(ValueError):
        ica.tensor_tables(3, torch.float16, MEAN[:2], STD[:3])
    with pytest.raises(ValueError):
        ica.tensor_tables(3, torch.int32)


@pytest.fixture(scope="module")
def dec(ica):
    return ica.TensorDecoder("cuda:0")  # no device is touched before the arguments pass


def test_decode_argument_errors_before_any_device_call(ica, dec):
    a, b = ica.synth_jpeg(64, 48, 1), ica.synth_jpeg(80, 40, 2)
    with pytest.raises(ValueError, match="different sizes"):
        dec.decode([a, b])
    with pytest.raises(ValueError, match="outside"):  # off the right edge
        dec.decode([a, b], crops=[(0, 0, 20, 10), (61, 0, 20, 10)])
    with pytest.raises(ValueError, match="outside"):  # off the bottom edge
        dec.decode([a, b], crops=[(0, 0, 20, 10), (0, 31, 20, 10)])
    with pytest.raises(ValueError, match="outside"):
        dec.decode([a], crops=[(-1, 0, 20, 10)])
    with pytest.raises(ValueError, match="different sizes"):  # unequal windows
        dec.decode([a, b], crops=[(0, 0, 20, 10), (0, 0, 21, 10)])
    with pytest.raises(ValueError, match="mean has 2 values"):
        dec.decode([a, a], mean=[0.5, 0.5], std=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="std has 4 values"):
        dec.decode([a], req_comp=3, mean=[0.5] * 3, std=[1.0] * 4)
    with pytest.raises(ValueError, match="mean"):
        dec.decode([a], req_comp=1, mean=[0.5] * 3)
    with pytest.raises(ValueError):
        dec.decode([a], layout="NCHW")
    with pytest.raises(ValueError):
        dec.decode([a], dtype=torch.float64)
    with pytest.raises(ValueError):
        dec.decode([a, b], crops=[(0, 0, 20, 10)])
    with pytest.raises(ValueError):
        dec.decode([a], dtype=torch.uint8, mean=[0.5] * 3)
    with pytest.raises(ValueError, match="flip_x"):
        dec.decode([a, a], flip_x=[True])
    with pytest.raises(ValueError):
        ica.TensorDecoder("cpu")


def test_out_on_another_device_is_refused(ica, dec):
    a = ica.synth_jpeg(64, 48, 1)
    with pytest.raises(ValueError, match="out is on"):
        dec.decode([a], out=torch.empty((1, 3, 48, 64), dtype=torch.float16))


def test_import_leaves_torch_out():
    code = "import sys, image_codecs_amd as ica; assert 'torch' not in sys.modules; ica.Batch; assert 'torch' not in sys.modules; " \
           "ica.TensorDecoder; assert 'torch' in sys.modules"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
