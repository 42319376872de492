"""Float pictures into the encoder, without a GPU: the de-normalising contract of include/mij.h (tests/denorm_model.py) inverts
tensor_tables to the byte, differs from a fused multiply-add where exact arithmetic says it must, and
TensorEncoder.encode_normalized refuses bad arguments before any device is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import denorm_model as dm

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
CASES = [(None, None), (dm.IM_MEAN, dm.IM_STD), ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("mean,std", CASES, ids=["plain", "imagenet", "half"])
def test_contract_inverts_tensor_tables(ica, dtype, mean, std):
    """what TensorDecoder writes for byte v comes back as v: every byte, every channel, all three dtypes"""
    tables = ica.tensor_tables(3, dtype, mean, std)
    scale, bias = dm.scale_bias(3, mean, std)
    for c in range(3):
        got = dm.denorm(dm.widen(tables[c]), scale[c], bias[c])
        assert np.array_equal(got, np.arange(256, dtype=np.uint8)), (c, np.flatnonzero(got != np.arange(256))[:8])


def test_scale_and_bias_are_the_binding_s(ica):
    """the model's derivation and the package's agree to the bit, and an InConvert holds those float32 values"""
    from image_codecs_amd.tensor_encode import denorm_scale_bias
    for mean, std in CASES + [((0.1, 0.2, 0.3, 0.4), (1 / 255, 2.0, 1e-3, 7.0))]:
        n = 3 if mean is None else len(mean)
        s, b = denorm_scale_bias(n, mean, std)
        ms, mb = dm.scale_bias(n, mean, std)
        assert np.array_equal(np.array(s, np.float32), ms) and np.array_equal(np.array(b, np.float32), mb)
        cv = ica.InConvert("bf16", s, b)
        assert cv.dtype == ica.MIJ_DT_BF16 and list(cv.scale)[:n] == [float(v) for v in ms] and list(cv.bias)[:n] == [float(v) for v in mb]
    assert C.sizeof(ica.InConvert) == 36
    assert hasattr(ica.lib(), "mij_enc_add_device_float")


def test_two_roundings_differ_from_a_fused_multiply_add():
    """at least 64 seeded (x, scale, bias) whose exactly-rounded fused result gives another byte; the model gives the contract's"""
    triples = dm.no_fma_triples()
    assert len(triples) >= 64, len(triples)
    for (x, scale, bias, two, one) in triples:
        assert two != one
        assert two == dm.two_roundings(x, scale, bias) and one == dm.one_rounding(x, scale, bias)
        assert int(dm.denorm(np.float32(x), np.float32(scale), np.float32(bias))) == two, (x, scale, bias)
    assert len({(float(x), float(s), float(b)) for (x, s, b, _, _) in triples}) == len(triples)


def test_model_special_values():
    """ties go to even, NaN and negatives to 0, +Inf and everything above to 255"""
    one, zero = np.float32(1), np.float32(0)
    x = np.array([0.5, 1.5, 2.5, 253.5, 254.5, 255.5, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-45, 254.50002, 300.0], np.float32)
    assert dm.denorm(x, one, zero).tolist() == [0, 2, 2, 254, 254, 255, 0, 0, 0, 255, 0, 0, 255, 255]
    for v in (0.5, 1.5, 2.5, 100.49999, 254.5, 7.0):
        assert dm.byte_of(np.float32(v)) == int(dm.denorm(np.float32(v), one, zero))


def test_encode_normalized_argument_errors_need_no_device(ica):
    enc = ica.TensorEncoder()
    a = torch.zeros((3, 16, 16), dtype=torch.float16)
    with pytest.raises(ValueError, match="uint8"):
        enc.encode([a])  # encode() keeps refusing float pictures
    with pytest.raises(ValueError, match="float"):
        enc.encode_normalized([torch.zeros((3, 16, 16), dtype=torch.uint8)])
    for dt in (torch.float64, torch.int32, torch.int8, torch.bool):
        with pytest.raises(ValueError, match="float16, bfloat16 or float32"):
            enc.encode_normalized([torch.zeros((3, 16, 16), dtype=dt)])
    with pytest.raises(ValueError, match="one dtype"):
        enc.encode_normalized([a, a.float()])
    for kw in ({"mean": [0.5, 0.5]}, {"std": [0.5] * 4}, {"mean": [0.5] * 3, "std": [0.5]}, {"mean": []}):
        with pytest.raises(ValueError, match="channels"):
            enc.encode_normalized([a], **kw)
    with pytest.raises(ValueError, match="channels"):
        enc.encode_normalized([a, torch.zeros((16, 16), dtype=torch.float16)], mean=[0.5] * 3)  # the grey picture has one channel
    with pytest.raises(ValueError, match="0"):
        enc.encode_normalized([a], std=[0.5, 0.0, 0.5])
    for bad in (float("nan"), float("inf"), -float("inf"), 1e38):  # 255e38 is not a float32
        with pytest.raises(ValueError, match="finite"):
            enc.encode_normalized([a], mean=[0.5, bad, 0.5])
        with pytest.raises(ValueError, match="finite"):
            enc.encode_normalized([a], std=[bad, 0.5, 0.5])
    with pytest.raises(ValueError, match="sequence"):
        enc.encode_normalized([a], mean=0.5)
    with pytest.raises(ValueError, match="finite"):
        enc.encode_normalized([], std=[float("nan")])  # checked even when there is nothing to encode
    # everything encode() refuses
    with pytest.raises(ValueError, match="GPU"):
        enc.encode_normalized([a])
    with pytest.raises(ValueError, match="GPU"):
        enc.encode_normalized([a], mean=dm.IM_MEAN, std=dm.IM_STD)
    with pytest.raises(ValueError, match="layout"):
        enc.encode_normalized([a], layout="NCHW")
    with pytest.raises(ValueError, match="channels"):
        enc.encode_normalized([torch.zeros((5, 16, 16), dtype=torch.float32)])
    for q in (-1, 101, 90.0, True, None):
        with pytest.raises(ValueError, match="quality"):
            enc.encode_normalized([a], quality=q)
    with pytest.raises(ValueError, match="optimize"):
        enc.encode_normalized([a], optimize=1)
    with pytest.raises(ValueError, match="4-D"):
        enc.encode_normalized(torch.zeros((2, 3, 16), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="stride"):
        enc.encode_normalized([torch.zeros((3, 16, 32), dtype=torch.float32)[:, :, ::2]])
    with pytest.raises(ValueError, match="stride"):
        enc.encode_normalized([torch.zeros((16, 16, 3), dtype=torch.float16).transpose(0, 1)], layout="HWC")
    with pytest.raises(ValueError, match="not a tensor"):
        enc.encode_normalized([np.zeros((3, 4, 4), np.float32)])
    assert enc.encode_normalized([]) == []
    assert enc._ctx is None and enc._enc is None  # nothing touched a device
