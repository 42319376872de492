"""The float loaders' host side (no GPU needed): the stbi__ldr_to_hdr tables of mjh_ldr_to_hdr_lut against libm, failures
that come before the device is needed, and a compiled C caller of the new prototypes."""
import numpy as np
import pytest

import loadf_expect as fx


@pytest.mark.parametrize("n_out", [1, 2, 3, 4])
def test_lut_equals_libm_expression(ica, n_out):
    for gamma in (2.2, 1.0, 0.5, 3.7):
        for scale in (1.0, 2.5):
            got = ica.ldr_to_hdr_lut(n_out, gamma, scale)
            assert fx.same_bits(got, fx.lut(n_out, gamma, scale)), (n_out, gamma, scale)


def test_lut_default_is_gamma_2_2_scale_1(ica):
    assert fx.same_bits(ica.ldr_to_hdr_lut(3), fx.lut(3, 2.2, 1.0))
    t = ica.ldr_to_hdr_lut(2)
    assert t[1, 255] == np.float32(1.0) and t[1, 51] == np.float32(51) / np.float32(255)  # alpha: v / 255.0f, no gamma


def test_bad_req_comp_reads_unknown_image_type(ica):
    data = ica.synth_jpeg(40, 24, seed=2)
    for req in (5, 6, -1):
        assert ica.stbi_load_from_memory(data, req) is None
        assert ica.stbi_failure_reason() == "bad req_comp"
        assert ica.stbi_loadf_from_memory(data, req) is None
        assert ica.stbi_failure_reason() == "unknown image type"  # convert.c:302 overwrites it


def test_header_failures_read_unknown_image_type(ica, golden):
    """Every golden stream the reference rejects: where the 8-bit loader gives the reference's own reason on this machine (the
    failure comes before the device is needed), the float loader gives "unknown image type"."""
    seen = 0
    for name in golden.names:
        for req in range(5):
            kind, why = golden.expect(name, req)
            if kind != "fail":
                continue
            data = golden.jpg(name)
            assert ica.stbi_load_from_memory(data, req) is None
            if ica.stbi_failure_reason() != why:
                continue  # fails later, on the device side
            assert ica.stbi_loadf_from_memory(data, req) is None, (name, req)
            assert ica.stbi_failure_reason() == "unknown image type", (name, req)
            seen += 1
    for data in (b"", b"garbage", b"\xff\xd8", b"\xff\xd8\xff\xc0\x00\x03"):
        assert ica.stbi_loadf_from_memory(data, 3) is None
        assert ica.stbi_failure_reason() == "unknown image type"
        seen += 1
    assert seen >= 8


def test_no_gpu_keeps_its_reason(ica):
    data = ica.synth_jpeg(40, 24, seed=3)
    got = ica.stbi_loadf_from_memory(data, 3)
    if ica.gpu_available():
        assert got is not None and got[0].dtype == np.float32
    else:
        assert got is None and ica.stbi_failure_reason() == "no gpu device"


def test_loadf_cannot_open(ica, tmp_path):
    assert ica.stbi_loadf(str(tmp_path / "missing.jpg"), 3) is None
    assert ica.stbi_failure_reason() == "can't fopen"


def test_c_caller_compiles_and_links(ica, tmp_path):
    exe = fx.build_caller(tmp_path)
    import os
    assert os.access(exe, os.X_OK)
