"""The LIBJPEG ENCODING contract (include/mij_host.h) on the CPU.  Pillow's files (tests/golden/libjpeg_pillow_enc.npz) are the judge:
tests/libjpeg_enc_model.py, the numpy restatement, gives their coefficients; the host twin (mjh_write_jpg_libjpeg_to_memory) gives their
bytes, whole files, and the model's units; the multiply-high quantiser divides exactly; what is refused is refused; and the default
writer's bytes are what they were."""
import hashlib
import os
import sys

import numpy as np
import pytest

import libjpeg_enc_model as EM
import libjpeg_model as LM

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "libjpeg_pillow_enc.npz")
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_libjpeg_enc as mg  # noqa: E402  (the set's sizes and its properties; Pillow is only needed to regenerate)

KINDS = {"b": {}, "o": {"optimize": True}, "p": {"progressive": True}, "r": {"restart_rows": 1}}


def parse(name):
    """-> (sampling, quality, kind, ycbcr)"""
    p = name.split("_")
    return ("444" if p[0] == "ycc444" else p[0]), int(p[2][1:]), p[4], p[0] == "ycc444"


def load_goldens():
    z = np.load(FIXTURE)
    return [(str(n), z["src_" + str(n)], z["jpg_" + str(n)].tobytes()) for n in z["names"]]


@pytest.fixture(scope="module")
def goldens():
    return load_goldens()


def test_fixture_holds_what_it_is_for(goldens):
    assert os.path.getsize(FIXTURE) < 700 * 1024
    mg.properties(goldens)


def test_model_coefficients_equal_every_golden(ica, goldens):
    """dummy blocks included: detile_coefficients gives the whole-MCU grids"""
    bad = []
    for name, src, jpg in goldens:
        sampling, quality, _, ycbcr = parse(name)
        planes, _, factors, size = LM.coefficients(jpg)
        got = EM.coefficients(src, sampling, quality, ycbcr=ycbcr)
        assert size == (src.shape[1], src.shape[0]) and len(got) == len(planes) == EM.SAMPLING[sampling][0], name
        assert factors[0] == EM.SAMPLING[sampling][1:], name
        if not all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, planes)):
            bad.append(name)
    assert not bad, "%d of %d differ from Pillow: %s" % (len(bad), len(goldens), bad[:8])


def test_model_tables_are_the_goldens_tables(ica, goldens):
    for name, src, jpg in goldens:
        sampling, quality, _, _ = parse(name)
        _, tables, _, _ = LM.coefficients(jpg)
        want = EM.quality_tables(quality)
        for c, t in enumerate(tables):
            assert np.array_equal(np.asarray(t).reshape(64), want[min(c, 1)]), (name, c)


def test_host_twin_writes_every_golden_whole(ica, goldens):
    bad = []
    for name, src, jpg in goldens:
        sampling, quality, kind, ycbcr = parse(name)
        if ycbcr:
            continue  # plane input: below
        got = ica.write_jpg_libjpeg_to_memory(src, quality, sampling, **KINDS[kind])
        if got != jpg:
            bad.append(name)
    assert not bad, "%d files differ from Pillow's: %s" % (len(bad), bad[:8])


def test_host_twin_units_equal_the_model(ica, goldens):
    for name, src, jpg in goldens:
        sampling, quality, kind, ycbcr = parse(name)
        if ycbcr or kind != "b":
            continue
        t, du = ica.host_transform_libjpeg(src, quality, sampling)
        assert np.array_equal(du, EM.units(src, sampling, quality)), name
        assert ica.sampling_name(t) == sampling


def test_plane_twin_equals_the_ycbcr_and_grey_goldens(ica, goldens):
    """the plane input's host twin: Pillow's "YCbCr"-mode file and its "L" files, data units and (reframed) bytes"""
    seen = 0
    for name, src, jpg in goldens:
        sampling, quality, kind, ycbcr = parse(name)
        if not (ycbcr or (sampling == "grey" and kind == "b")):
            continue
        picture = tuple(np.ascontiguousarray(src[..., c]) for c in range(3)) if ycbcr else src
        t, du = ica.host_transform_libjpeg_planes(picture, sampling, quality)
        assert np.array_equal(du, EM.units(src, sampling, quality, ycbcr=ycbcr)), name
        assert ica.libjpeg_reframe(ica.emit_transcoded(t, du)) == jpg, name
        seen += 1
    assert seen == 1 + len(mg.SIZES)


def test_flip_is_the_flipped_picture(ica, goldens):
    for name, src, jpg in goldens:
        if name.startswith(("420_17x15_", "grey_9x8_", "422_33x31_")):
            sampling, quality, _, _ = parse(name)
            assert ica.write_jpg_libjpeg_to_memory(src[::-1], quality, sampling, flip=True) == jpg, name


@pytest.mark.parametrize("value", [1, 255])
def test_custom_tables_against_the_model(ica, goldens, value):
    tables = ([value] * 64, [value] * 64)
    for name, src, jpg in goldens:
        sampling, _, kind, ycbcr = parse(name)
        if ycbcr or kind != "b" or src.shape[0] > 40:
            continue
        t, du = ica.host_transform_libjpeg(src, 90, sampling, qtables=tables)
        assert np.array_equal(du, EM.units(src, sampling, qtables=tables)), name
        data = ica.write_jpg_libjpeg_to_memory(src, 90, sampling, qtables=tables)
        planes, tabs, _, _ = LM.coefficients(data)
        assert all((np.asarray(tb) == value).all() for tb in tabs), name
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(EM.coefficients(src, sampling, qtables=tables), planes)), name


def test_multiply_high_quantiser_divides_exactly(ica):
    """every |x| <= 32768 against every divisor 8 q, q = 1..255"""
    x = np.arange(-32768, 32769, dtype=np.int64)
    for q in range(1, 256):
        want = np.sign(x) * ((np.abs(x) + 4 * q) // (8 * q))
        assert np.array_equal(ica.libjpeg_quantise_all(q), want), q


def test_default_sampling_is_420(ica):
    rgb = mg.picture([1], 24, 24, False, "natural")
    assert ica.write_jpg_libjpeg_to_memory(rgb, 95) == ica.write_jpg_libjpeg_to_memory(rgb, 95, "420")
    assert ica.sampling_name(ica.libjpeg_plan(24, 24, 3, 95)) == "420"


def test_refusals(ica):
    rgb = mg.picture([2], 16, 16, False, "noise")
    assert ica.write_jpg_libjpeg_to_memory(rgb, 90, "440") is None
    assert ica.libjpeg_plan(16, 16, 3, 90, "440") is None
    for comp in (2, 4):
        px = np.zeros((16, 16, comp), np.uint8)
        for sampling in (None, "444", "grey"):
            assert ica.write_jpg_libjpeg_to_memory(px, 90, sampling) is None, (comp, sampling)
            assert ica.host_transform_libjpeg(px, 90, sampling) == (None, None)
    with pytest.raises(ValueError):
        ica.write_jpg_libjpeg_to_memory(rgb, 90, "420", qtables=([0] * 64, [1] * 64))
    y = np.zeros((16, 16), np.uint8)
    assert ica.host_transform_libjpeg_planes((y, y[:8], y[:8]), "440") == (None, None)
    with pytest.raises(ValueError):
        ica.write_jpg_libjpeg_to_memory(rgb, 90, "420", restart_rows=1, progressive=True)
    assert ica.libjpeg_reframe(b"\x00\x01\x02\x03") is None
    assert ica.libjpeg_reframe(b"\xff\xd8\xff\xdb\x00\x05\x00\x01\x02\xff\xda") is None  # a DQT segment cut short


def test_grey_of_rgb_is_the_luma(ica, goldens):
    """ "grey" of an RGB picture codes jccolor's Y: the grey file of the Y plane"""
    for name, src, jpg in goldens:
        if name.startswith("444_33x31_"):
            _, quality, _, _ = parse(name)
            y = EM.rgb_to_ycc(src)[0].astype(np.uint8)
            assert ica.write_jpg_libjpeg_to_memory(src, quality, "grey") == ica.write_jpg_libjpeg_to_memory(y, quality, "grey")


def test_default_writer_is_unchanged(ica):
    """the bytes of the writer without the request, pinned by digest: the writer's own two samplings and a sampled and a plane stream"""
    rgb = ica.synth_rgb(97, 61, seed=5)
    got = [ica.stbi_write_jpg_to_memory(rgb, 90), ica.stbi_write_jpg_to_memory(rgb, 95), ica.write_jpg_sampled_to_memory(rgb, 75, "422"),
           ica.write_jpg_sampled_to_memory(rgb, 75, "420", optimize=True), ica.write_jpg_sampled_to_memory(rgb, 75, "grey", progressive=True),
           ica.write_jpg_sampled_to_memory(rgb, 75, "444", restart_rows=1)]
    assert [hashlib.sha256(g).hexdigest()[:16] for g in got] == DEFAULT_DIGESTS


DEFAULT_DIGESTS = ['a1ede0bc8fd12eb4', '2d482740f7e61ec5', '60c1f6971e312cfc', 'f3a690a1645d6375', 'd769e1d2ee34fcf6', 'bbb223ddea82750f']
