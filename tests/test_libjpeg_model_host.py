"""The LIBJPEG ARITHMETIC contract (include/mij.h) on the CPU: tests/libjpeg_model.py, the numpy restatement the kernels are tested
against, gives Pillow's pixels byte for byte -- for every file of tests/golden/libjpeg_pillow.npz, and, where Pillow is importable, for
freshly written files of a seeded sweep of sizes, samplings, qualities and contents."""
import io
import os
import sys

import numpy as np
import pytest

import libjpeg_model as LM

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "libjpeg_pillow.npz")
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_libjpeg as mg  # noqa: E402  (the set's sizes and its properties; Pillow is only needed to regenerate)


@pytest.fixture(scope="module")
def goldens():
    z = np.load(FIXTURE)
    return [(str(n), z["jpg_" + str(n)].tobytes(), z["pix_" + str(n)]) for n in z["names"]]


def test_fixture_holds_what_it_is_for(goldens):
    assert os.path.getsize(FIXTURE) < 700 * 1024
    mg.properties(goldens)
    names = [n for n, _, _ in goldens]
    for sampling in ("444", "422", "420", "grey"):
        for w, h in mg.SIZES:
            assert sum(n.startswith("%s_%dx%d_" % (sampling, w, h)) for n in names) == 2, (sampling, w, h)
    assert sum(n.startswith("440_") for n in names) == len(mg.SIZES_440)
    assert any(n.startswith("420_160x120_") for n in names)


def test_model_equals_every_golden(ica, goldens):
    bad = []
    for name, data, pix in goldens:
        got = LM.decode(data, 1 if pix.ndim == 2 else 3)
        if not np.array_equal(got if pix.ndim == 3 else got[..., 0], pix):
            bad.append(name)
    assert not bad, "%d of %d differ from Pillow: %s" % (len(bad), len(goldens), bad[:8])


def test_model_channel_forms(ica, goldens):
    """n_out 4 is n_out 3 with alpha 255; n_out 1 of a colour file is its luma plane alone; a grey file is replicated"""
    for name, data, pix in goldens:
        if not name.startswith(("420_15x17_", "grey_15x17_", "440_17x17_")):
            continue
        p3, p4, p1, p2 = (LM.decode(data, n) for n in (3, 4, 1, 2))
        assert np.array_equal(p4[..., :3], p3) and (p4[..., 3] == 255).all()
        assert np.array_equal(p2[..., 0], p1[..., 0]) and (p2[..., 1] == 255).all()
        planes, tables, factors, (w, h) = LM.coefficients(data)
        assert np.array_equal(p1[..., 0], LM.component_plane(planes[0], tables[0], w, h))
        if pix.ndim == 2:
            assert all(np.array_equal(p3[..., c], pix) for c in range(3))


def test_model_equals_pillow_on_fresh_files(ica):
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("Pillow is not installed")
    rng = np.random.default_rng(20261021)
    n = bad = 0
    for k in range(120):
        sampling = ("444", "422", "420", "grey", "440")[k % 5]
        w, h = (int(v) for v in rng.integers(1, 72, 2))
        if sampling == "440":
            h = w
        quality = int(rng.choice([1, 5, 30, 50, 75, 90, 95, 100]))
        content = ("noise", "ramp")[int(rng.integers(0, 2))]
        progressive = bool(rng.integers(0, 2)) and sampling != "440"
        img = mg.picture([k, w, h], w, h, sampling == "grey", content)
        data = mg.encode(img, "422" if sampling == "440" else sampling, quality, progressive)
        if sampling == "440":
            data = mg.as_440(data)
        im = Image.open(io.BytesIO(data))
        want = np.asarray(im if sampling == "grey" else im.convert("RGB"))
        got = LM.decode(data, 1 if sampling == "grey" else 3)
        n += 1
        bad += not np.array_equal(got if want.ndim == 3 else got[..., 0], want)
    assert n == 120 and bad == 0, "%d of %d fresh files differ from Pillow" % (bad, n)
