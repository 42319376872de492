"""The host contract of sampled encoding (include/mij_host.h, SAMPLED ENCODING: mjw_splan_init, mjw_stransform_host,
mjh_write_jpg_sampled_to_memory): default streams unchanged, luma independent of the sampling, the chroma means anchored on the
oracle's 4:4:4 stream, unit order and headers, given tables, and composition with optimised tables, restart intervals and progressive
scans.  No GPU."""
import numpy as np
import pytest

import helpers
import sampling_cases as sc


def enc(ica, img, q=90, sampling=None, **kw):
    data = ica.write_jpg_sampled_to_memory(img, q, sampling, **kw)
    assert data is not None
    return data


@pytest.fixture(scope="module")
def reference():
    return helpers.Reference() if helpers.Reference.available() else None


@pytest.mark.parametrize("q", [1, 50, 90, 91, 100])
def test_defaults_are_the_writers_bytes(ica, oracle, reference, q):
    """1: no sampling, and the writer's own sampling named, equal the oracle's (and the reference's) stream"""
    for comp in (1, 2, 3, 4):
        for k, (w, h) in enumerate(((1, 1), (7, 5), (16, 16), (33, 17))):
            img = sc.picture(w, h, comp, 100 * comp + k)
            want = oracle.encode(img, q)
            assert enc(ica, img, q) == want, (comp, w, h)
            assert enc(ica, img, q, sc.own_sampling(q)) == want, (comp, w, h)
            if reference is not None:
                assert reference.encode(img, q) == want, (comp, w, h)


@pytest.mark.parametrize("name", sc.SAMPLINGS)
@pytest.mark.parametrize("q", [50, 95])
def test_luma_does_not_depend_on_the_sampling(ica, oracle, name, q):
    """2: every luma block both streams hold, by block coordinates, has the oracle stream's quantised coefficients"""
    for k, (w, h) in enumerate(((17, 9), (9, 17), (1, 1), (40, 24))):
        img = sc.picture(w, h, 3, 7 * k + q)
        ours = sc.blocks(*sc.walk(ica, enc(ica, img, q, name)))[0]
        theirs = sc.blocks(*sc.walk(ica, oracle.encode(img, q)))[0]
        bh, bw = min(ours.shape[0], theirs.shape[0]), min(ours.shape[1], theirs.shape[1])
        assert bh >= (h + 7) // 8 and bw >= (w + 7) // 8
        assert np.array_equal(ours[:bh, :bw], theirs[:bh, :bw]), (name, q, w, h)


@pytest.mark.parametrize("w", [8, 12, 24])
@pytest.mark.parametrize("h", [8, 12, 24])
def test_means_anchored_on_the_oracles_444_stream(ica, oracle, w, h):
    """3: the mean of two equal floats is exact, so 4:2:2 of a picture with every column doubled, and 4:4:0 of one with every row
    doubled, carry the chroma blocks of the oracle's 4:4:4 stream of the picture itself; grey carries its luma blocks"""
    img = np.random.default_rng(w * 100 + h).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    _, cb, cr = sc.blocks(*sc.walk(ica, oracle.encode(img, 95)))
    for name, doubled in (("422", np.repeat(img, 2, axis=1)), ("440", np.repeat(img, 2, axis=0))):
        t, du = sc.walk(ica, enc(ica, doubled, 95, name))
        assert (t.ncomp, t.lh, t.lv) == sc.FACTORS[name]
        _, cb2, cr2 = sc.blocks(t, du)
        assert cb2.shape == cb.shape
        assert np.array_equal(cb2, cb) and np.array_equal(cr2, cr), (name, w, h)
    t, du = sc.walk(ica, enc(ica, img, 95, "grey"))
    assert np.array_equal(sc.blocks(t, du)[0], sc.blocks(*sc.walk(ica, oracle.encode(img, 95)))[0])


@pytest.mark.parametrize("name", sc.SAMPLINGS)
def test_unit_order_and_headers(ica, oracle, name):
    """4: the walk's descriptor reports the requested components and factors, the stream decodes to the right size, the DQT tables
    are the quality's, and the walked units are mjw_stransform_host's in order"""
    img = sc.picture(37, 21, 3, 11)
    data = enc(ica, img, 75, name)
    t, du = sc.walk(ica, data)
    ncomp, lh, lv = sc.FACTORS[name]
    assert t.ncomp == ncomp and (ncomp == 1 or (t.lh, t.lv) == (lh, lv))
    plan, want = ica.host_transform_sampled(img, 75, name)
    assert plan.plan.du_per_mcu == (1 if ncomp == 1 else lh * lv + 2) and plan.plan.subsample == int(name == "420")
    assert np.array_equal(du, want)
    kind, pixels, comp = oracle.load(data)
    assert kind == "ok" and pixels.shape == (21, 37, ncomp) and comp == ncomp
    luma, chroma = ica.quality_tables(75)
    tabs = sc.stream_tables(data)
    assert tabs[0] == list(luma) and (ncomp == 1) == (1 not in tabs) and (ncomp == 1 or tabs[1] == list(chroma))
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("Pillow is not installed")
    import io
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (37, 21) and im.mode == ("L" if ncomp == 1 else "RGB")


def test_tables(ica, oracle):
    """5: the tables of a quality given as qtables are that quality's bytes; other tables reach the stream; bad ones raise"""
    img = sc.picture(33, 17, 3, 5)
    for q in (10, 75, 95):
        assert enc(ica, img, 90, sc.own_sampling(q), qtables=ica.quality_tables(q)) == oracle.encode(img, q), q
    for pair in (([1] * 64, [1] * 64), ([255] * 64, [255] * 64), sc.random_tables(3)):
        for name in ("420", "422", "grey"):
            data = enc(ica, img, 90, name, qtables=pair)
            t, _ = sc.walk(ica, data)
            assert list(t.plan.ytab) == pair[0] and (name == "grey" or list(t.plan.ctab) == pair[1])
            assert sc.stream_tables(data)[0] == pair[0]
            assert oracle.load(data)[0] == "ok"
    for bad in (([0] * 64, [1] * 64), ([1] * 63, [1] * 64), ([256] * 64, [1] * 64), ([1] * 64,), 5, ([1.5] * 64, [1] * 64)):
        with pytest.raises(ValueError):
            ica.write_jpg_sampled_to_memory(img, 90, "420", qtables=bad)
    for bad in ("411", "4:2:0", 420, b"420", ""):
        with pytest.raises(ValueError):
            ica.write_jpg_sampled_to_memory(img, 90, bad)
    assert ica.sampled_plan(8, 8, 5, 90, "420") is None and ica.sampled_plan(0, 8, 3, 90, "grey") is None


@pytest.mark.parametrize("name", ["422", "grey"])
def test_composition_on_the_host(ica, name):
    """6: optimised tables, restart intervals and progressive scans carry the plain stream's coefficients"""
    img = sc.picture(40, 24, 3, 9)
    plain = enc(ica, img, 75, name)
    t0, du0 = sc.walk(ica, plain)
    for kw in ({"optimize": True}, {"restart_mcus": 1}, {"restart_rows": 1}, {"progressive": True}):
        data = enc(ica, img, 75, name, **kw)
        assert data != plain
        t, du = sc.walk(ica, data)
        assert (t.ncomp, t.lh, t.lv, t.plan.mcu_x, t.plan.mcu_y) == (t0.ncomp, t0.lh, t0.lv, t0.plan.mcu_x, t0.plan.mcu_y)
        if "progressive" not in kw:
            assert np.array_equal(du, du0), kw
            continue
        # a progressive stream codes the AC coefficients of luma in scans of luma alone, which cover ceil(W / 8) x ceil(H / 8) blocks
        # (T.81 A.2.3): the luma blocks that only pad the last MCU column keep their DC and lose nothing a decoder shows
        assert np.array_equal(du[:, 0], du0[:, 0]), kw
        for got, want in zip(sc.blocks(t, du), sc.blocks(t0, du0)):
            assert np.array_equal(got[:3, :5], want[:3, :5]), kw
    assert b"\xff\xdd\x00\x04\x00\x01" in enc(ica, img, 75, name, restart_mcus=1)
    mcu_x = t0.plan.mcu_x
    assert b"\xff\xdd\x00\x04" + bytes([mcu_x >> 8, mcu_x & 255]) in enc(ica, img, 75, name, restart_rows=1)
    with pytest.raises(ValueError):
        ica.write_jpg_sampled_to_memory(img, 75, name, restart_mcus=1, progressive=True)
