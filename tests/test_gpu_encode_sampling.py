"""Sampled encoding on the GPU (mij_enc_add_ex and its kin, k_encode422 / k_encode440 / k_encode_grey; TensorEncoder's subsampling= and
qtables=): data units bit for bit mjw_stransform_host's, streams byte for byte mjh_write_jpg_sampled_to_memory's, default streams
unchanged, and the streams decode inside the library to what the oracle decodes."""
import numpy as np
import pytest
import torch

import sampling_cases as sc

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def tenc(ica, gpu_ctx):
    e = ica.TensorEncoder()
    yield e
    e.close()


def unit_cases(name):
    """(picture, flip): comp 1..4 at the small sizes, the kernel's seam size, and a flipped picture"""
    out = []
    for comp in (1, 2, 3, 4):
        for k, (w, h) in enumerate(sc.SMALL_SIZES):
            out.append((sc.picture(w, h, comp, 10 * comp + k), False))
    w, h = sc.SEAM_SIZE[name]
    out.append((sc.picture(w, h, 3, 77), False))
    out.append((sc.picture(w, h, 3, 78), True))
    out.append((sc.picture(37, 21, 4, 79), True))
    return out


@pytest.mark.parametrize("name", sc.SAMPLINGS)
@pytest.mark.parametrize("q", [50, 95])
def test_gpu_units_equal_host_units(ica, gpu_ctx, name, q):
    """7: mij_enc_fetch against mjw_stransform_host, every slot of one upload"""
    cases = unit_cases(name)
    pix = sum(256 + (a.shape[1] + 16) * a.shape[0] * 3 for a, _ in cases)
    want = [ica.host_transform_sampled(a, q, name, flip=f) for a, f in cases]
    enc = ica.Encoder(gpu_ctx, len(cases), pix, sum(256 + t.du_elems() * 2 for t, _ in want))
    try:
        slots = [enc.add(a, q, f, sampling=name) for a, f in cases]
        enc.force_generic(True)  # sampled slots stay on their strip kernels
        enc.upload()
        enc.launch()
        for slot, (t, du), (a, f) in zip(slots, want, cases):
            got = enc.fetch(slot)
            assert got.shape == du.shape, (a.shape, f)
            assert np.array_equal(got, du), (name, q, a.shape, f, int(np.argmax((got != du).any(axis=1))))
            tp = enc.tplan(slot)
            assert (tp.ncomp, tp.lh, tp.lv, tp.plan.mcu_x, tp.plan.du_per_mcu) == (t.ncomp, t.lh, t.lv, t.plan.mcu_x, t.plan.du_per_mcu)
    finally:
        enc.close()


def test_gpu_units_under_given_tables(ica, gpu_ctx):
    """7, tables: the reciprocal tables of given qtables reach the kernels"""
    pair = sc.random_tables(4)
    img = sc.picture(50, 34, 3, 5)
    enc = ica.Encoder(gpu_ctx, 8, 1 << 20, 1 << 20)
    try:
        names = (None,) + sc.SAMPLINGS
        slots = [enc.add(img, 90, sampling=n, qtables=pair) for n in names]
        enc.upload()
        enc.launch()
        for n, slot in zip(names, slots):
            t, du = ica.host_transform_sampled(img, 90, n, pair)
            assert np.array_equal(enc.fetch(slot), du), n
            assert list(enc.tplan(slot).plan.ytab) == pair[0]
    finally:
        enc.close()


@pytest.mark.parametrize("name", sc.SAMPLINGS)
def test_tensor_encoder_streams_equal_the_host_twin(ica, tenc, name):
    """8: CHW, HWC and strided uint8 tensors, and float16 / float32 through encode_normalized"""
    a, b = sc.picture(*sc.SEAM_SIZE[name], 3, 21), sc.picture(45, 27, 3, 22)
    for q in (50, 95):
        want = [ica.write_jpg_sampled_to_memory(x, q, name) for x in (a, b)]
        assert tenc.encode([dev(a), dev(b)], quality=q, layout="HWC", subsampling=name) == want
        assert tenc.last_subsampling == [name, name]
        assert tenc.encode([dev(a).permute(2, 0, 1).contiguous(), dev(b).permute(2, 0, 1).contiguous()], quality=q, subsampling=name) == want
    big = dev(sc.picture(64, 40, 3, 23))
    view = big[5:32, 7:52]  # a strided HWC view
    assert tenc.encode([view], layout="HWC", subsampling=name) == [ica.write_jpg_sampled_to_memory(view.cpu().numpy(), 90, name)]
    chw = big.permute(2, 0, 1).contiguous()[:, 3:30, 1:40]  # a strided CHW view
    assert tenc.encode([chw], subsampling=name) == [ica.write_jpg_sampled_to_memory(big[3:30, 1:40].cpu().numpy(), 90, name)]
    for dt in (torch.float16, torch.float32):
        f = (dev(b).permute(2, 0, 1).contiguous().to(torch.float32) / 255.0).to(dt)
        assert tenc.encode_normalized([f], quality=75, subsampling=name) == [ica.write_jpg_sampled_to_memory(b, 75, name)], dt
    grey = sc.picture(45, 27, 1, 24)
    assert tenc.encode([dev(grey[:, :, 0])], subsampling=name) == [ica.write_jpg_sampled_to_memory(grey, 90, name)]


def test_mixed_samplings_in_one_call(ica, tenc):
    """8: one picture of each sampling, and one left to the quality, in one call: one upload carries every work list"""
    names = list(sc.SAMPLINGS) + [None]
    imgs = [sc.picture(70 + 9 * k, 33 + 5 * k, 3, 30 + k) for k in range(len(names))]
    for q in (90, 95):
        got = tenc.encode([dev(x) for x in imgs], quality=q, layout="HWC", subsampling=names)
        assert got == [ica.write_jpg_sampled_to_memory(x, q, n) for x, n in zip(imgs, names)]
        assert tenc.last_subsampling == list(sc.SAMPLINGS) + [sc.own_sampling(q)]
    pair = sc.random_tables(6)
    got = tenc.encode([dev(x) for x in imgs], layout="HWC", subsampling=names, qtables=pair)
    assert got == [ica.write_jpg_sampled_to_memory(x, 90, n, qtables=pair) for x, n in zip(imgs, names)]
    q75 = tuple(list(t) for t in ica.quality_tables(75))
    assert tenc.encode([dev(imgs[0])], layout="HWC", qtables=q75) == tenc.encode([dev(imgs[0])], layout="HWC", quality=75)


@pytest.mark.parametrize("name", ["422", "440", "grey"])
def test_emission_composes(ica, tenc, name):
    """9: optimised tables, restart intervals and progressive scans: GPU emission equals host emission"""
    imgs = [sc.picture(*sc.SEAM_SIZE[name], 3, 41), sc.picture(17, 9, 3, 42), sc.picture(544, 24, 3, 43)]
    ts = [dev(x) for x in imgs]
    for kw in ({"optimize": True}, {"restart_rows": 1}, {"restart_mcus": 3}, {"progressive": True}):
        got = tenc.encode(ts, quality=75, layout="HWC", subsampling=name, **kw)
        assert got == [ica.write_jpg_sampled_to_memory(x, 75, name, **kw) for x in imgs], kw
        assert tenc.last_host_emitted == 0 or "progressive" in kw
    mcu_x = [ica.sampled_plan(x.shape[1], x.shape[0], 3, 75, name).plan.mcu_x for x in imgs]
    tenc.encode(ts, quality=75, layout="HWC", subsampling=name, restart_rows=1)
    assert tenc.last_restarts == mcu_x


def test_a_small_arena_finishes_sampled_slots_on_the_host(ica, gpu_ctx):
    """9: a slot that does not fit the arena is finished from its units under its own plan"""
    t = ica.TensorEncoder()
    try:
        t.reserve_arena(1024)
        imgs = [sc.picture(120, 80, 3, 50 + k) for k in range(3)]
        names = ["422", "grey", "440"]
        got = t.encode([dev(x) for x in imgs], layout="HWC", subsampling=names)
        assert got == [ica.write_jpg_sampled_to_memory(x, 90, n) for x, n in zip(imgs, names)]
        assert t.last_host_emitted >= 1
    finally:
        t.close()


@pytest.mark.parametrize("q", [90, 95])
def test_default_streams_unchanged(ica, oracle, tenc, q):
    """10: without the new arguments, and with the writer's own sampling named, the oracle's bytes"""
    imgs = [sc.picture(w, h, c, 60 + w) for (w, h, c) in ((544, 48, 3), (33, 17, 3), (7, 5, 1), (40, 24, 4))]
    want = [oracle.encode(x, q) for x in imgs]
    ts = [dev(x if x.shape[2] > 1 else x[:, :, 0]) for x in imgs]
    assert tenc.encode(ts, quality=q, layout="HWC") == want
    assert tenc.encode(ts, quality=q, layout="HWC", subsampling=sc.own_sampling(q)) == want
    assert tenc.last_subsampling == [sc.own_sampling(q)] * len(imgs)


def test_argument_errors(ica, tenc):
    x = dev(sc.picture(16, 16, 3, 1))
    for kw in ({"subsampling": "411"}, {"subsampling": ["420", "444"]}, {"subsampling": 420}, {"qtables": ([1] * 64, [0] * 64)},
               {"qtables": ([1] * 64, [1] * 63)}, {"qtables": sc.random_tables(1), "quality": 75}):
        with pytest.raises(ValueError):
            tenc.encode([x], layout="HWC", **kw)


def test_round_trip_inside_the_library(ica, oracle, tenc):
    """11: TensorDecoder.decode of the new streams equals the oracle's decode of the same bytes"""
    img = sc.picture(75, 43, 3, 70)
    dec = ica.TensorDecoder()
    try:
        for name in ("422", "440", "grey"):
            data = tenc.encode([dev(img)], layout="HWC", subsampling=name)[0]
            out, reasons = dec.decode([data], req_comp=3, layout="HWC", dtype=torch.uint8)
            assert reasons == [None], (name, reasons)
            kind, want, _ = oracle.load(data, 3)
            assert kind == "ok" and np.array_equal(out[0].cpu().numpy(), want), name
    finally:
        dec.close()
