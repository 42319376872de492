"""Restart intervals written on the GPU (mij_enc_set_restart; the tile cut, the segmented scans and the markers of
csrc/mij_emit_kernels.h, the restarted predictor of k_coef_units): every stream byte for byte what the host contract writes
(include/mij_host.h, RESTART INTERVALS), which tests/test_restart_host.py holds against libjpeg; slots without an interval still
what they were."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import emit_model as em
import helpers
import orient_coef_model as om

pytestmark = pytest.mark.gpu

ARENA = 16 << 20
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "restart_libjpeg.npz")
LAYOUTS = {"444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)], "grey": [(1, 1)]}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def noise(w, h, seed, c=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def source(ica, layout, w, h, seed=1, flat=False):
    """a baseline file of that sampling: the 4:4:4 units of a noise (or flat) picture re-laid (helpers.baseline_layout_from_444)"""
    a = np.full((h, w, 3), 90, np.uint8) if flat else noise(w, h, seed)
    plan, du = ica.host_transform(a, 95)
    assert plan.du_per_mcu == 3
    return helpers.baseline_layout_from_444(plan, du, LAYOUTS[layout])


def host(ica, data, ri, optimize=False, **kw):
    got, why = ica.transcode_memory(data, optimize=optimize, restart_mcus=ri, **kw)
    assert got is not None, why
    return got


def markers(stream):
    """the RSTn markers of a stream's entropy-coded segment, in order (a stuffed FF 00 is data)"""
    i = stream.index(b"\xff\xda")
    body = stream[i + 2 + (stream[i + 2] << 8 | stream[i + 3]):-2]
    return [body[k + 1] - 0xD0 for k in range(len(body) - 1) if body[k] == 0xFF and 0xD0 <= body[k + 1] <= 0xD7]


def transcode(ica, datas, **kw):
    t = ica.Transcoder()
    try:
        t.reserve_arena(ARENA)
        out = t.transcode(datas, copy_markers="none", **kw)
        return out, t.last_restarts, t.last_reasons, t.last_host_emitted
    finally:
        t.close()


def test_every_slot_kind_in_one_mixed_batch(ica, gpu_ctx):
    """host pixels, a device tensor, a float tensor, given units and coefficient slots (plain, orientation 6, requantised, crop + grey), with
    and without an interval, plain and optimised, in ONE launch: each stream is the host contract's at its slot's interval, and the slots
    without one are today's streams"""
    rng = np.random.default_rng(5)
    srcs = [source(ica, "420", 64, 48, 2), source(ica, "422", 48, 40, 3), source(ica, "444", 40, 24, 4), source(ica, "420", 80, 64, 6)]
    b = ica.Batch(gpu_ctx, len(srcs), ARENA, ARENA, ARENA)
    enc = ica.Encoder(gpu_ctx, 64, 8 << 20, 8 << 20)
    keep, want = [], []
    try:
        ok, sl, why = b.decode_jpegs(srcs, 0, threads=4, gpu_entropy=False)
        assert ok == len(srcs), why
        b.upload()
        enc.stream_reserve(ARENA)
        for k, (ri, opt) in enumerate([(0, False), (3, False), (1, True), (0, True), (7, True)]):
            a = noise(50 + k, 37, k)
            q = 90 if k & 1 else 95
            plan, du = ica.host_transform(a, q)
            t = dev(a)
            f = dev((a.astype(np.float32) / 255.0))
            keep += [t, f]
            conv = ica.InConvert(ica.MIJ_DT_F32, [255.0] * 3, [0.0] * 3)
            slots = [enc.add(a, q), enc.add_device(ica.InTensor(t.data_ptr(), ica.MIJ_LAYOUT_HWC, 50 + k, 37, 3, t.stride(0), 0), q),
                     enc.add_device_float(ica.InTensor(f.data_ptr(), ica.MIJ_LAYOUT_HWC, 50 + k, 37, 3, f.stride(0), 0), conv, q)]
            p2 = ica.binding.WritePlan()
            assert ica.lib().mjw_plan_init(C.byref(p2), 48, 32, 3, q)
            units = em.adversarial_units(rng, p2.mcu_x * p2.mcu_y, p2.du_per_mcu)
            # given units were judged unbroken; an interval that makes them uncodable is refused, and the slot keeps what it had
            su = enc.add_units(48, 32, 3, q, units)
            fn = ica.lib().mjw_units_codable_restart
            fn.argtypes = [C.POINTER(ica.binding.WritePlan), C.c_void_p, C.c_int, C.c_void_p]
            codable = fn(C.byref(p2), np.ascontiguousarray(units, np.int16).ctypes.data_as(C.c_void_p), ri, None)
            for s in slots:
                want.append((s, ica.emit_jpeg(plan, du, opt, restart_mcus=ri), ri, opt))
            if codable:
                want.append((su, ica.emit_jpeg(p2, units, opt, restart_mcus=ri), ri, opt))
            else:
                with pytest.raises(ica.MijError):
                    enc.set_restart(su, ri)
                want.append((su, ica.emit_jpeg(p2, units, opt), 0, opt))
            # coefficient slots: plain, orientation 6, requantised to quality 60, crop + grey
            tables = tuple(t_.tobytes() for t_ in ica.binding.quality_tables(60))
            for i, kw in ((0, {}), (1, {"orientation": 6, "trim": True}), (2, {"tables": tables}), (3, {"crop": (16, 16, 40, 30), "grey": True})):
                s = enc.add_coef(b, sl[i], kw.get("orientation", 1), kw.get("trim", False), kw.get("tables"), True, kw.get("crop"), kw.get("grey", False))
                want.append((s, host(ica, srcs[i], ri, opt, **kw), ri, opt))
        for s, _, ri, opt in want:
            if opt:
                enc.set_optimize(s)
            if ri:
                enc.set_restart(s, ri)
            assert enc.slot_restart(s) == ri
        enc.upload()
        with pytest.raises(ica.MijError):
            enc.set_restart(0, 2)
        enc.launch()
        enc.fetch_streams()
        for s, w, ri, opt in want:
            got, n = enc.stream(s)
            assert got is not None and bytes(got) == w, (s, ri, opt, n, len(w))
            assert (b"\xff\xdd\x00\x04" in w[:700]) == (ri > 0)
        b.wait()
    finally:
        enc.close()
        b.close()


GEOMETRY = [
    ("420", 96, 64, 21),    # 24 MCUs, 144 units, intervals of 126: the tile end at 128 and the interval end two units apart
    ("420", 96, 64, 1),
    ("420", 96, 64, 6),     # one MCU row
    ("422", 256, 32, 32),   # 64 MCUs of 4 units: two intervals of exactly MIJ_EMIT_TILE = 128 units
    ("grey", 1024, 16, 128),  # the same at one unit per MCU: 128 x 2 MCUs
    ("420", 160, 96, 50),   # 60 MCUs: an interval of 300 units spans three tiles
    ("420", 176, 96, 1),    # 66 MCUs, one tile each: more than the 64 tiles one scan chunk holds
    ("444", 40, 24, 1),     # 15 intervals: the marker number wraps
    ("444", 40, 24, 15),    # Ri = the MCU count: no marker, only the DRI segment
    ("444", 40, 24, 16),
]


def test_interval_against_tile_geometry(ica):
    """the tile cut at interval ends, the segmented scans across tile and chunk seams, the marker wrap: one transcode call per optimize mode
    over every geometry == the host contract; and the same for flat pictures, whose intervals are a few bits each"""
    datas, ris = [], []
    for layout, w, h, ri in GEOMETRY:
        for flat in (False, True):
            datas.append(source(ica, layout, w, h, seed=ri, flat=flat))
            ris.append(ri)
    for optimize in (False, True):
        got, used, why, hosted = transcode(ica, datas, optimize=optimize, gpu_entropy=False, restart_mcus=ris)
        assert used == ris and hosted == 0, (used, hosted)
        for k, (d, ri) in enumerate(zip(datas, ris)):
            want = host(ica, d, ri, optimize)
            assert got[k] == want, (k, GEOMETRY[k // 2], k & 1, optimize, why[k], got[k] is not None and len(got[k]), len(want))
    # what the cases are there for
    w420 = host(ica, datas[2 * 6], 1)
    assert markers(w420) == [k & 7 for k in range(65)]
    assert len(markers(host(ica, datas[2 * 7], 1))) == 14 and markers(host(ica, datas[2 * 8], 15)) == [] and markers(host(ica, datas[2 * 9], 16)) == []
    assert markers(host(ica, datas[2 * 3], 32)) == [0] and markers(host(ica, datas[2 * 4], 128)) == [0]


def test_libjpeg_fixtures_through_both_front_ends(ica):
    """the Pillow-made pairs, among them intervals whose padded last byte is 0xFF (FF 00 FF Dn): the GPU's stream of the plain file at the
    pair's interval is libjpeg's restart file from DRI on, and the restart file transcodes to the same, through the GPU walk and the host walk"""
    z = np.load(FIXTURE)
    names, ris = [str(n) for n in z["names"]], [int(r) for r in z["ri"]]
    plains = [z["plain_" + n.split("_")[0]].tobytes() for n in names]
    rsts = [z["restart_" + n].tobytes() for n in names]
    assert any(any(b"\xff\x00\xff" + bytes([0xD0 + k]) in r for k in range(8)) for r in rsts)
    for gpu_entropy in (False, True):
        got, used, why, hosted = transcode(ica, plains + rsts, optimize=False, gpu_entropy=gpu_entropy, restart_mcus=ris + ris)
        assert used == ris + ris and hosted == 0
        for k, n in enumerate(names):
            i, j = rsts[k].index(b"\xff\xdd"), got[k].index(b"\xff\xdd")
            assert got[k][j:] == rsts[k][i:], (n, gpu_entropy)
            assert got[k + len(names)] == got[k], (n, gpu_entropy)
            assert got[k] == host(ica, plains[k], ris[k]), (n, gpu_entropy)


def test_transcoder_rows_refusals_and_host_fallback(ica):
    """restart_rows resolves on the destination (after orientation and crop), last_restarts says what was used, an interval above 65535
    refuses that picture alone, both given is a ValueError, and a slot that does not fit the arena is finished on the host to the same bytes"""
    a, b_ = source(ica, "420", 96, 64, 8), source(ica, "422", 64, 40, 9)
    wide = source(ica, "grey", 8 * 300, 8, 3, flat=True)  # 300 MCUs a row: 219 rows are 65700 MCUs
    for gpu_entropy in (False, True):
        got, used, why, hosted = transcode(ica, [a, b_, a, wide, a], optimize=True, gpu_entropy=gpu_entropy, restart_rows=[1, 1, 0, 219, 2],
                                           orientation=[1, 6, 1, 1, 1], edge="trim", crop=[None, None, None, None, (16, 16, 64, 40)])
        # 96 x 64 at 16 x 16: 6 MCUs a row; 64 x 40 4:2:2 turned by 6 is 40 x 64 at 8 x 16: 5 a row; the crop keeps 64 x 40 at 16 x 16: 4 a row
        assert used == [6, 5, 0, 0, 8] and hosted == 0, used
        assert got[3] is None and "65535" in why[3] and why[0] is None
        assert got[0] == host(ica, a, 6, True) and got[1] == host(ica, b_, 5, True, orientation=6, trim=True)
        assert got[2] == ica.transcode_memory(a, optimize=True)[0] and got[4] == host(ica, a, 8, True, crop=(16, 16, 64, 40))
        assert ica.transcode_memory(a, optimize=True, restart_rows=1)[0] == got[0]
    t = ica.Transcoder()
    try:
        with pytest.raises(ValueError):
            t.transcode([a], restart_rows=1, restart_mcus=2)
        with pytest.raises(ValueError):
            t.transcode([a], restart_mcus=-1)
        t.reserve_arena(len(host(ica, a, 1)) + 64)  # room for the first stream only
        got = t.transcode([a, a, b_], optimize=False, copy_markers="none", restart_mcus=[1, 1, 3])
        assert t.last_host_emitted == 2 and got == [host(ica, a, 1), host(ica, a, 1), host(ica, b_, 3)]
    finally:
        t.close()


def test_codability_follows_the_restarted_predictor(ica):
    """DC +1500 then -1500 is uncodable in one segment and codable at Ri = 1; DCs climbing to 3000 in steps are codable unbroken and not
    at Ri = 1: the conversion kernel's verdict is the host's either way"""
    for layout in ("grey", "444"):
        pair, climb = om.dc_grid(layout, (1500, -1500, 1500, -1500))[1], om.dc_grid(layout, (1000, 2000, 3000, 2000))[1]
        got, used, why, _ = transcode(ica, [pair, pair, climb, climb, pair], optimize=False, gpu_entropy=False, restart_mcus=[0, 1, 0, 1, 2])
        assert got[0] is None and "not codable" in why[0] and ica.transcode_memory(pair)[0] is None
        assert got[1] is not None and got[1] == host(ica, pair, 1)
        assert got[2] is not None and got[2] == ica.transcode_memory(climb)[0]
        assert got[3] is None and "not codable" in why[3] and ica.transcode_memory(climb, restart_mcus=1)[0] is None
        assert got[4] is None and ica.transcode_memory(pair, restart_mcus=2)[0] is None  # 1500 -> -1500 inside one interval


def test_tensor_encoder_and_round_trip_on_the_device(ica, gpu_ctx, oracle):
    """TensorEncoder.encode(restart_rows / restart_mcus) == mjw_emit_restart of the host transform, plain and optimised; and the restart
    streams decode through the default GPU front end to the planes of their Ri = 0 twins"""
    pics = [noise(83, 61, 1), noise(40, 24, 2), noise(200, 120, 3)]
    enc = ica.TensorEncoder()
    try:
        twins = enc.encode([dev(a) for a in pics], quality=90, layout="HWC")
        for optimize in (False, True):
            rows = enc.encode([dev(a) for a in pics], quality=90, layout="HWC", optimize=optimize, restart_rows=1)
            assert enc.last_restarts == [6, 3, 13] and enc.last_host_emitted == 0
            ones = enc.encode([dev(a) for a in pics], quality=90, layout="HWC", optimize=optimize, restart_mcus=[1, 0, 5])
            for k, a in enumerate(pics):
                plan, du = ica.host_transform(a, 90)
                assert rows[k] == ica.emit_jpeg(plan, du, optimize, restart_mcus=plan.mcu_x), (k, optimize)
                assert ones[k] == ica.emit_jpeg(plan, du, optimize, restart_mcus=[1, 0, 5][k]), (k, optimize)
        with pytest.raises(ValueError):
            enc.encode([dev(pics[0])], layout="HWC", restart_rows=1, restart_mcus=1)
        with pytest.raises(ValueError):
            enc.encode([dev(pics[0])], layout="HWC", restart_mcus=65536)
    finally:
        enc.close()
    datas = twins + rows + ones
    b = ica.Batch(gpu_ctx, len(datas), ARENA, ARENA, ARENA)
    try:
        ok, sl, why = b.decode_jpegs(datas, 3, threads=4)
        assert ok == len(datas), why
        b.submit()
        b.wait()
        out = [b.fetch(s) for s in sl]
        for k in range(len(pics)):
            assert np.array_equal(out[k], oracle.load(twins[k], 3)[1])
            assert np.array_equal(out[k + 3], out[k]) and np.array_equal(out[k + 6], out[k]), k
    finally:
        b.close()
