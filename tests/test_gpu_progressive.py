"""Progressive streams written on the GPU (mij_enc_set_progressive; csrc/mij_progressive_kernels.h and the segmented launches of
csrc/mij_emit_kernels.h): every stream byte for byte what the host contract writes (include/mij_host.h, PROGRESSIVE STREAMS), which
tests/test_progressive_host.py holds against libjpeg.  Only the forced-flush case may be finished on the host: the fallback must not hide a
broken kernel."""
import os

import numpy as np
import pytest
import torch

import progressive_cases as pc

pytestmark = pytest.mark.gpu

ARENA = 16 << 20
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "progressive_libjpeg.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(ica, data, **kw):
    got, why = ica.transcode_memory(data, progressive=True, **kw)
    assert got is not None, why
    return got


def plains():
    z = np.load(FIXTURE)
    return [str(n) for n in z["names"]], [z["plain_" + str(n)].tobytes() for n in z["names"]], [z["progressive_" + str(n)].tobytes() for n in z["names"]]


def as_baseline(ica, t, du):
    """a baseline file that holds these units: the transcoder's input"""
    s = ica.binding.emit_transcoded(t, du, True)
    assert s is not None
    return s


@pytest.fixture(scope="module")
def unit_cases(ica):
    return pc.cases(ica)


def test_cases_stay_clear_of_the_forced_flushes(ica, unit_cases):
    """on the CPU, with the host writer's counters: only the case made for it has a forced flush, so no other may reach the host route"""
    for name, t, du, forced in unit_cases:
        st = ica.binding.progressive_stats(t, du)
        assert (st.forced_bit_flushes + st.forced_run_flushes > 0) == (forced is not None), name
        if forced is None:
            assert st.longest_run < 32767 and st.most_pending_bits <= 937, name
    for n, p, _ in zip(*plains()):
        t = ica.binding.transcode_plan(ica.HostDecoder.probe(p, 0))[0]
        st = ica.binding.progressive_stats(t, pc.units_of(ica, p))
        assert st.forced_bit_flushes + st.forced_run_flushes == 0 and (st.longest_run > 1 or n != "smooth"), n


def test_given_units_through_the_encoder(ica, gpu_ctx, unit_cases):
    """mij_enc_add_units slots of the writer's own 4:2:0 and 4:4:4 layouts, and the request's life cycle: before upload only, refused with a
    restart interval (and the interval refused on a progressive slot), inherited by a clone and by nobody else, forgotten by reset"""
    rng = np.random.default_rng(3)
    enc = ica.Encoder(gpu_ctx, 16, 1 << 20, 8 << 20)
    try:
        enc.stream_reserve(ARENA)
        want = []
        for q, w, h in ((90, 83, 61), (95, 50, 33), (90, 200, 136)):
            a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            if w == 200:  # smooth: end-of-band runs
                a = np.clip(np.add.outer(np.arange(h), np.arange(w))[:, :, None] * 0.6 + rng.normal(0, 2, (h, w, 3)), 0, 255).astype(np.uint8)
            plan, du = ica.host_transform(a, q)
            s = enc.add_units(w, h, 3, q, du)
            enc.set_progressive(s)
            assert enc.slot_progressive(s)
            want.append((s, ica.emit_jpeg(plan, du, progressive=True)))
            plain = enc.add_units(w, h, 3, q, du)
            assert not enc.slot_progressive(plain)
            want.append((plain, ica.emit_jpeg(plan, du)))
        # hand-made units in the writer's own 4:2:0 layout and tables: runs, ZRLs and correction bits nobody's transform made
        name, tp, du, _ = [c for c in unit_cases if c[0] == "random_sparse_420"][0]
        s = enc.add_units(tp.plan.width, tp.plan.height, 3, 90, du)
        enc.set_progressive(s)
        want.append((s, ica.emit_jpeg(tp, du, progressive=True)))
        # host pixels, and a clone made after the request: it inherits it
        a = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)
        root = enc.add(a, 90)
        enc.set_progressive(root)
        twin = enc.add_clone(root)
        assert enc.slot_progressive(twin)
        plan, du = ica.host_transform(a, 90)
        want += [(root, ica.emit_jpeg(plan, du, progressive=True)), (twin, ica.emit_jpeg(plan, du, progressive=True))]
        with pytest.raises(ica.MijError):
            enc.set_restart(want[0][0], 2)
        enc.set_restart(want[1][0], 2)
        with pytest.raises(ica.MijError):
            enc.set_progressive(want[1][0])
        enc.set_restart(want[1][0], 0)
        enc.upload()
        with pytest.raises(ica.MijError):
            enc.set_progressive(0)
        enc.launch()
        enc.fetch_streams()
        for s, w in want:
            got, n = enc.stream(s)
            assert enc.slot_status(s) == "ok" and got is not None and bytes(got) == w, (s, n, len(w))
        enc.reset()
        s = enc.add_units(83, 61, 3, 90, ica.host_transform(np.zeros((61, 83, 3), np.uint8), 90)[1])
        assert not enc.slot_progressive(s)
    finally:
        enc.close()


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_fixtures_and_unit_cases_through_the_transcoder(ica, unit_cases, fmt, gpu_entropy):
    """the libjpeg pairs' plain files, the progressive files themselves and the hand-made unit cases in one call, both front ends and both
    plane formats: each stream is the host contract's -- for the fixtures libjpeg's own bytes from SOF2 on -- and only the forced-flush case is
    finished on the host, under its own status"""
    names, plain, prog = plains()
    made = [as_baseline(ica, t, du) for _, t, du, _ in unit_cases]
    datas = plain + prog + made
    t = ica.Transcoder()
    try:
        t.reserve_arena(ARENA)
        t.set_coef_format(fmt)
        got = t.transcode(datas, copy_markers="none", gpu_entropy=gpu_entropy, progressive=True)
        assert t.last_reasons == [None] * len(datas) and t.last_progressive == [True] * len(datas)
        assert t.last_host_emitted == sum(1 for c in unit_cases if c[3] is not None) == 1
    finally:
        t.close()
    for k, n in enumerate(names):
        i, j = prog[k].index(b"\xff\xc2"), got[k].index(b"\xff\xc2")
        assert got[k][j:] == prog[k][i:], n
        assert got[k + len(names)] == got[k], n
    for k, (name, tp, du, forced) in enumerate(unit_cases):
        assert got[2 * len(names) + k] == ica.emit_jpeg(tp, du, progressive=True), name


def test_forced_flush_status_and_exact_length_without_room(ica, gpu_ctx, unit_cases):
    """a slot with more than 937 pending correction bits reports MIJ_ENC_SLOT_HOST_FLUSH; a progressive slot that does not fit the arena
    still reports its exact length"""
    name, tp, du, forced = [c for c in unit_cases if c[3] == "bits"][0]
    _, t2, du2, _ = [c for c in unit_cases if c[0] == "random_sparse_grey"][0]
    srcs = [as_baseline(ica, tp, du), as_baseline(ica, t2, du2), as_baseline(ica, t2, du2)]
    want = ica.emit_jpeg(t2, du2, progressive=True)
    b = ica.Batch(gpu_ctx, 3, ARENA, ARENA, ARENA)
    enc = ica.Encoder(gpu_ctx, 8, 0, 8 << 20, stage_bytes=0)
    try:
        ok, sl, why = b.decode_jpegs(srcs, 0, threads=2, gpu_entropy=False)
        assert ok == 3, why
        b.upload()
        enc.stream_reserve(len(want) + 100)  # room for one of the two
        es = [enc.add_coef(b, s) for s in sl]
        for s in es:
            enc.set_progressive(s)
        enc.upload()
        enc.launch()
        assert enc.fetch_streams() == 1
        assert enc.slot_status(es[0]) == "host flush" and enc.stream(es[0])[0] is None
        got, n = enc.stream(es[1])
        assert enc.slot_status(es[1]) == "ok" and bytes(got) == want
        got, n = enc.stream(es[2])
        assert got is None and n == len(want) and enc.slot_status(es[2]) == "no room"
        assert ica.binding.emit_transcoded(enc.tplan(es[0]), enc.fetch(es[0]), progressive=True) == ica.emit_jpeg(tp, du, progressive=True)
        b.wait()
    finally:
        enc.close()
        b.close()


def test_mixed_batch_and_composition(ica):
    """progressive and baseline slots, some with restart intervals, in one call: each stream is what its slot gives alone; and the request
    composes with orientation, crop, grey and quality"""
    names, plain, _ = plains()
    a, b_, c = plain[names.index("420")], plain[names.index("422")], plain[names.index("smooth")]
    t = ica.Transcoder()
    try:
        t.reserve_arena(ARENA)
        datas = [a, a, b_, c, c, a]
        prog = [True, False, True, False, True, False]
        ris = [0, 2, 0, 0, 0, 0]
        got = t.transcode(datas, copy_markers="none", progressive=prog, restart_mcus=ris)
        assert t.last_host_emitted == 0 and t.last_progressive == prog
        for k, d in enumerate(datas):
            want = host(ica, d) if prog[k] else ica.transcode_memory(d, optimize=True, restart_mcus=ris[k])[0]
            assert got[k] == want, k
        kw = dict(orientation=6, edge="trim", crop=(8, 0, 100, 150), quality=75, grey=True)
        got = t.transcode([c, a], copy_markers="none", progressive=True, **kw)
        assert t.last_host_emitted == 0
        hk = dict(orientation=6, trim=True, crop=(8, 0, 100, 150), tables=tuple(x.tobytes() for x in ica.binding.quality_tables(75)), grey=True)
        assert got[0] == host(ica, c, **hk) and got[1] is None  # the window lies outside the small picture
        kw2 = dict(orientation=[6, 3], edge="trim", quality=60)
        got = t.transcode([c, a], copy_markers="all", progressive=True, only_if_smaller=True, **kw2)
        h2 = [ica.transcode_memory(d, copy_markers=True, progressive=True, orientation=o, trim=True, tables=tuple(x.tobytes() for x in ica.binding.quality_tables(60)))[0]
              for d, o in ((c, 6), (a, 3))]
        assert got == h2
        with pytest.raises(ValueError):
            t.transcode([a], progressive=True, restart_rows=1)
        with pytest.raises(ValueError):
            t.transcode([a], progressive=1)
    finally:
        t.close()


def test_tensor_encoder(ica):
    """TensorEncoder.encode(progressive=True) of a 64 x 48 batch at a 4:2:0 quality and at a 4:4:4 quality (above 90) == the host path"""
    rng = np.random.default_rng(9)
    pics = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8) for _ in range(3)]
    pics.append(np.clip(np.add.outer(np.arange(48), np.arange(64))[:, :, None] * 2.0 + rng.normal(0, 3, (48, 64, 3)), 0, 255).astype(np.uint8))
    enc = ica.TensorEncoder()
    try:
        for q in (90, 95):
            got = enc.encode(torch.stack([dev(a) for a in pics]), quality=q, layout="HWC", progressive=True)
            assert enc.last_host_emitted == 0
            for k, a in enumerate(pics):
                plan, du = ica.host_transform(a, q)
                assert got[k] == ica.emit_jpeg(plan, du, progressive=True), (q, k)
        f = torch.stack([dev(a) for a in pics]).float() / 255.0
        got = enc.encode_normalized(f, quality=90, layout="HWC", progressive=True)
        assert got[0] == ica.emit_jpeg(*ica.host_transform(pics[0], 90), progressive=True)
        with pytest.raises(ValueError):
            enc.encode([dev(pics[0])], layout="HWC", progressive=True, restart_rows=1)
        with pytest.raises(ValueError):
            enc.encode([dev(pics[0])], layout="HWC", progressive="yes")
    finally:
        enc.close()
