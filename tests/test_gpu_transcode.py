"""Lossless transcode on the GPU (Transcoder: decode front end -> k_coef_units -> emission kernels) against the host contract
(mjh_transcode_memory, pinned by tests/test_transcode_host.py): the same bytes for every layout, plane format and front end, across the
plane-tile and emission-tile seams, for escaped blocks, mixed calls, a tiny arena, uncodable sources and reused objects."""
import numpy as np
import pytest
import torch  # before the library is first loaded: one HIP runtime for both (tensor_out._one_hip_runtime)

import transcode_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sources(ica, gpu_ctx):
    srcs = [(n, s) for n, s, _, _ in tc.writer_sources()] + list(tc.layout_sources()) + [("escaped q100 72x56", tc.escaped_source())]
    want = {opt: [ica.transcode_memory(s, optimize=opt) for _, s in srcs] for opt in (False, True)}
    for opt in want:
        assert all(o is not None for o, _ in want[opt])
    return srcs, {opt: [o for o, _ in want[opt]] for opt in want}


@pytest.fixture(scope="module")
def coder(ica, gpu_ctx):
    t = ica.Transcoder()
    yield t
    t.close()


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("gpu_entropy", [True, False, None])
@pytest.mark.parametrize("optimize", [False, True])
def test_gpu_equals_host_for_every_layout(ica, sources, fmt, gpu_entropy, optimize):
    srcs, want = sources
    t = ica.Transcoder()
    try:
        t.set_coef_format(fmt)
        got = t.transcode([s for _, s in srcs], optimize=optimize, copy_markers="none", gpu_entropy=gpu_entropy)
        assert t.last_reasons == [None] * len(srcs)
        for (name, _), g, w in zip(srcs, got, want[optimize]):
            assert g == w, (name, fmt, gpu_entropy, optimize)
        b = t._batch
        fmts = {b.slot_coef_bytes(s) for s in range(len(srcs))}
        assert fmts == {1} if fmt == "compact" else 0 in fmts  # (a progressive file whose L1 bound the device takes is packed either way)
        if fmt == "compact":  # the progressive sources were staged as int16 (no STAGED_COMPACT flag) and packed on the device
            prog = [i for i, (n, _) in enumerate(srcs) if n.startswith("progressive")]
            assert len(prog) == 4 and all(b.slot_coef_bytes(i) == 1 and not b.slot_flags(i) & 4 for i in prog)
    finally:
        t.close()


def test_named_seams(ica, coder):
    """150 units cross the 128-unit emission tile and 100 luma blocks the 64-block plane tile (4:2:0 80x80); 147 units (4:4:4 56x56); grey
    with exactly one plane tile (64x64) and one block over (72x64); 4:2:2 40x24; 4:4:0 24x40"""
    by_name = dict(tc.layout_sources())
    for name, n_du, dpm in (("baseline 80x80 luma 2x2 rst 0", 150, 6), ("baseline 56x56 luma 1x1 rst 0", 147, 3), ("baseline grey 64x64", 64, 1),
                            ("baseline grey 72x64", 72, 1), ("baseline 40x24 luma 2x1 rst 0", 36, 4), ("baseline 24x40 luma 1x2 rst 3", 36, 4)):
        src = by_name[name]
        desc, _ = ica.HostDecoder.decode(src, 0)
        plan, _ = ica.transcode_plan(desc)
        assert (plan.du_elems() // 64, plan.plan.du_per_mcu) == (n_du, dpm), name
        for optimize in (False, True):
            got = coder.transcode([src], optimize=optimize, copy_markers="none")
            assert got == [ica.transcode_memory(src, optimize=optimize)[0]], (name, optimize)


@pytest.mark.parametrize("fmt", ["compact", "int16"])
def test_escaped_blocks(ica, fmt):
    src = tc.escaped_source()
    t = ica.Transcoder()
    try:
        t.set_coef_format(fmt)
        for gpu_entropy in (True, False):
            got = t.transcode([src], copy_markers="none", gpu_entropy=gpu_entropy)
            assert got == [ica.transcode_memory(src, optimize=True)[0]], gpu_entropy
            if fmt == "compact":
                assert t._batch.slot_escapes(0) > 0
    finally:
        t.close()


def test_mixed_call(ica, coder, golden):
    by_name = dict(tc.layout_sources())
    good = [tc.writer_sources()[5][1], by_name["baseline grey 72x64"], by_name["progressive 4:2:2 41x23"], by_name["baseline 24x40 luma 1x2 rst 0"]]
    srcs = [good[0], golden.jpg("cmyk_40x30"), good[1], b"not a jpeg", golden.jpg("s41_35x19"), good[2], good[0][:300], tc.different_chroma_tables(),
            golden.jpg("rgb_tagged_24x24"), good[3], tc.wide_table_entry()]
    got = coder.transcode(srcs, copy_markers="all")
    host = [ica.transcode_memory(s, optimize=True, copy_markers=True) for s in srcs]
    assert len(got) == len(srcs) == len(coder.last_reasons)
    for i, (g, (w, why)) in enumerate(zip(got, host)):
        assert g == w, i
        assert (coder.last_reasons[i] is None) == (g is not None), i
        if w is None and i not in (3, 6):  # the refusals: the host's verdict in the host's words
            assert coder.last_reasons[i].endswith(why), (i, coder.last_reasons[i], why)
    assert [g is not None for g in got] == [True, False, True, False, False, True, False, False, False, True, False]
    smaller = coder.transcode(srcs, copy_markers="none", only_if_smaller=True, optimize=False)
    assert smaller[0] is srcs[0] or smaller[0] == srcs[0]  # the writer's own file does not shrink under the plain tables
    with pytest.raises(ValueError):
        coder.transcode(srcs, copy_markers="some")
    with pytest.raises(ValueError):
        coder.transcode(srcs[0])
    with pytest.raises(ValueError):
        coder.transcode(srcs, optimize=1)


def test_arena_overflow_is_finished_on_the_host(ica, sources):
    srcs, want = sources
    t = ica.Transcoder()
    try:
        t.reserve_arena(4096)
        datas = [s for _, s in srcs]
        got = t.transcode(datas, copy_markers="none")
        assert t.last_host_emitted > 0
        assert got == want[True]
        assert t.arena_bytes > 4096
        assert t.transcode(datas, copy_markers="none") == want[True]
        assert t.last_host_emitted == 0
    finally:
        t.close()


@pytest.mark.parametrize("what,value,ok", [("ac", 1023, True), ("ac", -1024, False), ("ac", 1024, False), ("dc", -2047, True), ("dc", 2048, False)])
@pytest.mark.parametrize("fmt", ["compact", "int16"])
def test_codability_is_the_hosts_verdict(ica, coder, what, value, ok, fmt):
    """the test-side writer's optimal tables code any magnitude, so the source itself is a valid file"""
    for hv in ([(2, 2), (1, 1), (1, 1)], [(1, 1)]):
        def edit(planes, hv=hv):
            p = planes[len(hv) - 1]
            if what == "ac":
                p[-1, -1, 63] = value
            else:
                p[:, :, 0] = 0
                p[1, 2, 0] = value // 2
                p[1, 1, 0] = value // 2 - value
        src = tc.planes_source(88, 72, hv, edit)
        neighbour = tc.writer_sources()[4][1]
        coder.set_coef_format(fmt)
        for gpu_entropy in (True, False):
            for optimize in (False, True):
                got = coder.transcode([neighbour, src, neighbour], optimize=optimize, copy_markers="none", gpu_entropy=gpu_entropy)
                w, why = ica.transcode_memory(src, optimize=optimize)
                assert (w is not None) == ok
                assert got[1] == w
                assert got[0] == got[2] == ica.transcode_memory(neighbour, optimize=optimize)[0]
                assert (coder.last_reasons[1] is None) == ok
                if not ok:
                    assert "not codable" in coder.last_reasons[1] and ("AC" in why or "DC" in why)
    coder.set_coef_format("compact")


def test_repeat_and_reuse(ica, sources):
    srcs, want = sources
    t = ica.Transcoder()
    try:
        big = [s for n, s in srcs if "80x80" in n or "72x" in n]
        small = [s for n, s in srcs if "17x9" in n or "9x7" in n or "1x1" in n]
        assert big and small
        first = t.transcode(big, copy_markers="none")
        again = t.transcode(small, copy_markers="none")
        assert again == [ica.transcode_memory(s, optimize=True)[0] for s in small]
        assert t.transcode(small, copy_markers="none") == again
        assert t.transcode(big, copy_markers="none") == first == [ica.transcode_memory(s, optimize=True)[0] for s in big]
    finally:
        t.close()


def test_existing_slot_kinds_are_unmoved(ica, coder):
    """a TensorEncoder call before and after a transcode in one process: the generalised emission writes what it wrote"""
    enc = ica.TensorEncoder()
    try:
        imgs = [ica.synth_rgb(w, h, seed=w) for (w, h) in ((80, 80), (33, 17), (56, 56))]
        tens = [torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1))).cuda() for im in imgs]
        for round_ in range(2):
            for q in (90, 95):
                assert enc.encode(tens, quality=q) == [ica.stbi_write_jpg_to_memory(im, q) for im in imgs], (round_, q)
                plans = [ica.host_transform(im, q) for im in imgs]
                assert enc.encode(tens, quality=q, optimize=True) == [ica.emit_jpeg(p, du, True) for p, du in plans], (round_, q)
            srcs = [s for _, s in tc.layout_sources()[:6]]
            assert coder.transcode(srcs, copy_markers="none") == [ica.transcode_memory(s, optimize=True)[0] for s in srcs]
    finally:
        enc.close()
