"""Lossless transcode on the GPU at block level, from sources whose every coefficient is chosen (transcode_planes.py, pinned on the host
by test_transcode_host.py): the units k_coef_units writes against the numpy model, unit for unit; the emitted bytes across every
emission-tile seam for all five layouts against the host and the emission model; the codability flag at every branch of the
DC-predecessor rule and at the AC limits; and one encoder fed from two batches of different plane formats."""
import numpy as np
import pytest
import torch  # before the library is first loaded: one HIP runtime for both (tensor_out._one_hip_runtime)

import transcode_cases as tc
import transcode_planes as tp

pytestmark = pytest.mark.gpu

ARENA = 16 << 20
LAYOUTS = list(tp.LAYOUTS)
FRONT_ENDS = [False, None]  # the host walk; the default front end (the walk on the GPU where it applies)


@pytest.fixture(scope="module")
def units():
    """name -> the model's units of a source, computed once"""
    cache = {}

    def get(src):
        if src.name not in cache:
            cache[src.name] = tp.expected_units(src)
        return cache[src.name]
    return get


@pytest.fixture(scope="module")
def host(ica):
    """(name, optimize) -> the host's stream of a source (None for one it refuses), computed once"""
    cache = {}

    def get(src, optimize):
        if (src.name, optimize) not in cache:
            cache[(src.name, optimize)] = ica.transcode_memory(src.data, optimize=optimize)[0]
        return cache[(src.name, optimize)]
    return get


def _assert_units(got, want, what):
    if got.shape == want.shape and np.array_equal(got, want):
        return
    if got.shape != want.shape:
        pytest.fail("%s: %s units, want %s" % (what, got.shape, want.shape))
    diff = np.argwhere(got != want)
    u, k = (int(x) for x in diff[0])
    pytest.fail("%s: first difference at unit %d, k %d: got %d, want %d (%d coefficients in %d units differ)"
                % (what, u, k, got[u, k], want[u, k], len(diff), len(set(diff[:, 0].tolist()))))


def _convert(ica, gpu_ctx, batches):
    """batches: [(format, front end, [Source])] -> ([Batch], Encoder, [[encoder slot per source] per batch]) with the planes uploaded; the
    slots are added to the encoder round-robin over the batches.  The unit arena is the slots' sizes and one spare MiB."""
    opened, slots = [], []
    for fmt, gpu_entropy, srcs in batches:
        b = ica.Batch(gpu_ctx, len(srcs), ARENA, ARENA, ARENA)
        opened.append(b)
        b.set_coef_format(fmt)
        ok, sl, why = b.decode_jpegs([s.data for s in srcs], 0, threads=4, gpu_entropy=gpu_entropy)
        assert ok == len(srcs) and all(x >= 0 for x in sl), why
        b.upload()
        slots.append(sl)
    n = sum(len(srcs) for _, _, srcs in batches)
    du_bytes = sum((tp.Geom(s.w, s.h, s.hv).n_du * 128 + 255) // 256 * 256 for _, _, srcs in batches for s in srcs)
    enc = ica.Encoder(gpu_ctx, n, 0, du_bytes + (1 << 20), stage_bytes=0)
    es = [[None] * len(sl) for sl in slots]
    for i in range(max(len(sl) for sl in slots)):
        for k, sl in enumerate(slots):
            if i < len(sl):
                es[k][i] = enc.add_coef(opened[k], sl[i])
    return opened, enc, slots, es


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("gpu_entropy", FRONT_ENDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_units_at_block_level(ica, gpu_ctx, units, layout, gpu_entropy, fmt):
    """the whole geometry list with address content, the edge values and dense noise in one batch and one unit arena: every slot's
    units, as the kernel wrote them, equal the model's"""
    srcs = tp.address(layout) + [tp.edge_values(layout), tp.dense(layout)]
    (b,), enc, (slots,), (es,) = _convert(ica, gpu_ctx, [(fmt, gpu_entropy, srcs)])
    try:
        enc.upload()
        enc.launch()
        enc.wait()
        escapes = 0
        for src, sl, e in zip(srcs, slots, es):
            _assert_units(enc.fetch(e), units(src), "%s (%s, front end %s)" % (src.name, fmt, gpu_entropy))
            assert b.slot_coef_bytes(sl) == (1 if fmt == "compact" else 0), src.name
            if fmt == "compact":
                assert b.slot_escapes(sl) == tp.escaped_blocks(src.planes), src.name
                escapes += b.slot_escapes(sl)
        assert fmt != "compact" or escapes > 0
    finally:
        enc.close()
        b.close()


@pytest.fixture(scope="module")
def seam_sources(ica, host):
    srcs = [tp.emission(layout) for layout in LAYOUTS] + [tp.longest()] + [tp.dense(layout) for layout in LAYOUTS]
    want = {opt: [host(s, opt) for s in srcs] for opt in (False, True)}
    assert all(w is not None for opt in want for w in want[opt])
    return srcs, want


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("optimize", [False, True])
def test_bytes_at_every_seam(ica, gpu_ctx, seam_sources, fmt, optimize):
    """1300 units and more per layout -- ten 128-unit seams, one of them sharing a 0xFF byte and one on a byte boundary under the plain
    tables -- plus the longest units and dense noise: the device's streams equal the host's, and their entropy segments the model's"""
    srcs, want = seam_sources
    t = ica.Transcoder()
    try:
        t.set_coef_format(fmt)
        t.reserve_arena(sum(len(w) for w in want[False]) + (1 << 20))
        got = t.transcode([s.data for s in srcs], optimize=optimize, copy_markers="none")
        assert t.last_host_emitted == 0  # otherwise the host would be compared with itself
        assert t.last_reasons == [None] * len(srcs)
        for s, g, w in zip(srcs, got, want[optimize]):
            assert g == w, (s.name, fmt, optimize)
        for layout, g in zip(LAYOUTS, got):
            _, model_stream, stats, hdr = tp.emission_model(layout)
            assert stats["shared_ff"] >= 1 and stats["aligned"] >= 1 and stats["tiles"] >= 11
            n = hdr[optimize]
            assert g[n:-2] == model_stream[optimize][n:-2] and g[-2:] == b"\xff\xd9", (layout, fmt, optimize)
    finally:
        t.close()


@pytest.fixture(scope="module")
def verdict_cases(ica, units):
    """layout -> [(Source, the model's verdict)]: every DC pair, every AC limit and the triangle"""
    import transcode_model as model
    out = {}
    for layout in LAYOUTS:
        cases = tp.dc_pairs(layout) + tp.ac_limits(layout) + [(tp.triangle(layout), True)]
        for src, ok in cases:
            assert model.codable(tp.Geom(src.w, src.h, src.hv), units(src)) == ok, src.name
        out[layout] = cases
    return out


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_codability_at_every_branch(ica, gpu_ctx, verdict_cases, host, layout, fmt):
    """all the pictures of a layout in ONE call per front end and optimize, each between two good neighbours: the device's verdict is
    the model's for every branch of the predecessor rule, both tile relations and both limits; accepted streams are the host's, the
    neighbours are untouched, and the flagged slots take good pictures in the next call"""
    cases = verdict_cases[layout]
    neighbour = tc.writer_sources()[4][1]
    good = tp.address(layout)[7]
    datas = [neighbour]
    for src, _ in cases:
        datas += [src.data, neighbour]
    t = ica.Transcoder()
    try:
        t.set_coef_format(fmt)
        t.reserve_arena(4 << 20)
        for gpu_entropy in FRONT_ENDS:
            for optimize in (False, True):
                want_n = ica.transcode_memory(neighbour, optimize=optimize)[0]
                got = t.transcode(datas, optimize=optimize, copy_markers="none", gpu_entropy=gpu_entropy)
                assert t.last_host_emitted == 0
                wrong = [src.name for i, (src, ok) in enumerate(cases) if (got[2 * i + 1] is not None) != ok]
                assert not wrong, (fmt, gpu_entropy, optimize, wrong)
                for i, (src, ok) in enumerate(cases):
                    if ok:
                        assert got[2 * i + 1] == host(src, optimize), (src.name, fmt, gpu_entropy, optimize)
                        assert t.last_reasons[2 * i + 1] is None
                    else:
                        assert "not codable" in t.last_reasons[2 * i + 1], src.name
                assert all(g == want_n for g in got[0::2]) and all(r is None for r in t.last_reasons[0::2])
        # the flagged slots again, now with a good picture each
        again = [neighbour]
        for src, ok in cases:
            again += [src.data if ok else good.data, neighbour]
        got = t.transcode(again, optimize=True, copy_markers="none")
        assert t.last_reasons == [None] * len(again)
        for i, (src, ok) in enumerate(cases):
            assert got[2 * i + 1] == host(src if ok else good, True), src.name
    finally:
        t.close()


def test_two_batches_one_encoder(ica, gpu_ctx, units, host):
    """batch A compact, batch B int16, added to one encoder in the order A0 B0 A1 B1 A2 B2, so that the conversion's group lists are not
    in slot order; one picture of each is a refused DC pair"""
    bad_a = tp.dc_pair("420", 0, "d", False, -2048)
    bad_b = tp.dc_pair("444", 2, "c", False, 2048)
    A = [tp.address("420")[7], bad_a, tp.edge_values("422")]
    B = [tp.address("440")[11], bad_b, tp.dense("grey")]
    assert bad_a is not None and bad_b is not None
    batches, enc, slots, es = _convert(ica, gpu_ctx, [("compact", False, A), ("int16", False, B)])
    try:
        assert es == [[0, 2, 4], [1, 3, 5]]
        assert [batches[0].slot_coef_bytes(s) for s in slots[0]] == [1, 1, 1] and [batches[1].slot_coef_bytes(s) for s in slots[1]] == [0, 0, 0]
        enc.stream_reserve(4 << 20)
        enc.upload()
        enc.launch()
        enc.fetch_streams()
        for srcs, e in zip((A, B), es):
            for src, slot in zip(srcs, e):
                _assert_units(enc.fetch(slot), units(src), src.name)
        status = {slot: enc.slot_status(slot) for e in es for slot in e}
        assert status == {0: "ok", 1: "ok", 2: "uncodable", 3: "uncodable", 4: "ok", 5: "ok"}
        for srcs, e in zip((A, B), es):
            for src, slot in zip(srcs, e):
                data, _ = enc.stream(slot)
                assert data == host(src, False), src.name
        assert host(bad_a, False) is None and host(bad_b, False) is None
    finally:
        enc.close()
        for b in batches:
            b.close()
