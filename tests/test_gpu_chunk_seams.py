"""The chunk seams of the Python front ends (TensorEncoder._encode, Transcoder.transcode): both cut a call into launches of at most
MAX_SLOTS pictures and MAX_PIXEL_BYTES / MAX_COEF_BYTES of arena, and no other test makes a call large enough for a second chunk.  Here the
limits are shrunk (monkeypatch) until a call of about ten small pictures splits into three or more chunks, by count and -- separately -- by
bytes, one chunk being a single picture larger than the byte limit (the j == i / j == k escape of the loops).  What is indexed across the
seam -- convs[i:j], orients[it[0]], targets[it[0]], reasons, requantized, last_host_emitted, last_timing, the regrown arenas and the
reset() of the reused batch and encoder -- has to come out as in one chunk: per picture the host writer's / the host transcoder's bytes.
Every test counts the chunks taken, so a limit that stops biting fails."""
import numpy as np
import pytest
import torch

import sample_cases as S

pytestmark = pytest.mark.gpu

# (width, height, channels): mixed sizes and channel counts; picture 4 is the large one
PICTURES = ((33, 17, 3), (64, 48, 1), (17, 40, 4), (100, 30, 2), (250, 120, 3), (8, 8, 1), (40, 24, 3), (31, 33, 4), (16, 16, 2), (72, 56, 3), (9, 70, 1))


def _count(monkeypatch, obj, name):
    """wraps obj.name with a counter of its calls; -> the list the calls' first list argument lengths are appended to"""
    calls = []
    inner = getattr(obj, name)

    def wrapped(*a, **k):
        calls.append(len(a[1]) if name == "_chunk" else len(a[0]))
        return inner(*a, **k)
    monkeypatch.setattr(obj, name, wrapped)
    return calls


def _pictures(seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, (w, h, c) in enumerate(PICTURES):
        smooth = (np.add.outer(np.arange(h), np.arange(w)) * (i + 3) % 256).astype(np.uint8)[:, :, None]
        a = np.where(rng.random((h, w, c)) < 0.6, smooth, rng.integers(0, 256, (h, w, c))).astype(np.uint8)
        out.append(a)
    return out


def _pixel_bytes(ica, w, h, c, q):
    """the pixel-arena bytes TensorEncoder counts for a picture"""
    from image_codecs_amd import tensor_encode as te
    p = te._plan(w, h, c, q)
    return te._align(te._align(w, 16 if p.subsample else 8) * h * 3, 256)


@pytest.mark.parametrize("optimize", (False, True))
@pytest.mark.parametrize("layout", ("CHW", "HWC"))
def test_tensor_encoder_chunks(ica, gpu_ctx, monkeypatch, layout, optimize):
    """encode: by count (MAX_SLOTS 4: three chunks of eleven pictures), by bytes (a limit the large picture exceeds alone and three small
    ones fill), an emission arena so small that slots of two different chunks fall to the host; then the limits restored: the same bytes"""
    from image_codecs_amd import tensor_encode as te
    q = 90
    imgs = _pictures(7)
    want = [ica.emit_jpeg(*ica.host_transform(a, q), optimize) for a in imgs]
    ts = [torch.from_numpy(np.ascontiguousarray(a if layout == "HWC" else a.transpose(2, 0, 1))).cuda() for a in imgs]
    enc = ica.TensorEncoder()
    try:
        calls = _count(monkeypatch, enc, "_encode_chunk")
        whole = enc.encode(ts, quality=q, layout=layout, optimize=optimize)
        assert calls == [len(imgs)] and whole == want and enc.last_host_emitted == 0
        # by count
        del calls[:]
        monkeypatch.setattr(te, "MAX_SLOTS", 4)
        assert enc.encode(ts, quality=q, layout=layout, optimize=optimize) == want
        assert calls == [4, 4, 3] and enc.last_host_emitted == 0
        # by bytes: the large picture is a chunk of its own
        del calls[:]
        monkeypatch.setattr(te, "MAX_SLOTS", 4096)
        sizes = [_pixel_bytes(ica, w, h, c, q) for w, h, c in PICTURES]
        limit = sizes[0] + sizes[1] + sizes[2]
        assert sizes[4] > limit
        monkeypatch.setattr(te, "MAX_PIXEL_BYTES", limit)
        expect, i = [], 0
        while i < len(sizes):  # the documented rule, restated: pictures while they fit, one at least
            j, pix = i, 0
            while j < len(sizes) and (j == i or pix + sizes[j] <= limit):
                pix += sizes[j]
                j += 1
            expect.append(j - i)
            i = j
        assert len(expect) >= 3 and expect[0] == 3 and 1 in expect
        assert enc.encode(ts, quality=q, layout=layout, optimize=optimize) == want
        assert calls == expect and enc.last_host_emitted == 0
        # a small emission arena: the host finishes slots of two chunks, and the count is their sum.  A miss grows the arena past what
        # its chunk needed, so the second chunk to miss holds a picture of noise whose stream alone is larger than that
        del calls[:]
        per_chunk = []
        inner = enc._encode_chunk

        def spy(*a, **k):
            r = inner(*a, **k)
            per_chunk.append(r[1])
            return r
        monkeypatch.setattr(enc, "_encode_chunk", spy)
        monkeypatch.setattr(te, "MAX_SLOTS", 2)
        monkeypatch.setattr(te, "MAX_PIXEL_BYTES", 2 << 30)
        big = np.random.default_rng(9).integers(0, 256, (1100, 1536, 3), dtype=np.uint8)
        imgs2 = [imgs[0], imgs[6], big, imgs[9], imgs[5]]
        want2 = [ica.emit_jpeg(*ica.host_transform(a, q), optimize) for a in imgs2]
        assert len(want2[2]) > (1 << 20) + len(want2[3])
        ts2 = [torch.from_numpy(np.ascontiguousarray(a if layout == "HWC" else a.transpose(2, 0, 1))).cuda() for a in imgs2]
        enc.close()  # a new encoder: the arena is reserved before its first launch
        enc.reserve_arena(600)
        assert enc.encode(ts2, quality=q, layout=layout, optimize=optimize) == want2
        assert len(per_chunk) == 3 and per_chunk[0] >= 1 and per_chunk[1] >= 1, per_chunk
        assert enc.last_host_emitted == sum(per_chunk)
        # the limits restored
        monkeypatch.undo()
        assert enc.encode(ts, quality=q, layout=layout, optimize=optimize) == want and enc.last_host_emitted == 0
    finally:
        enc.close()


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16, torch.float32))
def test_tensor_encoder_float_chunks(ica, gpu_ctx, monkeypatch, dtype):
    """encode_normalized: channel counts 1 to 4 in one call, so that the conversion differs from picture to picture and convs[i:j] has to
    follow the chunk; the float pictures are made from uint8 ones, so the expected streams are those pictures' (the de-normalisation
    itself is test_gpu_tensor_encode_float.py's subject)"""
    from image_codecs_amd import tensor_encode as te
    q = 95
    imgs = _pictures(8)
    # v / 255 in float32 and then the dtype: exact for float32; for the 16-bit types take what the rounded value de-normalises to
    fl = [(torch.from_numpy(a.transpose(2, 0, 1).copy()).float() / 255).to(dtype) for a in imgs]
    back = [torch.clamp(torch.round(t.float() * 255.0), 0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy() for t in fl]
    want = [ica.emit_jpeg(*ica.host_transform(a, q)) for a in back]
    ts = [t.cuda() for t in fl]
    enc = ica.TensorEncoder()
    try:
        calls = _count(monkeypatch, enc, "_encode_chunk")
        assert enc.encode_normalized(ts, quality=q) == want and calls == [len(imgs)]
        del calls[:]
        monkeypatch.setattr(te, "MAX_SLOTS", 3)
        assert enc.encode_normalized(ts, quality=q) == want
        assert calls == [3, 3, 3, 2]
        del calls[:]
        monkeypatch.setattr(te, "MAX_SLOTS", 4096)
        monkeypatch.setattr(te, "MAX_PIXEL_BYTES", 20000)
        assert enc.encode_normalized(ts, quality=q, optimize=True) == [ica.emit_jpeg(*ica.host_transform(a, q), True) for a in back]
        assert len(calls) >= 3 and sum(calls) == len(imgs) and 1 in calls
    finally:
        enc.close()


# ------------------------------------------------------------------ Transcoder

def _bad_entropy(data):
    """the headers of a stream and, for entropy data, all-ones bits: no Huffman table assigns that code, so the walk fails behind a
    frame header that every check passes"""
    i = data.index(b"\xff\xda")
    n = (data[i + 2] << 8) | data[i + 3]
    return data[:i + 2 + n] + b"\xff\x00" * 64 + b"\xff\xd9"


def _sources(ica):
    """-> (sources, orientations, qualities): twelve sources; 2 is refused by the frame header (CMYK), 5 does not decode, 7 is refused at
    add_coef (orientation 2 mirrors a width that is no multiple of the MCU, edge "perfect"); 9 to 11 do not decode (10 and 11 are a chunk of their own
    under MAX_SLOTS 3).  Orientations and qualities differ across every seam of chunks of three."""
    pic = lambda w, h, s, q=90: ica.synth_jpeg(w, h, seed=s, quality=q)
    srcs = [pic(64, 48, 1), pic(33, 17, 2), S.make("poison", "cmyk", 37, 19).stream(), pic(48, 32, 3, 95), pic(320, 240, 4), _bad_entropy(pic(40, 40, 5)),
            pic(32, 32, 6), pic(50, 32, 7), pic(16, 64, 8, 95), _bad_entropy(pic(24, 24, 9)), _bad_entropy(pic(64, 16, 10)), _bad_entropy(pic(8, 8, 11))]
    orients = [1, 1, 6, 6, 3, 1, 5, 2, 8, 1, 6, 3]
    quals = [None, 50, None, 30, None, 75, 60, None, None, 40, None, None]
    return srcs, orients, quals


@pytest.mark.parametrize("gpu_entropy", (False, True))
def test_transcoder_chunks(ica, gpu_ctx, monkeypatch, gpu_entropy):
    from image_codecs_amd import transcode as tr
    srcs, orients, quals = _sources(ica)
    host = []
    for d, o, q in zip(srcs, orients, quals):
        tables = None if q is None else tuple(bytes(t.tobytes()) for t in ica.quality_tables(q))
        host.append(ica.transcode_memory(d, optimize=True, orientation=o, trim=False, tables=tables))
    # the premises of the sources that fail, each at its stage
    for i in (5, 9, 10, 11):
        ica.HostDecoder.probe(srcs[i], 0)
    assert [h[0] is None for h in host] == [i in (2, 5, 7, 9, 10, 11) for i in range(len(srcs))], [h[1] for h in host]
    assert "axis" in host[7][1]
    t = ica.Transcoder()
    try:
        calls = _count(monkeypatch, t, "_chunk")

        def run():
            del calls[:]
            got = t.transcode(srcs, copy_markers="none", gpu_entropy=gpu_entropy, orientation=orients, quality=quals)
            for i, (g, (w, why)) in enumerate(zip(got, host)):
                assert g == w, (i, gpu_entropy, t.last_reasons[i])
                assert (t.last_reasons[i] is None) == (w is not None), (i, t.last_reasons[i])
            assert t.last_reasons[7].endswith(host[7][1]) and t.last_reasons[2].startswith("not transcodable")
            return got, list(t.last_requantized), dict(t.last_timing)

        whole, requant, timing = run()
        assert calls == [11]  # the CMYK source never reaches a chunk
        assert requant == [q is not None and h[0] is not None for q, h in zip(quals, host)]
        # by count: 0 1 3 | 4 5 6 | 7 8 9 | 10 11 -- the failing sources in the middle of chunks, the last chunk without a picture
        monkeypatch.setattr(tr, "MAX_SLOTS", 3)
        got, rq, tm3 = run()
        assert calls == [3, 3, 3, 2] and got == whole and rq == requant
        assert tm3["convert_ms"] > 0 and tm3["emit_ms"] > 0
        # last_timing is a sum over the chunks: every launch adds a positive time, so it exceeds each single chunk's
        parts = []
        inner = t._chunk

        def spy(*a, **k):
            before, host_before = dict(t.last_timing), t.last_host_emitted
            inner(*a, **k)
            parts.append({key: t.last_timing[key] - before[key] for key in before})
            parts[-1]["host"] = t.last_host_emitted - host_before
        monkeypatch.setattr(t, "_chunk", spy)
        got, rq, tm_sum = run()
        assert len(parts) == 4 and got == whole
        for key in ("convert_ms", "emit_ms"):
            assert abs(sum(p[key] for p in parts) - tm_sum[key]) < 1e-6 * max(1.0, tm_sum[key]), (key, parts)
        assert [p["emit_ms"] > 0 for p in parts] == [True, True, True, False], parts
        # by bytes: the 320 x 240 picture alone exceeds the limit
        monkeypatch.setattr(tr, "MAX_SLOTS", 4096)
        cb = [ica.Batch.coef_bytes(ica.HostDecoder.probe(d, 0)) for i, d in enumerate(srcs) if i != 2]
        limit = cb[0] + cb[1] + cb[2]
        assert cb[3] > limit
        monkeypatch.setattr(tr, "MAX_COEF_BYTES", limit)
        del parts[:]
        got, rq, _ = run()
        assert got == whole and rq == requant
        expect, i = [], 0
        while i < len(cb):  # the documented rule, restated: sources while they fit, one at least
            j, coef = i, 0
            while j < len(cb) and (j == i or coef + cb[j] <= limit):
                coef += cb[j]
                j += 1
            expect.append(j - i)
            i = j
        assert len(expect) >= 3 and expect[:2] == [3, 1] and sum(expect) == 11
        assert calls == expect and len(parts) == len(expect), (calls, expect)
        # a small emission arena: the host finishes slots of two chunks (the second holds a stream larger than the regrown arena)
        monkeypatch.setattr(tr, "MAX_SLOTS", 2)
        monkeypatch.setattr(tr, "MAX_COEF_BYTES", 2 << 30)
        big = ica.stbi_write_jpg_to_memory(np.random.default_rng(9).integers(0, 256, (1100, 1536, 3), dtype=np.uint8), 90)
        srcs2 = [srcs[0], srcs[1], big, srcs[6], srcs[3]]
        host2 = [ica.transcode_memory(d, optimize=True)[0] for d in srcs2]
        assert None not in host2 and len(host2[2]) > (1 << 20) + len(host2[3])
        t.close()
        t.reserve_arena(600)
        del calls[:], parts[:]
        assert t.transcode(srcs2, copy_markers="none", gpu_entropy=gpu_entropy) == host2
        assert calls == [2, 2, 1] and t.last_reasons == [None] * 5
        # the host finished slots of the first two chunks, and the count is the sum over the chunks, not the last chunk's
        hosts = [p["host"] for p in parts]
        assert len(hosts) == 3 and hosts[0] >= 1 and hosts[1] >= 1 and t.last_host_emitted == sum(hosts), hosts
        # the limits restored
        monkeypatch.undo()
        t2 = t.transcode(srcs, copy_markers="none", gpu_entropy=gpu_entropy, orientation=orients, quality=quals)
        assert t2 == whole and t.last_requantized == requant
    finally:
        t.close()
