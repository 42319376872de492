"""What stands in front of the entropy data, through the GPU: the families of header_cases.py (segment arrangements, frame layouts, scan
structures, Huffman table shapes, one edit per failure reason, and the streams outside the reference's contract) through every front
end -- Batch.add_jpeg in compact and int16 batches, decode_jpegs on the host walk and on the GPU walk, stbi_load_from_memory with the GPU
walk switched on for every size -- and the streams the extraction gate passes through add_jpeg_stream + entropy_run in every form of
the walk.  Pixels are compared bit for bit with the oracle for 3 and 4 channels (one component: also 1), rejected streams must give the
oracle's reason and leave their neighbours alone, MIJ_FLAG_WIDE_IDCT must be what the host stage reports wherever a front end leaves a
slot to ask (stbi_load_from_memory hands out pixels only), and the kernel family of every frame layout is asserted
(header_cases.expected_path).

The GPU walk has to TAKE every stream of status 1: an odd table is not one of the anomalies the header comment of mij_entropy_kernels.h
lists, so entropy_run's fallback list must stay empty and fetch_coef must equal the host walk's planes.

Nothing here provokes a fault: every stream goes through the same gates as a caller's, and the streams outside the reference's contract
are ones the host stage defines (cleared tables, rejected table segments)."""
import time

import numpy as np
import pytest

import header_cases as hc

pytestmark = pytest.mark.gpu

SKIP = 2  # MIJ_FLAG_SKIP
ALL = list(hc.FAMILIES) + ["product_only"]
_expect = {}


def _reqs(c):
    return (3, 4, 1) if len(c.meta.get("hv", ())) == 1 else (3, 4)


def _want(oracle, c, req):
    """the oracle's answer for a case, computed once: ('ok', pixels) or ('fail', reason as the product words it)"""
    key = (c.family, c.name, req)
    if key not in _expect:
        kind, val, _ = oracle.load(c.data, req)
        _expect[key] = (kind, val if kind == "ok" else (val if val is not None else "decode failed"))
    return _expect[key]


_wide_flag = {}


def _wide(ica, c):
    """MIJ_FLAG_WIDE_IDCT as the host stage reports it for an accepted stream (it depends on the coefficients alone, not on the request)"""
    if (c.family, c.name) not in _wide_flag:
        _wide_flag[(c.family, c.name)] = ica.HostDecoder.decode(c.data, 3)[0].flags & 1
    return _wide_flag[(c.family, c.name)]


def _cases():
    return [c for fam in ALL for c in hc.family(fam)]


def _batch(ica, gpu_ctx, fmt="compact", entropy=False):
    b = ica.Batch(gpu_ctx, 256, 48 << 20, 48 << 20, 48 << 20)
    b.set_coef_format(fmt)
    if entropy:
        b.entropy_reserve(8 << 20)
    return b


@pytest.mark.parametrize("fmt", ["compact", "int16"])
def test_add_jpeg(ica, oracle, gpu_ctx, fmt):
    """Batch.add_jpeg (the host stage into the slot's staging): pixels, WIDE flag, kernel family; a stream rejected behind its frame
    header has a slot by then, which is skipped and does not disturb the others."""
    t0 = time.time()
    n_ok = n_fail = 0
    for req in (3, 4, 1):
        cases = [c for c in _cases() if req in _reqs(c)]
        for lo in range(0, len(cases), 200):
            part = cases[lo:lo + 200]
            b = _batch(ica, gpu_ctx, fmt)
            slots = []
            for c in part:
                kind, want = _want(oracle, c, req)
                before = len(b.descs)
                try:
                    slots.append(b.add_jpeg(c.data, req))
                    assert kind == "ok", (c.name, want)
                except ica.MijError as e:
                    # the probe raises the reason itself, the staging call prefixes its name; without a reason they say "decode failed"
                    # and "failed"
                    assert kind == "fail" and str(e) in (want, "mjh_decode_memory_fmt: " + ("failed" if want == "decode failed" else want)), \
                        (c.name, str(e), want)
                    if len(b.descs) > before:
                        b.set_flags(before, SKIP)
                    slots.append(-1)
                    n_fail += 1
            b.submit()
            b.wait()
            for c, s in zip(part, slots):
                if s < 0:
                    continue
                assert np.array_equal(b.fetch(s), _want(oracle, c, req)[1]), (fmt, req, c.family, c.name)
                assert (b.slot_flags(s) & 1) == _wide(ica, c), (c.name, b.slot_flags(s))
                if c.family == "frames":
                    assert b.slot_path(s) == hc.expected_path(c.meta["hv"], c.meta["ids"], c.meta["app14"], req), (c.name, req, b.slot_path(s))
                n_ok += 1
            b.close()
    print("add_jpeg %s: %d accepted, %d rejected, %.1f s" % (fmt, n_ok, n_fail, time.time() - t0))
    assert n_ok > 700 and n_fail > 80


@pytest.mark.parametrize("force", [1, 2])
def test_generic_layouts_on_the_two_pass_path(ica, oracle, gpu_ctx, force):
    """Factor 3, factors that do not divide the maximum, chroma above luma, a lone component with factors: the two-pass path with its
    compiled resamplers where they apply (force_generic 1) and with the run-time-general pass 2 alone (2) -- k_resample_fast must leave
    what its resamplers do not cover to k_resample_color."""
    t0 = time.time()
    cases = [c for c in hc.family("frames") if c.meta["generic"]] + [c for c in hc.family("frames") if "four components" in c.name]
    assert len(cases) >= 30
    for req in (3, 4):
        b = _batch(ica, gpu_ctx)
        b.force_generic(force)
        slots = [b.add_jpeg(c.data, req) for c in cases]
        b.submit()
        b.wait()
        for c, s in zip(cases, slots):
            assert b.slot_path(s) == 2, (c.name, b.slot_path(s))
            assert np.array_equal(b.fetch(s), _want(oracle, c, req)[1]), (force, req, c.name)
        b.close()
    print("force_generic %d: %d layouts, %.1f s" % (force, len(cases), time.time() - t0))


def _through_decode_jpegs(ica, oracle, gpu_ctx, cases, req, gpu_entropy, fmt="compact"):
    n_ok = n_fail = 0
    for lo in range(0, len(cases), 200):
        part = cases[lo:lo + 200]
        b = _batch(ica, gpu_ctx, fmt, entropy=bool(gpu_entropy))
        ok, slots, reasons = b.decode_jpegs([c.data for c in part], req, threads=4, gpu_entropy=gpu_entropy)
        b.submit()
        b.wait()
        for i, c in enumerate(part):
            kind, want = _want(oracle, c, req)
            if slots[i] >= 0:
                assert kind == "ok", (c.name, want)
                assert np.array_equal(b.fetch(slots[i]), want), (gpu_entropy, fmt, req, c.family, c.name)
                assert (b.slot_flags(slots[i]) & 1) == _wide(ica, c), (c.name, b.slot_flags(slots[i]))
                n_ok += 1
            else:
                assert kind == "fail" and reasons[i] == want, (c.name, reasons[i], want)
                n_fail += 1
        assert ok == sum(1 for s in slots if s >= 0)
        b.close()
    return n_ok, n_fail


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("gpu_entropy", [False, True], ids=["host walk", "gpu walk"])
def test_decode_jpegs(ica, oracle, gpu_ctx, gpu_entropy, fmt):
    t0 = time.time()
    n_ok = n_fail = 0
    for req in (3, 4, 1):
        a, f = _through_decode_jpegs(ica, oracle, gpu_ctx, [c for c in _cases() if req in _reqs(c)], req, gpu_entropy, fmt)
        n_ok, n_fail = n_ok + a, n_fail + f
    print("decode_jpegs %s / %s: %d accepted, %d rejected, %.1f s" % ("gpu walk" if gpu_entropy else "host walk", fmt, n_ok, n_fail, time.time() - t0))
    assert n_ok > 700 and n_fail > 80


def test_stbi_load_from_memory_with_the_gpu_walk(ica, oracle, gpu_ctx, monkeypatch):
    """the one-picture entry with MIJ_GPU_WALK_MIN_PIXELS=0: its own arena, 1024-bit subsequences"""
    monkeypatch.setenv("MIJ_GPU_WALK_MIN_PIXELS", "0")
    t0 = time.time()
    n_ok = n_fail = 0
    for c in _cases():
        for req in _reqs(c):
            kind, want = _want(oracle, c, req)
            got = ica.stbi_load_from_memory(c.data, req)
            if kind == "ok":
                assert got is not None, (c.name, ica.stbi_failure_reason())
                assert np.array_equal(got[0], want), (c.family, c.name, req)
                n_ok += 1
            else:
                assert got is None, c.name
                if want != "decode failed":
                    assert ica.stbi_failure_reason() == want, (c.name, ica.stbi_failure_reason(), want)
                n_fail += 1
    print("stbi_load_from_memory: %d accepted, %d rejected, %.1f s" % (n_ok, n_fail, time.time() - t0))
    assert n_ok > 700 and n_fail > 80


def _walk_cases():
    """`tables`, and what the gate takes of `frames`, `segments` and `scans`"""
    return [c for fam in ("tables", "frames", "segments", "scans") for c in hc.family(fam) if c.status == 1]


_host_planes = {}


def _host(ica, c):
    if (c.family, c.name) not in _host_planes:
        desc, arena = ica.HostDecoder.decode(c.data, 3)
        _host_planes[(c.family, c.name)] = (desc, ica.detile_coefficients(desc, arena))
    return _host_planes[(c.family, c.name)]


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("bits", [None, "1024"], ids=["default bits", "1024 bits"])
@pytest.mark.parametrize("records", [None, "0"], ids=["records", "zigzag image"])
def test_the_walk_takes_every_table_shape(ica, oracle, gpu_ctx, monkeypatch, records, bits, fmt):
    """add_jpeg_stream + entropy_run: status as tabulated, nothing handed back, anomaly 0, fetch_coef == the host walk's planes, pixels ==
    the oracle's."""
    if records is not None:
        monkeypatch.setenv("MIJ_ES_RECORDS", records)
    if bits is not None:
        monkeypatch.setenv("MIJ_ES_BITS_OVERRIDE", bits)
    t0 = time.time()
    cases = _walk_cases()
    assert len(cases) > 250
    for lo in range(0, len(cases), 200):
        part = cases[lo:lo + 200]
        b = _batch(ica, gpu_ctx, fmt, entropy=True)
        slots = []
        for c in part:
            st, slot = b.add_jpeg_stream(c.data, 3)
            assert st == 1, (c.name, st, b.last_reason)
            slots.append(slot)
        fallback = b.entropy_run()
        assert not fallback, "handed back to the host walk: %s" % [(part[slots.index(s)].name, b.entropy_anomaly(s)) for s in fallback][:20]
        for c, s in zip(part, slots):
            assert b.entropy_anomaly(s) == 0, c.name
            desc, want = _host(ica, c)
            for ci, (pg, pw) in enumerate(zip(ica.detile_coefficients(desc, b.fetch_coef(s)), want)):
                assert np.array_equal(pg, pw), (c.family, c.name, ci, int((pg != pw).sum()))
        b.submit()
        b.wait()
        for c, s in zip(part, slots):
            assert np.array_equal(b.fetch(s), _want(oracle, c, 3)[1]), (c.family, c.name)
            assert (b.slot_flags(s) & 1) == _wide(ica, c), (c.name, b.slot_flags(s))
        b.close()
    print("walk %s / %s / %s: %d streams, %.1f s" % (records or "records", bits or "default", fmt, len(cases), time.time() - t0))


def test_gate_declines_what_the_table_says(ica, gpu_ctx):
    """add_jpeg_stream on every case: the tabulated status, and nothing is added for 0 and 2"""
    b = _batch(ica, gpu_ctx, entropy=True)
    for fam in hc.FAMILIES:
        for c in hc.family(fam):
            n = len(b.descs)
            st, slot = b.add_jpeg_stream(c.data, 3)
            assert st == c.status, (c.name, st, c.status)
            assert (slot == n and len(b.descs) == n + 1) if st == 1 else (slot == -1 and len(b.descs) == n), c.name
            if len(b.descs) >= 250:
                b.close()
                b = _batch(ica, gpu_ctx, entropy=True)
    b.close()


def test_clones_take_the_tables_of_their_source(ica, oracle, gpu_ctx):
    """mij_batch_add + a clone + mjh_decode_memory, the order a C caller uses: the clone exists before the walk finds the DQT segments behind
    SOF, and mij_batch_set_dequant on the source has to reach it"""
    cases = [c for fam in ("segments", "scans") for c in hc.family(fam)
             if "DQT behind SOF" in c.name or "DQT redefined behind SOF" in c.name or "quantisation table redefined between scans" in c.name]
    assert len(cases) >= 5
    b = _batch(ica, gpu_ctx, "int16")
    pairs = []
    for c in cases:
        d = ica.HostDecoder.probe(c.data, 3)
        src = b.add(d)
        clone = b.add_clone(src)
        d2, _ = ica.HostDecoder.decode(c.data, 3, out=b.staging(src))
        assert bytes(d2.dequant) != bytes(d.dequant) or any(d2.comp[k].tq != d.comp[k].tq for k in range(d.ncomp)), c.name
        b.set_dequant(src, d2)
        if d2.flags:
            b.set_flags(src, d2.flags)
            b.set_flags(clone, d2.flags)
        pairs.append((c, src, clone))
    b.submit()
    b.wait()
    for c, src, clone in pairs:
        want = _want(oracle, c, 3)[1]
        assert np.array_equal(b.fetch(src), want), c.name
        assert np.array_equal(b.fetch(clone), want), c.name
    b.close()


def test_mixed_batch_run_twice(ica, oracle, gpu_ctx):
    """one case of every kind of every family in one batch through the default front end, launched twice without a reset"""
    seen, cases = set(), []
    for c in _cases():
        if (c.family, c.kind) not in seen:
            seen.add((c.family, c.kind))
            cases.append(c)
    assert len(cases) >= 20
    b = _batch(ica, gpu_ctx)
    ok, slots, reasons = b.decode_jpegs([c.data for c in cases], 3, threads=4)
    for rnd in range(2):
        b.submit()
        b.wait()
        for i, c in enumerate(cases):
            kind, want = _want(oracle, c, 3)
            if slots[i] >= 0:
                assert kind == "ok" and np.array_equal(b.fetch(slots[i]), want), (rnd, c.family, c.name)
                assert (b.slot_flags(slots[i]) & 1) == _wide(ica, c), (rnd, c.name, b.slot_flags(slots[i]))
            else:
                assert kind == "fail" and reasons[i] == want, (c.name, reasons[i], want)
    b.close()
