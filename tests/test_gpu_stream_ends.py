"""The GPU Huffman walk where the entropy data ENDS.  It hands an image back to the host walk through an anomaly word whose bits are separate
hand-written rules (es_decode, k_es_dc): 1 a run past coefficient 63 or a bad code, 2 an inconsistent chain, 4 the stream ends before the last block,
8 no convergence, 16 the data ran out inside a block, 32 a 0xff data byte behind the final bit position of the last interval, 64 a restart
interval that ends a byte or more before its marker, or past it.  A rule that is off by a bit or a byte would make the walk ACCEPT a stream
and deliver pixels the reference does not.  The cases are the ones test_stream_ends_host.py runs on the CPU (stream_cases.py): bytes behind
the last block, cuts, edits around restart markers, streams that end on and around subsequence boundaries.

Everything is compared bit for bit with the oracle (and the host walk's planes); which bits a case raises is predicted from the rules'
own comments by stream_cases.predict_anomaly, a plain sequential walk on the test side.  Bits 8 (a chain that does not settle in 96 rounds)
and 2 (its hand-over states do not chain up; only ever with 8) are not raised here: test_gpu_walk_seams.py holds them.

Nothing here provokes a fault: every stream sits in the entropy arena with the zero padding the kernels rely on."""
import numpy as np
import pytest

import helpers
import stream_cases as sc
from test_stream_ends_host import baseline_groups, boundary_inputs

pytestmark = pytest.mark.gpu

SKIP = 2  # MIJ_FLAG_SKIP


def _gpu_cases(ica):
    """-> [(label, base or None, Case)] for every case the extract gate passes (status 1), and the number it does not"""
    bases, small = boundary_inputs(ica)
    out, n_host = [], 0
    for group, base, cases in baseline_groups(ica):
        for c in cases:
            if sc.expected_extract_status(c.data) != 1:
                n_host += 1
                continue
            b = base
            if b is None and c.name.startswith("base"):
                b = bases[int(c.name[4:c.name.index(" ")])]
            elif b is None:
                b = small[int(c.name[5:c.name.index(" ")])]
            out.append(("%s %s" % (group, c.name), b, c))
    out.append(("hand-made run past 63", None, sc.Case("run past 63", "run past 63", sc.run_past_63_stream())))
    return out, n_host


def _host_decode_into(ica, b, slot, data, req):
    """the host walk for a slot the GPU walk handed back: -> None, or the failure reason (the slot is then skipped)"""
    b.fallback_prepare(slot)
    try:
        d2, _ = ica.HostDecoder.decode(data, req, out=b.staging(slot))
        if d2.flags:
            b.set_flags(slot, d2.flags)
        return None
    except ica.MijError as e:
        b.set_flags(slot, SKIP)
        return str(e)


def _walk(ica, oracle, gpu_ctx, part, fmt):
    """One batch through add_jpeg_stream + entropy_run, checked for soundness.  -> [anomaly word per case]"""
    b = ica.Batch(gpu_ctx, 512, 16 << 20, 16 << 20, 16 << 20)  # room for 512 pictures: the arena holds 16 restart intervals per picture + 1024
    b.set_coef_format(fmt)
    b.entropy_reserve(4 << 20)
    slots = []
    for label, _, c in part:
        st, slot = b.add_jpeg_stream(c.data, 3)
        assert st == 1, (label, st, b.last_reason)
        slots.append(slot)
    fallback = set(b.entropy_run())
    words, host_reason = [], {}
    for (label, _, c), s in zip(part, slots):
        an = b.entropy_anomaly(s)
        words.append(an)
        o = oracle.load(c.data, 3)
        if s not in fallback:
            assert an == 0, (fmt, label, an)
            assert o[0] == "ok", "%s %s: the GPU walk keeps a stream the oracle rejects (%s)" % (fmt, label, o[1])
            desc, want = ica.HostDecoder.decode(c.data, 3)
            for ci, (pg, pw) in enumerate(zip(ica.detile_coefficients(desc, b.fetch_coef(s)), ica.detile_coefficients(desc, want))):
                assert np.array_equal(pg, pw), (fmt, label, ci, int((pg != pw).sum()))
        else:
            assert an != 0, (fmt, label)
            host_reason[s] = _host_decode_into(ica, b, s, c.data, 3)
    b.submit()
    b.wait()
    for (label, _, c), s in zip(part, slots):
        o = oracle.load(c.data, 3)
        if host_reason.get(s) is not None:
            assert o[0] == "fail" and host_reason[s] == (o[1] if o[1] is not None else "decode failed"), (fmt, label, host_reason[s], o[:2])
        else:
            assert o[0] == "ok", (fmt, label, o[1])
            assert np.array_equal(b.fetch(s), o[1]), (fmt, label)
    b.close()
    return words


_words_cache = {}


def _all_words(ica, oracle, gpu_ctx, fmt):
    if fmt not in _words_cache:
        cases, n_host = _gpu_cases(ica)
        words = []
        for lo in range(0, len(cases), 64):
            words += _walk(ica, oracle, gpu_ctx, cases[lo:lo + 64], fmt)
        _words_cache[fmt] = (cases, words, n_host)
    return _words_cache[fmt]


@pytest.mark.parametrize("fmt", ["compact", "int16"])
def test_gpu_walk_is_sound_where_streams_end(ica, oracle, gpu_ctx, fmt):
    """Every status-1 case, both plane formats, batches of 64: a slot that is NOT handed back has anomaly 0, the oracle accepts its stream,
    fetch_coef equals the host walk's planes block for block, and the pixels after submit equal the oracle's.  A slot that is handed back
    goes through fallback_prepare + the host walk, and then verdict, reason and pixels equal the oracle's."""
    cases, words, n_host = _all_words(ica, oracle, gpu_ctx, fmt)
    per_bit = {bit: sum(1 for w in words if w & bit) for bit in (1, 2, 4, 8, 16, 32, 64)}
    kept = sum(1 for w in words if w == 0)
    print("GPU walk, %s planes: %d cases, kept %d, handed back %d (per anomaly bit %s), sent to the host walk by extraction %d"
          % (fmt, len(cases), kept, len(words) - kept, per_bit, n_host))
    assert len(cases) > 1200 and kept > 120 and len(words) - kept > 800


@pytest.mark.parametrize("fmt", ["compact", "int16"])
def test_each_completion_rule_fires_where_its_comment_says(ica, oracle, gpu_ctx, fmt):
    """The anomaly word of EVERY case equals the one stream_cases.predict_anomaly gives: a plain sequential walk on the test side that
    states the rules as es_decode's and k_es_dc's comments do, while the kernels reach their verdict in parallel from guessed starts.
    On top of that, per case kind, what those comments say outright:
      0xff 0x00 behind the last block -> 32 and nothing else;  one or two pad bytes in front of an RSTn -> 64 and nothing else;
      a byte removed in front of an RSTn -> 64 with 4 or 16;  a hand-made run past coefficient 63 -> 1;
      cut + EOI -> 4 or 16.  Which of the two: the walk finishes the symbol that straddles the end of the data and starts nothing behind
      it, so the block the data ends in is normally left open and the count comes up short -- 4, "the stream ends before the last block",
      also for a cut INSIDE the last block.  16 comes up only where the straddling symbol itself completes its block behind the end of
      the data; without 4 only if that block is the scan's last (confirmed on an MI355X: of 264 plain cuts 169 give 4 alone, 28 give
      4 | 16, 59 give 4 | 32 -- the final position was never recorded, so the 0xff search starts at the first byte -- and 1 gives 16 alone).
    Every combination listed at the end must have occurred, so no rule is asserted on an empty set."""
    cases, words, _ = _all_words(ica, oracle, gpu_ctx, fmt)
    seen, wrong = {}, []
    for (label, base, c), w in zip(cases, words):
        want = sc.predict_anomaly(c.data)
        if c.kind == "run past 63":
            assert want & 1, (label, want)
        if c.kind == "tail stuffed ff":
            assert want == 32, (label, want)
        if c.kind in ("rst pad byte", "rst 2 pad bytes"):
            assert want == 64, (label, want)
        if c.kind == "rst byte cut":
            assert want & 64 and want & (4 | 16) and not want & ~(1 | 4 | 16 | 64), (label, want)
        if c.kind in ("cut", "boundary cut", "rst cut") and sc.pieces(c.data) != sc.pieces(base):
            assert want & (4 | 16), (label, want)
        if w != want:
            wrong.append("%s: anomaly %d, predicted %d" % (label, w, want))
        key = "%s -> %d" % (c.kind, want)
        seen[key] = seen.get(key, 0) + 1
    print("anomaly words per kind (%s planes): %s" % (fmt, sorted(seen.items())))
    assert not wrong, "%d of %d cases: %s" % (len(wrong), len(cases), wrong[:40])
    for key in ("tail stuffed ff -> 32", "rst pad byte -> 64", "rst 2 pad bytes -> 64", "rst byte cut -> 68", "rst byte cut -> 80", "cut -> 4", "cut -> 16",
                "cut -> 20", "cut -> 36", "boundary cut -> 36", "rst cut -> 68", "rst cut -> 84", "run past 63 -> 1"):
        assert seen.get(key, 0) >= 1, (key, sorted(seen.items()))


def test_no_needless_fallback(ica, oracle, gpu_ctx):
    """What the GPU walk must keep (k_es_dc's comment, mjh_extract_scan): every intact base, non-0xff bytes behind the last block, EOI
    twice, renumbered RSTn, streams padded to and around a subsequence boundary, and flipped padding bits that leave the last byte != 0xff
    (flips that stay inside the padding: at most as many bits as lie behind the last block's end, by the test-side walk) -- anomaly 0, not
    handed back.  This also keeps the soundness test from passing on a walk that hands everything back."""
    cases, words, _ = _all_words(ica, oracle, gpu_ctx, "compact")
    n = {}
    for (label, base, c), w in zip(cases, words):
        keep = c.kind in ("intact", "tail plain", "eoi twice", "rst renumber", "boundary pad")
        if c.kind == "padflip":
            nbits, ends = sc.block_ends(base)[-1]
            keep = int(c.name.split()[-1]) <= nbits - ends[-1]
        if keep:
            assert w == 0, "%s: handed back with anomaly %d" % (label, w)
            n[c.kind] = n.get(c.kind, 0) + 1
    print("kept as they must be:", sorted(n.items()))
    assert n["intact"] >= 10 and n["tail plain"] >= 24 and n["eoi twice"] >= 8 and n["rst renumber"] >= 40 and n["boundary pad"] >= 8 and n.get("padflip", 0) >= 8, n


def _front_end_cases(ica, every):
    out = []
    for group, base, cases in baseline_groups(ica):
        if every or not group.endswith("/cut"):
            out += [("%s %s" % (group, c.name), c.data) for c in cases]
    out.append(("hand-made run past 63", sc.run_past_63_stream()))
    return out


def _through_batch_front_end(ica, oracle, gpu_ctx, cases):
    n_ok = n_fail = 0
    for lo in range(0, len(cases), 64):
        part = cases[lo:lo + 64]
        b = ica.Batch(gpu_ctx, 512, 16 << 20, 16 << 20, 16 << 20)  # as in _walk
        b.entropy_reserve(4 << 20)
        ok, slots, reasons = b.decode_jpegs([d for _, d in part], 3, threads=4, gpu_entropy=True)
        b.submit()
        b.wait()
        for i, (label, d) in enumerate(part):
            kind, want, _ = oracle.load(d, 3)
            if slots[i] >= 0:
                assert kind == "ok", (label, want)
                assert np.array_equal(b.fetch(slots[i]), want), label
                n_ok += 1
            else:
                assert kind == "fail" and reasons[i] == (want if want is not None else "decode failed"), (label, reasons[i], want)
                n_fail += 1
        b.close()
    return n_ok, n_fail


def test_stream_ends_through_the_batch_front_end(ica, oracle, gpu_ctx, monkeypatch):
    """The same cases -- those the extract gate leaves to the host walk included -- through decode_jpegs(gpu_entropy=True), and the
    structural and boundary ones once more with MIJ_ES_RECORDS=0 (the zigzag-image form of the write pass): verdict, reason, pixels."""
    n_ok, n_fail = _through_batch_front_end(ica, oracle, gpu_ctx, _front_end_cases(ica, True))
    assert n_ok > 1400 and n_fail > 800, (n_ok, n_fail)
    monkeypatch.setenv("MIJ_ES_RECORDS", "0")
    n_ok2, n_fail2 = _through_batch_front_end(ica, oracle, gpu_ctx, _front_end_cases(ica, False))
    assert n_ok2 > 700 and n_fail2 > 50, (n_ok2, n_fail2)
    print("batch front end: %d accepted, %d rejected; zigzag-image form: %d accepted, %d rejected" % (n_ok, n_fail, n_ok2, n_fail2))


def test_stream_ends_through_stbi_load_from_memory(ica, oracle, gpu_ctx, monkeypatch):
    """The structural and boundary cases through the one-picture entry with MIJ_GPU_WALK_MIN_PIXELS=0: its own arena, 1024-bit
    subsequences -- the boundary cases around multiples of 128 bytes end exactly on, one byte before and one byte behind a subsequence.
    Verdict, reason (where the reference sets one) and pixels against the oracle."""
    monkeypatch.setenv("MIJ_GPU_WALK_MIN_PIXELS", "0")
    n_ok = n_fail = 0
    for label, d in _front_end_cases(ica, False):
        kind, want, _ = oracle.load(d, 3)
        got = ica.stbi_load_from_memory(d, 3)
        if kind == "ok":
            assert got is not None, (label, ica.stbi_failure_reason())
            assert np.array_equal(got[0], want), label
            n_ok += 1
        else:
            assert got is None, label
            if want is not None:
                assert ica.stbi_failure_reason() == want, (label, ica.stbi_failure_reason(), want)
            n_fail += 1
    print("stbi_load_from_memory: %d accepted, %d rejected" % (n_ok, n_fail))
    assert n_ok > 700 and n_fail > 50, (n_ok, n_fail)
