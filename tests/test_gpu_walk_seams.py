"""The GPU Huffman walk at the seams of its subsequences and at the limits of its synchronisation rounds (families and model:
walk_seams.py; what makes them meaningful is checked without a device in test_walk_seams_host.py).

Every expected value is the host decoder's planes, the oracle's pixels or the plain sequential walk on the test side -- never the GPU
walk's own.  The seam, restart and chain-shape families must be kept whole: a member that is handed back, for whatever reason, is a failure.
The slow-settling family is documented as handed back once its chain needs more than ES_MAX_ROUNDS = 96 rounds: what is asserted there is
that every member is either kept and right or handed back whole (bit 8, 96 rounds, the host walk's result), that its neighbour in the
batch is untouched, and that the batch is as good as new after a reset.

Nothing here provokes a fault: all streams are conforming, and the write pass on a chain that has not settled keeps its stores inside
the picture's own regions by its ord < nblocks guards and the per-bit bound of the record region."""
import numpy as np
import pytest

import walk_seams as ws

pytestmark = pytest.mark.gpu

FORMS = ("records", "zigzag", "int16")
_last = {}


def _reference(ica, oracle, name, members):
    """[(desc, the host walk's planes, the oracle's pixels)] per member, made once per family (the last family is kept)"""
    if _last.get("name") != name:
        ref = []
        for d in members:
            desc, want = ica.HostDecoder.decode(d, 3)
            o = oracle.load(d, 3)
            assert o[0] == "ok", (name, o[1])
            ref.append((desc, ica.detile_coefficients(desc, want), o[1]))
        _last.update(name=name, ref=ref)
    return _last["ref"]


def _batch(ica, gpu_ctx, monkeypatch, form, L, n=512, rounds=None):
    """a batch whose arena walks with L-bit subsequences (None: the product's own choice) in one of the three forms of the write pass"""
    if L is None:
        monkeypatch.delenv("MIJ_ES_BITS_OVERRIDE", raising=False)
    else:
        monkeypatch.setenv("MIJ_ES_BITS_OVERRIDE", str(L))
    if form == "zigzag":
        monkeypatch.setenv("MIJ_ES_RECORDS", "0")
    else:
        monkeypatch.delenv("MIJ_ES_RECORDS", raising=False)
    if rounds is None:
        monkeypatch.delenv("MIJ_ES_ROUNDS", raising=False)
    else:
        monkeypatch.setenv("MIJ_ES_ROUNDS", str(rounds))
    b = ica.Batch(gpu_ctx, n, 64 << 20, 64 << 20, 64 << 20)
    b.set_coef_format("int16" if form == "int16" else "compact")
    b.entropy_reserve(8 << 20)
    return b


def _explain(name, L, j, data, ci, got, want):
    """the member, the component, the first differing block and what the model says stands at a seam there"""
    w = ws.walk(data)
    diff = np.argwhere((got != want).reshape(got.shape[0], got.shape[1], -1).any(axis=2))
    by, bx = (int(v) for v in diff[0])
    mcu_x = want.shape[1] // w.comps[ci][1]
    return "%s member %d component %d: %d blocks differ, the first at row %d column %d = %s" % (
        name, j, ci, len(diff), by, bx, ws.seam_notes(w, L, ws.scan_ordinal(w, ci, by, bx, mcu_x)))


def _walk_and_check(ica, oracle, b, name, L, members, ref, form):
    """add_jpeg_stream for all, entropy_run() == [], anomaly 0 everywhere, planes == host walk element for element, pixels == oracle"""
    slots = []
    for d in members:
        st, slot = b.add_jpeg_stream(d, 3)
        assert st == 1, (name, st, b.last_reason)
        slots.append(slot)
    fallback = b.entropy_run()
    words = [b.entropy_anomaly(s) for s in slots]
    assert fallback == [] and not any(words), "%s (%s): handed back %s, anomaly words %s, %d rounds" % (
        name, form, fallback, {j: wd for j, wd in enumerate(words) if wd}, b.entropy_rounds())
    assert {b.slot_coef_bytes(s) for s in slots} == {0 if form == "int16" else 1}
    for j, (d, s, (desc, want, _)) in enumerate(zip(members, slots, ref)):
        got = ica.detile_coefficients(desc, b.fetch_coef(s))
        for ci, (pg, pw) in enumerate(zip(got, want)):
            if not np.array_equal(pg, pw):
                raise AssertionError("%s: %s" % (form, _explain(name, L, j, d, ci, pg, pw)))
    b.submit()
    b.wait()
    for j, (s, (desc, _, pixels)) in enumerate(zip(slots, ref)):
        assert np.array_equal(b.fetch(s), pixels), (name, form, j)
        assert (b.slot_flags(s) & 1) == (desc.flags & 1), "%s (%s) member %d: MIJ_FLAG_WIDE_IDCT is %d, the host walk's is %d" % (
            name, form, j, b.slot_flags(s) & 1, desc.flags & 1)
    return slots


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("layout,tables,L", ws.SEAM_PARAMS)
def test_every_symbol_at_every_offset(ica, oracle, gpu_ctx, monkeypatch, layout, tables, L, form):
    """A whole seam family in one batch: the lead-ins put every symbol of the body at every offset modulo L, so every hand-over rule of the
    state passes and of the write pass meets every symbol kind at the seam, one bit before and one bit behind it."""
    fam = ws.seam_family(ica, layout, tables, L)
    ref = _reference(ica, oracle, fam.name, fam.members)
    b = _batch(ica, gpu_ctx, monkeypatch, form, L)
    _walk_and_check(ica, oracle, b, fam.name, L, fam.members, ref, form)
    assert b.entropy_rounds() <= 96
    b.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("layout", ("grey", "420"))
def test_block_l1_is_summed_once_across_a_seam(ica, oracle, gpu_ctx, monkeypatch, layout, form):
    """Blocks whose L1 is exactly MIJ_BLOCK_L1_LIMIT with each of their coefficients at every offset: the picture stays off the WIDE kernels
    (the host walk's flag) however a seam cuts the block.  In the int16 form the lane that begins a block sums the head and k_es_tails
    adds the rest: a symbol that starts exactly at the seam belongs to the rest alone."""
    fam = ws.seam_family(ica, layout, "annexk", 256, body="l1")
    ref = _reference(ica, oracle, fam.name, fam.members)
    assert not any(desc.flags & 1 for desc, _, _ in ref)
    b = _batch(ica, gpu_ctx, monkeypatch, form, 256)
    _walk_and_check(ica, oracle, b, fam.name, 256, fam.members, ref, form)
    b.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("L", (256, 288))
def test_restart_twins(ica, oracle, gpu_ctx, monkeypatch, L, form):
    """The 4:2:0 family as three scans per picture, the last a single MCU (nsub = 1, several scans in one work list): every interval its own
    chain, seams counted from its own first bit."""
    fam = ws.restart_twins(ica, L)
    ref = _reference(ica, oracle, fam.name, fam.members)
    b = _batch(ica, gpu_ctx, monkeypatch, form, L)
    _walk_and_check(ica, oracle, b, fam.name, L, fam.members, ref, form)
    b.close()


@pytest.mark.parametrize("form", ("records", "zigzag"))
def test_chain_shapes_and_round_counts(ica, oracle, gpu_ctx, monkeypatch, form):
    """nsub = 1, 2, 255, 256, 257, 512, 513 in one batch at 256 bits (a workgroup's 256 subsequences, k_es_offsets' per = ceil(nsub / 256),
    the queues of k_es_syncq), with the rounds queued up front left alone and set to 1, 2 and 96: the same planes every time.  96 rounds
    up front are 96 rounds, most of them idle -- they must leave the end states alone; one round is not enough, so finish() adds rounds
    and runs the passes behind them again on cleared verdicts."""
    members = [d for d, _ in ws.chain_shapes(ica)]
    assert [ws.Walk(d).nsub(ws.CHAIN_L) for d in members] == list(ws.CHAIN_NSUB)
    ref = _reference(ica, oracle, "chain shapes", members)
    rounds = {}
    for queued in (None, 1, 2, 96):
        b = _batch(ica, gpu_ctx, monkeypatch, form, ws.CHAIN_L, rounds=queued)
        _walk_and_check(ica, oracle, b, "chain shapes, rounds %s" % queued, ws.CHAIN_L, members, ref, form)
        rounds[queued] = b.entropy_rounds()
        b.close()
    print("chain shapes (%s): rounds run per rounds queued %s" % (form, rounds))
    assert all(1 <= r <= 96 for r in rounds.values())
    assert rounds[96] == 96
    assert rounds[1] > 1


def _one_slow_member(ica, oracle, gpu_ctx, monkeypatch, form, L, data, neighbour, seam):
    """-> (kept, rounds, anomaly word)"""
    b = _batch(ica, gpu_ctx, monkeypatch, form, L, n=32)
    want = [oracle.load(d, 3)[1] for d in (data, neighbour)]
    host = [ica.HostDecoder.decode(d, 3) for d in (data, neighbour)]
    slots = []
    for d in (data, neighbour):
        st, slot = b.add_jpeg_stream(d, 3)
        assert st == 1, (st, b.last_reason)
        slots.append(slot)
    fallback = b.entropy_run()
    rounds, word = b.entropy_rounds(), b.entropy_anomaly(slots[0])
    assert slots[1] not in fallback and b.entropy_anomaly(slots[1]) == 0, "the neighbour of an unsettled chain is handed back"
    assert rounds <= 96
    kept = slots[0] not in fallback
    if kept:
        assert word == 0
    else:
        assert fallback == [slots[0]] and word & 8 and rounds == 96, (fallback, word, rounds)
    for k, s in enumerate(slots):
        if k == 0 and not kept:
            continue
        desc, planes = host[k]
        for ci, (pg, pw) in enumerate(zip(ica.detile_coefficients(desc, b.fetch_coef(s)), ica.detile_coefficients(desc, planes))):
            assert np.array_equal(pg, pw), (form, L, "neighbour" if k else "member", ci, int((pg != pw).sum()))
    if not kept:  # handed back whole: the host walk into the slot's staging, as for any other anomaly
        b.fallback_prepare(slots[0])
        d2, _ = ica.HostDecoder.decode(data, 3, out=b.staging(slots[0]))
        if d2.flags:
            b.set_flags(slots[0], d2.flags)
    b.submit()
    b.wait()
    for s, px in zip(slots, want):
        assert np.array_equal(b.fetch(s), px), (form, L, kept, s)
    # the same batch after a reset: queues, round counters and verdicts of the unsettled run are gone
    b.reset()
    fam, ref = seam
    _walk_and_check(ica, oracle, b, fam.name + " behind a slow chain", L or 4096, fam.members[:32], ref[:32], form)
    b.close()
    return kept, rounds, word


@pytest.mark.parametrize("form", FORMS)
def test_slow_chains_are_kept_or_handed_back_whole(ica, oracle, gpu_ctx, monkeypatch, form):
    """tools/dbg/dense.py in graded sizes, each with an ordinary neighbour in a batch of its own, at 256 bits and at the product's own
    length.  Which sizes fall on which side of 96 rounds is measured, not asserted (DESIGN 4b has the table); asserted is that both sides
    occur, that a kept member ran through finish()'s extra rounds (more than the 32 queued up front at 256 bits) and came out right, and
    that a handed-back member is handed back whole."""
    fam = ws.seam_family(ica, "grey", "annexk", 256)
    seam = (fam, _reference(ica, oracle, fam.name, fam.members))
    table = []
    for data, neighbour in ws.slow_family(ica):
        bits = ws.Walk(data).nbits[0]
        for L in (256, None):
            kept, rounds, word = _one_slow_member(ica, oracle, gpu_ctx, monkeypatch, form, L, data, neighbour, seam)
            table.append((bits, L or "default", rounds, "kept" if kept else "handed back, anomaly %d" % word))
    print("slow chains (%s): (bits, subsequence length, rounds, outcome)" % form)
    for row in table:
        print("  %6d  %7s  %3d  %s" % row)
    at256 = [r for r in table if r[1] == 256]
    assert sum(1 for r in at256 if r[3] == "kept" and r[2] > 32) >= 1, "no member was kept by finish()'s extra rounds"
    assert sum(1 for r in at256 if r[3] != "kept") >= 1, "no member was handed back"
    if form != "records":
        return
    # the public entries: verdict and pixels are the oracle's whichever way the walk decided
    monkeypatch.setenv("MIJ_ES_BITS_OVERRIDE", "256")
    monkeypatch.setenv("MIJ_GPU_WALK_MIN_PIXELS", "0")
    for data, neighbour in ws.slow_family(ica):
        b = ica.Batch(gpu_ctx, 2, 16 << 20, 16 << 20, 16 << 20)
        b.entropy_reserve(1 << 20)
        ok, slots, reasons = b.decode_jpegs([data, neighbour], 3, threads=2, gpu_entropy=True)
        assert ok == 2 and min(slots) >= 0, reasons
        b.submit()
        b.wait()
        for d, s in zip((data, neighbour), slots):
            assert np.array_equal(b.fetch(s), oracle.load(d, 3)[1])
        b.close()
        got = ica.stbi_load_from_memory(data, 3)
        assert got is not None, ica.stbi_failure_reason()
        assert np.array_equal(got[0], oracle.load(data, 3)[1])
