"""What makes test_gpu_walk_seams.py mean something, checked without a device: the families of walk_seams.py put every symbol of their
body at every offset modulo the subsequence length, every (symbol kind, seam relation) pair a stream can show occurs in every family,
the bodies hold what the walk's rules need to be tried on, and the model the GPU test takes its messages and its subsequence counts from
agrees with the host decoder, the oracle and the anomaly rules on every member."""
import numpy as np
import pytest

import stream_cases as sc
import walk_seams as ws

FAMILIES = [("seam",) + p for p in ws.SEAM_PARAMS] + [("restart", "420", "annexk", L) for L in (256, 288)]
_seen = {}


def _family(ica, kind, layout, tables, L):
    return ws.restart_twins(ica, L) if kind == "restart" else ws.seam_family(ica, layout, tables, L)


def _walked(ica, oracle, key):
    """one pass over a family: every member walked (the first symbol by symbol, the others by shifted_walk, which decodes every symbol of
    the sibling at its moved place), compared with the host decoder, the oracle and predict_anomaly, its seam relations counted"""
    if key in _seen:
        return _seen[key]
    fam = _family(ica, *key)
    base = ws.walk(fam.members[0])
    table, shifts = None, []
    for d in fam.members:
        w, shift = ws.shifted_walk(base, d)
        shifts.append(shift)
        table = ws.relations(w, fam.L, table)
        desc, want = ica.HostDecoder.decode(d, 3)
        for ci, (a, b) in enumerate(zip(ica.detile_coefficients(desc, want), w.planes())):
            assert np.array_equal(a, b), (fam.name, len(shifts) - 1, ci)
        assert oracle.load(d, 3)[0] == "ok", (fam.name, len(shifts) - 1)
        assert sc.predict_anomaly(d) == 0, (fam.name, len(shifts) - 1)
        assert sc.expected_extract_status(d) == 1
    _seen[key] = (fam, base, table, shifts)
    return _seen[key]


@pytest.mark.parametrize("key", FAMILIES, ids=lambda k: "-".join(map(str, k)))
def test_lead_ins_cover_every_offset_and_the_model_agrees(ica, oracle, key):
    """The lead-in lengths of a family are L consecutive values, so they cover all L residues; behind the lead-in every member decodes,
    symbol by symbol, to the first member's symbols moved by the difference of the lead-ins (shifted_walk: by walking, not by comparing
    bytes); the model's coefficients are the host decoder's for every member, the oracle decodes every member, the anomaly rules
    predict 0 and the extract gate passes it."""
    fam, base, table, shifts = _walked(ica, oracle, key)
    assert len(fam.members) == fam.L
    assert fam.lead == list(range(fam.lead[0], fam.lead[0] + fam.L))
    assert sorted(x % fam.L for x in fam.lead) == list(range(fam.L))
    assert shifts == [x - fam.lead[0] for x in fam.lead]
    # the model reports the lead-in's length itself: the last bit of block 0
    assert max(s.last for s in base.syms if s.block == 0 and s.piece == 0) + 1 == fam.lead[0]


@pytest.mark.parametrize("key", FAMILIES, ids=lambda k: "-".join(map(str, k)))
def test_every_kind_meets_every_seam_relation(ica, oracle, key):
    """Each (kind, relation) pair occurs in each family, counted with the model over all members -- but for the cells walk_seams.impossible
    lists with their reasons (no stream of that table set can fill them), which must in turn stay empty."""
    fam, base, table, _ = _walked(ica, oracle, key)
    skip = ws.impossible(fam.layout, fam.tables)
    print(ws.format_table(fam.name, table, skip))
    for k, kn in enumerate(ws.KINDS):
        for r, rn in enumerate(ws.RELATIONS):
            if (k, r) in skip:
                assert table[k, r] == 0, (fam.name, kn, rn, "listed as impossible, yet it occurs")
            else:
                assert table[k, r] > 0, (fam.name, kn, rn)
    if fam.layout != "grey":  # the wrap of the block-in-MCU counter is not the same event as a block's end
        r7, r8 = ws.RELATIONS.index("block complete at seam"), ws.RELATIONS.index("MCU complete at seam")
        assert 0 < table[ws.KINDS.index("EOB"), r8] < table[ws.KINDS.index("EOB"), r7]


@pytest.mark.parametrize("key", FAMILIES, ids=lambda k: "-".join(map(str, k)))
def test_the_body_holds_what_the_rules_need(ica, oracle, key):
    fam, base, _, _ = _walked(ica, oracle, key)
    L, syms = fam.L, [s for s in base.syms if not (s.block == 0 and s.piece == 0)]
    dc = {s.size for s in syms if s.kind == ws.DC}
    assert 0 in dc and 11 in dc and max(dc) == 11
    ac = {s.size for s in syms if s.kind == ws.AC}
    assert 1 in ac and 10 in ac
    runs, n = [], 0  # lengths of the runs of consecutive ZRL symbols
    for s in syms:
        if s.kind == ws.ZRL:
            n += 1
        elif n:
            runs.append(n)
            n = 0
    assert 1 in runs and 3 in runs
    assert any(a.kind == ws.DC and b.kind == ws.EOB for a, b in zip(syms, syms[1:]))
    assert any(ws.ends_at_63(s) for s in syms)
    by_block = {}
    for s in base.syms:
        by_block.setdefault((s.piece, s.block), []).append(s)
    # a block longer than two whole subsequences: one subsequence completes no block and starts inside one
    assert any(b[-1].last - b[0].first + 1 > 2 * L for b in by_block.values())
    assert any(n == 0 and z != 0 for j in range(len(base.pieces)) for _, z, _, n in base.handover(L, j))
    # 63 consecutive size-8 coefficients, all beyond a byte
    dense = [b for b in by_block.values() if sum(1 for s in b if s.kind == ws.AC and s.size == 8 and ws.escaped(s) and s.z1 == s.z0 + 1) == 63]
    assert len(dense) >= 2
    if fam.tables == "long":
        # ... of twelve bits each under an entry table: the write pass takes two per iteration (24 <= 32 bits), four records, for 31 iterations
        # on end -- more than MIJ_ES_REC_EVERY = 7 between two flushes
        assert any(all(s.last - s.first + 1 == 12 and s.rank < 2 for s in b if s.kind == ws.AC) for b in dense)
    else:
        # Annex K: ten-bit (luma) or nine-bit (chroma) codes: 36 or 34 bits a pair, beyond the window -- one per iteration, two records
        assert all(s.last - s.first + 1 in (17, 18) for b in dense for s in b if s.kind == ws.AC)
    # the flat run: DC category 0 and an EOB, N_FLAT blocks on end; with one-bit codes (the "long" set) two bits a block, the densest
    # record stream there is -- whole subsequences of it, and a longer symbol behind it
    best = run = 0
    for key_, b in sorted(by_block.items()):
        flat = len(b) == 2 and b[0].size == 0 and b[1].kind == ws.EOB and key_ != (0, 0)
        run = run + 1 if flat else 0
        best = max(best, run)
    assert best >= (ws.N_FLAT if not fam.restart else ws.N_FLAT // 3)
    if fam.tables == "long":
        two = [b for b in by_block.values() if len(b) == 2 and b[1].last - b[0].first + 1 == 2]
        assert len(two) >= ws.N_FLAT and 2 * ws.N_FLAT > 2 * L
    if fam.restart:
        assert len(base.pieces) == 3 and base.nblocks[2] == base.bpm and base.nsub(L, 2) == 1
    assert max(base.nsub(L, j) for j in range(len(base.pieces))) < 96  # the true chain reaches the last subsequence inside ES_MAX_ROUNDS


@pytest.mark.parametrize("layout", ("grey", "420"))
def test_l1_family_sits_on_the_limit(ica, oracle, layout):
    """every member's largest block L1 is exactly MIJ_BLOCK_L1_LIMIT (the model's sum and the host walk's flag), its lead-ins cover every
    offset, and every coefficient of a strong block starts exactly at a seam in some member"""
    fam = ws.seam_family(ica, layout, "annexk", 256, body="l1")
    assert fam.lead == list(range(fam.lead[0], fam.lead[0] + 256))
    base = ws.walk(fam.members[0])
    at_seam = set()
    for d in fam.members:
        w, _ = ws.shifted_walk(base, d)
        l1 = np.abs(w.coef.astype(np.int64)).sum(axis=1)
        assert l1.max() == ws.L1_LIMIT and (l1 == ws.L1_LIMIT).sum() == 2
        desc, want = ica.HostDecoder.decode(d, 3)
        assert desc.flags & 1 == 0
        for a, b in zip(ica.detile_coefficients(desc, want), w.planes()):
            assert np.array_equal(a, b)
        assert oracle.load(d, 3)[0] == "ok" and sc.predict_anomaly(d) == 0
        strong = {int(b) for b in np.flatnonzero(l1 == ws.L1_LIMIT)}
        at_seam |= {(s.block, s.z0) for s in w.syms if s.block in strong and s.kind == ws.AC and s.first % 256 == 0}
    assert len(at_seam) == 24  # twelve coefficients in each of the two strong blocks


def test_handover_states_follow_the_rule_as_written(ica, oracle):
    """The model's hand-over states against the rule spelled out on the bits: a subsequence hands over behind the last symbol that
    starts before its end, and the blocks it completes add up"""
    fam, base, _, _ = _walked(ica, oracle, ("seam", "410", "annexk", 256))
    ho = base.handover(256)
    assert len(ho) == base.nsub(256) == (base.nbits[0] + 255) // 256
    assert ho[0][:3] == (0, 0, 0) and sum(h[3] for h in ho) == base.nblocks[0]
    starts = {s.first: s for s in base.syms}
    for i, (p, z, c, n) in enumerate(ho[1:], 1):
        assert 256 * i <= p < 256 * i + 32
        prev = max((s for s in base.syms if s.first < 256 * i), key=lambda s: s.first)
        assert prev.last + 1 == p and (prev.z1 % 64) == z
        assert starts[p].bim == c if p in starts else prev is base.syms[-1]


def test_chain_shapes_have_the_subsequence_counts(ica, oracle):
    """nsub = 1, 2, 255, 256, 257, 512, 513 at L = 256, from the model; two members an exact multiple of L long and three one byte more"""
    got, exact, plus = [], 0, 0
    for (data, nbytes), want in zip(ws.chain_shapes(ica), ws.CHAIN_NSUB):
        w = ws.walk(data)
        assert len(w.pieces) == 1 and w.nbits[0] == 8 * nbytes
        got.append(w.nsub(ws.CHAIN_L))
        assert len(w.handover(ws.CHAIN_L)) == want
        exact += w.nbits[0] % ws.CHAIN_L == 0
        plus += w.nbits[0] % ws.CHAIN_L == 8
        desc, planes = ica.HostDecoder.decode(data, 3)
        for a, b in zip(ica.detile_coefficients(desc, planes), w.planes()):
            assert np.array_equal(a, b)
        assert oracle.load(data, 3)[0] == "ok" and sc.predict_anomaly(data) == 0 and sc.expected_extract_status(data) == 1
    assert tuple(got) == ws.CHAIN_NSUB
    assert exact >= 2 and plus >= 2


def test_slow_family_is_conforming_and_graded(ica, oracle):
    bits = []
    for data, neighbour in ws.slow_family(ica):
        w = ws.walk(data)
        bits.append(w.nbits[0])
        desc, planes = ica.HostDecoder.decode(data, 3)
        for a, b in zip(ica.detile_coefficients(desc, planes), w.planes()):
            assert np.array_equal(a, b)
        for d in (data, neighbour):
            assert oracle.load(d, 3)[0] == "ok" and sc.predict_anomaly(d) == 0 and sc.expected_extract_status(d) == 1
    print("slow family, bits of entropy data:", bits, "subsequences of 256 bits:", [(b + 255) // 256 for b in bits])
    assert bits == sorted(bits) and bits[0] < 8000 and 36000 < bits[-1] < 48000
    # either side of ES_MAX_ROUNDS = 96 subsequences of 256 bits: the true chain settles one per round at the least
    assert sum(1 for b in bits if 32 * 256 < b <= 96 * 256) >= 3 and sum(1 for b in bits if b > 110 * 256) >= 3
