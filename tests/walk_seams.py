"""The GPU Huffman walk at the seams of its own work division (test_walk_seams_host.py, test_gpu_walk_seams.py).  The walk cuts the unstuffed
entropy data of a scan into subsequences of DevScan.sub_bits bits, one lane each; the state-only passes (es_state_walk, EsUni) and the write
pass (es_decode<true> / es_write_records) must hand every subsequence over at the same symbol: "a symbol that starts before p_end is
finished", a pair of the state passes only when both symbols END by p_end, the second symbol of the write pass when it STARTS before
p_end.  Those rules only fire when a particular symbol sits at a particular bit next to a multiple of sub_bits, so the families here PUT
every symbol of a rich body at every offset modulo the subsequence length.

The model: a symbol-level sequential walk (walk) of a one-scan baseline stream, restart intervals included, in bits of the unstuffed
interval -- the walk header_cases.walk_events and coef_cases.block_bit_ranges do, reporting every symbol instead of counting or
skipping it (marker parsing and tables are stream_cases').  From it: the true hand-over state and completed-block count of every
subsequence of a length L (Walk.handover), and the relation of every symbol to the seams (relations).

The families:
  seam_family(ica, layout, tables, L)   a body of some hundred feature blocks and three hundred flat ones behind a LEAD-IN, the scan's
      first block (DC 0, so the body's DC differences do not depend on it), whose AC symbols are chosen so that its bit length takes L
      consecutive values over the L members: every symbol of the body visits every offset modulo L.  Layouts grey (one block per MCU), 420
      (six), 410 = (4,2),(1,1),(1,1) (ten: the bound of DevScan.blk_comp); table sets "annexk" (the writer's), "long" (shape_table: DC and AC
      codes of 13..16 bits beside a one-bit DC category 0, a one-bit EOB and a four-bit 0x08) and "third" (helpers.third_tables).
  seam_family(..., body="l1")   the same lead-ins in front of blocks whose L1 is exactly MIJ_BLOCK_L1_LIMIT: the per-block L1 sum of the
      int16 write pass (head by the lane that begins the block, rest by k_es_tails) must count a coefficient at a seam once
  restart_twins(ica, L)     the 4:2:0 Annex-K family with a restart interval that leaves three scans, the last a single MCU
  chain_shapes(ica)         tame noise whose interval lengths give nsub = 1, 2, 255, 256, 257, 512, 513 at L = 256 (EsWork's 256
                            subsequences per workgroup, k_es_offsets' per = ceil(nsub / 256), the queue packing of k_es_syncq)
  slow_family(ica)          the recipe of tools/dbg/dense.py in graded sizes: chains that settle a subsequence per round

Two things the tables decide, found while building these: under the Annex-K luma table a size-8 coefficient costs 18 bits, two of them
36 -- more than the 32 valid bits of the write pass's window, so they are NOT taken as a pair; the four-records-per-iteration edge of
MIJ_ES_REC_BUF (two escaped coefficients in one iteration) needs a code of at most eight bits for symbol 0x08, which the "long" set has.
And Annex K has no one-bit code, so the flat run costs six (luma) or four (chroma) bits a block there; the two-bit block of
test_gpu_walk_densest_record_stream (the record region's bound) is the "long" set's."""
import collections

import numpy as np

import header_cases as hc
import helpers
import idct_model as M
import stream_cases as sc

# ---------------------------------------------------------------------------------------------- the model

DC, AC, ZRL, EOB = 0, 1, 2, 3
KIND_NAMES = ("DC", "AC", "ZRL", "EOB")
# one symbol: kind; first bit, last bit of the code, last bit (extra bits included) -- in bits of the interval's unstuffed bytes; block
# ordinal inside the interval and block inside the MCU; zigzag index before and after (after = 64: the symbol completes the block); code
# length; size (extra bits); value; rank of its table among the scan's tables of its class in order of first use (2 and more: no entry
# table in EsUni / EsW / EsPair, the search path); interval
Sym = collections.namedtuple("Sym", "kind first last_code last block bim z0 z1 codelen size value rank piece")


def ends_at_63(s):
    """a coefficient at index 63: the block ends without an EOB"""
    return s.kind == AC and s.z1 == 64


def escaped(s):
    """the coefficient lies beyond a byte (compact planes: an escape byte, the record form: an escape record)"""
    return s.kind == AC and not -128 <= s.value <= 127


def _lut(table):
    """{(length, code): symbol} -> 65536 entries length << 8 | symbol by the next sixteen bits (0: no code)"""
    a = np.zeros(65536, np.int32)
    for (ln, code), s in table.items():
        a[code << (16 - ln):(code + 1) << (16 - ln)] = (ln << 8) | s
    return a


def _windows(piece):
    """the next sixteen bits at every bit position of the interval (zeros behind its end, as the arena has them)"""
    bits = np.unpackbits(np.frombuffer(piece + b"\0" * 8, np.uint8)).astype(np.int32)
    n = 8 * len(piece) + 32
    w = np.zeros(n, np.int32)
    for i in range(16):
        w |= bits[i:i + n] << (15 - i)
    return w


class Walk:
    def __init__(self, data):
        self.data = data
        segs, _ = sc._segments(data)
        self.comps, self.nmcu, self.dri = sc._frame(segs)
        self.tabs = sc._huff(segs[0xC4])
        sos = segs[0xDA][0]
        sel = {sos[1 + 2 * c]: (sos[2 + 2 * c] >> 4, sos[2 + 2 * c] & 15) for c in range(sos[0])}
        self.order, self.blk_comp = [], []
        for ci, (cid, a, v) in enumerate(self.comps):
            self.order += [sel[cid]] * (a * v)
            self.blk_comp += [ci] * (a * v)
        self.bpm = len(self.order)
        dc_rank, ac_rank = {}, {}
        for td, ta in self.order:
            dc_rank.setdefault(td, len(dc_rank))
            ac_rank.setdefault(ta, len(ac_rank))
        self.rank = [(dc_rank[td], ac_rank[ta]) for td, ta in self.order]
        self.luts = {k: _lut(t) for k, t in self.tabs.items()}
        self.pieces = sc.pieces(data)
        self.nbits = [8 * len(p) for p in self.pieces]
        self.nblocks = [(min(self.dri, self.nmcu - j * self.dri) if self.dri else self.nmcu) * self.bpm for j in range(len(self.pieces))]
        self.syms = []    # every symbol of the scan in order
        self.first_sym = []  # per interval: index of its first symbol
        self.coef = np.zeros((self.nmcu * self.bpm, 64), np.int16)  # scan order, zigzag, DC predicted

    def run(self, stop_blocks=None):
        """the sequential walk (stop_blocks: only that many blocks of the first interval)"""
        b0 = 0
        for j, piece in enumerate(self.pieces):
            self.first_sym.append(len(self.syms))
            win = _windows(piece).tolist()
            if not hasattr(self, "list_luts"):  # (shifted_walk hands a sibling's on: the same tables)
                self.list_luts = {k: v.tolist() for k, v in self.luts.items()}
            luts = self.list_luts
            big, tot = int.from_bytes(piece + b"\0" * 8, "big"), 8 * len(piece) + 64
            pos, pred = 0, [0] * len(self.comps)
            n = self.nblocks[j] if stop_blocks is None else stop_blocks
            for b in range(n):
                bim = b % self.bpm
                td, ta = self.order[bim]
                rd, ra = self.rank[bim]
                e = luts[(0, td)][win[pos]]
                assert e, "no DC code at bit %d of interval %d" % (pos, j)
                ln, cat = e >> 8, e & 255
                v = 0
                if cat:
                    v = (big >> (tot - pos - ln - cat)) & ((1 << cat) - 1)
                    if not v >> (cat - 1):
                        v -= (1 << cat) - 1
                self.syms.append(Sym(DC, pos, pos + ln - 1, pos + ln + cat - 1, b, bim, 0, 1, ln, cat, v, rd, j))
                pos += ln + cat
                ci = self.blk_comp[bim]
                pred[ci] += v
                self.coef[b0 + b, 0] = pred[ci]
                k, lac = 1, luts[(1, ta)]
                while k < 64:
                    e = lac[win[pos]]
                    assert e, "no AC code at bit %d of interval %d" % (pos, j)
                    ln, rs = e >> 8, e & 255
                    r, sz = rs >> 4, rs & 15
                    if sz == 0:
                        kind, k1 = (ZRL, k + 16) if rs == 0xF0 else (EOB, 64)
                        assert k1 <= 64, "a ZRL past the block's end"
                        self.syms.append(Sym(kind, pos, pos + ln - 1, pos + ln - 1, b, bim, k, k1, ln, 0, 0, ra, j))
                        pos += ln
                        k = k1
                        continue
                    v = (big >> (tot - pos - ln - sz)) & ((1 << sz) - 1)
                    if not v >> (sz - 1):
                        v -= (1 << sz) - 1
                    assert k + r <= 63, "a run past coefficient 63"
                    self.coef[b0 + b, k + r] = v
                    self.syms.append(Sym(AC, pos, pos + ln - 1, pos + ln + sz - 1, b, bim, k, k + r + 1, ln, sz, v, ra, j))
                    pos += ln + sz
                    k += r + 1
            if stop_blocks is not None:
                return self
            assert 0 <= self.nbits[j] - pos < 8, "the walk does not end in the interval's last byte"
            b0 += n
        return self

    def interval(self, j):
        lo = self.first_sym[j]
        hi = self.first_sym[j + 1] if j + 1 < len(self.first_sym) else len(self.syms)
        return self.syms[lo:hi]

    def nsub(self, L, j=0):
        """subsequences of interval j (mij_batch_add_stream: at least one)"""
        return max(1, (self.nbits[j] + L - 1) // L)

    def handover(self, L, j=0):
        """-> [(p, z, c, blocks completed)] per subsequence of interval j: the true state it starts from (bit position, next coefficient
        index, block inside the MCU) and the blocks its symbols complete.  Subsequence i takes the symbols from its start state up to the
        last one that STARTS before min((i + 1) L, nbits)"""
        out, syms, k = [], self.interval(j), 0
        p, z, c = 0, 0, 0
        for i in range(self.nsub(L, j)):
            end, done = min((i + 1) * L, self.nbits[j]), 0
            start = (p, z, c)
            while k < len(syms) and syms[k].first < end:
                s = syms[k]
                p, z = s.last + 1, s.z1
                if z == 64:
                    z, c, done = 0, (c + 1) % self.bpm, done + 1
                k += 1
            out.append(start + (done,))
        return out

    def planes(self):
        """per component [bh, bw, 8, 8], natural order: what detile_coefficients gives"""
        hv = [(a, v) for _, a, v in self.comps]
        hmax = max(a for a, _ in hv)
        # (the frame's width is not kept by stream_cases._frame: read it from the SOF payload)
        segs, _ = sc._segments(self.data)
        sof = segs[0xC0][0]
        w = (sof[3] << 8) | sof[4]
        mcu_x = (w + 8 * hmax - 1) // (8 * hmax)
        mcu_y = self.nmcu // mcu_x
        out = [np.zeros((mcu_y * v, mcu_x * a, 64), np.int16) for a, v in hv]
        b = 0
        for m in range(self.nmcu):
            my, mx = divmod(m, mcu_x)
            for ci, (a, v) in enumerate(hv):
                for y in range(v):
                    for x in range(a):
                        out[ci][my * v + y, mx * a + x] = self.coef[b]
                        b += 1
        return [M.zz_to_nat(p) for p in out]


def walk(data):
    return Walk(data).run()


def shifted_walk(base, data):
    """The walk of a family member from the walk `base` of a sibling: the lead-in (the first block) is walked symbol by symbol; every later
    symbol of the first interval is then decoded AT the position the sibling's walk gives it, moved by the difference of the lead-ins, with
    the table of its block -- each must be the sibling's symbol, code length and extra bits (so, by induction over the symbols, the sequential
    walk of this member gives exactly them), and the later intervals must be the sibling's bytes.  -> (Walk, shift).  The check "the bodies
    are bit-identical up to the shift" by walking, at the cost of a few numpy gathers per member."""
    w = Walk(data)
    assert w.tabs == base.tabs
    w.list_luts = base.list_luts
    w.run(stop_blocks=1)
    lead = list(w.syms)
    nb = sum(1 for s in base.syms if s.block == 0 and s.piece == 0)
    body = base.interval(0)[nb:]
    shift = lead[-1].last + 1 - body[0].first
    assert w.order == base.order and w.tabs == base.tabs and w.pieces[1:] == base.pieces[1:] and w.nblocks == base.nblocks
    first = np.array([s.first for s in body]) + shift
    win = _windows(w.pieces[0])
    bits = np.unpackbits(np.frombuffer(w.pieces[0] + b"\0" * 8, np.uint8))
    for cls in (0, 1):
        for t in {(o[0] if cls == 0 else o[1]) for o in w.order}:
            idx = np.array([k for k, s in enumerate(body) if (s.kind == DC) == (cls == 0) and w.order[s.bim][cls] == t], np.int64)
            if not idx.size:
                continue
            e = w.luts[(cls, t)][win[first[idx]]]
            want = np.array([(body[k].codelen << 8) | (body[k].size if cls == 0 else _rs(body[k])) for k in idx])
            assert np.array_equal(e, want), "member and sibling differ behind the lead-in"
    # the extra bits: the same bits at the moved positions
    if not hasattr(base, "_extra"):
        b0 = np.unpackbits(np.frombuffer(base.pieces[0] + b"\0" * 8, np.uint8))
        at = np.concatenate([np.arange(s.last_code + 1, s.last + 1) for s in body if s.size])
        base._extra = (at, b0[at])
    assert np.array_equal(bits[base._extra[0] + shift], base._extra[1]), "extra bits differ behind the lead-in"
    end = body[-1].last + 1 + shift
    assert 0 <= w.nbits[0] - end < 8
    w.syms = lead + [Sym._make((s[0], s[1] + shift, s[2] + shift, s[3] + shift) + s[4:]) for s in body] + base.syms[len(base.interval(0)):]
    w.first_sym = [0] + [f - len(base.interval(0)) + len(lead) + len(body) for f in base.first_sym[1:]]
    w.coef = base.coef.copy()
    w.coef[0] = 0
    for s in lead:
        if s.kind == AC:
            w.coef[0, s.z1 - 1] = s.value
        elif s.kind == DC:
            assert s.value == 0
    return w, shift


def _rs(s):
    """the run/size byte of an AC-class symbol"""
    if s.kind == ZRL:
        return 0xF0
    if s.kind == EOB:
        return 0x00
    return ((s.z1 - 1 - s.z0) << 4) | s.size


# ---------------------------------------------------------------------------------------------- seam relations

KINDS = ("DC", "AC size 1", "AC size 10", "escaped AC", "ZRL", "EOB", "ends at 63", "code of 13+ bits", "third table")
RELATIONS = ("last bit at seam-1", "first bit at seam-1", "first bit at seam", "code before, extra bits behind", "pair second starts at seam-1",
             "pair second starts at seam", "pair second ends at seam", "block complete at seam", "MCU complete at seam")


def kinds_of(s):
    out = []
    if s.kind == DC:
        out.append(0)
    if s.kind == AC and s.size == 1:
        out.append(1)
    if s.kind == AC and s.size == 10:
        out.append(2)
    if escaped(s):
        out.append(3)
    if s.kind == ZRL:
        out.append(4)
    if s.kind == EOB:
        out.append(5)
    if ends_at_63(s):
        out.append(6)
    if s.codelen >= 13:
        out.append(7)
    if s.rank >= 2:
        out.append(8)
    return out


def relations(w, L, table=None):
    """Counts, per (kind, relation), of the symbols of a walk that stand in the relation to a seam (a multiple of L inside the interval's
    data; a symbol that ENDS at the data's end is not at a seam).  A "pair" is what EsUni folds into one entry: two consecutive AC-class
    symbols of a block, both under an entry table (rank < 2), the first no EOB, code and extra bits of both inside twelve bits."""
    table = np.zeros((len(KINDS), len(RELATIONS)), np.int64) if table is None else table
    for j in range(len(w.pieces)):
        syms, nbits = w.interval(j), w.nbits[j]
        prev = None
        for s in syms:
            rel = []
            seam_after = (s.last + 1) % L == 0 and s.last + 1 < nbits
            if seam_after:
                rel.append(0)
            if (s.first + 1) % L == 0 and s.first + 1 < nbits:
                rel.append(1)
            if s.first % L == 0 and s.first:
                rel.append(2)
            if s.size and (s.last_code + 1) % L == 0:
                rel.append(3)
            pair = prev is not None and prev.block == s.block and prev.kind in (AC, ZRL) and s.kind != DC and s.rank < 2 and \
                prev.z1 < 64 and (prev.last - prev.first + 1) + (s.last - s.first + 1) <= 12
            if pair:
                if (s.first + 1) % L == 0 and s.first + 1 < nbits:
                    rel.append(4)
                if s.first % L == 0:
                    rel.append(5)
                if seam_after:
                    rel.append(6)
            if s.z1 == 64 and seam_after:
                rel.append(7)
                if s.bim == w.bpm - 1:
                    rel.append(8)
            for k in kinds_of(s):
                for r in rel:
                    table[k, r] += 1
            prev = s
    return table


def scan_ordinal(w, ci, by, bx, mcu_x):
    """the place of block (by, bx) of component ci in the scan"""
    hv = [(a, v) for _, a, v in w.comps]
    a, v = hv[ci]
    j0 = sum(x * y for x, y in hv[:ci])
    return ((by // v) * mcu_x + bx // a) * w.bpm + j0 + (by % v) * a + bx % a


def seam_notes(w, L, ordinal):
    """for assertion messages: the symbols of the scan's block `ordinal` that touch a seam of length L, and how"""
    j, b = divmod(ordinal, w.dri * w.bpm if w.dri else w.nmcu * w.bpm)
    notes = []
    for s in w.interval(j):
        if s.block != b:
            continue
        how = []
        if s.first // L != s.last // L:
            how.append("straddles the seam at %d" % (s.last // L * L))
        if (s.last + 1) % L == 0:
            how.append("ends at the seam %d" % (s.last + 1))
        if s.first % L == 0 and s.first:
            how.append("starts at the seam %d" % s.first)
        if (s.first + 1) % L == 0:
            how.append("starts one bit before the seam %d" % (s.first + 1))
        if how:
            notes.append("%s z %d->%d bits %d..%d (code %d + %d) %s" % (KIND_NAMES[s.kind], s.z0, s.z1, s.first, s.last, s.codelen, s.size, ", ".join(how)))
    blk = [s for s in w.interval(j) if s.block == b]
    return "block %d of interval %d (block %d of its MCU), bits %d..%d, subsequences %d..%d: %s" % (
        b, j, b % w.bpm, blk[0].first, blk[-1].last, blk[0].first // L, blk[-1].last // L, "; ".join(notes) or "no symbol of it touches a seam")


def impossible(layout, tables):
    """the (kind, relation) cells no stream of a family can fill, each for a reason of the format or of the table set:
      a symbol without extra bits (ZRL, EOB) cannot have them behind a seam;
      only an EOB or a coefficient at index 63 completes a block (ZRL past the end is no conforming stream), so only they -- and what they
      are besides: a long code, a third table's symbol, a size-1 or escaped coefficient AT 63 -- can complete a block or an MCU at a seam;
      a DC symbol is never the second of a pair; a pair lies inside twelve bits behind a first symbol of two bits at least, so no size-10
      coefficient, no escaped one (size 8 and more), no code of 13 bits is its second, and no ZRL either (eleven bits under the Annex-K
      luma table, ten under the chroma table, behind a first symbol of three); a third table has no entries, hence no pairs;
      the "long" set's only short AC codes are the EOB (one bit) and 0x08 (four bits + eight): a pair there is a ZRL-free (first, EOB)
      with the first inside eleven bits -- none exists (0x08 alone takes twelve), so the set has no pairs at all;
      Annex K has no code of 13 and 14 bits but has 15- and 16-bit ones (kept); only the "third" set has third-table symbols."""
    K, R = {k: i for i, k in enumerate(KINDS)}, {r: i for i, r in enumerate(RELATIONS)}
    out = set()
    for k in ("ZRL", "EOB"):
        out.add((K[k], R["code before, extra bits behind"]))
    for k in ("DC", "ZRL"):
        out.add((K[k], R["block complete at seam"]))
        out.add((K[k], R["MCU complete at seam"]))
    for k in ("DC", "AC size 10", "escaped AC", "ZRL", "code of 13+ bits", "third table"):
        for r in ("pair second starts at seam-1", "pair second starts at seam", "pair second ends at seam"):
            out.add((K[k], R[r]))
    if tables == "long":
        for k in range(len(KINDS)):
            for r in ("pair second starts at seam-1", "pair second starts at seam", "pair second ends at seam"):
                out.add((k, R[r]))
    if tables != "third":
        for r in range(len(RELATIONS)):
            out.add((K["third table"], r))
    return out


def format_table(name, table, skip):
    lines = ["%s" % name, "%-18s" % "" + " ".join("%7d" % i for i in range(len(RELATIONS)))]
    for k, kn in enumerate(KINDS):
        lines.append("%-18s" % kn + " ".join("%7s" % ("n/a" if (k, r) in skip else int(table[k, r])) for r in range(len(RELATIONS))))
    lines.append("relations: " + "; ".join("%d %s" % (i, r) for i, r in enumerate(RELATIONS)))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------- writing from tokens

LAYOUT_HV = {"grey": [(1, 1)], "420": [(2, 2), (1, 1), (1, 1)], "410": [(4, 2), (1, 1), (1, 1)]}
TABLE_SETS = ("annexk", "long", "third")
LEAD_SIZES = range(1, 9)  # the lead-in's coefficients: run 0, sizes 1..8


def annex_k(ica):
    """the Annex-K tables as the product's writer puts them into its streams: -> [(class, id, bits, vals)]"""
    segs, _ = sc._segments(ica.stbi_write_jpg_to_memory(np.zeros((8, 8, 3), np.uint8), 90))
    out = []
    for p in segs[0xC4]:
        j = 0
        while j < len(p):
            cnt = sum(p[j + 1:j + 17])
            out.append((p[j] >> 4, p[j] & 15, tuple(p[j + 1:j + 17]), tuple(p[j + 17:j + 17 + cnt])))
            j += 17 + cnt
    t = {(c, i): (b, v) for c, i, b, v in out}
    # what makes them Annex K: twelve DC categories, 162 AC symbols, the luma EOB at four bits and 0x01 at two
    assert sorted(t) == [(0, 0), (0, 1), (1, 0), (1, 1)] and len(t[(0, 0)][1]) == 12 and len(t[(1, 0)][1]) == 162 and len(t[(1, 1)][1]) == 162
    enc = hc.canonical(*t[(1, 0)])
    assert enc[0x00] == (0b1010, 4) and enc[0x01] == (0b00, 2) and enc[0x08][1] == 10
    return sorted(out)


def _bitstring(tokens, enc):
    out = []
    for cls, ci, sym, extra, nx in tokens:
        code, ln = enc[(cls, ci)][sym]
        out.append(format(code, "0%db" % ln))
        if nx:
            out.append(format(extra & ((1 << nx) - 1), "0%db" % nx))
    return "".join(out)


def _entropy(intervals):
    """bit strings, one per restart interval -> stuffed bytes with RSTn between, each interval padded with one bits"""
    out = bytearray()
    for j, bits in enumerate(intervals):
        if j:
            out += bytes([0xFF, 0xD0 + (j - 1) % 8])
        bits += "1" * (-len(bits) % 8)
        out += int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00") if bits else b""
    return bytes(out)


def planes_of_units(w, h, hv, blocks):
    """[nblocks, 64] in scan order -> per-component planes [bh][bw][64]"""
    planes = hc.blank(w, h, hv)
    wr = hc.Writer(w, h, hc.default_comps(hv), planes)
    b = 0
    for mcu in wr._units(list(range(len(hv)))):
        for ci, by, bx in mcu:
            planes[ci][by, bx] = blocks[b]
            b += 1
    assert b == len(blocks)
    return planes


def _fill_costs(enc_ac, sizes=LEAD_SIZES):
    return {n: enc_ac[n][1] + n for n in sizes}


def _fill_plan(costs, lo, hi, most=62):
    """fewest coefficients (sizes from `costs`) whose bits sum to t, for every t in lo..hi: -> {t: [sizes]} (a missing t cannot be made)"""
    best = {0: []}
    for t in range(1, hi + 1):
        for n, c in costs.items():
            p = best.get(t - c)
            if p is not None and len(p) < most and (t not in best or len(p) + 1 < len(best[t])):
                best[t] = p + [n]
    return {t: best[t] for t in range(lo, hi + 1) if t in best}


def _fill_values(sizes):
    """a block's AC coefficients (zigzag 1...) of these sizes, run 0, signs alternating"""
    blk = np.zeros(64, np.int16)
    for k, n in enumerate(sizes, 1):
        blk[k] = ((1 << n) - 1) * (1 if k & 1 else -1)
    return blk


# ---------------------------------------------------------------------------------------------- the seam families

N_FEATURE, N_FLAT, N_TAIL = 120, 300, 12
DC_STEPS = (0, 1, -3, 2000, -2000, 5, 0, -17, 100, -86)  # categories 0, 1, 2, 11, 11, 3, 0, 5, 7, 7; sums to zero


def _feature(t, f):
    blk = np.zeros(64, np.int16)
    sg = -1 if f & 1 else 1
    if t == 0:      # EOB directly behind the DC term
        pass
    elif t == 1:    # a few small ones: pairs inside twelve bits
        blk[1], blk[2], blk[5] = sg, 2 * sg, -3 * sg
    elif t == 2:    # size 10 (a 16-bit code under Annex K, escaped) and size 1; a size-10 coefficient ends the block at 63
        blk[3], blk[4], blk[63] = sg * (512 + 37 * (f % 13)), -sg, -sg * (600 + f % 7)
    elif t == 3:    # ZRL alone
        blk[2], blk[20] = -sg, 2 * sg
    elif t == 4:    # three ZRL in a row
        blk[1], blk[52] = sg, -sg
    elif t == 5:    # the run ends at 63 without EOB: the second of a pair of small ones
        blk[1], blk[61], blk[62], blk[63] = 3 * sg, -sg, sg, -sg
    elif t == 6:    # many small ones
        for k in range(1, 11):
            blk[k] = (1 + (k + f) % 2) * (1 if (k + f) % 3 else -1)
    elif t == 7:    # escaped, sizes 8 and 9, and a coefficient at 63 beyond a byte
        blk[1], blk[2], blk[63] = 200 * sg, -300 * sg, 129 * sg
    elif t == 8:    # ZRL, then the end at 63 with a size-1 coefficient; a lone size-1 pair
        blk[1], blk[40], blk[63] = -sg, sg, sg
    return blk


def _dense63(f):
    """63 consecutive size-8 coefficients (magnitude 129..255: all beyond a byte, -128 is not): longer than two subsequences of 288 bits
    under every table set here"""
    k = np.arange(1, 64)
    blk = np.zeros(64, np.int16)
    blk[1:] = (129 + (k * 37 + f) % 127) * np.where((k + f) % 3 == 0, -1, 1)
    return blk


def body_blocks(layout):
    """the scan's blocks [n, 64] in scan order; block 0 (the lead-in) is left empty"""
    bpm = sum(a * v for a, v in LAYOUT_HV[layout])
    n = 1 + N_FEATURE + N_FLAT + N_TAIL
    n = (n + bpm - 1) // bpm * bpm
    blocks = np.zeros((n, 64), np.int16)
    comp_of = []
    for ci, (a, v) in enumerate(LAYOUT_HV[layout]):
        comp_of += [ci] * (a * v)
    flat = range(1 + N_FEATURE, 1 + N_FEATURE + N_FLAT)
    dense = (3 * bpm, 8 * bpm - 1)  # the first block of an MCU (the first component) and the last block of one (the last component)
    seen, dc = collections.Counter(), [0] * 3
    for f in range(1, n):
        ci = comp_of[f % bpm]
        if f in flat:
            blocks[f, 0] = dc[ci]
            continue
        if f >= n - bpm:  # the last MCU stays short: as a restart interval of its own it is one subsequence
            blocks[f] = _feature(f % 2, f)
        else:
            blocks[f] = _dense63(f) if f in dense else _feature((f + f // bpm) % 9, f)
        dc[ci] += DC_STEPS[seen[ci] % len(DC_STEPS)]
        seen[ci] += 1
        blocks[f, 0] = dc[ci]
    return blocks


def _long_tables(wr, sel):
    """DC and AC tables with codes of 13..16 bits beside a one-bit code for DC category 0 / the EOB and, in the first AC table, four bits
    for 0x08 (see the module comment)"""
    dc, ac = wr.symbols([s[0] for s in sel])
    need = collections.defaultdict(set)
    for ci, td, ta in sel:
        need[(0, td)] |= set(dc[ci])
        need[(1, ta)] |= set(ac[ci])
    need[(1, sel[0][2])] |= set(LEAD_SIZES) | {0x00}
    need[(0, sel[0][1])] |= {0}
    out = []
    for key in sorted(need):
        syms = sorted(need[key])
        short = {0: 1} if key[0] == 0 else ({0x00: 1, 0x08: 4} if key == (1, sel[0][2]) else {0x00: 1})
        short = {s: ln for s, ln in short.items() if s in syms}
        rest = [s for s in syms if s not in short]
        # (0x01 and 0x02 both at 13 bits: lead-in costs of 14 and 15 bits, so that every lead-in length can be made)
        place = {s: (13 if s in (0x01, 0x02) else 13 + k % 4) for k, s in enumerate(rest)}
        place.update(short)
        out.append(key + hc.shape_table(list(short) + rest, hc.profile_of(list(place.values())), place))
    return out


class Family:
    """members: the streams; lead: the bit length of each member's lead-in block"""
    def __init__(self, name, layout, tables, L, members, lead, restart=0):
        self.name, self.layout, self.tables, self.L, self.members, self.lead, self.restart = name, layout, tables, L, members, lead, restart


_families = {}


L1_LIMIT = M.L1_LIMIT
L1_LEAD_SIZES = range(1, 6)  # 62 coefficients of at most 31: a lead-in far below the limit


def l1_blocks(layout):
    """Two MCUs behind the lead-in in which one block of the first component and the last block of the second MCU have an L1 of exactly
    MIJ_BLOCK_L1_LIMIT (quantisers of one: the sum of the magnitudes), in size-10 coefficients of some 26 bits each: the picture is NOT
    wide, and it is as soon as the L1 of the int16 write pass -- the head of a block summed by the lane that begins it, the rest added by
    k_es_tails -- counts one coefficient at a seam twice."""
    bpm = sum(a * v for a, v in LAYOUT_HV[layout])
    blocks = np.zeros((3 * bpm, 64), np.int16)
    strong = np.zeros(64, np.int16)
    # ... and six small ones behind them, each the second symbol of its iteration of the write pass in some member
    strong[1:13] = (1023, -1023, 1023, -1023, 1023, -(L1_LIMIT - 5 * 1023 - 8), 1, -1, 2, -2, 1, -1)
    assert int(np.abs(strong).sum()) == L1_LIMIT
    for f in range(1, len(blocks)):
        blocks[f] = _feature(f % 2, f)
    blocks[bpm], blocks[3 * bpm - 1] = strong, -strong
    return blocks


def seam_family(ica, layout, tables, L, restart=0, body="rich"):
    key = (layout, tables, L, restart, body)
    if key in _families:
        return _families[key]
    hv = LAYOUT_HV[layout]
    assert tables != "third" or len(hv) == 3
    blocks = body_blocks(layout) if body == "rich" else l1_blocks(layout)
    bpm = sum(a * v for a, v in hv)
    nmcu = len(blocks) // bpm
    hmax, vmax = max(a for a, _ in hv), max(v for _, v in hv)
    w, h = 8 * hmax * nmcu, 8 * vmax
    wr = hc.Writer(w, h, hc.default_comps(hv), planes_of_units(w, h, hv, blocks))
    sel = hc.default_sel(len(hv))
    wr.restart = restart
    tabs = _long_tables(wr, sel) if tables == "long" else [t for t in annex_k(ica) if len(hv) > 1 or t[1] == 0]
    for t in sorted({c[3] for c in wr.comps}):
        wr.dqt([(0, t, hc.ONES64)])
    wr.sof()
    for t in tabs:
        wr.dht([t])
    if restart:
        wr.dri(restart)
    wr.seg(0xDA, wr.sos_payload(sel))
    header = wr.bytes()
    enc = {}
    for ci, td, ta in sel:
        enc[(0, ci)] = hc.canonical(*wr.huff[(0, td)])
        enc[(1, ci)] = hc.canonical(*wr.huff[(1, ta)])
    intervals = wr._tokens([s[0] for s in sel])
    assert intervals[0][0][:3] == (0, 0, 0) and intervals[0][1][:3] == (1, 0, 0x00)  # the empty lead-in: DC category 0, EOB
    rest = [_bitstring(iv, enc) for iv in intervals]
    body0 = _bitstring(intervals[0][2:], enc)
    fixed = enc[(0, 0)][0][1] + enc[(1, 0)][0x00][1]
    costs = _fill_costs(enc[(1, 0)], LEAD_SIZES if body == "rich" else L1_LEAD_SIZES)
    plan = _fill_plan(costs, 0, 40 * L)
    t0 = next(t for t in sorted(plan) if all(t + d in plan for d in range(L)))
    members, lead = [], []
    for d in range(L):
        sizes = plan[t0 + d]
        blk = _fill_values(sizes)
        toks = [(0, 0, 0, 0, 0)] + [(1, 0, n, int(blk[k]) if blk[k] >= 0 else int(blk[k]) - 1, n) for k, n in enumerate(sizes, 1)] + [(1, 0, 0x00, 0, 0)]
        lb = _bitstring(toks, enc)
        assert len(lb) == fixed + t0 + d
        data = header + _entropy([lb + body0] + rest[1:]) + hc.EOI
        members.append(helpers.third_tables(data) if tables == "third" else data)
        lead.append(len(lb))
    name = "%s/%s/L%d%s%s" % (layout, tables, L, "/DRI%d" % restart if restart else "", "" if body == "rich" else "/" + body)
    _families[key] = Family(name, layout, tables, L, members, lead, restart)
    return _families[key]


def restart_twins(ica, L):
    """the 4:2:0 Annex-K seam family as three scans: two intervals of half the MCUs (rounded down) and one of a single MCU"""
    nmcu = len(body_blocks("420")) // 6
    assert nmcu % 2 == 1  # (N_TAIL is chosen for it)
    return seam_family(ica, "420", "annexk", L, restart=nmcu // 2)


SEAM_PARAMS = [(layout, tables, L) for layout in ("grey", "420", "410") for tables in TABLE_SETS for L in (256, 288) if not (layout == "grey" and tables == "third")]


# ---------------------------------------------------------------------------------------------- chain shapes

CHAIN_L = 256
# unstuffed bytes of the one interval -> nsub = ceil(bytes / 32): 1, 2 (= 1 L + 1 byte), 255 and 256 (exact multiples of L), 257 (256 L + 1 byte),
# 512 (an exact multiple), 513 (512 L + 1 byte)
CHAIN_BYTES = (20, 33, 255 * 32, 256 * 32, 256 * 32 + 1, 512 * 32, 512 * 32 + 1)
CHAIN_NSUB = (1, 2, 255, 256, 257, 512, 513)
_chain = {}


def chain_shapes(ica):
    """-> [(stream, bytes of its interval)]: grey pictures 64 blocks wide of tame coefficients with a little seeded noise on top, Annex-K tables
    (fixed tables: a block's bits do not depend on the others'), the last eight blocks padded with coefficients so that the interval
    has exactly the wanted length"""
    if _chain:
        return _chain["all"]
    tabs = [t for t in annex_k(ica) if t[1] == 0]
    enc = {(0, 0): hc.canonical(*tabs[0][2:]), (1, 0): hc.canonical(*tabs[1][2:])}
    costs = _fill_costs(enc[(1, 0)])
    plan = _fill_plan(costs, 0, 1100)
    out = []
    for target in CHAIN_BYTES:
        pad, bw = (1, 2) if target < 64 else (8, 64)
        def picture(bh):
            wpx, hpx = 8 * bw, 8 * bh
            planes = hc.tame(wpx, hpx, LAYOUT_HV["grey"], seed=target)
            p = planes[0]
            v = np.random.default_rng(target).integers(0, 70, p[:, :, 1:12].shape)  # one call, row-major: a taller picture keeps the rows above
            p[:, :, 1:12] += np.where(v < 7, v - 3, 0).astype(np.int16)
            flat = p.reshape(-1, 64)
            flat[-pad:] = 0
            flat[-pad:, 0] = flat[-pad - 1, 0]
            wr = hc.Writer(wpx, hpx, hc.default_comps(LAYOUT_HV["grey"]), planes)
            return wpx, hpx, planes, len(_bitstring(wr._tokens([0])[0], enc))

        lo, hi = 1, 512  # the tallest picture whose bits, the padding blocks still empty, fit the wanted length
        assert picture(lo)[3] <= 8 * target < picture(hi)[3], target
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if picture(mid)[3] <= 8 * target else (lo, mid)
        wpx, hpx, planes, have = picture(lo)
        # the padding blocks share what is missing up to the last bit of the wanted byte
        missing, flat = 8 * target - have, planes[0].reshape(-1, 64)
        for k in range(pad):
            share = missing // (pad - k)
            share = max(t for t in plan if t <= share)
            flat[len(flat) - pad + k] += _fill_values(plan[share])
            missing -= share
        assert 0 <= missing < 8, (target, missing)
        wr = hc.plain(wpx, hpx, LAYOUT_HV["grey"], planes, tables=tabs)
        data = wr.bytes()
        assert len(sc.pieces(data)[0]) == target, (target, len(sc.pieces(data)[0]))
        out.append((data, target))
    _chain["all"] = out
    return out


# ---------------------------------------------------------------------------------------------- slow chains

SLOW_MCUS = (10, 25, 35, 45, 55, 65, 75, 85, 95, 105)
_slow = {}


def slow_family(ica):
    """tools/dbg/dense.py in graded sizes: pictures one block row high (quality 95: the writer's 4:4:4) whose blocks are full of +-1 with a few 0 and 2, through
    helpers.baseline_from_du.  A stream of near-equal symbol lengths has little for a wrong start to re-synchronise on: its chain settles
    a subsequence per round.  -> [(stream, its ordinary neighbour)]"""
    if _slow:
        return _slow["all"]
    out = []
    for m in SLOW_MCUS:
        plan, du = ica.host_transform(np.full((8, 8 * m, 3), 40, np.uint8), 95)
        du = du.copy()
        rng = np.random.default_rng(11 + m)
        du[:, 1:] = rng.choice(np.array([-1, 1, 0, 2], np.int16), size=(du.shape[0], 63), p=[0.46, 0.46, 0.06, 0.02])
        out.append((helpers.baseline_from_du(plan, du, 0, "native"), ica.synth_jpeg(64, 64, 1, 90)))
    _slow["all"] = out
    return out
