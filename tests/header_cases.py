"""Case generators for the header tests (test_headers_host.py, test_gpu_headers.py): what stands IN FRONT of the entropy data -- marker
segments and how tables are packed into them, frame layouts, scan structures, and the shapes of the Huffman tables.  Every other stream
test holds these fixed (one DQT per table, generated tables, component ids 1..3, one interleaved scan); here they are what varies.

The Writer below is a pure-Python writer for sequential JPEG from quantised coefficient planes (the plane convention of
coef_cases.Case.planes: per component [bh][bw][64], zigzag order, bh = MCU rows * v, bw = MCU columns * h).  Nothing is implied: the
caller emits every segment in the order it wants, and a scan is coded with the Huffman tables and the restart interval that are current
where it stands -- as a decoder sees them.

Every case has a name, a family, a kind and the status mjh_extract_scan must give it, tabulated per kind (KIND_STATUS) from the rule in
that function's comment: 0 the headers up to the frame header are rejected, 1 the GPU walk takes the stream, 2 the host walk.

Outside the contract (the reference does not define its answer; no reference answer is recorded): a table used before any segment
defined it, a file with no scan or a component no scan covers, DHT counts summing to more than 256, a DC symbol that asks
extend_receive for more than 16 bits -- and a fifth class found while recording: a table of 256 codes whose LAST code is nine bits or
shorter and is used.  stbi__build_huffman stores the index of a code in a byte of its fast table, where 255 means "not here" (codec/
jpeg.c:119-131), so that code is searched among the longer ones and the reference's own assertion (:237) fires.  The families hold
none of them; product_only() holds a handful of each."""
import collections

import numpy as np

import coef_cases as cc
import helpers

Case = collections.namedtuple("Case", "name family kind status data meta")

EOI = b"\xff\xd9"
ONES64 = (1,) * 64
SIZE = (134, 70)    # three components and more: no multiple of any MCU, several 1024-bit subsequences
TSIZE = (136, 72)   # the size of the `tables` family

# extraction verdict per kind (mjh_extract_scan's comment: one baseline scan carrying all of one or three components interleaved in
# frame order, at most ten blocks per MCU, a lone component 1x1, the entropy data followed by EOI; everything else is the host walk's)
KIND_STATUS = {
    "plain": 1,                 # ... whatever the segments in front of SOS hold
    "reject header": 0,         # the failure lies at or in front of the frame header
    "reject late": 2,           # ... behind it: the host walk reproduces the reference's reason
    "bad entropy": 1,           # whole headers, one scan, EOI behind the data: the GPU walk raises an anomaly and hands it back
    "four components": 2,
    "over ten blocks": 2,
    "lone sampled": 2,
    "permuted scan": 2,
    "several scans": 2,
    "progressive": 2,
    "not one scan then EOI": 2, # a DNL segment anywhere, fill bytes in front of a marker, anything but EOI behind the entropy data
    "no marker at sos": 2,      # padding behind SOF that the reference does not skip
}


# ---------------------------------------------------------------------------------------------- Huffman tables

def kraft(bits):
    """Kraft sum of a BITS list (counts per length 1..16) as a fraction of 65536"""
    return sum(int(n) << (16 - ln) for ln, n in enumerate(bits, 1))


def canonical(bits, vals, pick="first"):
    """-> {symbol: (code, length)} of a table as stbi__build_huffman numbers it; a symbol that occurs more than once is coded with its
    first or its last occurrence (pick)"""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            if pick == "last" or vals[k] not in out:
                out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def shape_table(symbols, profile, place=None, last=(), filler=None):
    """A table from a shape: `profile` (counts per length 1..16) is filled with `symbols`, canonical codes following.  place {symbol:
    length} pins symbols; the others take the free slots from the shortest on, in the order given.  Symbols in `last` stand behind the
    others of their length (the last code of the longest length of a complete profile is all ones).  Slots left over are filled with
    symbols the data does not need (`filler`, then repeats of the last symbol: a table may hold a symbol twice).  Refuses a profile
    that cannot hold the symbols, pins that find no slot, and a Kraft sum above one.  -> (bits, vals)"""
    profile = [int(n) for n in profile]
    assert len(profile) == 16
    place = dict(place or {})
    symbols = list(dict.fromkeys(symbols))
    if kraft(profile) > 65536:
        raise ValueError("Kraft sum above one")
    if sum(profile) < len(symbols):
        raise ValueError("the profile holds %d codes, the data needs %d symbols" % (sum(profile), len(symbols)))
    if sum(profile) > 256:
        raise ValueError("more than 256 codes")
    per = [[] for _ in range(16)]
    for s in symbols:
        if s in place:
            per[place[s] - 1].append(s)
            if len(per[place[s] - 1]) > profile[place[s] - 1]:
                raise ValueError("no slot of %d bits left for symbol 0x%02x" % (place[s], s))
    free = [s for s in symbols if s not in place]
    fill = [f for f in (filler if filler is not None else range(256)) if f not in symbols]
    for ln in range(16):
        while len(per[ln]) < profile[ln]:
            if free:
                per[ln].append(free.pop(0))
            elif fill:
                per[ln].append(fill.pop(0))
            else:
                per[ln].append(symbols[-1])
    assert not free
    vals = []
    for ln in range(16):
        vals += [s for s in per[ln] if s not in last] + [s for s in per[ln] if s in last]
    return tuple(profile), tuple(vals)


def profile_of(lengths):
    """the BITS list that has exactly one code per entry of `lengths`"""
    p = [0] * 16
    for ln in lengths:
        p[ln - 1] += 1
    return p


def optimal_table(freq):
    """T.81 Annex K.2 as tests/support/prog_writer.c (gen_table) states it: lengths from frequencies, limited to 16 bits, symbol 256
    reserved so that no real symbol gets the all-ones code.  freq: 257 counts.  -> (bits, vals)"""
    freq = list(freq) + [0] * (257 - len(freq))
    codesize, others = [0] * 257, [-1] * 257
    freq[256] = 1
    while True:
        c1, v = -1, -1
        for i in range(257):
            if freq[i] and (c1 < 0 or freq[i] <= v):
                v, c1 = freq[i], i
        c2, v = -1, -1
        for i in range(257):
            if freq[i] and i != c1 and (c2 < 0 or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    cnt = [0] * 33
    for i in range(257):
        if codesize[i]:
            cnt[min(codesize[i], 32)] += 1
    for i in range(32, 16, -1):
        while cnt[i] > 0:
            j = i - 2
            while cnt[j] == 0:
                j -= 1
            cnt[i] -= 2
            cnt[i - 1] += 1
            cnt[j + 1] += 2
            cnt[j] -= 1
    i = 16
    while cnt[i] == 0:
        i -= 1
    cnt[i] -= 1
    vals = [j for i in range(1, 33) for j in range(256) if codesize[j] == i]
    return tuple(cnt[1:17]), tuple(vals)


# ---------------------------------------------------------------------------------------------- the writer

def geometry(w, h, hv):
    """-> (mcu_x, mcu_y, [(bh, bw) per component]) for sampling factors hv = [(h, v), ...]"""
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    mcu_x, mcu_y = (w + 8 * hmax - 1) // (8 * hmax), (h + 8 * vmax - 1) // (8 * vmax)
    return mcu_x, mcu_y, [(mcu_y * v, mcu_x * a) for a, v in hv]


def blank(w, h, hv):
    return [np.zeros((bh, bw, 64), np.int16) for bh, bw in geometry(w, h, hv)[2]]


def tame(w, h, hv, seed=0):
    return cc._tame(blank(w, h, hv), seed)


def _size(v):
    return int(abs(int(v))).bit_length()


class Writer:
    """One stream, written front to back.  comps: [(id, h, v, tq)]; planes as above.  fill: 0xff fill bytes in front of every marker."""

    def __init__(self, w, h, comps, planes, fill=0):
        self.w, self.h, self.comps = w, h, [tuple(c) for c in comps]
        self.planes = [np.ascontiguousarray(p, np.int16) for p in planes]
        hv = [(c[1], c[2]) for c in self.comps]
        self.mcu_x, self.mcu_y, shapes = geometry(w, h, hv)
        for p, s in zip(self.planes, shapes):
            assert p.shape == s + (64,), (p.shape, s)
        self.hmax, self.vmax = max(a for a, _ in hv), max(b for _, b in hv)
        self.fill = fill
        self.huff = {}          # (class, id) -> (bits, vals, pick): the tables current at this point of the stream
        self.restart = 0        # the restart interval current at this point
        self.eob = 0x00         # the symbol the coder ends a block with (anything with a zero low nibble but 0xf0 is an end of block)
        self.out = bytearray()
        self.scans = []         # [(component indices, restart interval)] of the scans written, in order
        self.marker(0xD8)

    # -- bytes
    def raw(self, b):
        self.out += bytes(b)
        return self

    def marker(self, m):
        self.out += b"\xff" * self.fill + bytes([0xFF, m])
        return self

    def seg(self, m, payload=b"", length=None):
        """a marker segment; length: the length field, where it is not to say what the payload is"""
        self.marker(m)
        n = len(payload) + 2 if length is None else length
        self.out += bytes([n >> 8, n & 255]) + bytes(payload)
        return self

    # -- tables and headers
    @staticmethod
    def dqt_payload(tables):
        out = bytearray()
        for pq, tq, vals in tables:
            out.append((pq << 4) | tq)
            for v in vals:
                out += bytes([v >> 8, v & 255]) if pq else bytes([v])
        return bytes(out)

    def dqt(self, tables):
        """tables: [(Pq, Tq, 64 values in zigzag order)], all in ONE segment"""
        return self.seg(0xDB, self.dqt_payload(tables))

    @staticmethod
    def dht_payload(tables):
        out = bytearray()
        for t in tables:
            out.append((t[0] << 4) | t[1])
            out += bytes(t[2]) + bytes(t[3])
        return bytes(out)

    def dht(self, tables):
        """tables: [(class, id, bits[16], vals[, pick])], all in ONE segment; they are current from here on"""
        for t in tables:
            self.huff[(t[0], t[1])] = (tuple(t[2]), tuple(t[3]), t[4] if len(t) > 4 else "first")
        return self.seg(0xC4, self.dht_payload(tables))

    def dri(self, n, length=4):
        self.restart = n
        return self.seg(0xDD, bytes([n >> 8, n & 255]), length)

    def sof_payload(self, precision=8, w=None, h=None, comps=None, ncomp=None):
        comps = self.comps if comps is None else comps
        w, h = self.w if w is None else w, self.h if h is None else h
        out = bytes([precision, h >> 8, h & 255, w >> 8, w & 255, len(comps) if ncomp is None else ncomp])
        for cid, a, v, tq in comps:
            out += bytes([cid, (a << 4) | v, tq])
        return out

    def sof(self, marker=0xC0, length=None, **kw):
        return self.seg(marker, self.sof_payload(**kw), length)

    def sos_payload(self, sel, ss=0, se=63, ahal=0, ns=None, ids=None):
        out = bytes([len(sel) if ns is None else ns])
        for k, (ci, td, ta) in enumerate(sel):
            out += bytes([self.comps[ci][0] if ids is None else ids[k], (td << 4) | ta])
        return out + bytes([ss, se, ahal])

    # -- entropy data
    def _units(self, cis):
        """the blocks of a scan as [[(component index, block row, block column), ...] per MCU]"""
        if len(cis) == 1:
            ci = cis[0]
            _, a, v, _ = self.comps[ci]
            cw = ((self.w * a + self.hmax - 1) // self.hmax + 7) // 8
            ch = ((self.h * v + self.vmax - 1) // self.vmax + 7) // 8
            return [[(ci, j, i)] for j in range(ch) for i in range(cw)]
        out = []
        for my in range(self.mcu_y):
            for mx in range(self.mcu_x):
                mcu = []
                for ci in cis:
                    _, a, v, _ = self.comps[ci]
                    mcu += [(ci, my * v + y, mx * a + x) for y in range(v) for x in range(a)]
                out.append(mcu)
        return out

    def _tokens(self, cis):
        """-> [[(class, component index, symbol, extra value, extra bits), ...] per restart interval]"""
        intervals, cur, pred = [], [], {}
        for m, mcu in enumerate(self._units(cis)):
            if self.restart and m and m % self.restart == 0:
                intervals.append(cur)
                cur, pred = [], {}
            for ci, by, bx in mcu:
                blk = self.planes[ci][by, bx].astype(np.int64)
                diff = int(blk[0]) - pred.get(ci, 0)
                pred[ci] = int(blk[0])
                n = _size(diff)
                cur.append((0, ci, n, diff if diff >= 0 else diff - 1, n))
                last = 0
                for k in np.flatnonzero(blk[1:]) + 1:  # the non-zero coefficients: a block of zeros costs one call
                    k, v = int(k), int(blk[k])
                    r = k - last - 1
                    last = k
                    while r > 15:
                        cur.append((1, ci, 0xF0, 0, 0))
                        r -= 16
                    n = _size(v)
                    cur.append((1, ci, (r << 4) | n, v if v >= 0 else v - 1, n))
                if last < 63:
                    cur.append((1, ci, self.eob, 0, 0))
        intervals.append(cur)
        return intervals

    def symbols(self, cis):
        """-> ({component index: Counter of its DC symbols}, {...: of its AC symbols}) of a scan over these components, with the restart
        interval and end-of-block symbol current now: what the scan's tables have to hold"""
        dc, ac = collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter)
        for iv in self._tokens(cis):
            for cls, ci, sym, _, _ in iv:
                (ac if cls else dc)[ci][sym] += 1
        return dc, ac

    def entropy(self, sel):
        """the entropy-coded data of a scan (sel: [(component index, Td, Ta)]): stuffed, every interval padded with one bits, RSTn between"""
        enc = {}
        for ci, td, ta in sel:
            enc[(0, ci)] = canonical(*self.huff[(0, td)])
            enc[(1, ci)] = canonical(*self.huff[(1, ta)])
        out = bytearray()
        for j, iv in enumerate(self._tokens([s[0] for s in sel])):
            if j:
                out += bytes([0xFF, 0xD0 + (j - 1) % 8])
            acc, n, done = 0, 0, bytearray()
            for cls, ci, sym, extra, nx in iv:
                code, ln = enc[(cls, ci)][sym]
                acc = (acc << (ln + nx)) | (code << nx) | (extra & ((1 << nx) - 1))
                n += ln + nx
                if n >= 2048:  # whole bytes leave the accumulator, so that it stays short
                    keep = n & 7
                    done += (acc >> keep).to_bytes((n - keep) // 8, "big")
                    acc, n = acc & ((1 << keep) - 1), keep
            pad = -n % 8
            acc = (acc << pad) | ((1 << pad) - 1)
            done += acc.to_bytes((n + pad) // 8, "big")
            out += bytes(done).replace(b"\xff", b"\xff\x00")
        return bytes(out)

    def scan(self, sel, data=None, length=None, **kw):
        """SOS + entropy data.  sel: [(component index, Td, Ta)] in the order the scan names them; data: bytes to put in place of the coded data"""
        self.seg(0xDA, self.sos_payload(sel, **kw), length)
        self.scans.append(([s[0] for s in sel], self.restart))
        self.out += self.entropy(sel) if data is None else data
        return self

    def eoi(self):
        return self.marker(0xD9)

    def bytes(self):
        return bytes(self.out)


# ---------------------------------------------------------------------------------------------- a stream the ordinary way

def std_tables(wr, groups):
    """Optimal tables (Annex K.2) for the scan structure `groups` = [[(component index, Td, Ta), ...] per scan], one table per id over
    all the scans that use the id: -> [(class, id, bits, vals)] sorted DC first"""
    freq = collections.defaultdict(lambda: [0] * 257)
    for sel in groups:
        dc, ac = wr.symbols([s[0] for s in sel])
        for ci, td, ta in sel:
            for s, n in dc[ci].items():
                freq[(0, td)][s] += n
            for s, n in ac[ci].items():
                freq[(1, ta)][s] += n
    return [(k[0], k[1]) + optimal_table(freq[k]) for k in sorted(freq)]


def default_sel(ncomp):
    return [(0, 0, 0)] + [(c, 1, 1) for c in range(1, ncomp)]


def default_comps(hv, ids=None, tq=None):
    return [((ids[c] if ids else c + 1), a, v, (tq[c] if tq else (0 if c == 0 else 1))) for c, (a, v) in enumerate(hv)]


APP14 = lambda transform: b"Adobe" + bytes([0, 100, 0, 0, 0, 0, transform])


def plain(w, h, hv, planes=None, restart=0, app14=-1, ids=None, tq=None, qt=None, seed=0, fill=0, pre=None, mid=None, post=None, sof=0xC0,
          tables=None, sel=None, tail=b""):
    """The arrangement of the test-side writer (pw_write_baseline_ex): [APP14] DQT per table, SOF, DHT per table, [DRI], one interleaved
    scan, EOI.  pre / mid / post: called with the writer behind SOI / behind SOF / in front of SOS.  qt {Tq: 64 values}."""
    comps = default_comps(hv, ids, tq)
    wr = Writer(w, h, comps, tame(w, h, hv, seed) if planes is None else planes, fill)
    if pre:
        pre(wr)
    if app14 >= 0:
        wr.seg(0xEE, APP14(app14))
    for t in sorted({c[3] for c in comps}):
        wr.dqt([(0, t, (qt or {}).get(t, ONES64))])
    wr.sof(sof)
    if mid:
        mid(wr)
    sel = sel or default_sel(len(hv))
    wr.restart = restart  # the coder has to know it before the tables are made
    for t in (tables or std_tables(wr, [sel])):
        wr.dht([t])
    if restart:
        wr.dri(restart)
    if post:
        post(wr)
    wr.scan(sel).eoi().raw(tail)
    return wr


def parse_arrangement(data):
    """What a pw_write_baseline_ex stream says about itself: -> dict(w, h, comps, qt {Tq: values}, tables [(class, id, bits, vals)],
    restart, app14, sel) -- enough for plain() to write it again"""
    out = {"qt": {}, "tables": [], "restart": 0, "app14": -1}
    i = 2
    while True:
        assert data[i] == 0xFF
        m, n = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        p = data[i + 4:i + 2 + n]
        if m == 0xEE:
            out["app14"] = p[11]
        elif m == 0xDB:
            out["qt"][p[0] & 15] = tuple(p[1:65])
        elif m == 0xC0:
            out["h"], out["w"] = (p[1] << 8) | p[2], (p[3] << 8) | p[4]
            out["comps"] = [(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]) for c in range(p[5])]
        elif m == 0xC4:
            cnt = sum(p[1:17])
            out["tables"].append((p[0] >> 4, p[0] & 15, tuple(p[1:17]), tuple(p[17:17 + cnt])))
        elif m == 0xDD:
            out["restart"] = (p[0] << 8) | p[1]
        elif m == 0xDA:
            ids = [c[0] for c in out["comps"]]
            out["sel"] = [(ids.index(p[1 + 2 * k]), p[2 + 2 * k] >> 4, p[2 + 2 * k] & 15) for k in range(p[0])]
            return out
        i += 2 + n


def rewrite(data, planes):
    """the stream plain() writes from the arrangement parsed out of `data` and the planes it was made from"""
    a = parse_arrangement(data)
    hv = [(c[1], c[2]) for c in a["comps"]]
    return plain(a["w"], a["h"], hv, planes, a["restart"], a["app14"], [c[0] for c in a["comps"]], [c[3] for c in a["comps"]], a["qt"],
                 tables=a["tables"], sel=a["sel"]).bytes()


# ---------------------------------------------------------------------------------------------- the families

def _case(name, family, kind, data, **meta):
    return Case(name, family, kind, KIND_STATUS[kind], bytes(data), meta)


HV420 = [(2, 2), (1, 1), (1, 1)]
HV444 = [(1, 1)] * 3
HVGREY = [(1, 1)]
LAYOUT_HV = {"420": HV420, "444": HV444, "grey": HVGREY}

# every failure reason of the marker parser and the frame and scan headers (None: the three failures that set none)
REASONS = ("expected marker", "unknown marker", "no SOF", "bad DRI len", "bad DQT type", "bad DQT table", "bad DHT header", "bad code lengths",
           "bad COM len", "bad APP len", "bad SOS component count", "bad SOS len", "bad DC huff", "bad AC huff", "bad SOS", "bad SOF len",
           "only 8-bit", "no header height", "0 width", "bad component count", "bad H", "bad V", "bad TQ", "too large", "bad DNL len",
           "bad DNL height", "can't merge dc and ac", "bad huffman code")


def _edited_scan(hv, **kw):
    """a good stream whose scan header is edited through sos_payload's arguments"""
    w, h = 24, 16
    comps = default_comps(hv)
    wr = Writer(w, h, comps, tame(w, h, hv))
    wr.dqt([(0, 0, ONES64)]).dqt([(0, 1, ONES64)]).sof()
    sel = default_sel(len(hv))
    for t in std_tables(wr, [sel]):
        wr.dht([t])
    length = kw.pop("length", None)
    return wr.scan(sel, length=length, **kw).eoi().bytes()


def reasons():
    """one minimal edit of a good stream per failure reason (and per site where a reason has several)"""
    F = "reasons"
    w, h = 24, 16
    out = []

    def header(name, pre=None, mid=None, post=None, kind=None, **kw):
        wr = plain(w, h, HV420, pre=pre, mid=mid, post=post, **kw)
        out.append(_case(name, F, kind or ("reject header" if pre else "reject late"), wr.bytes()))

    header("expected marker: padding behind SOF", mid=lambda wr: wr.raw(b"\x00\x00"), kind="no marker at sos")
    header("unknown marker: SOF3 in front of SOF", pre=lambda wr: wr.seg(0xC3, b"\x00" * 4))
    header("unknown marker: TEM behind SOF", mid=lambda wr: wr.seg(0x01, b"\x00" * 4))
    out.append(_case("no SOF: the file ends behind DQT", F, "reject header", Writer(w, h, default_comps(HV420), tame(w, h, HV420)).dqt([(0, 0, ONES64)]).bytes()))
    header("bad DRI len: 5", pre=lambda wr: wr.seg(0xDD, b"\x00\x04\x00"))
    header("bad DRI len: 2 behind SOF", mid=lambda wr: wr.seg(0xDD, b""))
    header("bad DQT type: Pq 2", pre=lambda wr: wr.dqt([(2, 0, ONES64)]))
    header("bad DQT table: Tq 4", pre=lambda wr: wr.seg(0xDB, bytes([0x04]) + bytes(ONES64)))
    header("bad DQT table behind SOF: Tq 15", mid=lambda wr: wr.seg(0xDB, bytes([0x0F]) + bytes(ONES64)))
    good = (tuple([0, 2] + [0] * 14), (0, 1))
    header("bad DHT header: class 2", pre=lambda wr: wr.seg(0xC4, Writer.dht_payload([(2, 0) + good])))
    header("bad DHT header: id 4", mid=lambda wr: wr.seg(0xC4, Writer.dht_payload([(1, 4) + good])))
    header("bad code lengths: three codes of one bit", pre=lambda wr: wr.seg(0xC4, Writer.dht_payload([(0, 0, tuple([3] + [0] * 15), (0, 1, 2))])))
    header("bad code lengths: 255 codes of seven bits", mid=lambda wr: wr.seg(0xC4, Writer.dht_payload([(1, 0, tuple([0] * 6 + [255] + [0] * 9), tuple(range(255)))])))
    header("bad COM len: 1", pre=lambda wr: wr.seg(0xFE, b"", length=1))
    header("bad COM len: 0 behind SOF", mid=lambda wr: wr.seg(0xFE, b"", length=0))
    header("bad APP len: APP3 1", pre=lambda wr: wr.seg(0xE3, b"", length=1))
    header("bad APP len: APP0 0 behind SOF", mid=lambda wr: wr.seg(0xE0, b"", length=0))
    out.append(_case("bad SOS component count: 0", F, "reject late", _edited_scan(HV420, ns=0, length=12)))
    out.append(_case("bad SOS component count: 5", F, "reject late", _edited_scan(HV420, ns=5, length=12)))
    out.append(_case("bad SOS component count: 3 of 1", F, "reject late", _edited_scan(HVGREY, ns=3)))
    out.append(_case("bad SOS len: 13", F, "reject late", _edited_scan(HV420, length=13)))
    good_scan = _edited_scan(HV420)
    at = good_scan.rindex(b"\xff\xda") + 5  # the first component's selector pair
    assert good_scan[at:at + 6] == b"\x01\x00\x02\x11\x03\x11"
    out.append(_case("bad DC huff: Td 4", F, "reject late", good_scan[:at + 1] + b"\x40" + good_scan[at + 2:]))
    out.append(_case("bad AC huff: Ta 4", F, "reject late", good_scan[:at + 3] + b"\x14" + good_scan[at + 4:]))
    out.append(_case("bad DC huff: Td 15 in the last component", F, "reject late", good_scan[:at + 5] + b"\xf1" + good_scan[at + 6:]))
    out.append(_case("bad SOS: Ss 1", F, "reject late", _edited_scan(HV420, ss=1)))
    out.append(_case("bad SOS: Ah 1", F, "reject late", _edited_scan(HV420, ahal=0x10)))
    out.append(_case("bad SOS: Al 1", F, "reject late", _edited_scan(HV420, ahal=0x01)))
    out.append(_case("no reason: SOS names a component the frame has not", F, "reject late", _edited_scan(HV420, ids=[1, 2, 9])))
    # progressive frames: the scan header's own test, and a DC scan with Se != 0
    for name, kw in (("bad SOS: progressive, Ss 64", dict(ss=64, se=64)), ("bad SOS: progressive, Ss > Se", dict(ss=5, se=3)),
                     ("bad SOS: progressive, Al 14", dict(ss=0, se=0, ahal=0x0E)), ("can't merge dc and ac: progressive, Ss 0 Se 63", dict(ss=0, se=63)),
                     ("can't merge dc and ac: progressive, Ss 0 Se 5", dict(ss=0, se=5))):
        wr = Writer(w, h, default_comps(HV420), tame(w, h, HV420))
        wr.dqt([(0, 0, ONES64)]).dqt([(0, 1, ONES64)]).sof(0xC2)
        sel = default_sel(3)
        for t in std_tables(wr, [sel]):
            wr.dht([t])
        out.append(_case(name, F, "progressive", wr.scan(sel, **kw).eoi().bytes()))

    def frame(name, **kw):
        wr = Writer(w, h, default_comps(HV420), tame(w, h, HV420))
        wr.dqt([(0, 0, ONES64)]).dqt([(0, 1, ONES64)]).sof(**kw)
        sel = default_sel(3)
        for t in std_tables(wr, [sel]):
            wr.dht([t])
        out.append(_case(name, F, "reject header", wr.scan(sel).eoi().bytes()))

    frame("bad SOF len: 10", length=10)
    frame("bad SOF len: 18 for three components", length=18)
    frame("bad SOF len: component count 4 under length 17", ncomp=4)
    frame("only 8-bit: precision 12", precision=12)
    frame("no header height", h=0)
    frame("0 width", w=0)
    frame("bad component count: 2", comps=default_comps(HV420)[:2])
    frame("bad H: 0", comps=[(1, 0, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)])
    frame("bad H: 5", comps=[(1, 2, 2, 0), (2, 5, 1, 1), (3, 1, 1, 1)])
    frame("bad V: 0", comps=[(1, 2, 0, 0), (2, 1, 1, 1), (3, 1, 1, 1)])
    frame("bad V: 5", comps=[(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 5, 1)])
    frame("bad TQ: 4", comps=[(1, 2, 2, 4), (2, 1, 1, 1), (3, 1, 1, 1)])
    frame("too large: 65535 x 65535 x 3", w=65535, h=65535)
    for name, length, nl in (("bad DNL len: 5", 5, h), ("bad DNL height", 4, h + 1)):
        wr = plain(w, h, HV420)
        data = wr.bytes()[:-2] + b"\xff\xdc" + bytes([0, length, nl >> 8, nl & 255]) + EOI
        out.append(_case(name, F, "not one scan then EOI", data))
    wr = plain(w, h, HV420)
    ent = helpers.entropy_ranges(wr.bytes())[0]
    out.append(_case("bad huffman code: all ones", F, "bad entropy", wr.bytes()[:ent[0]] + b"\xff\x00" * 12 + EOI))
    # the failures that set no reason: a DQT / DHT segment whose length is not used up
    header("no reason: DQT length one short", pre=lambda wr: wr.seg(0xDB, bytes([0x02]) + bytes(ONES64), length=66))
    header("no reason: DHT length one short", mid=lambda wr: wr.seg(0xC4, Writer.dht_payload([(0, 3) + good]), length=2 + 17 + 1))
    return out


def segments():
    """legal arrangements of the segments (and two the reference rejects where it does not skip: padding behind SOF is among `reasons`)"""
    F = "segments"
    out = []
    w, h = SIZE
    q_a = tuple(1 + (k % 3) for k in range(64))
    q_b = tuple(2 + (k % 5) for k in range(64))
    q_big = tuple(1 + (k * 5) % 300 for k in range(64))

    def build(name, body, hv=HV420, kind="plain", restart=0, fill=0, tq=None, sof=0xC0, tail=b""):
        """body(wr, tables) emits everything between SOI and SOS"""
        comps = default_comps(hv, tq=tq)
        wr = Writer(w, h, comps, tame(w, h, hv, len(name)), fill)
        sel = default_sel(len(hv))
        wr.restart = restart
        tables = std_tables(wr, [sel])
        wr.restart = 0
        body(wr, tables)
        assert wr.restart == restart, name
        out.append(_case(name, F, kind, wr.scan(sel).eoi().raw(tail).bytes(), hv=hv))
        return wr

    def usual(wr, tables, dqt=True, sof=0xC0, dht=True):
        if dqt:
            wr.dqt([(0, 0, q_a)]).dqt([(0, 1, q_b)])
        wr.sof(sof)
        if dht:
            for t in tables:
                wr.dht([t])

    build("all DQT in one segment", lambda wr, t: (wr.dqt([(0, 0, q_a), (0, 1, q_b)]), usual(wr, t, dqt=False)))
    build("8-bit and 16-bit DQT mixed in one segment", lambda wr, t: (wr.dqt([(1, 0, q_big), (0, 1, q_b), (1, 3, q_big), (0, 2, q_a)]), usual(wr, t, dqt=False)))
    build("a DQT defined twice: the later one holds", lambda wr, t: (wr.dqt([(0, 0, q_b), (0, 1, q_a)]), wr.dqt([(1, 0, q_big)]), usual(wr, t)))
    build("a DQT defined twice in one segment", lambda wr, t: (wr.dqt([(0, 0, q_b), (0, 1, q_b), (0, 0, q_a)]), usual(wr, t, dqt=False)))
    build("a DQT no component uses", lambda wr, t: (wr.dqt([(1, 3, q_big)]), usual(wr, t), wr.dqt([(0, 2, q_b)])))
    build("DQT behind SOF", lambda wr, t: (wr.sof(), wr.dqt([(0, 0, q_a), (0, 1, q_b)]), [wr.dht([x]) for x in t]))
    build("DQT redefined behind SOF", lambda wr, t: (usual(wr, t), wr.dqt([(0, 1, q_a)]), wr.dqt([(1, 0, q_big)])))
    build("all DHT in one segment", lambda wr, t: (usual(wr, t, dht=False), wr.dht(t)))
    build("DHT in two segments: DC, AC", lambda wr, t: (usual(wr, t, dht=False), wr.dht(t[:2]), wr.dht(t[2:])))
    build("all DHT in front of SOF", lambda wr, t: (wr.dht(t), usual(wr, t, dht=False)))
    comb = lambda cls, th: (cls, th) + shape_table(range(16) if cls == 0 else [0x00, 0xF0] + [r << 4 | s for r in range(3) for s in range(1, 5)], [1] * 16)
    build("a DHT defined twice with different shapes", lambda wr, t: (usual(wr, t, dht=False), wr.dht([comb(0, 0), comb(1, 0), comb(0, 1), comb(1, 1)]), wr.dht(t)))
    build("a DHT defined twice in one segment", lambda wr, t: (usual(wr, t, dht=False), wr.dht([comb(0, 0), comb(1, 1)] + list(t))))
    build("a DHT nobody uses", lambda wr, t: (usual(wr, t), wr.dht([comb(0, 3), comb(1, 2)])))
    mcu_row = (w + 15) // 16
    build("DRI in front of SOF", lambda wr, t: (wr.dri(mcu_row), usual(wr, t)), restart=mcu_row)
    build("DRI behind SOF", lambda wr, t: (wr.dqt([(0, 0, q_a)]).dqt([(0, 1, q_b)]).sof().dri(3), [wr.dht([x]) for x in t]), restart=3)
    build("DRI given twice", lambda wr, t: (wr.dri(2), usual(wr, t), wr.dri(5)), restart=5)
    build("DRI set back to 0", lambda wr, t: (wr.dri(7), usual(wr, t), wr.dri(0)))
    build("DRI of 65535", lambda wr, t: (usual(wr, t), wr.dri(65535)), restart=65535)
    for m, nm in ((0xE0, "APP0"), (0xE1, "APP1"), (0xEF, "APP15"), (0xFE, "COM")):
        build("%s of length 2" % nm, lambda wr, t, m=m: (wr.seg(m, b""), usual(wr, t)))
    build("APP2 of length 65535", lambda wr, t: (wr.seg(0xE2, bytes(range(256)) * 255 + bytes(253)), usual(wr, t)))
    build("COM of length 65535 behind SOF", lambda wr, t: (usual(wr, t), wr.seg(0xFE, b"\xff\xd9\xff\xda" * 16383 + b"\xff")))
    build("APP0 that is not JFIF", lambda wr, t: (wr.seg(0xE0, b"JFXX\x00\x10" + bytes(8)), usual(wr, t)))
    build("APP0 JFIF", lambda wr, t: (wr.seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"), usual(wr, t)))
    build("APP0 shorter than five bytes", lambda wr, t: (wr.seg(0xE0, b"JFIF"), usual(wr, t)))
    build("APP14 shorter than twelve bytes", lambda wr, t: (wr.seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00"), usual(wr, t)), hv=HV444)
    build("APP14 with another tag", lambda wr, t: (wr.seg(0xEE, b"Adobf" + APP14(0)[5:]), usual(wr, t)), hv=HV444)
    build("APP14 transform 0 behind SOF", lambda wr, t: (usual(wr, t), wr.seg(0xEE, APP14(0))), hv=HV444)
    build("JFIF and APP14 transform 0", lambda wr, t: (wr.seg(0xE0, b"JFIF\x00" + bytes(9)), wr.seg(0xEE, APP14(0)), usual(wr, t)), hv=HV444)
    for n in (1, 7):
        build("%d fill bytes in front of every marker" % n, lambda wr, t: usual(wr, t), fill=n, kind="not one scan then EOI")
    build("fill bytes in front of the header markers only", lambda wr, t: (setattr(wr, "fill", 3), usual(wr, t), wr.raw(b"\xff" * 3), setattr(wr, "fill", 0)))
    build("padding in front of SOF", lambda wr, t: (wr.dqt([(0, 0, q_a)]).dqt([(0, 1, q_b)]), wr.raw(b"\x00\x12\x34" * 5), wr.sof(), [wr.dht([x]) for x in t]))
    build("SOF1", lambda wr, t: usual(wr, t, sof=0xC1))
    build("SOF1 with 16-bit DQT and a restart interval", lambda wr, t: (wr.dqt([(1, 0, q_big), (1, 1, q_big)]), usual(wr, t, dqt=False, sof=0xC1), wr.dri(4)), restart=4)
    build("bytes behind EOI", lambda wr, t: usual(wr, t), tail=b"\x00\x11\xff\xda\x00\x08tail")
    second = plain(16, 8, HVGREY).bytes()
    build("a second picture behind EOI", lambda wr, t: usual(wr, t), tail=second)
    wr = plain(w, h, HV420, qt={0: q_a, 1: q_b})
    out.append(_case("DNL with the right height", F, "not one scan then EOI", wr.bytes()[:-2] + b"\xff\xdc\x00\x04" + bytes([h >> 8, h & 255]) + EOI, hv=HV420))
    out.append(_case("DNL in front of SOS", F, "not one scan then EOI", plain(w, h, HV420, post=lambda wr: wr.seg(0xDC, bytes([h >> 8, h & 255]))).bytes(), hv=HV420))
    out.append(_case("a second SOI behind the first", F, "reject header", plain(w, h, HV420, pre=lambda wr: wr.marker(0xD8)).bytes(), hv=HV420))
    out.append(_case("grey: everything in one DQT and one DHT, DRI 1", F, "plain",
                     _grey_packed(w, h), hv=HVGREY))
    return out


def _grey_packed(w, h):
    wr = Writer(w, h, [(7, 1, 1, 2)], tame(w, h, HVGREY, 3))
    wr.restart = 1
    t = std_tables(wr, [[(0, 3, 2)]])
    wr.dqt([(0, 2, tuple(1 + k % 2 for k in range(64)))]).dri(1).sof().dht(t)
    return wr.scan([(0, 3, 2)]).eoi().bytes()


def frame_sizes(hv):
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    return [(1, 1), (8 * hmax + 1, 8 * vmax + 1), SIZE]


def expected_path(hv, ids, app14, n_out):
    """The kernel family classify() gives a layout (its comment: fused 4:2:0, grey, 4:2:2, 4:4:0, 4:4:4, 1x1 colour, else the two-pass
    path), for 3 or 4 output channels (and 1 for a lone component): coef_cases.PATH_OF's numbers"""
    if len(hv) == 1:
        return 5
    if n_out < 3:
        return 5 if len(hv) == 3 and hv[0] == (max(a for a, _ in hv), max(b for _, b in hv)) else 2
    one = all(x == (1, 1) for x in hv)
    rgb = len(hv) == 3 and (tuple(ids) == (82, 71, 66) or app14 == 0)
    if len(hv) == 4:
        return (7 if app14 in (0, 2) else 3) if one else 2
    if rgb:
        return 7 if one else 2
    if hv[1] == (1, 1) and hv[2] == (1, 1):
        return {(2, 2): 1, (2, 1): 4, (1, 2): 6, (1, 1): 3}.get(hv[0], 2)
    return 2


def _frame_kind(hv):
    if len(hv) == 4:
        return "four components"
    if len(hv) == 1 and hv[0] != (1, 1):
        return "lone sampled"
    return "over ten blocks" if sum(a * v for a, v in hv) > 10 else "plain"


# layouts the specialised kernels do not serve: also run with force_generic 1 and 2
GENERIC = ([(3, 1), (1, 1), (1, 1)], [(3, 3), (1, 1), (1, 1)], [(3, 1), (2, 1), (1, 1)], [(4, 4), (3, 3), (1, 1)], [(2, 1), (1, 2), (1, 1)],
           [(1, 1), (2, 2), (2, 2)], [(2, 2)], [(4, 3)])


def frames():
    F = "frames"
    out = []

    def add(name, hv, sizes=None, ids=None, tq=None, qt=None, app14=-1):
        for (w, h) in (sizes or frame_sizes(hv)):
            wr = plain(w, h, hv, ids=ids, tq=tq, qt=qt, app14=app14, seed=len(name))
            out.append(_case("%s %dx%d" % (name, w, h), F, _frame_kind(hv), wr.bytes(), hv=hv, ids=ids or list(range(1, len(hv) + 1)), app14=app14,
                             generic=any(hv == g for g in GENERIC)))

    # component ids and Tq are no layouts: they change which names the scan header and the table lookup use, not the block grid, so they
    # are built at the family size only; every (h, v) layout below comes at 1 x 1, one MCU plus one pixel and the family size (frame_sizes)
    for ids in ((0, 1, 2), (255, 254, 253), (82, 71, 66), (82, 71, 88), (3, 1, 2)):
        add("ids %s 4:4:4" % (ids,), HV444, [SIZE], ids=ids)
        add("ids %s 4:2:0" % (ids,), HV420, [SIZE], ids=ids)
    qts = {t: tuple(1 + (k + 2 * t) % (3 + t) for k in range(64)) for t in range(4)}
    for tq in ((3, 2, 0), (1, 1, 1), (2, 3, 3), (0, 1, 2)):
        add("Tq %s" % (tq,), HV420, [SIZE], tq=tq, qt=qts)
    add("Tq 3 grey", HVGREY, [SIZE], tq=(3,), qt=qts)
    for a in range(1, 5):
        for v in range(1, 5):
            add("luma %dx%d chroma 1x1" % (a, v), [(a, v), (1, 1), (1, 1)])
    add("factors (3,1)/(2,1)/(1,1)", [(3, 1), (2, 1), (1, 1)])
    add("factors (4,4)/(3,3)/(1,1)", [(4, 4), (3, 3), (1, 1)])
    add("maxima from two components (2,1)/(1,2)/(1,1)", [(2, 1), (1, 2), (1, 1)])
    add("chroma above luma (1,1)/(2,2)/(2,2)", [(1, 1), (2, 2), (2, 2)])
    add("lone component 2x2", [(2, 2)])
    add("lone component 4x3", [(4, 3)])
    for app14 in (-1, 0, 2):
        add("four components (2,2)/(1,1)/(1,1)/(2,2) app14 %d" % app14, [(2, 2), (1, 1), (1, 1), (2, 2)], app14=app14)
        add("four components (1,1)/(1,1)/(1,1)/(3,1) app14 %d" % app14, [(1, 1), (1, 1), (1, 1), (3, 1)], app14=app14)
        add("four components 1x1 app14 %d" % app14, [(1, 1)] * 4, app14=app14)
    add("RGB-tagged by APP14 4:2:0", HV420, [SIZE], app14=0)
    return out


def _multi_scan(w, h, hv, groups, restart=0, redefine=None, seed=0, qt=None, between=None):
    """a baseline stream with the scans `groups` ([[component index, ...], ...]); table ids as in default_sel.  redefine: the DHT tables are
    given in front of every scan, made for that scan alone (another shape under the same id); otherwise once, for all scans.
    between(wr, k): called in front of scan k's tables."""
    comps = default_comps(hv)
    wr = Writer(w, h, comps, tame(w, h, hv, seed))
    for t in sorted({c[3] for c in comps}):
        wr.dqt([(0, t, (qt or {}).get(t, ONES64))])
    wr.sof()
    base = default_sel(len(hv))
    sels = [[base[ci] for ci in g] for g in groups]
    if restart:
        wr.dri(restart)
    if not redefine:
        for t in std_tables(wr, sels):
            wr.dht([t])
    for k, sel in enumerate(sels):
        if between:
            between(wr, k)
        if redefine:
            wr.dht(std_tables(wr, [sel]))
        wr.scan(sel)
    return wr.eoi()


def scans():
    F = "scans"
    out = []
    w, h = SIZE
    for lay, hv in (("420", HV420), ("444", HV444), ("(2,1)/(1,2)/(1,1)", [(2, 1), (1, 2), (1, 1)])):
        mcu_row = geometry(w, h, hv)[0]
        for restart in (0, mcu_row, 3):
            tag = "%s%s" % (lay, " DRI %d" % restart if restart else "")
            for name, groups, kind in (("one scan, frame order", [[0, 1, 2]], "plain"), ("one scan, order 2 0 1", [[2, 0, 1]], "permuted scan"),
                                       ("one scan, order 0 2 1", [[0, 2, 1]], "permuted scan"),
                                       ("one scan per component", [[0], [1], [2]], "several scans"), ("one scan per component, order 2 0 1", [[2], [0], [1]], "several scans"),
                                       ("Y then CbCr", [[0], [1, 2]], "several scans"), ("CrCb then Y", [[2, 1], [0]], "several scans")):
                out.append(_case("%s: %s" % (tag, name), F, kind, _multi_scan(w, h, hv, groups, restart, seed=len(name)).bytes(), hv=hv, groups=groups))
        out.append(_case("%s: Huffman tables redefined between scans" % lay, F, "several scans", _multi_scan(w, h, hv, [[0], [1], [2]], redefine=True).bytes(), hv=hv,
                         groups=[[0], [1], [2]]))
        out.append(_case("%s: Huffman tables redefined between scans, Y then CbCr, DRI" % lay, F, "several scans",
                         _multi_scan(w, h, hv, [[0], [1, 2]], 5, redefine=True).bytes(), hv=hv, groups=[[0], [1, 2]]))
        q1 = tuple(1 + k % 4 for k in range(64))
        q2 = tuple(3 - k % 3 for k in range(64))
        out.append(_case("%s: quantisation table redefined between scans" % lay, F, "several scans",
                         _multi_scan(w, h, hv, [[0], [1], [2]], qt={0: q1, 1: q1}, between=lambda wr, k: k == 2 and wr.dqt([(0, 1, q2)])).bytes(), hv=hv, groups=[[0], [1], [2]]))
        out.append(_case("%s: quantisation table redefined behind the last scan" % lay, F, "not one scan then EOI",
                         plain(w, h, hv, qt={0: q1, 1: q1}).bytes()[:-2] + b"\xff\xdb\x00\x43\x00" + bytes(q2) + EOI, hv=hv, groups=[[0, 1, 2]]))
    out.append(_case("grey: the scan again, a second time", F, "several scans", _multi_scan(w, h, HVGREY, [[0], [0]]).bytes(), hv=HVGREY, groups=[[0], [0]]))
    out.append(_case("lone component 2x2 with DRI 4", F, "lone sampled", _multi_scan(w, h, [(2, 2)], [[0]], 4).bytes(), hv=[(2, 2)], groups=[[0]]))
    out.append(progressive_requantised())
    return out


def progressive_requantised():
    """the progressive twin of the quantisation redefinition: a pw_write_progressive stream with a DQT for table 1 in front of its
    LAST scan -- the reference de-quantises a progressive file when all scans are in, with the last definition (stbi__jpeg_finish)"""
    w, h = 72, 40
    q = np.array([1 + k % 4 for k in range(64)] * 2, np.int64)
    data = cc.Case("prog", "prog", "420", w, h, cc._tame(cc.blank("420", w, h)), qt=q, progressive=1).stream()
    at = data.rindex(b"\xff\xda")
    # (the writer gives every scan its tables in front of it: the DQT goes in front of the last scan's DHT)
    at = data.rindex(b"\xff\xc4", 0, at)
    seg = b"\xff\xdb\x00\x43\x01" + bytes(3 - k % 3 for k in range(64))
    return _case("progressive: quantisation table redefined in front of the last scan", "scans", "progressive", data[:at] + seg + data[at:], hv=HV420, groups=None)


# ---------------------------------------------------------------------------------------------- Huffman table shapes

def rich(w, h, hv, what, seed=0):
    """tame planes plus what a shape needs the data to hold"""
    planes = tame(w, h, hv, seed)
    for c, p in enumerate(planes):
        bh, bw, _ = p.shape
        i = np.arange(bh * bw).reshape(bh, bw) + 3 * c
        if what == "ones":          # runs of +1: under an all-ones code the data holds 0xff 0xff
            for k in range(1, 7):
                p[:, :, k] = np.where(i % 3 == 0, 1, p[:, :, k] if k in (1, 2, 4) else 0)
        elif what == "big":         # AC sizes 11..15, both signs
            for n in range(11, 16):
                v = (1 << (n - 1)) + (i * 37) % (1 << (n - 1))
                p[:, :, 3 + (n - 11) * 2] = np.where(i % 11 == n - 11, np.where(i & 1, -v, v), 0)
            p[:, :, 63] = np.where(i % 13 == 5, 32767, 0)
        elif what == "dc":          # DC differences of every category 0..11
            steps = np.array([0, 1, -3, 6, -12, 25, -50, 100, -200, 400, -800, 1600, -2047, 2047, -1024, 0], np.int64)
            p[:, :, 0] = np.cumsum(steps[(np.arange(bh * bw) * 5 + c) % 16] * np.where(np.arange(bh * bw) % 32 < 16, 1, -1)).reshape(bh, bw) % 2048 - 1024
        elif what == "dc0":         # DC category 0 only
            p[:, :, 0] = 0
        elif what == "noac":        # end of block only
            p[:, :, 1:] = 0
        elif what == "zrl":         # long runs of zeros: ZRL, and a coefficient at position 63
            p[:, :, 40] = np.where(i % 4 == 0, 2, 0)
            p[:, :, 63] = np.where(i % 6 == 1, -1, 0)
    return planes


def _spread(n, lengths):
    """a profile with room for n symbols, spread evenly over `lengths`"""
    p = [0] * 16
    for k in range(n):
        p[lengths[k % len(lengths)] - 1] += 1
    return p


def table_shapes():
    """name -> (what the data must hold, end-of-block symbol, maker(class, symbols Counter) -> (bits, vals[, pick]) or None for the
    optimal table, {event: minimum count} the stream must show)"""
    def by_freq(c):
        return [s for s, _ in sorted(c.items(), key=lambda kv: (-kv[1], kv[0]))]

    def comb(eob_len):
        def make(cls, c, eob):
            syms = by_freq(c)
            assert len(syms) <= 16, len(syms)
            if eob_len == 1:    # the commonest symbol (AC: the end of block) at one bit, the others from sixteen bits downwards
                first = eob if cls and eob in c else syms[0]
                rest = [s for s in syms if s != first]
                place = {s: 16 - k for k, s in enumerate(rest)}
                place[first] = 1
            else:               # the end of block at sixteen bits, the others from one bit upwards
                place = {eob: eob_len} if cls and eob in c else {}
            return shape_table(syms, [1] * 16, place, filler=range(16) if cls == 0 else None)
        return make

    def lengths(ls, dc_ls=None):
        return lambda cls, c, eob: shape_table(by_freq(c), _spread(len(c), ls if cls or dc_ls is None else dc_ls), filler=range(16) if cls == 0 else None)

    def uniform(n):
        return lambda cls, c, eob: None if cls == 0 else shape_table(by_freq(c), profile_of([n] * len(c)))

    def totals(cls, c, eob):
        """the most frequent symbols with extra bits: code + extra bits exactly 12, then exactly 13, in turn; the others at 5 bits"""
        if cls == 0:
            return None
        place, k = {}, 0
        for s in by_freq(c):
            if s & 15 and k < 6:
                place[s] = 12 + (k & 1) - (s & 15)
                k += 1
        rest = [s for s in c if s not in place]
        return shape_table(by_freq(c), profile_of(list(place.values()) + [5] * len(rest)), place)

    def ffff(cls, c, eob):
        """a complete profile: one code per length 1..15 and two of sixteen bits, symbol 0x01 (a coefficient of +-1) on the all-ones code"""
        if cls == 0:
            return None
        syms = by_freq(c)
        assert len(syms) <= 17 and 0x01 in c, (len(syms), sorted(c))
        return shape_table(syms, [1] * 15 + [2], {0x01: 16}, last=(0x01,))

    def sized(short):
        def make(cls, c, eob):
            if cls == 0:
                return None
            big = [s for s in c if (s & 15) >= 11]
            rest = [s for s in by_freq(c) if s not in big]
            if short:
                place = {s: 4 + k // 4 for k, s in enumerate(big)}
                return shape_table(big + rest, profile_of(list(place.values()) + [9] * len(rest)), place)
            place = {s: 14 + k % 3 for k, s in enumerate(big)}
            return shape_table(rest + big, profile_of([6] * len(rest) + list(place.values())), place)
        return make

    def dc_long(cls, c, eob):
        if cls:
            return None
        syms = sorted(c)
        place = {s: (9, 10, 16)[k % 3] for k, s in enumerate(syms)}
        return shape_table(syms, profile_of(list(place.values())), place)

    def full256(cls, c, eob):
        """256 codes: 120 of eight bits, 100 of nine, 36 of ten; every needed symbol twice -- among the first codes of eight bits and
        as the last codes of ten, the 256th entry included -- and coded with its LAST occurrence; the rest unused.  (The 256th entry
        must be longer than nine bits: see full256_short)"""
        if cls == 0:
            return None
        syms = by_freq(c)
        assert len(syms) <= 36
        unused = [s for s in range(256) if s not in c][:256 - 2 * len(syms)]
        vals = syms + unused + syms[::-1]
        assert len(vals) == 256
        return (tuple([0] * 7 + [120, 100, 36] + [0] * 6), tuple(vals), "last")

    return collections.OrderedDict([
        ("comb, end of block at one bit", ("tame", 0, comb(1), {"ac len 1": 1, "ac len 10+": 1, "dc len 10+": 1})),
        ("comb, end of block at sixteen bits", ("tame", 0, comb(16), {"ac len 16": 1, "eob len 16": 1})),
        ("every code 10..16 bits", ("tame", 0, lengths(list(range(10, 17))), {"ac len 10+": 1, "dc len 10+": 1, "ac len 1..9": 0, "dc len 1..9": 0})),
        ("codes of 9 and 10 bits", ("tame", 0, lengths([9, 10]), {"ac len 9": 1, "ac len 10": 1, "dc len 9": 1, "dc len 10": 1})),
        ("codes of 12 and 13 bits", ("tame", 0, lengths([12, 13]), {"ac len 12": 1, "ac len 13": 1})),
        ("first symbol of 12 and of 13 bits with its extra bits", ("tame", 0, totals, {"first total 12": 1, "first total 13": 1})),
        ("second symbol ends at the window's end and one bit behind it", ("tame", 0, uniform(5), {"second ends at 12": 1, "second ends at 13": 1})),
        ("pairs that end in an end of block, blocks of DC alone", ("tame", 0, lambda cls, c, eob: None, {"second is eob": 1, "first ac is eob": 1})),
        ("two codes of sixteen bits, one all ones", ("ones", 0, ffff, {"ff ff in the data": 1, "ac len 16": 1})),
        ("DC table of one symbol", ("dc0", 0, lambda cls, c, eob: shape_table(sorted(c), profile_of([1])) if cls == 0 else None, {"dc len 1": 1})),
        ("AC table of one symbol", ("noac", 0, lambda cls, c, eob: shape_table(sorted(c), profile_of([1])) if cls else None, {"first ac is eob": 1})),
        ("both tables of one symbol", ("dc0noac", 0, lambda cls, c, eob: shape_table(sorted(c), profile_of([1])), {"first ac is eob": 1})),
        ("blocks ended by 0x10", ("tame", 0x10, lambda cls, c, eob: None, {"eob 0x10": 1})),
        ("blocks ended by 0x50", ("tame", 0x50, lambda cls, c, eob: None, {"eob 0x50": 1})),
        ("blocks ended by 0xe0, long codes", ("tame", 0xE0, lengths([11, 12, 13], [3, 4, 5]), {"eob 0xe0": 1})),
        ("AC sizes 11..15 under short codes", ("big", 0, sized(True), {"ac size %d" % n: 1 for n in range(11, 16)})),
        ("AC sizes 11..15 under long codes", ("big", 0, sized(False), {"ac size %d" % n: 1 for n in range(11, 16)})),
        ("DC codes of 9, 10 and 16 bits", ("dc", 0, dc_long, dict({"dc cat %d" % n: 1 for n in range(12)}, **{"dc len 9": 1, "dc len 10": 1, "dc len 16": 1}))),
        ("256-entry AC table with unused and duplicated symbols", ("tame", 0, full256, {"ac len 10": 1})),
        ("ZRL and position 63 under codes of 10..16 bits", ("zrl", 0, lengths(list(range(10, 17)), [3, 4, 5]), {"zrl": 1, "ends at 63": 1})),
    ])


def _shape_stream(w, h, hv, what, eob, make, restart, sel=None, seed=0):
    planes = rich(w, h, hv, "dc0" if what == "dc0noac" else what, seed)
    if what == "dc0noac":
        for p in planes:
            p[:, :, 1:] = 0
    wr = Writer(w, h, default_comps(hv), planes)
    wr.eob = eob
    wr.restart = restart
    sel = sel or default_sel(len(hv))
    dc, ac = wr.symbols([s[0] for s in sel])
    need = collections.defaultdict(collections.Counter)
    for ci, td, ta in sel:
        need[(0, td)].update(dc[ci])
        need[(1, ta)].update(ac[ci])
    std = {(t[0], t[1]): t for t in std_tables(wr, [sel])}
    tables = []
    for key in sorted(need):
        t = make(key[0], need[key], eob)
        tables.append(std[key] if t is None else key + tuple(t))
    wr.restart = 0
    for t in sorted({c[3] for c in wr.comps}):
        wr.dqt([(0, t, ONES64)])
    wr.sof()
    for t in tables:
        wr.dht([t])
    if restart:
        wr.dri(restart)
    return wr.scan(sel).eoi(), tables


def tables():
    F = "tables"
    out = []
    w, h = TSIZE
    for name, (what, eob, make, events) in table_shapes().items():
        for lay in ("420", "444", "grey"):
            hv = LAYOUT_HV[lay]
            for restart in (0, geometry(w, h, hv)[0]):
                wr, tabs = _shape_stream(w, h, hv, what, eob, make, restart, seed=len(name))
                out.append(_case("%s, %s%s" % (name, lay, ", DRI %d" % restart if restart else ""), F, "plain", wr.bytes(), hv=hv, events=events, tables=tabs))
    # Td != Ta over {0..3}^2: component 0 takes (Td, Ta), the others the pair two further on
    for td in range(4):
        for ta in range(4):
            for restart in (0, 9):
                sel = [(0, td, ta), (1, (td + 2) % 4, (ta + 1) % 4), (2, (td + 2) % 4, (ta + 1) % 4)]
                wr, tabs = _shape_stream(w, h, HV420, "tame", 0, lambda cls, c, eob: None, restart, sel, seed=4 * td + ta)
                out.append(_case("Td %d Ta %d, 420%s" % (td, ta, ", DRI 9" if restart else ""), F, "plain", wr.bytes(), hv=HV420, events={}, tables=tabs))
    # three distinct pairs in one scan (the third has no entry table), and four in a four-component file (the host walk's)
    for lay, hv in (("420", HV420), ("444", HV444)):
        for restart in (0, geometry(w, h, hv)[0]):
            for sel in ([(0, 0, 0), (1, 1, 1), (2, 2, 2)], [(0, 3, 1), (1, 0, 2), (2, 2, 3)], [(0, 2, 3), (1, 0, 3), (2, 1, 0)]):
                wr, tabs = _shape_stream(w, h, hv, "tame", 0, lambda cls, c, eob: shape_table(sorted(c), _spread(len(c), [3, 4, 10, 11])) if cls else None, restart, sel)
                out.append(_case("tables %s, %s%s" % (sel, lay, ", DRI" if restart else ""), F, "plain", wr.bytes(), hv=hv, events={"third table": 1}, tables=tabs))
    for restart in (0, 17):
        sel = [(0, 0, 3), (1, 1, 2), (2, 2, 1), (3, 3, 0)]
        wr, tabs = _shape_stream(w, h, [(1, 1)] * 4, "tame", 0, lambda cls, c, eob: None, restart, sel)
        out.append(_case("four table pairs, four components%s" % (", DRI" if restart else ""), F, "four components", wr.bytes(), hv=[(1, 1)] * 4, events={}, tables=tabs))
    return out


def walk_events(data):
    """A plain sequential walk of a one-scan baseline stream (as coef_cases.block_bit_ranges does, restart intervals included) that counts
    what the stream makes a decoder do, in the terms the GPU walk's tables branch on (mij_entropy_kernels.h): code lengths per class, the
    end-of-block symbols, AC sizes and DC categories, and per pair of consecutive AC symbols of a block (the first not an end of block,
    its code inside twelve bits) where the first and the second end relative to a twelve-bit window.  -> Counter"""
    import stream_cases as sc
    ev = collections.Counter()
    segs, _ = sc._segments(data)
    comps, nmcu, dri = sc._frame(segs)
    tabs = sc._huff(segs[0xC4])
    sos = segs[0xDA][0]
    sel = {sos[1 + 2 * c]: (sos[2 + 2 * c] >> 4, sos[2 + 2 * c] & 15) for c in range(sos[0])}
    order = []
    for cid, a, v in comps:
        order += [sel[cid]] * (a * v)
    # the tables of each class in order of first use: the GPU walk builds entry tables for the first two, a block under a later one counts
    dc_rank, ac_rank = {}, {}
    for td, ta in order:
        dc_rank.setdefault(td, len(dc_rank))
        ac_rank.setdefault(ta, len(ac_rank))
    left = nmcu
    for piece in sc.pieces(data):
        if b"\xff\xff" in piece:
            ev["ff ff in the data"] += 1
        bits = np.unpackbits(np.frombuffer(piece + b"\0" * 8, np.uint8))
        pos = 0

        def symbol(t):
            nonlocal pos
            code = 0
            for ln in range(1, 17):
                code = (code << 1) | int(bits[pos + ln - 1])
                s = t.get((ln, code))
                if s is not None:
                    pos += ln
                    return s, ln
            raise AssertionError("no code")

        def tally(cls, ln):
            ev["%s len %d" % (cls, ln)] += 1
            ev["%s len %s" % (cls, "1..9" if ln <= 9 else "10+")] += 1

        for _ in range(min(left, dri) if dri else left):
            for td, ta in order:
                if dc_rank[td] >= 2 or ac_rank[ta] >= 2:
                    ev["third table"] += 1
                cat, ln = symbol(tabs[(0, td)])
                tally("dc", ln)
                ev["dc cat %d" % cat] += 1
                pos += cat
                k, prev, first = 1, None, True
                while k < 64:
                    rs, ln = symbol(tabs[(1, ta)])
                    tally("ac", ln)
                    n, r = rs & 15, rs >> 4
                    eob = n == 0 and r != 15
                    if first and eob:
                        ev["first ac is eob"] += 1
                    if eob:
                        ev["eob 0x%02x" % rs] += 1
                        ev["eob len %d" % ln] += 1
                    if n:
                        ev["ac size %d" % n] += 1
                    if rs == 0xF0:
                        ev["zrl"] += 1
                    if not eob and ln <= 12 and ln + n in (12, 13):
                        ev["first total %d" % (ln + n)] += 1
                    if prev is not None and prev < 12:
                        if prev + ln + n in (12, 13):
                            ev["second ends at %d" % (prev + ln + n)] += 1
                        if eob and prev + ln <= 12:
                            ev["second is eob"] += 1
                    prev = ln + n if (not eob and ln <= 12) else None
                    first = False
                    pos += n
                    if eob:
                        break
                    k += 16 if rs == 0xF0 else r + 1
                    if k == 64:
                        ev["ends at 63"] += 1
        left -= dri if dri else left
        assert 0 <= 8 * len(piece) - pos < 8, "the walk does not end in the interval's last byte"
    return ev


# ---------------------------------------------------------------------------------------------- outside the contract

def product_only():
    """Streams for which the reference does not define its answer (see the module comment): the product must neither fault nor disagree
    with the restatement on them.  No reference answer is recorded."""
    F = "product_only"
    out = []
    w, h = 40, 24

    def undefined_tables(name, hv, drop):
        wr = Writer(w, h, default_comps(hv), tame(w, h, hv))
        for t in sorted({c[3] for c in wr.comps}):
            wr.dqt([(0, t, ONES64)])
        wr.sof()
        sel = default_sel(len(hv))
        tabs = std_tables(wr, [sel])
        for t in tabs:
            wr.huff[(t[0], t[1])] = (t[2], t[3], "first")
            if (t[0], t[1]) not in drop:
                wr.dht([t])
        out.append(Case(name, F, "undefined table", None, wr.scan(sel).eoi().bytes(), {"hv": hv}))

    undefined_tables("no DC table 1", HV420, {(0, 1)})
    undefined_tables("no AC table 0", HV420, {(1, 0)})
    undefined_tables("no Huffman table at all", HV444, {(0, 0), (0, 1), (1, 0), (1, 1)})
    undefined_tables("grey without its AC table", HVGREY, {(1, 0)})
    wr = Writer(w, h, default_comps(HV420), tame(w, h, HV420))
    wr.sof()
    for t in std_tables(wr, [default_sel(3)]):
        wr.dht([t])
    out.append(Case("no quantisation table", F, "undefined table", None, wr.scan(default_sel(3)).eoi().bytes(), {"hv": HV420}))
    base = plain(w, h, HV420).bytes()
    sos = base.index(b"\xff\xda")
    out.append(Case("no scan: EOI behind the tables", F, "no scan", None, base[:sos] + EOI, {"hv": HV420}))
    out.append(Case("no scan, grey 1x1", F, "no scan", None, (lambda b: b[:b.index(b"\xff\xda")] + EOI)(plain(1, 1, HVGREY).bytes()), {"hv": HVGREY}))
    out.append(Case("a component no scan covers: Y alone", F, "uncovered component", None, _multi_scan(w, h, HV420, [[0]]).bytes(), {"hv": HV420}))
    out.append(Case("a component no scan covers: CbCr alone", F, "uncovered component", None, _multi_scan(w, h, HV444, [[1, 2]]).bytes(), {"hv": HV444}))
    over = tuple([0] * 7 + [255, 2] + [0] * 7)
    for name, where in (("in front of SOF", "pre"), ("behind SOF", "mid")):
        out.append(Case("DHT counts of 257 " + name, F, "dht over 256", None,
                        plain(w, h, HV420, **{where: lambda wr: wr.seg(0xC4, Writer.dht_payload([(1, 3, over, tuple(k & 255 for k in range(257)))]))}).bytes(), {"hv": HV420}))
    # a DC table whose symbols ask for 17 and more extra bits
    for sym in (0x11, 0x1F, 0xFF):
        wr = Writer(w, h, default_comps(HVGREY), tame(w, h, HVGREY))
        wr.dqt([(0, 0, ONES64)]).sof()
        tabs = std_tables(wr, [[(0, 0, 0)]])
        dc = tabs[0]
        bad = (0, 0, dc[2], tuple(sym if k == 0 else v for k, v in enumerate(dc[3])))
        wr.huff[(0, 0)] = (dc[2], dc[3], "first")
        wr.seg(0xC4, Writer.dht_payload([bad]))
        wr.dht([tabs[1]])
        out.append(Case("DC symbol 0x%02x" % sym, F, "dc over 16", None, wr.scan([(0, 0, 0)]).eoi().bytes(), {"hv": HVGREY}))
    # 256 codes, the last one of nine bits and in use
    def full256_short(cls, c, eob):
        if cls == 0:
            return None
        syms = [s for s, _ in sorted(c.items(), key=lambda kv: (-kv[1], kv[0]))]
        unused = [s for s in range(256) if s not in c][:256 - 2 * len(syms)]
        return (tuple([0] * 7 + [128, 128] + [0] * 7), tuple(syms + unused + syms[::-1]), "last")
    for lay in ("420", "grey"):
        wr, _ = _shape_stream(w, h, LAYOUT_HV[lay], "tame", 0, full256_short, 0)
        out.append(Case("256 codes, the last of nine bits and in use, %s" % lay, F, "fast index 255", None, wr.bytes(), {"hv": LAYOUT_HV[lay]}))
    return out


FAMILIES = collections.OrderedDict([("reasons", reasons), ("segments", segments), ("frames", frames), ("scans", scans), ("tables", tables)])
_cache = {}


def family(name):
    """the cases of one family, made once"""
    if name not in _cache:
        _cache[name] = product_only() if name == "product_only" else FAMILIES[name]()
        names = [c.name for c in _cache[name]]
        assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return _cache[name]
