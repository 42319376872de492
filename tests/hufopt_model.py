"""Python model of the encoder's optimised Huffman tables (include/mij_host.h, mjw_emit_optimized; csrc/mij_emit_kernels.h,
k_emit_hist / k_emit_build), written from ITU-T T.81 K.2 and Annex C only:

  histogram           the symbols mjw_emit emits for a slot's units, counted per table with numpy
  optimal_table       counts -> (BITS[16], HUFFVAL) by K.2 with the tie-breaking of libjpeg's jpeg_gen_optimal_table, None when a
                      length before the K.3 shortening exceeds 32
  header              the writer's plain header with the four tables in its DHT segment
  tables_from_header  any such header's DHT segment -> canonical codes (Annex C), for emit_model.emit_entropy
  emit_optimized      model header + emit_model.emit_entropy + EOI: the whole optimised stream
  scan_symbol_counts  a baseline JPEG file's own DHT tables and the counts of the symbols in its scan (a small Huffman walk), to hold
                      optimal_table against files another encoder wrote
  deep_counts         Fibonacci-like counts whose code tree is a chain of a given depth

Tables are ordered luma DC, chroma DC, luma AC, chroma AC everywhere."""
import heapq

import numpy as np

import emit_model as em

DHT_AT = 173  # offset of the DHT marker in the writer's headers
_IDS = (0x00, 0x10, 0x01, 0x11)  # identifiers in the segment's order: luma DC, luma AC, chroma DC, chroma AC
_ORDER = (0, 2, 1, 3)
_SOS = bytes([0xFF, 0xDA, 0, 0xC, 3, 1, 0, 2, 0x11, 3, 0x11, 0, 0x3F, 0])


def code_sizes_literal(freq):
    """K.2's code-size loop over 256 counts plus the pseudo-symbol, step for step as the contract spells it -> codesize[257]"""
    f = [int(x) for x in freq] + [1]
    assert len(f) == 257
    size, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):
            if f[i] and (v is None or f[i] <= v):
                c1, v = i, f[i]
        c2, v = -1, None
        for i in range(257):
            if f[i] and i != c1 and (v is None or f[i] <= v):
                c2, v = i, f[i]
        if c2 < 0:
            return size
        f[c1] += f[c2]
        f[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1


def code_sizes(freq):
    """The same result from a heap ordered by (count, largest index first): c1 and c2 are its two smallest entries, the merged tree
    keeps c1's index, and a tree's leaves (the `others` chain) are a list.  The tests hold it against code_sizes_literal."""
    f = [int(x) for x in freq] + [1]
    assert len(f) == 257
    size = [0] * 257
    heap = [(v, -i) for i, v in enumerate(f) if v]
    heapq.heapify(heap)
    leaves = {-i: [-i] for (_, i) in heap}
    while len(heap) > 1:
        v1, i1 = heapq.heappop(heap)
        v2, i2 = heapq.heappop(heap)
        leaves[-i1] += leaves.pop(-i2)
        for j in leaves[-i1]:
            size[j] += 1
        heapq.heappush(heap, (v1 + v2, i1))
    return size


def unlimited_depth(freq):
    return max(code_sizes(freq))


def optimal_table(freq):
    """-> (bits, vals): bits[l - 1] codes of length l, vals the symbols in code order; None for the over-32 case"""
    size = code_sizes(freq)
    if max(size) > 32:
        return None
    bits = [0] * 33
    for s in size:
        if s:
            bits[s] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while i > 0 and bits[i] == 0:
        i -= 1
    if i:
        bits[i] -= 1
    vals = [j for s in range(1, 33) for j in range(256) if size[j] == s]
    assert sum(bits[1:17]) == len(vals)
    return bits[1:17], vals


def _cat(v):
    """magnitude category of an int64 array (0 for 0)"""
    a = np.abs(v.astype(np.int64))
    return np.where(a > 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1, 0)


def histogram(du, dpm, ny=None):
    """[4][256] counts of the symbols of units du ([n, 64] int16, MCU order, dpm units per MCU of which ny are luma: emit_model.luma_units;
    a grey slot, dpm = ny = 1, counts nothing in the chroma tables)"""
    du = np.asarray(du, np.int16).reshape(-1, 64).astype(np.int64)
    n = du.shape[0]
    ny = em.luma_units(dpm, ny)
    p = np.arange(n) % dpm
    luma = p < ny
    comp = np.where(luma, 0, p - ny + 1)
    freq = np.zeros((4, 256), np.int64)
    for c in range(3):
        dc = du[comp == c, 0]
        freq[0 if c == 0 else 1] += np.bincount(_cat(np.diff(np.concatenate([[0], dc]))), minlength=256)
    for chroma in (0, 1):
        u = du[luma == (not chroma)]
        f = freq[2 + chroma]
        rows, cols = np.nonzero(u[:, 1:])
        cols = cols + 1
        first = np.concatenate([[True], rows[1:] != rows[:-1]]) if len(rows) else np.zeros(0, bool)
        prev = np.where(first, 0, np.concatenate([[0], cols[:-1]]))
        run = cols - prev - 1
        f[0xF0] += int((run >> 4).sum())
        f += np.bincount(((run & 15) << 4) + _cat(u[rows, cols]), minlength=256)
        f[0x00] += int((u[:, 63] == 0).sum())
    return freq


def tables(freq4):
    """four (bits, vals), or None when any of them is the over-32 case"""
    t = [optimal_table(f) for f in freq4]
    return None if any(x is None for x in t) else t


def _dht_span(hdr):
    """(start, end) of the one DHT segment of a writer's header: DHT_AT for three components, further in front for a grey stream"""
    i = 2
    while hdr[i + 1] != 0xC4:
        assert hdr[i] == 0xFF and hdr[i + 1] != 0xDA, i
        i += 2 + ((hdr[i + 2] << 8) | hdr[i + 3])
    return i, i + 2 + ((hdr[i + 2] << 8) | hdr[i + 3])


def header(plain, tabs):
    """the plain header's bytes with `tabs` in the DHT segment, for the tables that segment holds: four, or the two luma tables of a
    grey stream"""
    a, b = _dht_span(plain)
    have = dht_tables(plain[a + 4:b])
    seg = bytearray()
    for ident, k in zip(_IDS, _ORDER):
        if ident not in have:
            continue
        bits, vals = tabs[k]
        seg += bytes([ident]) + bytes(bits) + bytes(vals)
    n = len(seg) + 2
    return bytes(plain[:a]) + bytes([0xFF, 0xC4, n >> 8, n & 255]) + bytes(seg) + bytes(plain[b:])


class _Codes(dict):
    """{symbol: (code, len)}; a symbol the table lacks reads as a code of no bits, as in the encoder's tables"""

    def __missing__(self, key):
        return (0, 0)


def _canonical(bits, vals):
    t, code, k = _Codes(), 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            t[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return t


def dht_tables(seg):
    """the payload of DHT segments -> {identifier: (bits, vals)}"""
    out, i = {}, 0
    while i < len(seg):
        ident, bits = seg[i], list(seg[i + 1:i + 17])
        n = sum(bits)
        out[ident] = (bits, list(seg[i + 17:i + 17 + n]))
        i += 17 + n
    return out


def tables_from_header(hdr):
    """-> [ {symbol: (code, len)} ] x 4 from the one DHT segment of a writer's header, plain or optimised (a grey header's chroma tables
    are empty)"""
    a, b = _dht_span(hdr)
    d = dht_tables(hdr[a + 4:b])
    if a == DHT_AT:
        assert list(d) == [0x00, 0x10, 0x01, 0x11]
        assert bytes(hdr[b:]) == _SOS
    else:
        assert list(d) == [0x00, 0x10] and hdr[b + 1] == 0xDA and hdr[b + 4] == 1
    return [_canonical(*d[i]) if i in d else _Codes() for i in (0x00, 0x01, 0x10, 0x11)]


def emit_optimized(plain_hdr, du, dpm, ny=None):
    """the optimised stream of units du whose plain header is plain_hdr, or None for the over-32 fallback"""
    t = tables(histogram(du, dpm, ny))
    if t is None:
        return None
    h = header(plain_hdr, t)
    return h + em.emit_entropy(tables_from_header(h), du, dpm, ny=ny) + b"\xff\xd9"


def deep_counts(depth):
    """depth counts c[0] < c[1] < ... with c[k + 1] above the sum of the pseudo-symbol and c[0 .. k - 1]: every merge joins the
    running tree and the next symbol, so the unlimited code tree is a chain and its longest code has `depth` bits"""
    c, total = [1, 2], 4
    while len(c) < depth:
        c.append(total - c[-1] + 1)
        total += c[-1]
    return c[:depth]


# ---------------------------------------------------------------- a baseline file's own tables and symbol counts

def scan_symbol_counts(data):
    """A baseline, single-scan, interleaved JPEG file -> [(bits, vals, counts[256])] for each (class, id) table the scan uses, in
    the order of first use.  Walks every MCU with the file's own codes; no restart markers."""
    data = bytes(data)
    i, dht, comps, sel = 2, {}, None, None
    while True:
        assert data[i] == 0xFF, i
        m = data[i + 1]
        ln = (data[i + 2] << 8) | data[i + 3]
        seg = data[i + 4:i + 2 + ln]
        if m == 0xC4:
            dht.update(dht_tables(seg))
        elif m == 0xC0:
            h, w = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            comps = [(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15) for k in range(seg[5])]
        elif m in (0xC1, 0xC2):
            raise AssertionError("not a baseline file")
        elif m == 0xDD:
            assert ((seg[0] << 8) | seg[1]) == 0, "restart interval"
        elif m == 0xDA:
            sel = {seg[1 + 2 * k]: (seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(seg[0])}
            i += 2 + ln
            break
        i += 2 + ln
    ecs = data[i:data.rindex(b"\xff\xd9")].replace(b"\xff\x00", b"\xff")
    nbits = len(ecs) * 8
    acc = int.from_bytes(ecs, "big")
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    if len(comps) == 1:
        mx, my, blocks = (w + 7) // 8, (h + 7) // 8, [(comps[0][0], 1)]
    else:
        mx, my = (w + 8 * hmax - 1) // (8 * hmax), (h + 8 * vmax - 1) // (8 * vmax)
        blocks = [(cid, hs * vs) for (cid, hs, vs) in comps]
    look, counts, order = {}, {}, []
    for cid, _ in blocks:
        td, ta = sel[cid]
        for ident in (td, 0x10 | ta):
            if ident not in look:
                bits, vals = dht[ident]
                look[ident] = {(ln, code): s for s, (code, ln) in _canonical(bits, vals).items()}
                counts[ident] = [0] * 256
                order.append(ident)
    pos = 0

    def sym(ident):
        nonlocal pos
        t, code = look[ident], 0
        for ln in range(1, 17):
            code = (code << 1) | ((acc >> (nbits - 1 - pos)) & 1)
            pos += 1
            if (ln, code) in t:
                s = t[(ln, code)]
                counts[ident][s] += 1
                return s
        raise AssertionError("bad code at bit %d" % pos)

    for _ in range(mx * my):
        for cid, nb in blocks:
            td, ta = sel[cid]
            for _ in range(nb):
                cat = sym(td)
                pos += cat
                k = 1
                while k < 64:
                    s = sym(0x10 | ta)
                    if s == 0:
                        break
                    k += (s >> 4) + 1 if s != 0xF0 else 16
                    pos += s & 15 if s != 0xF0 else 0
    assert nbits - pos < 8 + 8, (nbits, pos)
    return [(dht[i][0], dht[i][1], counts[i]) for i in order]
