"""numpy / Python model of the GPU Huffman emission (csrc/mij_emit_kernels.h), stage for stage, so that the decomposition itself is
checked on the CPU against mjw_emit (ica.emit_jpeg):

  unit_pieces   what each lane of a unit's wavefront emits: lane 0 the DC difference, a non-zero lane its ZRLs and run/size
                symbol, lane 63 the EOB (coefficient 63 zero) and, in the slot's last unit, the 7 fill bits
  tile_bits     k_emit_len: the bits of each tile of `tile` units
  scan          k_emit_scan: each tile's bit offset in the slot
  count         k_emit_count: the tile's bits packed from bit h = offset % 8 on; its 0xFF bytes among the bytes whose 8 bits all
                lie in the tile; its head (bits before its first byte boundary) and tail (bits after its last)
  stuff         k_emit_stuff: the tile's stuffed size (the byte shared with the previous tile -- previous tail + head -- belongs to
                this tile) scanned into its output offset
  write         k_emit_write: each tile's bytes, stuffed, at that offset

The code tables come from the DHT segment of the stream's own headers (Annex C canonical codes), not from the library's tables."""
import numpy as np

HDR = 607
# offsets of BITS (16 bytes) and HUFFVAL in the writer's headers: luma DC, chroma DC, luma AC, chroma AC
_DHT = ((178, 194, 12), (386, 402, 12), (207, 223, 162), (415, 431, 162))


def tables_from_header(hdr):
    """-> [ {symbol: (code, len)} ] x 4 in the order luma DC, chroma DC, luma AC, chroma AC"""
    out = []
    for (b, v, n) in _DHT:
        bits, vals = hdr[b:b + 16], hdr[v:v + n]
        t, code, k = {}, 0, 0
        for ln in range(1, 17):
            for _ in range(bits[ln - 1]):
                t[vals[k]] = (code, ln)
                code += 1
                k += 1
            code <<= 1
        out.append(t)
    return out


def tables_from_stream(data):
    """(the four tables in the order luma DC, chroma DC, luma AC, chroma AC, the length of the headers) of any baseline stream with one
    scan, read from its own DHT segments; a table the stream lacks (a grey stream has no chroma tables) is empty"""
    dht, i = {}, 2
    while True:
        assert data[i] == 0xFF, i
        m, n = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        if m == 0xC4:
            j = i + 4
            while j < i + 2 + n:
                ident, bits = data[j], data[j + 1:j + 17]
                cnt = sum(bits)
                vals = data[j + 17:j + 17 + cnt]
                t, code, k = {}, 0, 0
                for ln in range(1, 17):
                    for _ in range(bits[ln - 1]):
                        t[vals[k]] = (code, ln)
                        code += 1
                        k += 1
                    code <<= 1
                dht[ident] = t
                j += 17 + cnt
            assert j == i + 2 + n
        i += 2 + n
        if m == 0xDA:
            return [dht.get(ident, {}) for ident in (0x00, 0x01, 0x10, 0x11)], i


def _mag(v):
    n = abs(int(v)).bit_length()
    return n, (v - 1 if v < 0 else v) & ((1 << n) - 1)


def luma_units(dpm, ny=None):
    """the luma units per MCU: given, or what the writer's own two layouts have (6 -> 4, 3 -> 1)"""
    return (4 if dpm == 6 else 1) if ny is None else ny


def unit_pieces(T, du, u, dpm, n_du, ny=None):
    """[(lane, [(code, len), ...])] for unit u of a slot (du: [n_du, 64] int16); ny: the luma units per MCU (luma_units), the other
    dpm - ny units being Cb and Cr -- a grey slot has dpm = ny = 1"""
    ny = luma_units(dpm, ny)
    m, p = divmod(u, dpm)
    luma = p < ny
    if luma:  # the luma unit before it; for an MCU's first one, the last luma unit of the MCU before
        prev = u - 1 if p > 0 else (u - (dpm - ny + 1) if m > 0 else -1)
    else:
        prev = u - dpm if m > 0 else -1
    dc, ac = (T[0], T[2]) if luma else (T[1], T[3])
    v = [int(x) for x in du[u]]
    lanes = []
    diff = v[0] - (int(du[prev][0]) if prev >= 0 else 0)
    if diff == 0:
        lanes.append((0, [dc[0]]))
    else:
        n, b = _mag(diff)
        c, ln = dc[n]
        lanes.append((0, [((c << n) | b, ln + n)]))
    last = 0
    for k in range(1, 64):
        pieces = []
        if v[k]:
            run = k - last - 1
            last = k
            pieces += [ac[0xF0]] * (run >> 4)
            n, b = _mag(v[k])
            c, ln = ac[((run & 15) << 4) + n]
            pieces.append(((c << n) | b, ln + n))
        if k == 63:
            if not v[63]:
                pieces.append(ac[0])
            if u + 1 == n_du:
                pieces.append((0x7F, 7))
        if pieces:
            lanes.append((k, pieces))
    return lanes


def unit_bits(T, du, u, dpm, n_du, ny=None):
    return sum(ln for _, ps in unit_pieces(T, du, u, dpm, n_du, ny) for _, ln in ps)


def _pack(T, du, first, n, dpm, n_du, h, ny=None):
    """the tile's bits as a Python int of h + bits bits (the first h zero), MSB first; and that bit count"""
    acc, nb = 0, h
    for u in range(first, first + n):
        for _, ps in unit_pieces(T, du, u, dpm, n_du, ny):
            for c, ln in ps:
                acc = (acc << ln) | c
                nb += ln
    return acc, nb


def _bytes_of(acc, nb, nbytes):
    """the first nbytes whole bytes of an nb-bit MSB-first buffer"""
    return [(acc >> (nb - 8 * (j + 1))) & 0xFF for j in range(nbytes)]


def emit_entropy(T, du, dpm, tile=128, stats=None, ny=None):
    """The stuffed entropy-coded segment the kernels write for one slot (fill included, the bits below the last byte dropped).
    stats, when given, receives the bits, the tiles, and of the seams between tiles those that fall on a byte boundary (aligned) and those
    whose shared byte is 0xFF (shared_ff)."""
    du = np.asarray(du, dtype=np.int16).reshape(-1, 64)
    n_du = du.shape[0]
    tiles = [(f, min(tile, n_du - f)) for f in range(0, n_du, tile)]
    # k_emit_len, k_emit_scan
    t_bits = [sum(unit_bits(T, du, u, dpm, n_du, ny) for u in range(f, f + n)) for (f, n) in tiles]
    t_boff = np.concatenate([[0], np.cumsum(t_bits, dtype=np.int64)[:-1]]).tolist()
    # k_emit_count
    t_ff, t_head, t_tail = [], [], []
    for (f, n), b0, nbit in zip(tiles, t_boff, t_bits):
        b1, h = b0 + nbit, b0 % 8
        n_own = (b1 >> 3) - (b0 >> 3)
        acc, nb = _pack(T, du, f, n, dpm, n_du, h, ny)
        by = _bytes_of(acc, nb, n_own)
        t_ff.append(sum(1 for j in range(1 if h else 0, n_own) if by[j] == 0xFF))
        t_head.append(by[0] & ((1 << (8 - h)) - 1) if h and n_own else 0)
        tb = b1 % 8
        t_tail.append(acc & ((1 << tb) - 1) if tb else 0)
    # k_emit_stuff
    sizes = []
    for t, ((f, n), b0, nbit) in enumerate(zip(tiles, t_boff, t_bits)):
        b1, h = b0 + nbit, b0 % 8
        v = (b1 >> 3) - (b0 >> 3) + t_ff[t]
        if stats is not None and t > 0 and not h:
            stats["aligned"] = stats.get("aligned", 0) + 1
        if h and t > 0:
            shared = (t_tail[t - 1] << (8 - h)) | t_head[t]
            v += shared == 0xFF
            if stats is not None and shared == 0xFF:
                stats["shared_ff"] = stats.get("shared_ff", 0) + 1
        sizes.append(v)
    t_out = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)[:-1]]).tolist()
    total = int(sum(sizes))
    # k_emit_write
    out = bytearray(total)
    for t, ((f, n), b0, nbit) in enumerate(zip(tiles, t_boff, t_bits)):
        b1, h = b0 + nbit, b0 % 8
        n_own = (b1 >> 3) - (b0 >> 3)
        acc, nb = _pack(T, du, f, n, dpm, n_du, h, ny)
        if h:
            acc |= t_tail[t - 1] << (nb - h)
        o = t_out[t]
        for b in _bytes_of(acc, nb, n_own):
            out[o] = b
            o += 1
            if b == 0xFF:
                out[o] = 0
                o += 1
        assert o == t_out[t] + sizes[t]
    if stats is not None:
        stats["bits"] = int(sum(t_bits))
        stats["tiles"] = len(tiles)
    return bytes(out)


# ---------------------------------------------------------------- adversarial data units

def _unit(rng, kind):
    d = np.zeros(64, np.int16)
    if kind == "zero":
        return d
    if kind in (15, 16, 17, 31, 32, 48):  # a run of that many zeros before a value, and again later where it fits
        d[1 + kind] = rng.choice([-1, 1]) * int(rng.integers(1, 1024))
        if 1 + kind + 1 + kind < 64:
            d[2 + 2 * kind] = rng.choice([-1, 1]) * int(rng.integers(1, 1024))
        return d
    if kind == "last":  # coefficient 63 non-zero: no EOB
        d[63] = rng.choice([-1023, 1023, 1, -1, 77])
        d[int(rng.integers(1, 63))] = int(rng.integers(-1023, 1024))
        return d
    if kind == "ff":  # magnitudes of all ones and long codes: streams dense in 0xFF
        d[1:] = rng.choice([1023, 511, 255, 127, -1024 + 1, 0], size=63)
        return d
    if kind == "max":
        d[1:] = rng.choice([1023, -1023], size=63)
        return d
    d[1:] = np.where(rng.random(63) < 0.3, rng.integers(-1023, 1024, size=63), 0)
    return d


KINDS = ["zero", 15, 16, 17, 31, 32, 48, "last", "ff", "max", "rand"]


def _components(dpm, ny=None):
    """the component of each of an MCU's units"""
    ny = luma_units(dpm, ny)
    return [0 if p < ny else p - ny + 1 for p in range(dpm)]


def adversarial_units(rng, n_mcu, dpm, dc_extremes=True, ny=None):
    """[n_mcu * dpm, 64] int16 units covering every case of KINDS, DC differences of +-2047 per component when dc_extremes,
    and every AC value inside -1023..1023; ny as in unit_pieces"""
    n = n_mcu * dpm
    du = np.stack([_unit(rng, KINDS[(i * 7 + int(rng.integers(0, 3))) % len(KINDS)]) for i in range(n)])
    # DC: per component, differences walk the full range; +-2047 appear when asked
    comp = np.array(_components(dpm, ny) * n_mcu)
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        vals = np.zeros(len(idx), np.int64)
        for j in range(len(idx)):
            if dc_extremes and j % 5 == 1:
                vals[j] = 1023 if j % 10 == 1 else -1024  # from -1024 to 1023 and back: +-2047
            elif dc_extremes and j % 5 == 2:
                vals[j] = -1024 if vals[j - 1] == 1023 else 1023
            else:
                vals[j] = int(rng.integers(-1024, 1024))
        du[idx, 0] = vals
    return du


def dc_diffs(du, dpm, ny=None):
    du = np.asarray(du).reshape(-1, 64)
    comp = np.array(_components(dpm, ny) * (du.shape[0] // dpm))
    out = []
    for c in range(3):
        v = du[comp == c, 0].astype(np.int64)
        out.append(np.diff(np.concatenate([[0], v])))
    return np.concatenate(out)
