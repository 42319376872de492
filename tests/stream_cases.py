"""Case generators for the stream-end tests (test_stream_ends_host.py, test_gpu_stream_ends.py): JPEG streams whose entropy data is cut,
padded, followed by the wrong marker, or edited around a restart marker.  Pure Python, deterministic from a seed; every case has a
readable name (used in assertion messages) and a kind (what the tests key their expectations on).

Headers and tables always stay whole: the reference reads damaged tables with undefined behaviour (a DHT whose counts are stream bytes
runs stbi__build_huffman past its arrays), which no restatement can match -- the same class helpers.mutate excludes."""
import collections

import numpy as np

import helpers

Case = collections.namedtuple("Case", "name kind data")

EOI = b"\xff\xd9"
TAILS = (b"", EOI) + tuple(bytes([0xFF, 0xD0 + i]) for i in range(8)) + (b"\xff\xc4", b"\xff\xda")
OTHER_TAILS = tuple(t for t in TAILS if t != EOI)


def _tail_name(t):
    return t.hex() if t else "nothing"


def cut_offsets(base):
    """every cut offset inside the entropy-coded ranges: from right behind a range's first byte to right behind its last byte"""
    out = []
    for a, b in helpers.entropy_ranges(base):
        out.extend(range(a + 1, b + 1))
    return out


def cut_cases(base, n=None, seed=0, tails=(EOI,), extra=()):
    """base[:cut] + tail for cuts inside the entropy-coded ranges (helpers.entropy_ranges; every scan of a progressive file; right behind
    a range's first byte and right behind its last byte are both in).  n None: every byte offset; otherwise n seeded offsets (without
    repetition) plus the offsets in `extra`.  The tails rotate over the cuts in ascending order."""
    allowed = cut_offsets(base)
    if n is None or n >= len(allowed):
        cuts = allowed
    else:
        rng = np.random.default_rng(seed)
        cuts = sorted(set(int(c) for c in rng.choice(np.array(allowed), n, replace=False)) | set(int(c) for c in extra))
    return [Case("cut@%d+%s" % (c, _tail_name(tails[i % len(tails)])), "cut", base[:c] + tails[i % len(tails)]) for i, c in enumerate(cuts)]


def refinement_tail_offsets(base, last=64):
    """the last `last` byte offsets of every AC/DC refinement scan (Ah != 0) of a progressive stream"""
    out = []
    for a, b in helpers.entropy_ranges(base):
        # the SOS header ends right in front of the range: ... Ss Se AhAl
        if base[a - 1] >> 4:
            out.extend(range(max(a + 1, b + 1 - last), b + 1))
    return out


def restart_positions(base):
    """offsets of the RSTn markers inside the entropy-coded data"""
    rs = helpers.entropy_ranges(base)
    if not rs:
        return []
    a, b = rs[0][0], rs[-1][1]
    return [i for i in range(a, b - 1) if base[i] == 0xFF and 0xD0 <= base[i + 1] <= 0xD7]


# extract-gate verdict per kind, as tabulated from the rule in mjh_extract_scan (1: the GPU walk takes the stream, 2: host walk); kinds
# that are missing here ("cut", "rst cut", "boundary cut") are decided by the marker structure the cut leaves: expected_extract_status
TAIL_BYTES = (b"\x00", b"\x12\x34\x56", b"\xff\x00", b"\x00\xff\x00\x00", b"\x7f" * 40, b"\xff\xff", b"\xff\xff\xff", b"\xff\xff\x00")
KIND_STATUS = {
    "intact": 1, "tail plain": 1, "tail stuffed ff": 1, "eoi twice": 1, "padflip": 1, "rst renumber": 1, "rst pad byte": 1, "rst 2 pad bytes": 1,
    "rst byte cut": 1, "boundary pad": 1,
    "tail fill ff": 2, "no eoi": 2, "rst dropped": 2, "rst doubled": 2, "rst fill ff": 2, "stray rst": 2, "fill ff mid": 2,
}


def tail_cases(base):
    """Structural variants of one baseline stream that ends in EOI: bytes after the last block, EOI missing or twice, flipped padding bits,
    edits around the restart markers (the first six and the last three), stray markers, and cuts at every byte of the last 40 followed by
    EOI -- for restart streams the same cuts in front of the first, a middle and the last RSTn (bytes removed in front of the marker, at
    most the marker's own interval)."""
    assert base[-2:] == EOI
    body = base[:-2]
    out = [Case("intact", "intact", base)]
    for t in TAIL_BYTES:
        kind = "tail fill ff" if t[:2] == b"\xff\xff" else ("tail stuffed ff" if 0xFF in t else "tail plain")
        out.append(Case("tail %s" % t[:6].hex() + ("x%d" % len(t) if len(t) > 6 else ""), kind, body + t + EOI))
    out.append(Case("no eoi", "no eoi", body))
    out.append(Case("eoi twice", "eoi twice", base + EOI))
    if base[-4] != 0xFF:  # not the 0x00 of a stuffed pair
        for k in range(1, 8):
            b = bytearray(base)
            b[-3] ^= (1 << k) - 1
            if b[-3] != 0xFF:
                out.append(Case("padflip %d" % k, "padflip", bytes(b)))
    pos = restart_positions(base)
    for p in pos[:6] + pos[6:][-3:]:
        b = bytearray(base)
        b[p + 1] = 0xD0 + ((b[p + 1] - 0xD0 + 3) % 8)
        out.append(Case("rst renumber @%d" % p, "rst renumber", bytes(b)))
        out.append(Case("rst dropped @%d" % p, "rst dropped", base[:p] + base[p + 2:]))
        out.append(Case("rst doubled @%d" % p, "rst doubled", base[:p] + base[p:p + 2] + base[p:]))
        out.append(Case("rst pad byte before @%d" % p, "rst pad byte", base[:p] + b"\x00" + base[p:]))
        out.append(Case("rst 2 pad bytes before @%d" % p, "rst 2 pad bytes", base[:p] + b"\xaa\x55" + base[p:]))
        out.append(Case("rst fill ff before @%d" % p, "rst fill ff", base[:p] + b"\xff" + base[p:]))
        out.append(Case("rst byte cut before @%d" % p, "rst byte cut", base[:p - 1] + base[p:]))
    start = helpers.entropy_ranges(base)[0][0]
    mid = (start + len(base)) // 2
    if base[mid - 1] == 0xFF:
        mid += 1
    out.append(Case("stray rst", "stray rst", base[:mid] + b"\xff\xd3" + base[mid:]))
    out.append(Case("fill ff mid + stuffed", "fill ff mid", base[:mid] + b"\xff\xff\x00" + base[mid:]))
    for c in range(max(start + 1, len(base) - 42), len(base) - 2):
        out.append(Case("cut %d + eoi" % (len(base) - 2 - c), "cut", base[:c] + EOI))
    if pos:
        for which, p in (("first", pos[0]), ("middle", pos[len(pos) // 2]), ("last", pos[-1])):
            prev = max([q + 2 for q in pos if q < p] + [start])
            for k in range(2, min(40, p - prev) + 1):  # k = 1 is "rst byte cut"
                out.append(Case("cut %d before %s rst @%d" % (k, which, p), "rst cut", base[:p - k] + base[p:]))
    return out


def unstuffed_length(data):
    """bytes of entropy data of a single-scan stream with the 0xff00 stuffing removed (restart markers not counted)"""
    rs = helpers.entropy_ranges(data)
    assert len(rs) == 1
    seg = data[rs[0][0]:rs[0][1]]
    n = len(seg) - seg.count(b"\xff\x00")
    for i in range(8):
        n -= 2 * seg.count(bytes([0xFF, 0xD0 + i]))
    return n


def boundary_cases(bases, small=()):
    """Baseline streams whose unstuffed entropy length sits on and around a multiple of 512 bytes (the 4096-bit subsequences of a batch) and
    of 128 bytes (the 1024-bit ones of a single picture).  bases: streams without restart markers that end in EOI; each is padded behind
    its last block with bytes the reference skips (0x2a: it looks for the next 0xff, codec/jpeg.c:1727-1737) to k*S-1, k*S, k*S+1 -- and cut,
    with an EOI behind the cut, to (k-1)*S-1, (k-1)*S, (k-1)*S+1 where that leaves data.  small: streams passed through as they are (shorter
    than one subsequence; a restart interval of one MCU on a flat picture), each also cut in the middle and one byte before its end + EOI."""
    out = []
    for bi, base in enumerate(bases):
        assert base[-2:] == EOI and not restart_positions(base)
        body = base[:-2]
        start = helpers.entropy_ranges(base)[0][0]
        n = unstuffed_length(base)
        for S in (512, 128):
            k = (n + 1 + S - 1) // S
            for d in (-1, 0, 1):
                pad = k * S + d - n
                if pad >= 0:
                    out.append(Case("base%d padded to %d*%d%+d" % (bi, k, S, d), "boundary pad", body + b"\x2a" * pad + EOI))
                want = (k - 1) * S + d
                if want <= 0:
                    continue
                # the cut that leaves `want` unstuffed bytes
                cnt, i = 0, start
                while cnt < want:
                    i += 2 if base[i] == 0xFF else 1
                    cnt += 1
                out.append(Case("base%d cut to %d*%d%+d" % (bi, k - 1, S, d), "boundary cut", base[:i] + EOI))
    for si, base in enumerate(small):
        assert base[-2:] == EOI
        out.append(Case("small%d intact" % si, "intact", base))
        a, b = helpers.entropy_ranges(base)[0][0], len(base) - 2
        for c in sorted({(a + b) // 2, b - 1}):
            if c > a:
                out.append(Case("small%d cut@%d + eoi" % (si, c), "boundary cut", base[:c] + EOI))
    return out


# ------------------------------------------------------------------ what the structure of a stream says, stated independently of the product

def _segments(data):
    """marker segments up to and including SOS: -> ({marker: [payload, ...]}, offset of the entropy data)"""
    segs = collections.defaultdict(list)
    i = 2
    while True:
        assert data[i] == 0xFF, i
        m = data[i + 1]
        n = (data[i + 2] << 8) | data[i + 3]
        segs[m].append(data[i + 4:i + 2 + n])
        i += 2 + n
        if m == 0xDA:
            return segs, i


def _frame(segs):
    sof = segs[0xC0][0]
    h, w, nc = (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4], sof[5]
    comps = [(sof[6 + 3 * c], sof[7 + 3 * c] >> 4, sof[7 + 3 * c] & 15) for c in range(nc)]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    nmcu = ((w + 8 * hmax - 1) // (8 * hmax)) * ((h + 8 * vmax - 1) // (8 * vmax))
    dri = 0
    if 0xDD in segs:
        dri = (segs[0xDD][-1][0] << 8) | segs[0xDD][-1][1]
    return comps, nmcu, dri


def expected_extract_status(data):
    """The rule mjh_extract_scan states in its own comments, on a baseline single-scan stream with whole headers: the entropy data is runs of
    bytes up to a 0xff that is not followed by 0x00; without a restart interval that marker must be EOI, with one the data is cut at every
    RSTn into exactly ceil(MCUs / interval) pieces, the last one ending at EOI.  Anything else -- no marker behind the data, fill bytes
    (0xff 0xff), any other marker, too many or too few pieces -- is for the host walk (2)."""
    segs, i = _segments(data)
    _, nmcu, dri = _frame(segs)
    want = (nmcu + dri - 1) // dri if dri else 1
    nseg = 0
    while True:
        f = data.find(b"\xff", i)
        if f < 0 or f + 1 >= len(data):
            return 2
        m = data[f + 1]
        i = f + 2
        if m == 0x00:
            continue
        if m != 0xD9 and not (dri and 0xD0 <= m <= 0xD7):
            return 2
        if nseg >= want:
            return 2
        nseg += 1
        if m == 0xD9:
            return 1 if nseg == want else 2


def _huff(payloads):
    """DHT payloads -> {(class, id): {(length, code): symbol}}"""
    tabs = {}
    for p in payloads:
        j = 0
        while j < len(p):
            tc_th = p[j]
            counts = p[j + 1:j + 17]
            vals = p[j + 17:j + 17 + sum(counts)]
            code, k, t = 0, 0, {}
            for ln in range(1, 17):
                for _ in range(counts[ln - 1]):
                    t[(ln, code)] = vals[k]
                    code += 1
                    k += 1
                code <<= 1
            tabs[(tc_th >> 4, tc_th & 15)] = t
            j += 17 + sum(counts)
    return tabs


def pieces(data):
    """the entropy data of a single-scan stream that ends in EOI, unstuffed and split at its markers: what the GPU walk is handed, one
    byte string per restart interval"""
    _, j = _segments(data)
    out, cur = [], bytearray()
    while data[j:j + 2] != EOI:
        if data[j] == 0xFF and data[j + 1] == 0x00:
            cur.append(0xFF)
            j += 2
        elif data[j] == 0xFF:
            out.append(bytes(cur))
            cur = bytearray()
            j += 2
        else:
            cur.append(data[j])
            j += 1
    out.append(bytes(cur))
    return out


def predict_anomaly(data):
    """The anomaly word the GPU walk's rules give a stream the extract gate passes (status 1), from a plain sequential walk on the test
    side that states them as es_decode and k_es_dc do -- the kernels reach the same verdict in parallel, from guessed starts that have to
    converge.  Per restart interval (unstuffed bytes `piece`, nb bits, zero bits behind them):
      symbols are decoded while the bit position is in front of nb -- a symbol that starts in front of it is finished, nothing is started
      at or behind it; no code within 16 bits, or a DC category above 11: 1, the walk stops; a coefficient that would land behind index
      63: 1, and the block counts as complete; a block that completes behind nb: 16 (the data ran out inside it); the walk stops at the
      interval's last block and records the final position;
      fewer blocks than the interval holds: 4;
      the last interval: 32 if a 0xff byte lies behind the byte of the final position (position 0 where none was recorded); every other
      interval: 64 if the final position lies behind nb, or a byte or more in front of it."""
    segs, _ = _segments(data)
    comps, nmcu, dri = _frame(segs)
    tabs = _huff(segs[0xC4])
    sos = segs[0xDA][0]
    sel = {sos[1 + 2 * c]: (sos[2 + 2 * c] >> 4, sos[2 + 2 * c] & 15) for c in range(sos[0])}
    order = []
    for cid, h, v in comps:
        order += [sel[cid]] * (h * v)
    ps = pieces(data)
    word = 0
    for j, piece in enumerate(ps):
        nblocks = (min(dri, nmcu - j * dri) if dri else nmcu) * len(order)
        nb = 8 * len(piece)
        bits = "".join("{:08b}".format(b) for b in piece) + "0" * 64
        p, z, done, pfinal = 0, 0, 0, 0
        while p < nb and done < nblocks:
            td, ta = order[done % len(order)]
            t = tabs[(0, td)] if z == 0 else tabs[(1, ta)]
            sym = None
            for ln in range(1, 17):
                sym = t.get((ln, int(bits[p:p + ln], 2)))
                if sym is not None:
                    break
            if sym is None or (z == 0 and sym > 11):
                word |= 1
                break
            if z == 0:
                p += ln + sym
                z = 1
            elif (sym & 15) == 0:
                p += ln
                z = z + 16 if sym == 0xF0 else 64
            else:
                p += ln + (sym & 15)
                k = z + (sym >> 4)
                if k > 63:
                    word |= 1
                    z = 64
                else:
                    z = k + 1
            if z >= 64:
                z = 0
                if p > nb:
                    word |= 16
                done += 1
                if done == nblocks:
                    pfinal = p
        if done < nblocks:
            word |= 4
        if j == len(ps) - 1:
            if 0xFF in piece[(pfinal + 7) >> 3:]:
                word |= 32
        elif pfinal > nb or nb - pfinal >= 8:
            word |= 64
    return word


def block_ends(data):
    """A plain sequential walk of an INTACT baseline single-scan stream: -> [(segment bits, [end bit position of every block])] per restart
    interval (one entry without restart markers), positions counted in the unstuffed bytes of the interval.  Only the symbol lengths are
    followed; this is what the GPU tests predict the walk's completion rules from."""
    segs, i = _segments(data)
    comps, nmcu, dri = _frame(segs)
    tabs = _huff(segs[0xC4])
    sos = segs[0xDA][0]
    sel = {sos[1 + 2 * c]: (sos[2 + 2 * c] >> 4, sos[2 + 2 * c] & 15) for c in range(sos[0])}
    order = []
    for cid, h, v in comps:
        order += [sel[cid]] * (h * v)
    out, left = [], nmcu
    for piece in pieces(data):
        bits = "".join("{:08b}".format(b) for b in piece) + "0" * 64
        p, ends = 0, []

        def symbol(t):
            nonlocal p
            for ln in range(1, 17):
                s = t.get((ln, int(bits[p:p + ln], 2)))
                if s is not None:
                    p += ln
                    return s
            raise AssertionError("no code")

        for _ in range(min(left, dri) if dri else left):
            for td, ta in order:
                cat = symbol(tabs[(0, td)])  # (not p += symbol(...): the call moves p)
                p += cat
                k = 1
                while k < 64:
                    rs = symbol(tabs[(1, ta)])
                    if (rs & 15) == 0:
                        if rs != 0xF0:
                            break
                        k += 16
                        continue
                    k += (rs >> 4) + 1
                    p += rs & 15
                ends.append(p)
        left -= dri if dri else left
        out.append((8 * len(piece), ends))
    return out


def run_past_63_stream():
    """A grey 8x8 baseline stream made by hand whose only block runs past coefficient 63: a one-code DC table (category 0), an AC table of
    two two-bit codes (00: run 15 + a one-bit coefficient, 01: EOB), and the symbols DC, four times (run 15, +1), EOB.  The fourth run ends
    at index 64, where the reference writes through its padded de-zigzag table (codec/jpeg.c:304, :360) and stops."""
    dqt = b"\xff\xdb" + (67).to_bytes(2, "big") + b"\x00" + b"\x01" * 64
    sof = b"\xff\xc0" + (11).to_bytes(2, "big") + b"\x08" + (8).to_bytes(2, "big") + (8).to_bytes(2, "big") + b"\x01\x01\x11\x00"
    dc = b"\x00" + bytes([1] + [0] * 15) + b"\x00"
    ac = b"\x10" + bytes([0, 2] + [0] * 14) + b"\xf1\x00"
    dht = b"\xff\xc4" + (2 + len(dc) + len(ac)).to_bytes(2, "big") + dc + ac
    sos = b"\xff\xda" + (8).to_bytes(2, "big") + b"\x01\x01\x00\x00\x3f\x00"
    bits = "0" + "001" * 4 + "01"
    bits += "1" * (-len(bits) % 8)
    ent = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    assert 0xFF not in ent
    return b"\xff\xd8" + dqt + sof + dht + sos + ent + EOI
