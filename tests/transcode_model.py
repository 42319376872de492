"""The lossless transcode's contract restated in numpy, independent of the C code (include/mij_host.h, mjw_tplan): which unit of the
writer's order holds which coefficient of the decoder's planes, and where copied marker segments go."""
import numpy as np

# zigzag index k -> natural index 8 * row + col (ITU-T T.81 figure A.6)
ZIGZAG_NATURAL = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def units_from_planes(desc, planes):
    """planes: per component an array [bh, bw, 8, 8] in natural (row, col) order, as detile_coefficients gives them.
    -> int16 [n_du, 64]: MCU after MCU in raster order; inside an MCU the luma blocks in raster order, then Cb, then Cr; zigzag order."""
    out = []
    for my in range(desc.mcu_y):
        for mx in range(desc.mcu_x):
            for c in range(desc.ncomp):
                h, v = desc.comp[c].h, desc.comp[c].v
                for sy in range(v):
                    for sx in range(h):
                        out.append(np.asarray(planes[c][my * v + sy, mx * h + sx]).reshape(64)[ZIGZAG_NATURAL])
    return np.stack(out).astype(np.int16)


def blocks_in_planes(desc, planes):
    """the blocks of every component as [bh, bw, 64] in zigzag order: what two streams with the same coefficients agree on"""
    return [np.asarray(planes[c]).reshape(desc.comp[c].bh, desc.comp[c].bw, 64)[:, :, ZIGZAG_NATURAL] for c in range(desc.ncomp)]


def codable(desc, units):
    """every AC in -1023..1023 and every DC difference, against the previous unit of the component in MCU order, in -2047..2047"""
    units = np.asarray(units, np.int64)
    if np.abs(units[:, 1:]).max(initial=0) > 1023:
        return False
    ny = 1 if desc.ncomp == 1 else desc.comp[0].h * desc.comp[0].v
    dpm = ny if desc.ncomp == 1 else ny + 2
    comp = np.array([0] * ny + [1, 2][:dpm - ny])
    which = comp[np.arange(len(units)) % dpm]
    for c in range(desc.ncomp):
        dc = units[which == c, 0]
        if np.abs(np.diff(np.concatenate([[0], dc]))).max(initial=0) > 2047:
            return False
    return True


def segments(data):
    """[(marker, start, end)] of the marker segments between SOI and the first SOS; None for a malformed or truncated length"""
    out, i = [], 2
    while True:
        if i + 2 > len(data) or data[i] != 0xFF:
            return None
        m = data[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m == 0xDA:
            return out
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            i += 2
            continue
        if m in (0xD9, 0x00) or i + 4 > len(data):
            return None
        n = (data[i + 2] << 8) | data[i + 3]
        if n < 2 or i + 2 + n > len(data):
            return None
        out.append((m, i, i + 2 + n))
        i += 2 + n


def splice_markers(src, stream):
    """`stream` as the writer emitted it (SOI, its 18-byte JFIF APP0, the rest) with the source's APPn and COM segments behind SOI, in
    source order; the writer's APP0 stays, in front of them, unless the source has a JFIF APP0 or an Adobe APP14.  None: refused."""
    segs = segments(src)
    if segs is None or src[:2] != b"\xff\xd8":
        return None
    kept = [src[a:b] for m, a, b in segs if 0xE0 <= m <= 0xEF or m == 0xFE]
    own = not any((s[1] == 0xE0 and s[4:9] == b"JFIF\0") or (s[1] == 0xEE and s[4:9] == b"Adobe") for s in kept)
    assert stream[2:4] == b"\xff\xe0" and stream[4:6] == b"\x00\x10"
    return stream[:2] + (stream[2:20] if own else b"") + b"".join(kept) + stream[20:]
