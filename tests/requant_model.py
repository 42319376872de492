"""The requantising transcode's rule (include/mij_host.h, mjw_tplan_requant / mjw_units_requant) restated in numpy, without the library:
destination tables, the rounding of one coefficient, units and planes, and the writer's quality tables from their formula."""
import numpy as np

import transcode_model as model

# Annex K tables in natural (row-major) order, as stbi_write_jpg holds them
K_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
          103, 99)
K_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + \
    (99,) * 32


def quality_tables(q):
    """(luma, chroma) in zigzag order at quality 1..100: scale = 5000 / q below 50 and 200 - 2q from there, (base * scale + 50) / 100
    in integers, clamped to 1..255"""
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    out = []
    for base in (K_LUMA, K_CHROMA):
        nat = np.clip((np.array(base, np.int64) * scale + 50) // 100, 1, 255)
        out.append(nat[model.ZIGZAG_NATURAL].astype(np.uint8))
    return tuple(out)


def dest_tables(s, t, coarsen_only=True):
    """d of source tables s = (luma, chroma) and targets t, entry by entry"""
    s = [np.asarray(x, np.int64) for x in s]
    t = [np.asarray(x, np.int64) for x in t]
    return tuple((np.maximum(a, b) if coarsen_only else b).astype(np.uint8) for a, b in zip(s, t))


def requant(c, a, b):
    """y of the rule for values c (any shape) and steps a, b (broadcast): magnitudes, // on them, halves away from zero, the int16 clamp"""
    x = np.asarray(c, np.int64) * np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    y = np.sign(x) * ((np.abs(x) + (b >> 1)) // b)
    return np.clip(y, -32767, 32767).astype(np.int16)


def requant_units(units, ny, dpm, s, d):
    """units [n_du, 64] in MCU order, the first ny of every dpm being luma -> the destination's; s, d = (luma, chroma) zigzag tables"""
    units = np.asarray(units, np.int16).reshape(-1, 64)
    chroma = (np.arange(units.shape[0]) % dpm) >= ny
    a = np.where(chroma[:, None], np.asarray(s[1], np.int64)[None], np.asarray(s[0], np.int64)[None])
    b = np.where(chroma[:, None], np.asarray(d[1], np.int64)[None], np.asarray(d[0], np.int64)[None])
    return requant(units, a, b)


def requant_planes(planes, s, d):
    """planes [bh, bw, 64] per component in zigzag order (luma first) -> the destination's"""
    return [requant(p, s[0 if c == 0 else 1], d[0 if c == 0 else 1]) for c, p in enumerate(planes)]
