"""Shared by the plane-encoding tests (include/mij_host.h, PLANE ENCODING): sizes, planes, views of them, and the values on which the
reference writer's luma is exact."""
import numpy as np

import sampling_cases as sc

SAMPLINGS = sc.SAMPLINGS
FACTORS = sc.FACTORS
# the strip of k_encode_planes per sampling, in MCUs (MIJ_ENCP_STRIP), and the MCU's size in pixels
STRIP = {"444": 64, "422": 64, "440": 64, "420": 32, "grey": 256}
MCU = {"444": (8, 8), "422": (16, 8), "440": (8, 16), "420": (16, 16), "grey": (8, 8)}
# one MCU more than the strip, two MCU rows high, odd width and height: the second strip starts one MCU before the end of the first MCU
# row and runs over it, the last strip is partial, and both edges replicate on luma and on chroma
SEAM_SIZE = {s: (STRIP[s] * MCU[s][0] + 3, MCU[s][1] + 5) for s in SAMPLINGS}
for _s in SAMPLINGS:
    assert -(-SEAM_SIZE[_s][0] // MCU[_s][0]) == STRIP[_s] + 1 and -(-SEAM_SIZE[_s][1] // MCU[_s][1]) == 2


def sizes(sampling):
    return sc.SMALL_SIZES + (SEAM_SIZE[sampling],)


def exact_luma_values():
    """the grey values v for which the reference writer's luma, 0.299f * v + 0.587f * v + 0.114f * v - 128 associated left to right
    (codec/jpeg_write.c:298), is exactly v - 128 in float32: on them a Y plane and a grey picture enter the fDCT with the same floats"""
    v = np.arange(256, dtype=np.float32)
    y = np.float32(0.299) * v + np.float32(0.587) * v
    y = y + np.float32(0.114) * v
    y = y - np.float32(128)
    assert y.dtype == np.float32
    return [int(k) for k in np.nonzero(y == v - np.float32(128))[0]]


def shapes(w, h, sampling):
    ncomp, lh, lv = FACTORS[sampling]
    return [(h, w)] + [(-(-h // lv), -(-w // lh))] * (ncomp - 1)


def planes(w, h, sampling, seed, values=None):
    """random-walk planes (smooth enough to leave zeros, rough enough to leave AC coefficients) -> [Y, Cb, Cr] or [Y]; values: draw the
    Y plane from this list instead"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (ph, pw) in enumerate(shapes(w, h, sampling)):
        y, x = np.mgrid[0:ph, 0:pw]
        base = (x * (5 + k) + y * (3 + 2 * k) + 60 * k) % 256
        p = np.clip(base + rng.integers(-24, 25, size=(ph, pw)), 0, 255).astype(np.uint8)
        if k == 0 and values is not None:
            p = np.asarray(values, np.uint8)[p.astype(np.int64) * len(values) // 256]
        out.append(p)
    return out


def arg(pl):
    """what the calls take: Y alone for grey"""
    return pl[0] if len(pl) == 1 else tuple(pl)


def views(pl, seed=0):
    """-> {name: picture}: the same samples through other layouts; every picture encodes to the bytes of `pl` (for "flipped": with
    flip_vertically).  NV12 / NV21 and packed need chroma (and packed 4:4:4 shapes)."""
    rng = np.random.default_rng(seed)
    out = {}
    wide = []
    for p in pl:  # a row pitch wider than the row, cut out of a larger array
        big = rng.integers(0, 256, size=(p.shape[0] + 5, p.shape[1] + 9), dtype=np.uint8)
        big[2:2 + p.shape[0], 3:3 + p.shape[1]] = p
        wide.append(big[2:2 + p.shape[0], 3:3 + p.shape[1]])
    out["cut"] = arg(wide)
    out["flipped"] = arg([np.ascontiguousarray(p[::-1]) for p in pl])
    if len(pl) == 3:
        nv12 = np.stack([pl[1], pl[2]], axis=-1)
        out["nv12"] = (pl[0], nv12)
        nv21 = np.ascontiguousarray(nv12[:, :, ::-1])
        out["nv21"] = (pl[0], nv21[:, :, 1], nv21[:, :, 0])
        pitched = np.zeros((nv12.shape[0], nv12.shape[1] + 4, 2), np.uint8)
        pitched[:, :nv12.shape[1]] = nv12
        out["nv12_pitched"] = (pl[0], pitched[:, :nv12.shape[1]])
        if pl[1].shape == pl[0].shape:
            hwc = np.stack(pl, axis=-1)  # packed YCbCr: x_pitch 3
            out["packed"] = (hwc[:, :, 0], hwc[:, :, 1], hwc[:, :, 2])
    return out


def video_range_luts():
    """the contract restated in numpy float32 -> (luma lut, chroma lut), uint8 [256] each"""
    x = np.arange(256, dtype=np.float32)
    out = []
    for scale, bias in ((255.0 / 219.0, -16.0 * 255.0 / 219.0), (255.0 / 224.0, 128.0 - 128.0 * 255.0 / 224.0)):
        t = x * np.float32(scale)
        t = t + np.float32(bias)
        assert t.dtype == np.float32
        out.append(np.rint(np.clip(t, np.float32(0), np.float32(255))).astype(np.uint8))
    return out


ONES = ([1] * 64, [1] * 64)
