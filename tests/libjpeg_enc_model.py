"""The LIBJPEG ENCODING contract (include/mij_host.h) in numpy integers: libjpeg's default compression -- the jccolor
constants, the jcsample chroma filter with its edge rules, the ISLOW forward DCT (jfdctint.c), the quantiser and the DC of dummy
blocks -- restated from the formulas, the normative model the host twin (mjw_lj_transform_host) and the kernels
(mij_libjpeg_enc_kernels.h) are tested against.  tests/golden/libjpeg_pillow_enc.npz holds Pillow's files for the same pictures:
test_encode_libjpeg_host.py checks this model against their coefficients, so the formulas here are the contract and Pillow is the judge.

All arithmetic is integer (int64 here; nothing leaves 32 bits) and every shift is arithmetic."""
import numpy as np

SAMPLING = {"444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2), "grey": (1, 1, 1)}

K_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def zigzag_positions():
    """natural position (8 * row + column) of zigzag index k"""
    order = sorted(range(64), key=lambda p: (p // 8 + p % 8, (p // 8) if (p // 8 + p % 8) % 2 else (p % 8)))
    return np.array(order)


ZIGZAG = zigzag_positions()


def quality_tables(quality):
    """libjpeg's jpeg_set_quality (force_baseline) -> (luma, chroma), 64 entries each in natural order"""
    quality = min(max(int(quality), 1), 100)
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((np.array(t, np.int64) * scale + 50) // 100, 1, 255) for t in (K_LUMA, K_CHROMA))


def rgb_to_ycc(rgb):
    """jccolor.c, 16 fraction bits: uint8 [..., 3] -> Y, Cb, Cr as int64"""
    r, g, b = (np.asarray(rgb[..., c], np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _extend(p, rows, cols):
    """p with its last row and last column repeated up to rows x cols"""
    h, w = p.shape
    return np.pad(p, ((0, rows - h), (0, cols - w)), mode="edge")


def downsample(p, lh, lv):
    """jcsample.c on a plane whose width is whole MCUs and whose height is a multiple of lv; the bias follows the OUTPUT column"""
    p = np.asarray(p, np.int64)
    if lh == 1 and lv == 1:
        return p
    x = np.arange(p.shape[1] // 2) & 1
    if lv == 1:
        return (p[:, 0::2] + p[:, 1::2] + x) >> 1
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + x) >> 2


def sample_planes(ycc, width, height, sampling):
    """the component planes as the forward DCT sees them: whole MCUs both ways.  ycc: the [height, width] planes Y (, Cb, Cr)"""
    ncomp, lh, lv = SAMPLING[sampling]
    mcu_x, mcu_y = -(-width // (8 * lh)), -(-height // (8 * lv))
    out = [_extend(np.asarray(ycc[0], np.int64), mcu_y * 8 * lv, mcu_x * 8 * lh)]
    for c in range(1, ncomp):
        rows = -(-height // lv) * lv  # the pixel rows to a multiple of lv, then the filter, then the last SAMPLE row repeated
        s = downsample(_extend(np.asarray(ycc[c], np.int64), rows, mcu_x * 8 * lh), lh, lv)
        out.append(_extend(s, mcu_y * 8, mcu_x * 8))
    return out


def D(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_1d(d, first):
    """jfdctint.c's pass over the list d[0..7]: first (rows) scales up by 4, the second (columns) descales"""
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else D(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else D(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = D(z1 + t13 * 6270, n)
    o[6] = D(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = D(t4 + z1 + z3, n), D(t5 + z2 + z4, n), D(t6 + z2 + z3, n), D(t7 + z1 + z4, n)
    return o


def fdct_blocks(s):
    """samples [..., 8, 8] -> coefficients [..., 8, 8] (natural order, scaled by 8 as jfdctint leaves them)"""
    d = np.asarray(s, np.int64) - 128
    r = np.stack(fdct_1d([d[..., :, k] for k in range(8)], True), axis=-1)    # along every row
    return np.stack(fdct_1d([r[..., k, :] for k in range(8)], False), axis=-2)  # down every column


def quantise(x, q):
    """y = sign(x) * ((|x| + 4q) div 8q), q the table entry"""
    x, q = np.asarray(x, np.int64), np.asarray(q, np.int64)
    return np.sign(x) * ((np.abs(x) + 4 * q) // (8 * q))


def component_coefficients(planes, tables, width, height, sampling):
    """the quantised coefficients of every component, [block rows, block columns, 8, 8] natural order over the whole-MCU grid, dummy
    luma blocks included"""
    ncomp, lh, lv = SAMPLING[sampling]
    out = []
    for c, p in enumerate(planes):
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        blocks = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        out.append(quantise(fdct_blocks(blocks), np.asarray(tables[min(c, 1)], np.int64).reshape(8, 8)))
    if ncomp == 3 and (lh > 1 or lv > 1):
        y, rw, rh = out[0], -(-width // 8), -(-height // 8)
        for by in range(y.shape[0]):
            for bx in range(y.shape[1]):
                if bx < rw and by < rh:
                    continue
                if by < rh:  # a real block row: the block to the left
                    dc = y[by, bx - 1, 0, 0]
                else:        # a row below the picture: the last block of the MCU's previous block row
                    dc = y[by - 1, bx // lh * lh + lh - 1, 0, 0]
                y[by, bx] = 0
                y[by, bx, 0, 0] = dc
    return out


def units_of(coefs, sampling):
    """component coefficients -> int16 [units, 64] in zigzag order, mjw_tplan's unit order"""
    ncomp, lh, lv = SAMPLING[sampling]
    mcu_y, mcu_x = coefs[-1].shape[0] // (lv if ncomp == 1 else 1), coefs[-1].shape[1] // (lh if ncomp == 1 else 1)
    du = []
    for my in range(mcu_y):
        for mx in range(mcu_x):
            for sy in range(lv):
                for sx in range(lh):
                    du.append(coefs[0][my * lv + sy, mx * lh + sx].reshape(64)[ZIGZAG])
            for c in range(1, ncomp):
                du.append(coefs[c][my, mx].reshape(64)[ZIGZAG])
    return np.array(du, np.int16)


def tables_of(quality=None, qtables=None):
    """(luma, chroma) in natural order: those of a quality, or the given pair (64 entries each in ZIGZAG order, as DQT carries them)"""
    if qtables is None:
        return quality_tables(quality)
    out = []
    for t in qtables:
        n = np.empty(64, np.int64)
        n[ZIGZAG] = np.asarray(t, np.int64).reshape(64)
        out.append(n)
    return tuple(out)


def coefficients(pixels, sampling, quality=None, qtables=None, ycbcr=False):
    """uint8 pixels [H, W, 3] (RGB, or YCbCr with ycbcr=True) or [H, W] (grey) -> component_coefficients"""
    pixels = np.asarray(pixels)
    h, w = pixels.shape[:2]
    if pixels.ndim == 2:
        ycc = [pixels.astype(np.int64)] * 3
    elif ycbcr:
        ycc = [pixels[..., c].astype(np.int64) for c in range(3)]
    else:
        ycc = rgb_to_ycc(pixels)
    planes = sample_planes(ycc, w, h, sampling)
    return component_coefficients(planes, tables_of(quality, qtables), w, h, sampling)


def units(pixels, sampling, quality=None, qtables=None, ycbcr=False):
    return units_of(coefficients(pixels, sampling, quality, qtables, ycbcr), sampling)
