"""A plain model of what the decode kernels compute from a block's coefficients, in numpy integers only (no ctypes, nothing of the
oracle's C): de-quantisation with its 16-bit wrap, the per-block L1 sum behind MIJ_FLAG_WIDE_IDCT (include/mij.h, MIJ_BLOCK_L1_LIMIT), the
reference's two-pass integer IDCT (codec/jpeg.c:560-680) in wrapping 32-bit arithmetic, the same transform with every first-pass output
cut to int16 (what the kernels' non-WIDE second pass works on), and the sparse class of a block (mij_kernels.h, "sparse blocks").

Blocks are arrays [..., 8, 8] in natural order (row, column) unless a function says zigzag."""
import numpy as np

L1_LIMIT = 5903  # MIJ_BLOCK_L1_LIMIT

# natural (row-major) position of every zigzag index
NAT_OF_ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57,
                      50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
ZZ_OF_NAT = np.argsort(NAT_OF_ZZ)


def zz_to_nat(zz):
    """[..., 64] in zigzag order -> [..., 8, 8] natural"""
    zz = np.asarray(zz)
    out = np.zeros(zz.shape, zz.dtype)
    out[..., NAT_OF_ZZ] = zz
    return out.reshape(zz.shape[:-1] + (8, 8))


def nat_to_zz(nat):
    nat = np.asarray(nat)
    return nat.reshape(nat.shape[:-2] + (64,))[..., NAT_OF_ZZ]


def _wrap32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _wrap16(x):
    return ((np.asarray(x, np.int64) + (1 << 15)) & 0xFFFF) - (1 << 15)


def dequant(coef, q):
    """(short)(coef * q): the 16-bit wrap of the product (codec/jpeg.c:325-365); coef and q broadcast, q up to 65535"""
    return _wrap16(np.asarray(coef, np.int64) * np.asarray(q, np.int64))


def block_l1(block, q):
    """sum of |(short)(coef * q)| over the 64 positions of each block ([..., 8, 8] or [..., 64]; q in the same order); |-32768| = 32768"""
    d = np.abs(dequant(block, q))
    if d.ndim >= 2 and d.shape[-1] == 8 and d.shape[-2] == 8:
        return d.sum(axis=(-1, -2))
    return d.sum(axis=-1)


def needs_wide(blocks, q):
    """the verdict every producer must reach: some block's L1 is above the limit"""
    l1 = block_l1(blocks, q)
    return bool(np.max(l1) > L1_LIMIT) if np.size(l1) else False


def _f2f(x):
    return int(float(np.float32(x)) * 4096 + 0.5)


_K = dict(c0541=_f2f(0.5411961), c1847=_f2f(-1.847759065), c0765=_f2f(0.765366865), c1175=_f2f(1.175875602), c0298=_f2f(0.298631336),
          c2053=_f2f(2.053119869), c3072=_f2f(3.072711026), c1501=_f2f(1.501321110), c0899=_f2f(-0.899976223), c2562=_f2f(-2.562915447),
          c1961=_f2f(-1.961570560), c0390=_f2f(-0.390180644))


def _idct_1d(s, bias):
    """the reference's 1-D kernel on s[0..7] (int64 arrays): -> the eight outputs before the shift, wrapped to 32 bits.  Sums and products
    only, so wrapping once at the end equals wrapping after every operation."""
    K = _K
    p2, p3 = s[2], s[6]
    p1 = (p2 + p3) * K["c0541"]
    t2 = p1 + p3 * K["c1847"]
    t3 = p1 + p2 * K["c0765"]
    p2, p3 = s[0], s[4]
    t0 = (p2 + p3) * 4096
    t1 = (p2 - p3) * 4096
    x0, x3, x1, x2 = t0 + t3 + bias, t0 - t3 + bias, t1 + t2 + bias, t1 - t2 + bias
    t0, t1, t2, t3 = s[7], s[5], s[3], s[1]
    p3, p4, p1, p2 = t0 + t2, t1 + t3, t0 + t3, t1 + t2
    p5 = (p3 + p4) * K["c1175"]
    t0 = t0 * K["c0298"]
    t1 = t1 * K["c2053"]
    t2 = t2 * K["c3072"]
    t3 = t3 * K["c1501"]
    p1 = p5 + p1 * K["c0899"]
    p2 = p5 + p2 * K["c2562"]
    p3 = p3 * K["c1961"]
    p4 = p4 * K["c0390"]
    t3 = t3 + p1 + p4
    t2 = t2 + p2 + p3
    t1 = t1 + p2 + p4
    t0 = t0 + p1 + p3
    return [_wrap32(v) for v in (x0 + t3, x1 + t2, x2 + t1, x3 + t0, x3 - t0, x2 - t1, x1 - t2, x0 - t3)]


def first_pass(block):
    """column pass: [..., 8, 8] de-quantised int16 values -> first-pass outputs v[row, column] (32-bit values, >> 10 done).  The reference's
    shortcut for a column with rows 1..7 zero (d[0] * 4) is the general formula on such a column, so it needs no branch here."""
    b = _wrap16(block)
    o = _idct_1d([b[..., r, :] for r in range(8)], 512)
    return np.stack([v >> 10 for v in o], axis=-2)


def _second_pass(v):
    o = _idct_1d([v[..., :, c] for c in range(8)], 65536 + (128 << 17))
    return np.clip(np.stack([x >> 17 for x in o], axis=-1), 0, 255).astype(np.uint8)


def idct_exact(block):
    """the reference's stbi__idct_block on de-quantised blocks [..., 8, 8]: -> uint8 [..., 8, 8]"""
    return _second_pass(first_pass(block))


def idct_narrow(block):
    """the same with every first-pass output cut to int16 before the second pass (v_dot2_i32_i16 reads 16-bit halves): what the kernels'
    non-WIDE path computes -- equal to idct_exact whenever the block's L1 is within the limit"""
    return _second_pass(_wrap16(first_pass(block)))


def first_pass_weights():
    """w[r_out, r_in]: weight of column input row r_in in first-pass output row r_out (before bias and shift)"""
    w = np.zeros((8, 8), np.int64)
    for r in range(8):
        s = [np.int64(1 if k == r else 0) for k in range(8)]
        w[:, r] = [int(v) for v in _idct_1d(s, 0)]
    return w


def block_class(block):
    """0: DC only; 1: every non-zero AC inside the top-left 2x2; 2: inside the 4x4; 3: anything else ([..., 8, 8] natural, quantised)"""
    nz = np.asarray(block) != 0
    out4 = nz[..., 4:, :].any(axis=(-1, -2)) | nz[..., :, 4:].any(axis=(-1, -2))
    out2 = nz[..., 2:, :].any(axis=(-1, -2)) | nz[..., :, 2:].any(axis=(-1, -2))
    ac = nz.reshape(nz.shape[:-2] + (64,))[..., 1:].any(axis=-1)
    return np.where(out4, 3, np.where(out2, 2, np.where(ac, 1, 0)))


def escaped(block):
    """the block holds a quantised AC coefficient outside a byte (compact planes: such a block is class 3 whatever its extent)"""
    b = np.asarray(block, np.int64).reshape(np.shape(block)[:-2] + (64,))[..., 1:]
    return ((b < -128) | (b > 127)).any(axis=-1)
