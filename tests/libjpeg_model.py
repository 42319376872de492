"""The LIBJPEG ARITHMETIC contract (include/mij.h, mij_batch_set_arith) in numpy integers: libjpeg's default decode --
ISLOW inverse DCT (jidctint.c), fancy upsampling (jdsample.c), the jdcolor tables -- restated from the formulas, the normative model
the kernels (mij_libjpeg_kernels.h) are tested against.  tests/golden/libjpeg_pillow.npz holds Pillow's pixels for the same files:
test_libjpeg_model_host.py checks this model against them, so the formulas here are the contract and Pillow is the judge.

Input: quantised coefficients c[u][v] and tables q[u][v] in natural order.  All arithmetic is 32-bit two's-complement and wrapping
(int64 here, wrapped after every step that can leave 32 bits); shifts are arithmetic."""
import numpy as np


def wrap32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def idct_1d(s):
    """jidctint.c's 1-D transform on the list s[0..7] of int64 arrays (32-bit values) -> the eight outputs, wrapped, not descaled"""
    w = wrap32
    s0, s1, s2, s3, s4, s5, s6, s7 = s
    z1 = w(w(s2 + s6) * 4433)
    t2 = w(z1 - w(s6 * 15137))
    t3 = w(z1 + w(s2 * 6270))
    t0 = w(w(s0 + s4) << 13)
    t1 = w(w(s0 - s4) << 13)
    e0, e3, e1, e2 = w(t0 + t3), w(t0 - t3), w(t1 + t2), w(t1 - t2)
    a, b, c, d = s7, s5, s3, s1
    z1, z2, z3, z4 = w(a + d), w(b + c), w(a + c), w(b + d)
    z5 = w(w(z3 + z4) * 9633)
    a, b, c, d = w(a * 2446), w(b * 16819), w(c * 25172), w(d * 12299)
    z1, z2 = w(z1 * -7373), w(z2 * -20995)
    z3, z4 = w(w(z3 * -16069) + z5), w(w(z4 * -3196) + z5)
    a, b, c, d = w(a + w(z1 + z3)), w(b + w(z2 + z4)), w(c + w(z2 + z3)), w(d + w(z1 + z4))
    return [w(e0 + d), w(e1 + c), w(e2 + b), w(e3 + a), w(e3 - a), w(e2 - b), w(e1 - c), w(e0 - d)]


def idct_blocks(c, q):
    """c: quantised coefficients [..., 8, 8] (natural order: [u][v], u down the rows), q: the table [8, 8] -> uint8 samples [..., 8, 8]"""
    d = wrap32(np.asarray(c, np.int64) * np.asarray(q, np.int64))  # the 32-bit product
    cols = idct_1d([d[..., u, :] for u in range(8)])                # down the columns: one array [..., 8 columns] per output row
    ws = np.stack([wrap32(x + 1024) >> 11 for x in cols], axis=-2)  # the workspace [..., row, column]
    rows = idct_1d([ws[..., :, v] for v in range(8)])               # along the rows: one array [..., 8 rows] per output column
    out = np.stack([wrap32(x + 131072) >> 18 for x in rows], axis=-1)
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def component_plane(c, q, pw, ph):
    """[bh, bw, 8, 8] -> the component's ph x pw samples: those of the padding blocks and columns beyond are never anybody's neighbours"""
    s = idct_blocks(c, q)
    bh, bw = s.shape[:2]
    return s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:ph, :pw]


def _nb(p, axis, step):
    """p shifted by one along axis with the edge clamped: p[i + step]"""
    n = p.shape[axis]
    idx = np.clip(np.arange(n) + step, 0, n - 1)
    return np.take(p, idx, axis=axis)


def _interleave(even, odd, axis):
    shape = list(even.shape)
    shape[axis] *= 2
    out = np.empty(shape, np.int64)
    sl = [slice(None)] * even.ndim
    sl[axis] = slice(0, None, 2)
    out[tuple(sl)] = even
    sl[axis] = slice(1, None, 2)
    out[tuple(sl)] = odd
    return out


def upsample(p, hs, vs):
    """a chroma plane [ph, pw] -> [ph * vs, pw * hs] by jdsample.c's fancy upsampling; hs, vs in (1, 2)"""
    p = np.asarray(p, np.int64)
    pw = p.shape[1]
    if hs == 1 and vs == 1:
        return p
    if hs == 2 and pw <= 2:  # libjpeg's small-width rule: h2v1 and h2v2 replicate, unfiltered
        return np.repeat(np.repeat(p, vs, axis=0), 2, axis=1)
    if hs == 2 and vs == 1:
        return _interleave((3 * p + _nb(p, 1, -1) + 1) >> 2, (3 * p + _nb(p, 1, 1) + 2) >> 2, 1)
    if hs == 1 and vs == 2:
        return _interleave((3 * p + _nb(p, 0, -1) + 1) >> 2, (3 * p + _nb(p, 0, 1) + 2) >> 2, 0)
    assert hs == 2 and vs == 2
    s = _interleave(3 * p + _nb(p, 0, -1), 3 * p + _nb(p, 0, 1), 0)  # vertical sums, unshifted
    return _interleave((3 * s + _nb(s, 1, -1) + 8) >> 4, (3 * s + _nb(s, 1, 1) + 7) >> 4, 1)


def ycc_to_rgb(y, cb, cr):
    """jdcolor.c, SCALEBITS 16 -> uint8 [..., 3]"""
    y, cb, cr = np.asarray(y, np.int64), np.asarray(cb, np.int64) - 128, np.asarray(cr, np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def picture(planes, tables, factors, size, n_out):
    """planes: per component the quantised coefficients [bh, bw, 8, 8]; tables: per component its [8, 8] table; factors: per component
    (h, v); size (W, H); n_out 1..4 -> uint8 [H, W, n_out].  One component: its samples, replicated for n_out >= 3; three components:
    R, G, B (, 255), or Y alone (, 255) for n_out < 3."""
    w, h = size
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    use = 1 if (len(factors) == 1 or n_out < 3) else 3
    comp = []
    for c in range(use):
        fh, fv = factors[c]
        pw, ph = -(-w * fh // hmax), -(-h * fv // vmax)
        p = component_plane(planes[c], tables[c], pw, ph)
        assert hmax % fh == 0 and vmax % fv == 0 and hmax // fh in (1, 2) and vmax // fv in (1, 2), "layout not served"
        comp.append(upsample(p, hmax // fh, vmax // fv)[:h, :w])
        assert comp[-1].shape == (h, w)
    out = np.empty((h, w, n_out), np.uint8)
    if use == 1:
        out[..., :3 if n_out >= 3 else 1] = comp[0][..., None].astype(np.uint8)
    else:
        out[..., :3] = ycc_to_rgb(comp[0], comp[1], comp[2])
    if n_out in (2, 4):
        out[..., n_out - 1] = 255
    return out


def coefficients(data):
    """a JPEG file -> (planes, tables, factors, (W, H)) through the library's host Huffman walk (no GPU): what picture() takes"""
    import image_codecs_amd as ica

    d, arena = ica.HostDecoder.decode(data, 0)
    planes = ica.detile_coefficients(d, arena)
    tables = [np.array(d.dequant[d.comp[c].tq][:], np.int64).reshape(8, 8) for c in range(d.ncomp)]
    factors = [(int(d.comp[c].h), int(d.comp[c].v)) for c in range(d.ncomp)]
    return planes, tables, factors, (int(d.width), int(d.height))


def decode(data, n_out=3):
    """a grey or YCbCr JPEG file -> uint8 [H, W, n_out]: what libjpeg's default decode gives (Pillow's convert("RGB"), or "L")"""
    planes, tables, factors, size = coefficients(data)
    return picture(planes, tables, factors, size, n_out)
