"""PLANE OUTPUT (include/mij.h) restated without product code: the planes of a picture's stored components from its de-quantised blocks
through the checker's IDCT (helpers.Oracle.idct: the reference's stbi__idct_block, clamp included), cropped to pw_c x ph_c and to a window.

Blocks come from coef_cases.Case.dequantised() for synthetic pictures and, for real files, from Oracle.coef(data): the de-quantised
blocks in the order the reference transforms them (helpers._dequantised_in_call_order shows that order) -- MCU by MCU for a baseline
file of several components, plane by plane over the blocks that hold picture, (y + 7) >> 3 rows of (x + 7) >> 3, for a file of one
component and for a progressive file."""
import numpy as np


def frame(data):
    """the frame header of a stream -> (W, H, [(h, v) per component], progressive)"""
    data = bytes(data)
    i = 2
    while i + 4 <= len(data):
        assert data[i] == 0xFF, "marker expected at %d" % i
        m = data[i + 1]
        if m == 0xFF:
            i += 1
            continue
        n = (data[i + 2] << 8) | data[i + 3]
        if m in (0xC0, 0xC1, 0xC2):
            seg = data[i + 4:i + 2 + n]
            h, w, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            return w, h, [(seg[6 + 3 * c + 1] >> 4, seg[6 + 3 * c + 1] & 15) for c in range(nc)], m == 0xC2
        i += 2 + n
    raise AssertionError("no frame header")


def geometry(w, h, hv):
    """-> (h_max, v_max, mcu_x, mcu_y)"""
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    return hmax, vmax, -(-w // (8 * hmax)), -(-h // (8 * vmax))


def shapes(w, h, hv):
    """[(ph_c, pw_c)]: pw_c = ceil(W * h_c / h_max), ph_c = ceil(H * v_c / v_max)"""
    hmax, vmax, _, _ = geometry(w, h, hv)
    return [(-(-h * b // vmax), -(-w * a // hmax)) for a, b in hv]


def on_grid(w, h, hv, window, comps):
    """whether the window's origin is a multiple of h_max / h_c and v_max / v_c for every component of comps"""
    hmax, vmax, _, _ = geometry(w, h, hv)
    return all((window[0] * hv[c][0]) % hmax == 0 and (window[1] * hv[c][1]) % vmax == 0 for c in comps)


def rect(w, h, hv, c, window=None):
    """(x0, y0, w, h) of the picture window in component c's own samples"""
    hmax, vmax, _, _ = geometry(w, h, hv)
    x0, y0, ww, wh = (0, 0, w, h) if window is None else window
    a, b = hv[c]
    assert (x0 * a) % hmax == 0 and (y0 * b) % vmax == 0, "window off the grid of component %d" % c
    sx0, sy0 = x0 * a // hmax, y0 * b // vmax
    return sx0, sy0, -(-(x0 + ww) * a // hmax) - sx0, -(-(y0 + wh) * b // vmax) - sy0


class Idct:
    """Oracle.idct with a memo: pictures repeat blocks (flat areas, padding)"""

    def __init__(self, oracle):
        self.oracle, self.memo = oracle, {}

    def __call__(self, block):
        b = np.ascontiguousarray(block, np.int16).reshape(64)
        k = b.tobytes()
        if k not in self.memo:
            self.memo[k] = self.oracle.idct(b).reshape(8, 8)
        return self.memo[k]


def planes_from_blocks(oracle, blocks, w, h, hv):
    """blocks: per component an array [rows, columns, 8, 8] of de-quantised coefficients in natural order that covers at least the blocks
    holding picture -> [plane of ph_c x pw_c]"""
    idct = oracle if isinstance(oracle, Idct) else Idct(oracle)
    out = []
    for (ph, pw), blk in zip(shapes(w, h, hv), blocks):
        nby, nbx = (ph + 7) >> 3, (pw + 7) >> 3
        full = np.zeros((8 * nby, 8 * nbx), np.uint8)
        for by in range(nby):
            for bx in range(nbx):
                full[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = idct(np.asarray(blk[by, bx]).astype(np.int64).astype(np.int16))
        out.append(np.ascontiguousarray(full[:ph, :pw]))
    return out


def blocks_of_call_order(flat, w, h, hv, progressive):
    """Oracle.coef's blocks (int16, 64 each, natural order) -> per component [rows, columns, 8, 8] over the blocks that hold picture"""
    hmax, vmax, mcu_x, mcu_y = geometry(w, h, hv)
    flat = np.asarray(flat, np.int16).reshape(-1, 8, 8)
    sh = shapes(w, h, hv)
    out = [np.zeros(((ph + 7) >> 3, (pw + 7) >> 3, 8, 8), np.int16) for ph, pw in sh]
    k = 0
    if progressive or len(hv) == 1:
        for c in range(len(hv)):
            for by in range(out[c].shape[0]):
                for bx in range(out[c].shape[1]):
                    out[c][by, bx] = flat[k]
                    k += 1
    else:
        for my in range(mcu_y):
            for mx in range(mcu_x):
                for c, (a, b) in enumerate(hv):
                    for y in range(b):
                        for x in range(a):
                            by, bx = my * b + y, mx * a + x
                            if by < out[c].shape[0] and bx < out[c].shape[1]:
                                out[c][by, bx] = flat[k]
                            k += 1
    assert k == flat.shape[0], (k, flat.shape)
    return out


def planes_of_case(oracle, case, hv):
    """a coef_cases.Case -> its planes"""
    return planes_from_blocks(oracle, case.dequantised(), case.w, case.h, hv)


def planes_of_stream(oracle, data):
    """a real file -> (planes, (W, H, hv, progressive))"""
    w, h, hv, prog = frame(data)
    orc = oracle.oracle if isinstance(oracle, Idct) else oracle
    return planes_from_blocks(oracle, blocks_of_call_order(orc.coef(data), w, h, hv, prog), w, h, hv), (w, h, hv, prog)


def window_of(planes, w, h, hv, window=None, comps=None):
    """{c: the part of plane c the window holds} for the wanted components"""
    out = {}
    for c in (range(len(planes)) if comps is None else comps):
        x0, y0, ww, wh = rect(w, h, hv, c, window)
        out[c] = planes[c][y0:y0 + wh, x0:x0 + ww]
    return out
