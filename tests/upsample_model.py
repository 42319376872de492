"""The reference's output stage (load_jpeg_image, codec/jpeg.c:2241-2430) from sample planes to pixels, in numpy integers only: the row
scheduler, the five resamplers with their first, last and last-but-one forms, and every colour branch with channel replication and alpha.
It is the normative restatement the upsampling kernels (mij_kernels.h: fused_band, fused422_band, k_resample_fast, k_resample_color) are
tested against, as idct_model.py is for the transform, scaled_model.py for the reduced-size decode and resize_model.py for the resize.

A picture's component c with sampling factors (h, v) under (h_max, v_max) has hs = h_max // h, vs = v_max // v, the padded plane
uint8 [bh * 8, bw * 8], w_lores = ceil(W / hs) samples per row that the resampler reads and comp.y = ceil(H * v / v_max) effective rows.
The reference never reads a row at or beyond comp.y and, in the interpolating resamplers, never a column at or beyond w_lores: the MCU
padding behind them is in the stream and in the plane, and is not part of the picture.

BLUNDERS are four ways of getting that wrong which an encoder-made picture cannot show (tests/test_upsample_host.py); the model makes
them on request so that the test inputs can be shown to expose them.  blunder = 0 is the reference."""
import numpy as np

import idct_model as M

NEAR_FAR_SWAPPED, WRONG_SIDE, NO_RIGHT_CLAMP, NO_BOTTOM_CLAMP = 1, 2, 3, 4
BLUNDERS = (NEAR_FAR_SWAPPED, WRONG_SIDE, NO_RIGHT_CLAMP, NO_BOTTOM_CLAMP)


def colour_tag(ncomp, app14):
    """the colour branch of a stream of the test-side writer (no JFIF segment, component ids 1..n): codec/jpeg.c:2244 and :2323-2371"""
    if ncomp == 1:
        return "grey"
    if ncomp == 3:
        return "rgb" if app14 == 0 else "ycc"
    return {0: "cmyk", 2: "ycck"}.get(app14, "ycca")


def ycbcr_to_rgb(y, cb, cr):
    """the reference's stbi__YCbCr_to_RGB_row per pixel (codec/jpeg.c:1976-2018): uint8 arrays -> [..., 3]"""
    f = lambda x: int(np.float32(x) * np.float32(4096.0) + np.float32(0.5)) << 8  # stbi__float2fixed
    yf = (y.astype(np.int64) << 20) + (1 << 19)
    cr, cb = cr.astype(np.int64) - 128, cb.astype(np.int64) - 128
    r = yf + cr * f(1.40200)
    g = yf + cr * -f(0.71414) + ((cb * -f(0.34414)) & -65536)  # "& 0xffff0000" on a 32-bit int keeps the sign bits
    b = yf + cb * f(1.77200)
    return np.stack([np.clip(v >> 20, 0, 255) for v in (r, g, b)], axis=-1).astype(np.uint8)


def blinn8(x, y):
    """stbi__blinn_8x8 (codec/jpeg.c:2218-2222): 0..255 * 0..255 -> 0..255, rounded"""
    t = np.asarray(x, np.int64) * np.asarray(y, np.int64) + 128
    return ((t + (t >> 8)) >> 8).astype(np.uint8)


def compute_y(r, g, b):
    """stbi__compute_y (common.c:173-176)"""
    return ((np.asarray(r, np.int64) * 77 + np.asarray(g, np.int64) * 150 + np.asarray(b, np.int64) * 29) >> 8).astype(np.uint8)


# ---------------------------------------------------------------- the row scheduler

def schedule(H, vs, comp_y, rows, blunder=0):
    """-> (near[H], far[H]): the plane rows the reference hands its resampler as in_near and in_far for every output row
    (codec/jpeg.c:2273-2278, :2301-2318).  ystep starts at vs >> 1; a row is "bottom" when ystep >= vs >> 1 and then takes line1 as near;
    after vs rows line0 becomes line1, and line1 moves on only while ++ypos < comp.y -- it never passes row comp.y - 1.
    NO_BOTTOM_CLAMP: line1 always moves on (within the `rows` the padded plane has)."""
    near, far = np.empty(H, np.int64), np.empty(H, np.int64)
    ystep, ypos, line0, line1 = vs >> 1, 0, 0, 0
    for j in range(H):
        bot = ystep >= (vs >> 1)
        near[j], far[j] = (line1, line0) if bot else (line0, line1)
        ystep += 1
        if ystep >= vs:
            ystep = 0
            line0 = line1
            ypos += 1
            if ypos < comp_y or (blunder == NO_BOTTOM_CLAMP and line1 + 1 < rows):
                line1 += 1
    return (far, near) if blunder == NEAR_FAR_SWAPPED else (near, far)


# ---------------------------------------------------------------- the resamplers, on all rows at once: near, far int64 [H, w]

def resample_row_1(near, far, w, hs):
    return near


def resample_row_v_2(near, far, w, hs):
    return (3 * near + far + 2) >> 2


def resample_row_h_2(near, far, w, hs):
    """codec/jpeg.c:1784-1812.  w == 1: both outputs are the sample.  Else the first output is sample 0, the last sample w - 1, the
    interior 3 : 1 towards the nearer neighbour -- and the last but one, pixel 2 (w - 1), is 3 * in[w - 2] + in[w - 1]: three parts of the
    NEIGHBOUR, unlike every other even pixel."""
    out = np.empty(near.shape[:-1] + (2 * w,), np.int64)
    if w == 1:
        out[..., 0] = out[..., 1] = near[..., 0]
        return out
    out[..., 0] = near[..., 0]
    out[..., 1] = (near[..., 0] * 3 + near[..., 1] + 2) >> 2
    n = 3 * near[..., 1:w - 1] + 2
    out[..., 2:2 * w - 2:2] = (n + near[..., 0:w - 2]) >> 2
    out[..., 3:2 * w - 2:2] = (n + near[..., 2:w]) >> 2
    out[..., 2 * w - 2] = (near[..., w - 2] * 3 + near[..., w - 1] + 2) >> 2
    out[..., 2 * w - 1] = near[..., w - 1]
    return out


def resample_row_hv_2(near, far, w, hs):
    """codec/jpeg.c:1816-1840 (and its SIMD twin :1843-1959, which computes the same)"""
    t = 3 * near[..., :w] + far[..., :w]
    out = np.empty(t.shape[:-1] + (2 * w,), np.int64)
    out[..., 0] = (t[..., 0] + 2) >> 2
    out[..., 2 * w - 1] = (t[..., w - 1] + 2) >> 2
    if w > 1:
        out[..., 1:2 * w - 1:2] = (3 * t[..., :w - 1] + t[..., 1:] + 8) >> 4
        out[..., 2:2 * w - 1:2] = (3 * t[..., 1:] + t[..., :w - 1] + 8) >> 4
    return out


def resample_row_generic(near, far, w, hs):
    return np.repeat(near[..., :w], hs, axis=-1)


def _wrong_side(kind, near, far, w):
    """WRONG_SIDE: every pixel x of sample i = x >> 1 leans on sample i + 1 where the reference takes i - 1 and the other way round
    (clamped to the row), three parts of its own sample throughout"""
    x = np.arange(2 * w)
    i = x >> 1
    n = np.clip(np.where(x & 1, i - 1, i + 1), 0, w - 1)
    if kind == "h_2":
        return np.where(n == i, near[..., i], (3 * near[..., i] + near[..., n] + 2) >> 2)
    t = 3 * near[..., :w] + far[..., :w]
    return (3 * t[..., i] + t[..., n] + 8) >> 4


RESAMPLERS = {"row_1": resample_row_1, "v_2": resample_row_v_2, "h_2": resample_row_h_2, "hv_2": resample_row_hv_2, "generic": resample_row_generic}


def kind_of(hs, vs):
    """codec/jpeg.c:2280-2289"""
    return {(1, 1): "row_1", (1, 2): "v_2", (2, 1): "h_2", (2, 2): "hv_2"}.get((hs, vs), "generic")


def upsample(plane, hs, vs, W, H, comp_y, blunder=0):
    """one component: the padded plane uint8 [rows, w2] -> its H x W samples at the picture's resolution.  Rows are read as the
    reference reads them, from the row's first sample on in the flat plane: an hs == 1 plane narrower than the picture is read past its row
    end into the next row (the kernels' CompView::at: and no further than the plane's last sample)."""
    rows, w2 = plane.shape
    w = (W + hs - 1) // hs
    kind = kind_of(hs, vs)
    near, far = schedule(H, vs, comp_y, rows, blunder if kind in ("v_2", "hv_2") else 0)  # the blunders are the interpolating resamplers'
    # NO_RIGHT_CLAMP: the resampler is told of one sample more -- where the plane has that column, or where the last pixel does not read it
    # (odd W: pixel 2 (w - 1) takes the interior form in place of h_2's last-but-one form)
    lores = w + 1 if (blunder == NO_RIGHT_CLAMP and kind in ("h_2", "hv_2") and (w < w2 or W & 1)) else w
    flat = plane.reshape(-1).astype(np.int64)
    col = np.arange(max(lores, W if hs == 1 else lores))
    take = lambda r: flat[np.minimum(r[:, None] * w2 + col[None, :], flat.size - 1)]
    n, f = take(near), take(far)
    if blunder == WRONG_SIDE and kind in ("h_2", "hv_2"):
        out = _wrong_side(kind, n, f, lores)
    else:
        out = RESAMPLERS[kind](n, f, lores, hs)
    return out[:, :W].astype(np.uint8)


# ---------------------------------------------------------------- the output stage

def decoded_components(tag, ncomp, n_out):
    """decode_n (codec/jpeg.c:2244-2249): YCbCr asked for with one or two channels resamples its luma only"""
    return 1 if (ncomp == 3 and n_out < 3 and tag != "rgb") else ncomp


def colour(co, tag, n_out):
    """the resampled components co[k] uint8 [H, W] -> uint8 [H, W, n_out] (codec/jpeg.c:2320-2431)"""
    H, W = co[0].shape
    out = np.empty((H, W, n_out), np.uint8)
    if n_out >= 3:
        if tag == "grey":
            out[..., :3] = co[0][..., None]
        elif tag == "rgb":
            out[..., :3] = np.stack(co[:3], axis=-1)
        elif tag == "cmyk":
            out[..., :3] = np.stack([blinn8(co[k], co[3]) for k in range(3)], axis=-1)
        else:
            rgb = ycbcr_to_rgb(co[0], co[1], co[2])  # "ycc", "ycck", and "ycca": the fourth component is ignored
            out[..., :3] = blinn8(255 - rgb.astype(np.int64), co[3][..., None]) if tag == "ycck" else rgb
    else:
        if tag == "rgb":
            out[..., 0] = compute_y(co[0], co[1], co[2])
        elif tag == "cmyk":
            out[..., 0] = compute_y(*[blinn8(co[k], co[3]) for k in range(3)])
        elif tag == "ycck":
            out[..., 0] = blinn8(255 - co[0].astype(np.int64), co[3])
        else:
            out[..., 0] = co[0]
    if n_out in (2, 4):
        out[..., n_out - 1] = 255
    return out


def resampled(planes, hv, tag, size, n_out, blunder=0):
    """-> the decode_n components at the picture's resolution"""
    W, H = size
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    co = []
    for c in range(decoded_components(tag, len(hv), n_out)):
        h, v = hv[c]
        co.append(upsample(planes[c], hmax // h, vmax // v, W, H, (H * v + vmax - 1) // vmax, blunder))
    return co


def stage(planes, hv, tag, size, n_out, blunder=0):
    """per-component padded sample planes uint8 [bh * 8, bw * 8], the (h, v) factors per component, the colour tag (colour_tag),
    (W, H) and n_out 1..4 -> uint8 [H, W, n_out]"""
    assert 1 <= n_out <= 4
    return colour(resampled(planes, hv, tag, size, n_out, blunder), tag, n_out)


def sample_planes(case, hv):
    """what the transform makes of the coefficients the case's stream holds: per component uint8 [bh * 8, bw * 8]"""
    out = []
    for d in case.dequantised():
        s = M.idct_exact(d)
        bh, bw = s.shape[:2]
        out.append(np.ascontiguousarray(s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)))
    return out


_planes = {}


def picture(case, n_out, layouts=None, blunder=0):
    """a coef_cases.Case -> its pixels: idct_model.idct_exact on the de-quantised coefficients, then the stage above.  The expected pixels
    come from the coefficients the stream holds, never from samples a generator intended."""
    import coef_cases as CC
    hv, app14 = (layouts or CC.all_layouts())[case.layout]
    if case.name not in _planes:
        if len(_planes) > 64:
            _planes.clear()
        _planes[case.name] = sample_planes(case, hv)
    return stage(_planes[case.name], hv, colour_tag(len(hv), app14), (case.w, case.h), n_out, blunder)
