"""The reduced-size decode contract (include/mij.h, mij_batch_set_scale) in numpy integers, built on idct_model: the
normative restatement the kernels (mij_scaled_kernels.h) are tested against, as resize_model.py is for the resized tensor output.

Scale s in 2, 4, 8 and N = 8 // s.  A component with sampling factors (h, v) in a picture with (h_max, v_max) is transformed with
NH = N * h_max // h along the rows and NV = N * v_max // v down the columns, on the low NV x NH coefficients of each block:
    t[y][v] = (sum_u K_NV[y][u] * d[u][v] + 512) >> 10
    p[y][x] = clamp255((sum_v K_NH[x][v] * t[y][v] + 65536 + (128 << 17)) >> 17)
in wrapping 32-bit arithmetic.  Pixel (X, Y) of the ceil(W / s) x ceil(H / s) picture takes sample (Y mod NV, X mod NH) of block
(Y div NV, X div NH) of every component; then the full-size path's colour row and channel replication."""
import numpy as np

import idct_model as M
from upsample_model import ycbcr_to_rgb  # the colour row: stated once, with the rest of the output stage

# K_n[x][u] = rint(4096 * sqrt(2) * a(u) * cos((2x + 1) u pi / 2n)), a(0) = 1 / sqrt(2): the reference's scale, DC weight 4096
K = {
    1: np.array([[4096]], np.int64),
    2: np.array([[4096, 4096], [4096, -4096]], np.int64),
    4: np.array([[4096, 5352, 4096, 2217], [4096, 2217, -4096, -5352], [4096, -2217, -4096, 5352], [4096, -5352, 4096, -2217]], np.int64),
}

LAYOUTS = {"grey": [(1, 1)], "444": [(1, 1)] * 3, "420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)]}


def k_formula(n):
    x, u = np.arange(n)[:, None], np.arange(n)[None, :]
    a = np.where(u == 0, 1 / np.sqrt(2.0), 1.0)
    return np.rint(4096 * np.sqrt(2.0) * a * np.cos((2 * x + 1) * u * np.pi / (2 * n))).astype(np.int64)


def idct_1d(s, n, bias):
    """n-point transform of the list s[0 .. n-1] (int64 arrays) plus bias -> the n outputs wrapped to 32 bits; n = 8 is the reference's"""
    if n == 8:
        return M._idct_1d(list(s), bias)
    return [M._wrap32(sum(int(K[n][x][u]) * s[u] for u in range(n)) + bias) for x in range(n)]


def block_transform(d, nv, nh):
    """de-quantised blocks [..., 8, 8] (natural order) -> uint8 samples [..., nv, nh]; coefficients outside rows < nv, columns < nh are not read"""
    d = M._wrap16(np.asarray(d)[..., :nv, :nh])
    t = np.stack([v >> 10 for v in idct_1d([d[..., u, :] for u in range(nv)], nv, 512)], axis=-2)          # [..., nv, nh]
    o = idct_1d([t[..., :, v] for v in range(nh)], nh, 65536 + (128 << 17))
    return np.clip(np.stack([x >> 17 for x in o], axis=-1), 0, 255).astype(np.uint8)


def component_plane(d, nv, nh):
    """[bh, bw, 8, 8] -> the component at reduced size [bh * nv, bw * nh]"""
    s = block_transform(d, nv, nh)
    bh, bw = s.shape[:2]
    return s.transpose(0, 2, 1, 3).reshape(bh * nv, bw * nh)


def scaled_picture(planes, layout, size, s, n_out):
    """planes: per component de-quantised [bh, bw, 8, 8]; layout: a name of LAYOUTS or the (h, v) factors per component; size (W, H);
    s 2, 4 or 8; n_out 1..4 -> uint8 [ceil(H / s), ceil(W / s), n_out].  One component, or YCbCr asked for with n_out 1 / 2: component 0
    replicated as y | y, 255 | y, y, y | y, y, y, 255 (codec/jpeg.c:2373-2430); YCbCr with n_out 3 / 4: the colour row, alpha 255."""
    hv = LAYOUTS[layout] if isinstance(layout, str) else list(layout)
    assert s in (2, 4, 8) and 1 <= n_out <= 4
    n = 8 // s
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    w, h = size
    ow, oh = -(-w // s), -(-h // s)
    use = 1 if (len(hv) == 1 or n_out < 3) else 3
    comp = []
    for c in range(use):
        nh, nv = n * hmax // hv[c][0], n * vmax // hv[c][1]
        assert nh <= 8 and nv <= 8, "layout has no reduced-size decode"
        comp.append(component_plane(planes[c], nv, nh)[:oh, :ow])
        assert comp[-1].shape == (oh, ow)
    out = np.empty((oh, ow, n_out), np.uint8)
    if use == 1:
        out[..., :3 if n_out >= 3 else 1] = comp[0][..., None]
    else:
        out[..., :3] = ycbcr_to_rgb(comp[0], comp[1], comp[2])
    if n_out in (2, 4):
        out[..., n_out - 1] = 255
    return out
