"""Model of the resized tensor output (mij_batch_set_out_tensor_resized / TensorDecoder.decode(size=...)) on the CPU: the contract of
include/mij.h restated in numpy -- coefficients in Python doubles, sums in int64 -- then flips, table and layout through tensor_model.
Used as the expected value of the GPU tests and compared with the library's host coefficients and with Pillow by the CPU tests."""
import math

import numpy as np
import torch

import tensor_model as tm

FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")  # MIJ_FILTER_BOX .. MIJ_FILTER_LANCZOS
SUPPORT = {"box": 0.5, "bilinear": 1.0, "hamming": 1.0, "bicubic": 2.0, "lanczos": 3.0}
_F32_054, _F32_046 = float(np.float32(0.54)), float(np.float32(0.46))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def filt(name, x):
    if name == "box":
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if name == "bilinear":
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if name == "hamming":
        x = abs(x)
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (_F32_054 + _F32_046 * math.cos(x))
    if name == "bicubic":
        a = -0.5
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    if name == "lanczos":
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    raise ValueError(name)


def coeffs(n_in, n_out, name):
    """-> (lo [n_out], n [n_out], k [n_out, ksize] int64, ksize): one axis of the contract.  An axis whose size does not change is
    skipped by the contract; its coefficients here are still the formula's (the caller skips)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[name] * fs
    ksize = 2 * int(math.ceil(support)) + 1
    lo = np.zeros(n_out, np.int64)
    n = np.zeros(n_out, np.int64)
    k = np.zeros((n_out, ksize), np.int64)
    for o in range(n_out):
        center = (o + 0.5) * scale
        a = max(int(center - support + 0.5), 0)
        m = min(int(center + support + 0.5), n_in) - a
        w = [filt(name, (t + a - center + 0.5) / fs) for t in range(m)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        lo[o], n[o] = a, m
        for t, v in enumerate(w):
            k[o, t] = int(v * (1 << 22) + (-0.5 if v < 0 else 0.5))  # int() truncates toward zero, as C's cast
    return lo, n, k, ksize


def _pass(x, lo, n, k):
    """x: int64 [in, ...] -> uint8 [out, ...] along axis 0"""
    s = np.full((len(lo),) + x.shape[1:], 1 << 21, np.int64)
    kz = np.where(np.arange(k.shape[1])[None, :] < n[:, None], k, 0)  # taps t >= n[o] add nothing
    extra = (1,) * (x.ndim - 1)
    for t in range(k.shape[1]):
        s += x[np.minimum(lo + t, x.shape[0] - 1)] * kz[:, t].reshape((-1,) + extra)
    return np.clip(s >> 22, 0, 255)


def resize(a, out_w, out_h, name):
    """a: uint8 [h, w] or [h, w, C] -> uint8 of the same rank at out_h x out_w: horizontal pass first (skipped when out_w == w), then
    vertical (skipped when out_h == h), every channel on its own"""
    x = a.astype(np.int64)
    h, w = x.shape[:2]
    if out_w != w:
        lo, n, k, _ = coeffs(w, out_w, name)
        x = np.moveaxis(_pass(np.moveaxis(x, 1, 0), lo, n, k), 0, 1)
    if out_h != h:
        lo, n, k, _ = coeffs(h, out_h, name)
        x = _pass(x, lo, n, k)
    return x.astype(np.uint8)


def window(px, win, size, name="bilinear", flip_x=False, flip_y=False, layout="CHW", table=None, dtype=torch.uint8):
    """px: uint8 [H, W, C] numpy; win (x0, y0, w, h); size (out_h, out_w) -> torch tensor [C, out_h, out_w] or [out_h, out_w, C]:
    crop, resize, then flips, table and layout as tensor_model.window"""
    if px.ndim == 2:
        px = px[:, :, None]
    x0, y0, w, h = win
    out_h, out_w = size
    r = resize(np.ascontiguousarray(px[y0:y0 + h, x0:x0 + w]), out_w, out_h, name)
    return tm.window(r, (0, 0, out_w, out_h), flip_x, flip_y, layout, table, dtype)
