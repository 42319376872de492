"""The de-normalising contract of float device-pixel slots (include/mij.h, mij_enc_add_device_float) in numpy, and exact judges for it.

    t = fl32(fl32(x) * scale[c]);  t = fl32(t + bias[c]);  u = uint8(rint(min(max(t, 0), 255)))   NaN -> 0

numpy multiplies and adds float32 arrays in two separate passes, each correctly rounded, so nothing here can fuse; float16 widens
exactly in numpy, bfloat16 through torch.  no_fma_triples() searches (x, scale, bias) where one rounding of the exact x*scale + bias
gives another byte than the contract's two, judged in exact rationals (fractions.Fraction)."""
from fractions import Fraction

import numpy as np

IM_MEAN, IM_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def widen(t):
    """a torch tensor of float16 / bfloat16 / float32 -> float32 numpy, exactly"""
    import torch
    return t.detach().cpu().to(torch.float32).numpy()


def scale_bias(n, mean=None, std=None):
    """scale[c] = float32(255.0 * std[c]), bias[c] = float32(255.0 * mean[c]), products in Python doubles; omitted: mean 0, std 1"""
    mean = [0.0] * n if mean is None else [float(v) for v in mean]
    std = [1.0] * n if std is None else [float(v) for v in std]
    assert len(mean) == n and len(std) == n
    return np.array([255.0 * v for v in std], np.float32), np.array([255.0 * v for v in mean], np.float32)


def denorm(x, scale, bias):
    """elementwise contract: x, scale, bias float32 (broadcast against each other) -> uint8"""
    x, scale, bias = np.asarray(x), np.asarray(scale), np.asarray(bias)
    assert x.dtype == np.float32 and scale.dtype == np.float32 and bias.dtype == np.float32
    with np.errstate(all="ignore"):
        t = np.multiply(x, scale, dtype=np.float32)
        t = np.add(t, bias, dtype=np.float32)
    t = np.where(np.isnan(t), np.float32(0), t)
    return np.rint(np.clip(t, np.float32(0), np.float32(255))).astype(np.uint8)


def picture(x, scale, bias):
    """a float32 picture [h, w, c] (or [h, w]: grey) -> the uint8 picture that is encoded; channel c takes scale[c], bias[c]"""
    x = np.asarray(x)
    if x.ndim == 2:
        return denorm(x, scale[0], bias[0])
    c = x.shape[2]
    return denorm(x, np.asarray(scale)[None, None, :c], np.asarray(bias)[None, None, :c])


# ---- exact judges

def fl32(q):
    """a Fraction -> the nearest float32 (ties to the even mantissa), decided in exact arithmetic; finite values below overflow"""
    c = np.float32(float(q))
    best = None
    for v in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        d = abs(Fraction(float(v)) - q)
        even = (int(np.float32(v).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, v)
    return np.float32(best[1])


def byte_of(t):
    """rint(min(max(t, 0), 255)) of a finite float32 as an int, in exact arithmetic"""
    q = min(max(Fraction(float(t)), Fraction(0)), Fraction(255))
    f = q.numerator // q.denominator
    r = q - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return int(f)


def two_roundings(x, scale, bias):
    return byte_of(fl32(Fraction(float(fl32(Fraction(float(x)) * Fraction(float(scale))))) + Fraction(float(bias))))


def one_rounding(x, scale, bias):
    return byte_of(fl32(Fraction(float(x)) * Fraction(float(scale)) + Fraction(float(bias))))


_TRIPLES = None


def no_fma_triples(want=96, seed=20261, tries=200000):
    """-> [(x, scale, bias, contract byte, fused byte)], float32 triples whose fused result rounds to another byte.  The search aims
    x * scale + bias at a tie k + 0.5: the two-rounding sum then lands exactly on the tie where the fused one falls beside it."""
    global _TRIPLES
    if _TRIPLES is not None:
        return _TRIPLES
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(tries):
        if len(out) >= want:
            break
        k = int(rng.integers(0, 255))
        scale = np.float32(rng.uniform(20.0, 300.0) * (1 if rng.random() < 0.8 else -1))
        bias = np.float32(rng.uniform(-200.0, 400.0))
        x = np.float32((k + 0.5 - float(bias)) / float(scale))
        a, b = two_roundings(x, scale, bias), one_rounding(x, scale, bias)
        if a != b:
            out.append((x, scale, bias, a, b))
    _TRIPLES = out
    return out
