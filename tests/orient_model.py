"""The displayed picture of the oriented tensor output (include/mij.h, mij_batch_set_out_tensor_oriented) on the CPU: orient(px, o)
turns a stored picture into the one EXIF orientation o (1..8) displays, as PIL.ImageOps.exif_transpose does.  The expected value of
an oriented request is tensor_model.window / resize_model.window applied to orient(px, o)."""
import numpy as np


def _t(a):
    return np.swapaxes(a, 0, 1)


# D as a function of S, in numpy; the table of include/mij.h
ORIENT = {
    1: lambda s: s,
    2: lambda s: s[:, ::-1],
    3: lambda s: s[::-1, ::-1],
    4: lambda s: s[::-1],
    5: lambda s: _t(s),
    6: lambda s: _t(s[::-1]),
    7: lambda s: _t(s[::-1, ::-1]),
    8: lambda s: _t(s[:, ::-1]),
}


def orient(px, o):
    """px: [H, W] or [H, W, C] numpy -> the displayed picture, contiguous"""
    return np.ascontiguousarray(ORIENT[int(o)](np.asarray(px)))


def displayed_size(w, h, o):
    """(w, h) of the displayed picture of a w x h stored one"""
    return (h, w) if int(o) >= 5 else (w, h)
