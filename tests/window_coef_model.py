"""Greyscale and crop in the lossless transcode (include/mij_host.h, mjw_tplan_grey / mjw_tplan_cropped) restated in numpy, independent
of the C code: slices of transcode_planes' planes composed with orient_coef_model.orient, in the contract's order
    grey -> orient (edge mode) -> crop
Requantisation (requant_model) comes after.  Also: which 64-block plane tiles of the SOURCE a window needs, counted from the model's own
bookkeeping of where every kept block came from."""
import collections

import numpy as np

import orient_coef_model as om
import transcode_model as model
import transcode_planes as tp

Windowed = collections.namedtuple("Windowed", "w h hv planes geom units rect greyed tiles")


class Outside(Exception):
    """the window does not lie inside the (oriented) picture"""

    def __init__(self, crop, w, h):
        Exception.__init__(self, "window %r outside %d x %d" % (crop, w, h))
        self.crop, self.w, self.h = crop, w, h


def grey(w, h, hv, planes):
    """-> (hv, planes) of the one-component picture: the luma blocks inside ceil(W / 8) x ceil(H / 8)"""
    if len(hv) == 1:
        return list(hv), list(planes)
    return [(1, 1)], [planes[0][:(h + 7) // 8, :(w + 7) // 8]]


def kept_rect(w, h, hv, crop):
    """the window's kept rectangle in a w x h picture with sampling hv: the origin moved down to the MCU grid, the far edges where they
    were asked; Outside for a window that is none"""
    x0, y0, cw, ch = crop
    if cw < 1 or ch < 1 or x0 < 0 or y0 < 0 or x0 + cw > w or y0 + ch > h:
        raise Outside(crop, w, h)
    mw, mh = 8 * hv[0][0], 8 * hv[0][1]
    return (x0 - x0 % mw, y0 - y0 % mh, cw + x0 % mw, ch + y0 % mh)


def _tagged(planes):
    """per component an int64 [bh, bw] of the blocks' raster indices in the source plane: carried through the same slices and
    permutations as the coefficients, it says where every kept block came from"""
    return [np.arange(p.shape[0] * p.shape[1], dtype=np.int64).reshape(p.shape[0], p.shape[1]) for p in planes]


def _orient_tags(w, h, hv, tags, o, trim):
    _, _, ex, ey = om.kept_mcus(w, h, hv, o, trim)
    out = []
    for (a, v), t in zip(hv, tags):
        t = t[:ey * v, :ex * a]
        if o in om.MIRROR_X:
            t = t[:, ::-1]
        if o in om.MIRROR_Y:
            t = t[::-1]
        out.append(t.T if o in om.TRANSPOSE else t)
    return out


def window(w, h, hv, planes, o=1, trim=False, crop=None, greyed=False):
    """planes: per component [bh, bw, 64] in zigzag order (padding blocks included) -> Windowed: the destination's size, sampling, planes
    (zigzag), Geom, units in its MCU order, the kept rectangle (None without a crop), whether chroma was dropped, and the number of
    64-block tiles of the source's planes that hold a kept block.  om.Refused / Outside where the contract refuses."""
    tags = _tagged(planes)
    dropped = greyed and len(hv) == 3
    if greyed:
        hv1, planes = grey(w, h, hv, planes)
        tags = grey(w, h, hv, tags)[1]
        hv = hv1
    r = om.orient(w, h, hv, planes, o, trim)
    tags = _orient_tags(w, h, hv, tags, o, trim)
    w2, h2, hv2, zz = r.w, r.h, r.hv, r.planes
    rect = None
    if crop is not None:
        rect = kept_rect(w2, h2, hv2, crop)
        mw, mh = 8 * hv2[0][0], 8 * hv2[0][1]
        mx0, my0 = rect[0] // mw, rect[1] // mh
        nx, ny = (rect[2] + mw - 1) // mw, (rect[3] + mh - 1) // mh
        zz = [p[my0 * v:(my0 + ny) * v, mx0 * a:(mx0 + nx) * a] for (a, v), p in zip(hv2, zz)]
        tags = [t[my0 * v:(my0 + ny) * v, mx0 * a:(mx0 + nx) * a] for (a, v), t in zip(hv2, tags)]
        w2, h2 = rect[2], rect[3]
    g = tp.Geom(w2, h2, hv2)
    assert [q.shape[:2] for q in zz] == [(c.bh, c.bw) for c in g.comp], (o, trim, crop, greyed)
    units = model.units_from_planes(g, tp.natural(zz))
    tiles = sum(len(np.unique(t // 64)) for t in tags)
    return Windowed(w2, h2, list(hv2), [np.ascontiguousarray(p) for p in zz], g, units, rect, dropped, tiles)


def codable(res):
    return model.codable(res.geom, res.units)


def windows(w, h, hv):
    """the named windows of a w x h picture with sampling hv, in its own frame: one MCU at each corner, an unaligned origin (which must
    grow to the grid), one ending in the partial last MCU, the last MCU row, one MCU column from top to bottom, the whole picture"""
    mw, mh = 8 * hv[0][0], 8 * hv[0][1]
    lx, ly = (w - 1) // mw * mw, (h - 1) // mh * mh  # the last MCU's origin
    out = collections.OrderedDict()
    out["whole"] = (0, 0, w, h)
    out["corner nw"] = (0, 0, min(mw, w), min(mh, h))
    out["corner ne"] = (lx, 0, w - lx, min(mh, h))
    out["corner sw"] = (0, ly, min(mw, w), h - ly)
    out["corner se"] = (lx, ly, w - lx, h - ly)
    if h > mh:
        out["last row"] = (0, ly, w, h - ly)  # at orientation 1, in the pictures of the GPU tests: every block in the plane's second tile
    if w > mw:
        out["column"] = (mw, 0, min(mw, w - mw), h)  # every block row: whatever tiles the plane has
    if w > mw + 3 and h > mh + 2:
        out["unaligned"] = (mw + 3, mh + 2, min(mw, w - mw - 3), min(mh, h - mh - 2))
        out["to the end"] = (mw, mh, w - mw, h - mh)
    return out


REFUSALS = (lambda w, h: (0, 0, 0, h), lambda w, h: (0, 0, w, 0), lambda w, h: (-1, 0, 1, 1), lambda w, h: (0, -1, 1, 1),
            lambda w, h: (1, 0, w, 1), lambda w, h: (0, 1, 1, h), lambda w, h: (w, 0, 1, 1), lambda w, h: (0, 0, w + 1, h),
            lambda w, h: (0, 0, -3, 4), lambda w, h: (2 ** 31 - 1, 0, 2, 1))
