"""The lossless reorientation's contract restated in numpy, independent of the C code (include/mij_host.h, mjw_tplan_oriented): from
coefficient planes to the destination's geometry, tables and units, written from the block rules alone.  test_transcode_orient_host.py
anchors the coefficient rule on the DCT itself; the GPU tests compare the kernel against this model.

Orientation o is mirrors of the SOURCE's axes first, then an optional transpose:
    o        1  2  3  4  5  6  7  8
    mirror x    *  *           *  *
    mirror y       *  *     *  *
    transpose            *  *  *  *"""
import collections

import numpy as np

import header_cases as hc
import transcode_model as model
import transcode_planes as tp

ORIENTATIONS = range(1, 9)
MIRROR_X = {2, 3, 7, 8}
MIRROR_Y = {3, 4, 6, 7}
TRANSPOSE = {5, 6, 7, 8}
INVERSE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}

Oriented = collections.namedtuple("Oriented", "w h hv planes geom units")


class Refused(Exception):
    """the picture cannot be transformed under the edge mode; axis is 'x' or 'y', size and mcu what the reason has to name"""

    def __init__(self, kind, axis, size, mcu):
        Exception.__init__(self, "%s: %s axis, size %d, MCU %d" % (kind, axis, size, mcu))
        self.kind, self.axis, self.size, self.mcu = kind, axis, size, mcu


def orient_pixels(S, o):
    """the displayed picture of a stored one [h, w] or [h, w, c]: the table of include/mij.h"""
    S = np.asarray(S)
    if o in MIRROR_X:
        S = S[:, ::-1]
    if o in MIRROR_Y:
        S = S[::-1]
    return np.swapaxes(S, 0, 1) if o in TRANSPOSE else S


def orient_block(nat, o):
    """coefficient blocks [..., 8, 8] in natural order (row = vertical frequency v, column = horizontal frequency u) of the SAME block
    position -> the blocks of the oriented picture: a mirrored x negates odd u, a mirrored y odd v, a transpose swaps u and v"""
    nat = np.asarray(nat)
    odd = np.where(np.arange(8) % 2 == 1, -1, 1)
    if o in MIRROR_X:
        nat = nat * odd[None, :]
    if o in MIRROR_Y:
        nat = nat * odd[:, None]
    return np.swapaxes(nat, -1, -2) if o in TRANSPOSE else nat


def orient_table(zz, o):
    """a quantisation table in zigzag order -> the destination's"""
    nat = np.empty(64, np.int64)
    nat[model.ZIGZAG_NATURAL] = np.asarray(zz)
    nat = nat.reshape(8, 8)
    return (nat.T if o in TRANSPOSE else nat).reshape(64)[model.ZIGZAG_NATURAL]


def kept_mcus(w, h, hv, o, trim):
    """-> (width, height, MCU columns, MCU rows) of the source that stay, in the source's frame; Refused where the edge mode says so"""
    mcu_x, mcu_y, _ = hc.geometry(w, h, hv)
    mw, mh = 8 * hv[0][0], 8 * hv[0][1]
    if o in MIRROR_X and w % mw:
        if not trim:
            raise Refused("perfect", "x", w, mw)
        if w < mw:
            raise Refused("nothing left", "x", w, mw)
        mcu_x, w = w // mw, w // mw * mw
    if o in MIRROR_Y and h % mh:
        if not trim:
            raise Refused("perfect", "y", h, mh)
        if h < mh:
            raise Refused("nothing left", "y", h, mh)
        mcu_y, h = h // mh, h // mh * mh
    return w, h, mcu_x, mcu_y


def orient(w, h, hv, planes, o, trim=False):
    """planes: per component [bh, bw, 64] in zigzag order, as transcode_planes makes them (padding blocks included) -> Oriented: the
    destination's size, sampling factors, planes (zigzag again), Geom and units in the destination's MCU order"""
    w2, h2, ex, ey = kept_mcus(w, h, hv, o, trim)
    out = []
    for (a, v), p in zip(hv, tp.natural(planes)):
        p = p[:ey * v, :ex * a]  # an axis that is not mirrored keeps everything: ex, ey are the whole grid there
        if o in MIRROR_X:
            p = p[:, ::-1]
        if o in MIRROR_Y:
            p = p[::-1]
        p = orient_block(p, o)
        if o in TRANSPOSE:
            p = np.swapaxes(p, 0, 1)
        out.append(np.ascontiguousarray(p).astype(np.int16))
    if o in TRANSPOSE:
        w2, h2, hv = h2, w2, [(v, a) for a, v in hv]
    g = tp.Geom(w2, h2, hv)
    assert [q.shape[:2] for q in out] == [(c.bh, c.bw) for c in g.comp], (o, trim, [q.shape for q in out])
    units = model.units_from_planes(g, out)
    zz = [q.reshape(q.shape[0], q.shape[1], 64)[:, :, model.ZIGZAG_NATURAL] for q in out]
    return Oriented(w2, h2, list(hv), zz, g, units)


def codable(res):
    return model.codable(res.geom, res.units)


# ---------------------------------------------------------------- crafted DC steps: codable in one unit order and not in the other

def dc_grid(layout, values):
    """a 2 x 2 MCU picture of 1x1 components whose DCs are [[A, B], [C, D]] in every component, every AC zero"""
    hv = tp.LAYOUTS[layout]
    planes = hc.blank(16, 16, hv)
    for p in planes:
        p[:, :, 0] = np.array(values).reshape(2, 2)
    return planes, hc.plain(16, 16, hv, planes).bytes()


# raster order A B C D steps by 1000, 1100, 1000; the transposed order A C B D steps from A to C by 2100
DC_ROWS_OK = (-1500, -500, 600, 1600)
DC_COLS_OK = (-1500, 600, -500, 1600)
