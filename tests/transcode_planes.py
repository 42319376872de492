"""Transcode sources made from CHOSEN coefficient planes (test_transcode_host.py, test_gpu_transcode_blocks.py).  transcode_cases.py
holds pictures an encoder made: smooth DCs, high frequencies mostly zero.  Here every coefficient is set on purpose, so that a block in
the wrong unit, a coefficient at the wrong zigzag place, a wrong DC predecessor or a tile seam changes what a test compares.

Every source is written with header_cases.plain (optimal tables: any magnitude can be coded) from planes [bh, bw, 64] in zigzag order,
for the five transcodable layouts.  A Source carries the planes it was written from, so the expected units need no decoder."""
import collections
import functools

import numpy as np

import emit_model as em
import header_cases as hc
import transcode_model as model

LAYOUTS = collections.OrderedDict([("grey", [(1, 1)]), ("444", [(1, 1)] * 3), ("422", [(2, 1), (1, 1), (1, 1)]),
                                   ("440", [(1, 2), (1, 1), (1, 1)]), ("420", [(2, 2), (1, 1), (1, 1)])])

# MCU grids (columns, rows) around the 64-block plane tile of each component and the 128-unit emission tile
GRIDS = ((1, 1), (1, 3), (3, 1), (7, 9), (8, 8), (5, 13), (1, 65), (65, 1), (16, 8), (43, 3))

EDGE_VALUES = (-1023, -257, -256, -255, -129, -128, -1, 1, 127, 128, 255, 256, 257, 1023)

Source = collections.namedtuple("Source", "name layout w h hv planes data")


class Geom:
    """what transcode_model wants of a descriptor, from a size and sampling factors alone"""
    Comp = collections.namedtuple("Comp", "h v bw bh")

    def __init__(self, w, h, hv):
        self.width, self.height, self.ncomp = w, h, len(hv)
        self.mcu_x, self.mcu_y, shapes = hc.geometry(w, h, hv)
        self.comp = [Geom.Comp(a, v, bw, bh) for (a, v), (bh, bw) in zip(hv, shapes)]
        self.ny = hv[0][0] * hv[0][1]
        self.dpm = sum(a * v for a, v in hv)
        self.n_du = self.mcu_x * self.mcu_y * self.dpm


def size(layout, grid, short):
    """the picture size of an MCU grid: the exact multiple, or 3 px / 1 px short of it"""
    a, v = LAYOUTS[layout][0]
    return grid[0] * 8 * a - (3 if short else 0), grid[1] * 8 * v - (1 if short else 0)


def source(name, layout, w, h, planes):
    hv = LAYOUTS[layout]
    return Source(name, layout, w, h, hv, planes, hc.plain(w, h, hv, planes).bytes())


def natural(planes):
    """zigzag planes [bh, bw, 64] -> [bh, bw, 8, 8] in natural order, as transcode_model.units_from_planes takes them"""
    out = []
    for p in planes:
        n = np.empty_like(p)
        n[:, :, model.ZIGZAG_NATURAL] = p
        out.append(n.reshape(p.shape[0], p.shape[1], 8, 8))
    return out


def expected_units(src):
    """the model's units of the planes a source was written from"""
    return model.units_from_planes(Geom(src.w, src.h, src.hv), natural(src.planes))


def units_to_planes(du, w, h, hv):
    """the inverse of transcode_model.units_from_planes, in zigzag planes: units [n_du, 64] in MCU order -> the planes of a w x h picture
    with sampling factors hv.  Lets emission-shaped content (emit_model.adversarial_units) enter through a file."""
    g = Geom(w, h, hv)
    du = np.asarray(du, np.int16).reshape(-1, 64)
    assert du.shape[0] == g.n_du, (du.shape, g.n_du)
    m = du.reshape(g.mcu_y, g.mcu_x, g.dpm, 64)
    planes, first = hc.blank(w, h, hv), 0
    for c, (a, v) in enumerate(hv):
        blk = m[:, :, first:first + a * v].reshape(g.mcu_y, g.mcu_x, v, a, 64)
        planes[c][:] = blk.transpose(0, 2, 1, 3, 4).reshape(g.mcu_y * v, g.mcu_x * a, 64)
        first += a * v
    return planes


def mcu_order(g, c):
    """[(by, bx)] of component c's blocks in the order the scan codes them: each one's DC predecessor is the entry before it"""
    a, v = g.comp[c].h, g.comp[c].v
    return [(my * v + sy, mx * a + sx) for my in range(g.mcu_y) for mx in range(g.mcu_x) for sy in range(v) for sx in range(a)]


def escaped_blocks(planes):
    """the blocks that hold an AC coefficient outside -128..127: what compact planes flag"""
    return sum(int(((p[:, :, 1:] < -128) | (p[:, :, 1:] > 127)).any(axis=2).sum()) for p in planes)


# ---------------------------------------------------------------- contents

def address_planes(w, h, hv):
    """every coefficient a function of (component, by, bx, k) within -1023..1023; blocks with L % 3 == 0 stay within -128..127, so escaped
    and plain blocks alternate inside each 64-block tile.  DCs lie within -1023..1023: any two differ by 2046 at most."""
    planes = hc.blank(w, h, hv)
    k = np.arange(64)
    for c, p in enumerate(planes):
        bh, bw, _ = p.shape
        by, bx = np.mgrid[0:bh, 0:bw]
        mix = c * 1000003 + by[:, :, None] * 7919 + bx[:, :, None] * 104729 + k * 1299709
        p[:] = np.where(((by * bw + bx) % 3 == 0)[:, :, None], mix % 256 - 128, mix % 2047 - 1023)
    return planes


def edge_planes(w, h, hv):
    """block b holds EDGE_VALUES[(b + k) % 14] at position k: each value at every zigzag position 1..63 once there are 14 blocks"""
    planes = hc.blank(w, h, hv)
    vals = np.array(EDGE_VALUES)
    for p in planes:
        bh, bw, _ = p.shape
        b = np.arange(bh * bw).reshape(bh, bw)
        p[:, :, 1:] = vals[(b[:, :, None] + np.arange(1, 64)) % len(vals)]
    return planes


def dense_planes(w, h, hv, seed):
    rng = np.random.default_rng(seed)
    planes = hc.blank(w, h, hv)
    for p in planes:
        p[:] = rng.integers(-1023, 1024, size=p.shape)
    return planes


@functools.lru_cache(maxsize=None)
def address(layout):
    """the whole geometry list with address content"""
    out = []
    for grid in GRIDS:
        for short in (False, True):
            w, h = size(layout, grid, short)
            out.append(source("address %s %dx%d MCUs %dx%d" % (layout, grid[0], grid[1], w, h), layout, w, h, address_planes(w, h, LAYOUTS[layout])))
    return out


@functools.lru_cache(maxsize=None)
def edge_values(layout):
    w, h = size(layout, (5, 13), True)
    return source("edge values %s %dx%d" % (layout, w, h), layout, w, h, edge_planes(w, h, LAYOUTS[layout]))


@functools.lru_cache(maxsize=None)
def dense(layout):
    """uniform noise in -1023..1023 at every coefficient: every block is escaped, and a unit takes some 200 bytes under the Annex-K tables"""
    w, h = size(layout, (7, 9), True)
    return source("dense %s %dx%d" % (layout, w, h), layout, w, h, dense_planes(w, h, LAYOUTS[layout], 11))


@functools.lru_cache(maxsize=None)
def longest():
    """4:4:4, 43 x 3 MCUs, every AC +-1023 and every DC difference +-2047: about the longest codable units there are"""
    w, h = size("444", (43, 3), False)
    planes = hc.blank(w, h, LAYOUTS["444"])
    for p in planes:
        bh, bw, _ = p.shape
        b = np.arange(bh * bw).reshape(bh, bw)
        p[:, :, 1:] = np.where((b[:, :, None] + np.arange(1, 64)) % 2 == 0, 1023, -1023)
        p[:, :, 0] = np.where(b % 2 == 0, -1024, 1023)  # 1x1 blocks: the plane's raster order is the MCU order
    return source("longest 444 %dx%d" % (w, h), "444", w, h, planes)


TRIANGLE_GRID = (16, 4)


@functools.lru_cache(maxsize=None)
def triangle(layout):
    """all AC zero; each component's DC a triangle wave of amplitude 1100 over its MCU-order index with a period of two MCU rows.  No
    MCU-order difference is large, while the first blocks of consecutive MCU rows differ by 2200: only the right predecessor rule
    accepts the picture."""
    w, h = size(layout, TRIANGLE_GRID, True)
    hv = LAYOUTS[layout]
    g = Geom(w, h, hv)
    planes = hc.blank(w, h, hv)
    for c, p in enumerate(planes):
        seq = mcu_order(g, c)
        row = len(seq) // g.mcu_y
        for i, (by, bx) in enumerate(seq):
            t = i % (2 * row)
            p[by, bx, 0] = -1100 + 2200 * (t if t <= row else 2 * row - t) // row
    return source("triangle %s %dx%d" % (layout, w, h), layout, w, h, planes)


# ---------------------------------------------------------------- one DC pair per branch of the predecessor rule

BRANCHES = "abcde"
# grids of at most 68 MCUs; a chroma plane crosses its 64-block tile from 65 MCUs on
PAIR_GRIDS = ((3, 3), (9, 4), (4, 9), (13, 5), (5, 13), (17, 4), (4, 17))
DELTAS = (2047, -2047, 2048, -2048)


def branch_of(sx, sy, mx, my):
    """(a) sx > 0; (b) sx == 0, sy > 0; (c) an MCU's first block, mx > 0; (d) an MCU row's first block, my > 0; (e) the first block"""
    return "a" if sx > 0 else "b" if sy > 0 else "c" if mx > 0 else "d" if my > 0 else "e"


@functools.lru_cache(maxsize=None)
def pair_site(layout, comp, branch, same_tile):
    """-> (grid, (by, bx) of the block, (by, bx) of its MCU-order predecessor or None for branch e), or None when no grid of PAIR_GRIDS
    has such a pair.  same_tile: block and predecessor lie in the same 64-block plane tile / the predecessor in an earlier one.  The last
    such block of the picture is taken, so that where the grid allows it neither lies in the plane's first tile.
    Branch (a) never crosses a tile: h is 2 there, so bw is even, the block's index L = by * bw + bx is odd, and L - 1 shares its tile."""
    hv = LAYOUTS[layout]
    a, v = hv[comp]
    for grid in (reversed(PAIR_GRIDS) if same_tile else PAIR_GRIDS):
        g = Geom(*size(layout, grid, True), hv)
        seq, bw, found = mcu_order(g, comp), g.comp[comp].bw, None
        for i, (by, bx) in enumerate(seq):
            if branch_of(bx % a, by % v, bx // a, by // v) != branch:
                continue
            if branch == "e":
                found = (grid, (by, bx), None) if same_tile else None
                break
            pby, pbx = seq[i - 1]
            if (((by * bw + bx) >> 6) == ((pby * bw + pbx) >> 6)) == same_tile:
                found = (grid, (by, bx), (pby, pbx))
        if found:
            return found
    return None


def dc_pair(layout, comp, branch, same_tile, delta):
    """all coefficients zero except one block and its true MCU-order predecessor, whose DCs differ by delta: (-1024, -1024 + delta) for
    a positive delta and the mirror image for a negative one; branch e sets the first block to delta against the predictor 0.  Every
    other DC is 0, so any other predecessor rule sees a difference of about 1024.  None where pair_site finds no such pair."""
    site = pair_site(layout, comp, branch, same_tile)
    if site is None:
        return None
    grid, blk, pred = site
    w, h = size(layout, grid, True)
    planes = hc.blank(w, h, LAYOUTS[layout])
    if pred is None:
        planes[comp][blk[0], blk[1], 0] = delta
    else:
        base = -1024 if delta > 0 else 1024
        planes[comp][pred[0], pred[1], 0] = base
        planes[comp][blk[0], blk[1], 0] = base + delta
    return source("dc pair %s comp %d branch %s %s tile delta %d" % (layout, comp, branch, "same" if same_tile else "earlier", delta), layout, w, h, planes)


@functools.lru_cache(maxsize=None)
def dc_pairs(layout):
    """[(Source, accepted)] for every component, every branch the layout has, both tile relations where the geometry allows, every delta"""
    out = []
    for comp in range(len(LAYOUTS[layout])):
        for branch in BRANCHES:
            for same_tile in (True, False):
                for delta in DELTAS:
                    s = dc_pair(layout, comp, branch, same_tile, delta)
                    if s is not None:
                        out.append((s, abs(delta) <= 2047))
    return out


# ---------------------------------------------------------------- one AC value at the limit

AC_GRID = (13, 5)  # 65 MCUs: a chroma plane has blocks 63 and 64


@functools.lru_cache(maxsize=None)
def ac_limits(layout):
    """[(Source, accepted)]: +-1023 (accepted: every site in one picture, once with each sign at each site) and +-1024 (refused: one site
    and one sign per picture) at zigzag positions 1, 32 and 63 of the first block, the last block and blocks 63 and 64 of a plane, luma
    and chroma"""
    hv = LAYOUTS[layout]
    w, h = size(layout, AC_GRID, True)
    sites = []
    for c in sorted({0, len(hv) - 1}):
        bh, bw, _ = hc.blank(w, h, hv)[c].shape
        for bi, L in enumerate((0, bh * bw - 1, 63, 64)):
            for pi, k in enumerate((1, 32, 63)):
                sites.append((c, L // bw, L % bw, k, 1 if (bi + pi) % 2 == 0 else -1))
    out = []
    for sign in (1, -1):
        planes = hc.blank(w, h, hv)
        for c, by, bx, k, s in sites:
            planes[c][by, bx, k] = sign * s * 1023
        out.append((source("ac limit %s every site, first %+d" % (layout, sign * 1023), layout, w, h, planes), True))
    for c, by, bx, k, _ in sites:
        for value in (1024, -1024):
            planes = hc.blank(w, h, hv)
            planes[c][by, bx, k] = value
            out.append((source("ac limit %s comp %d block (%d, %d) k %d value %d" % (layout, c, by, bx, k, value), layout, w, h, planes), False))
    return out


# ---------------------------------------------------------------- emission-shaped content through a file

# per layout: an MCU grid of at least 1300 units (eleven 128-unit emission tiles: ten seams), and the seed with which, under the Annex-K
# tables, at least one seam shares a 0xFF byte between two tiles and at least one falls on a byte boundary (the tests assert it)
EMISSION = {"grey": ((36, 37), 1), "444": ((21, 21), 1), "422": ((18, 19), 1), "440": ((18, 19), 1), "420": ((15, 15), 1)}


def emission_source(layout, seed=None):
    grid, chosen = EMISSION[layout]
    seed = chosen if seed is None else seed
    hv = LAYOUTS[layout]
    w, h = size(layout, grid, True)
    g = Geom(w, h, hv)
    du = em.adversarial_units(np.random.default_rng(seed), g.mcu_x * g.mcu_y, g.dpm, ny=g.ny)
    assert du.shape[0] >= 1300
    return source("emission %s seed %d %d units" % (layout, seed, du.shape[0]), layout, w, h, units_to_planes(du, w, h, hv))


@functools.lru_cache(maxsize=None)
def emission(layout):
    return emission_source(layout)


@functools.lru_cache(maxsize=None)
def emission_model(layout):
    """-> (units, {optimize: the model's whole stream}, the plain entropy segment's stats, the header length per optimize): the plain
    header is the library's (mjw_theader, pinned elsewhere), everything behind it and the optimised DHT segment are the models'"""
    import image_codecs_amd as ica
    import hufopt_model as hm
    src = emission(layout)
    g = Geom(src.w, src.h, src.hv)
    du = expected_units(src)
    desc, _ = ica.HostDecoder.decode(src.data, 0)
    hdr = ica.transcode_header(ica.transcode_plan(desc)[0])
    T, n = em.tables_from_stream(hdr)
    assert n == len(hdr)
    stats = {}
    plain = hdr + em.emit_entropy(T, du, g.dpm, stats=stats, ny=g.ny) + hc.EOI
    opt = hm.emit_optimized(hdr, du, g.dpm, g.ny)
    return du, {False: plain, True: opt}, stats, {False: n, True: em.tables_from_stream(opt)[1]}


def all_sources(layout):
    """[(Source, accepted or None where only the model says)] of every family above"""
    out = [(s, True) for s in address(layout)] + [(edge_values(layout), True), (dense(layout), True), (triangle(layout), True)]
    if layout == "444":
        out.append((longest(), True))
    return out + dc_pairs(layout) + ac_limits(layout)
