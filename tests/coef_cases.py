"""Deterministic stream families that put single coefficients ON the two decisions every decode kernel takes from the coefficients
themselves: the per-block L1 limit behind MIJ_FLAG_WIDE_IDCT (include/mij.h) and the sparse class of a wavefront (mij_kernels.h, "sparse
blocks").  Every picture is written from explicit per-component planes of quantised coefficients through the test-side writer
(tests/support/prog_writer.c, the code behind helpers.baseline_from_du / baseline_layout_from_444 / progressive_from_du), so that a
block's place in its plane -- and with it its lane in a wavefront -- is the generator's to choose, MCU padding included.  Tables are
all ones (what the writer's plan has at quality 100: coefficient == de-quantised value) unless a case says otherwise; tables with
entries beyond a byte are written as real Pq = 1 segments.

A Case knows its planes, so the model (idct_model.py) can say what every producer and kernel has to make of it."""
import ctypes as C

import numpy as np

import helpers
import idct_model as M

# layout -> sampling factors per component, Adobe transform byte (-1: no APP14 segment)
LAYOUTS = {
    "420": ([(2, 2), (1, 1), (1, 1)], -1), "440": ([(1, 2), (1, 1), (1, 1)], -1), "422": ([(2, 1), (1, 1), (1, 1)], -1),
    "444": ([(1, 1), (1, 1), (1, 1)], -1), "grey": ([(1, 1)], -1), "411": ([(4, 1), (1, 1), (1, 1)], -1),
    "rgb": ([(1, 1), (1, 1), (1, 1)], 0), "cmyk": ([(1, 1)] * 4, 0), "ycck": ([(1, 1)] * 4, 2),
}
# the kernel family mij_batch_slot_path reports for a layout asked for with 3 or 4 output channels (mij_runtime.hip, classify)
PATH_OF = {"420": 1, "440": 6, "422": 4, "444": 3, "grey": 5, "411": 2, "rgb": 7, "cmyk": 7, "ycck": 7}
# the layouts the GPU Huffman walk serves (mjh_extract_scan: baseline files of one or three components in one interleaved scan;
# four-component files it declines with status 2, like progressive ones)
GPU_WALK_LAYOUTS = ("420", "440", "422", "444", "grey", "411", "rgb")

# layouts other test modules add for their own pictures (sample_cases.py): known to the writer and the geometry below, and to none of this
# module's families, tables or everything()
EXTRA_LAYOUTS = {}


def all_layouts():
    return {**LAYOUTS, **EXTRA_LAYOUTS}


def _layout(name):
    return LAYOUTS[name] if name in LAYOUTS else EXTRA_LAYOUTS[name]


ONES = np.ones(128, np.int64)


class Case:
    def __init__(self, name, family, layout, w, h, planes, qt=None, restart=0, progressive=None, strong=None):
        self.name, self.family, self.layout, self.w, self.h = name, family, layout, w, h
        self.planes = [np.ascontiguousarray(p, np.int16) for p in planes]  # [bh][bw][64], zigzag order, quantised
        self.qt = np.asarray(ONES if qt is None else qt, np.int64)          # [2][64] zigzag: table 0 (component 0), table 1 (the others)
        self.restart, self.progressive = restart, progressive               # progressive: None (baseline) or the writer's script 0 / 1
        self.strong = strong                                                # (component, block row, block column) of the one strong block
        if progressive is not None and len(self.planes) > 1:
            # the AC scans of a progressive file carry one component each and, like every non-interleaved scan, only the blocks that hold
            # picture (T.81 A.2.2): the AC terms of the MCU padding are not in the stream, only its DC terms (interleaved scan) are
            hv, _ = _layout(layout)
            hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
            for p, (hh, vv) in zip(self.planes, hv):
                cw, ch = ((w * hh + hmax - 1) // hmax + 7) // 8, ((h * vv + vmax - 1) // vmax + 7) // 8
                p[ch:, :, 1:] = 0
                p[:, cw:, 1:] = 0
        self._bytes = None

    @property
    def sixteen_bit(self):
        return bool((self.qt > 255).any())

    def q_of(self, c):
        return self.qt[:64] if c == 0 else self.qt[64:]

    def quantised(self):
        """per component [bh, bw, 8, 8], natural order"""
        return [M.zz_to_nat(p) for p in self.planes]

    def dequantised(self):
        return [M.zz_to_nat(M.dequant(p.astype(np.int64), self.q_of(c))) for c, p in enumerate(self.planes)]

    def max_l1(self):
        return max(int(M.block_l1(p.astype(np.int64), self.q_of(c)).max()) for c, p in enumerate(self.planes))

    def needs_wide(self):
        return self.max_l1() > M.L1_LIMIT

    def dc_category(self):
        """the largest category (bits) of a DC difference in the stream.  T.81 stops at 11 for 8-bit samples and every conforming stream
        does; the reference takes any, and so does the host walk, but the GPU walk keeps DC differences in twelve bits and hands a stream
        with a larger one back to the host (mij_entropy_kernels.h: the anomaly list, the DC record)"""
        worst = 0
        for c, p in enumerate(self.planes):
            mcu, by, bx = scan_order(self.layout, self.w, self.h, c)
            dc = p[by, bx, 0].astype(np.int64)
            pred = np.concatenate([[0], dc[:-1]])
            if self.restart:
                pred[np.concatenate([[False], (mcu[1:] != mcu[:-1]) & (mcu[1:] % self.restart == 0)])] = 0
            worst = max(worst, int(np.abs(dc - pred).max()))
        return worst.bit_length()

    def stream(self):
        if self._bytes is None:
            self._bytes = _write(self)
        return self._bytes


def geometry(layout, w, h):
    """-> (mcu_x, mcu_y, [(bh, bw) per component])"""
    hv, _ = _layout(layout)
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    mcu_x, mcu_y = (w + 8 * hmax - 1) // (8 * hmax), (h + 8 * vmax - 1) // (8 * vmax)
    return mcu_x, mcu_y, [(mcu_y * v, mcu_x * hh) for hh, v in hv]


def scan_order(layout, w, h, comp):
    """-> (MCU index, block row, block column) of component `comp`'s blocks in the order an interleaved scan codes them"""
    hv, _ = _layout(layout)
    mcu_x, mcu_y, _ = geometry(layout, w, h)
    hh, vv = hv[comp]
    m = np.repeat(np.arange(mcu_x * mcu_y), hh * vv)
    k = np.tile(np.arange(hh * vv), mcu_x * mcu_y)
    return m, (m // mcu_x) * vv + k // hh, (m % mcu_x) * hh + k % hh


def blank(layout, w, h):
    return [np.zeros((bh, bw, 64), np.int16) for bh, bw in geometry(layout, w, h)[2]]


def sixteen_bit_tables(data, qt):
    """Rewrite every DQT segment of a finished stream (one table of 64 bytes each, as the writer emits them) as Pq = 1 with 128 bytes"""
    out, i = bytearray(), 0
    data = bytes(data)
    while True:
        j = data.find(b"\xff\xdb\x00\x43", i)
        if j < 0 or j > data.index(b"\xff\xda"):
            break
        t = data[j + 4] & 15
        out += data[i:j] + b"\xff\xdb\x00\x83" + bytes([0x10 | t])
        for k in range(64):
            v = int(qt[64 * t + k])
            out += bytes([v >> 8, v & 255])
        i = j + 5 + 64
    return bytes(out + data[i:])


def _write(case):
    L = C.CDLL(helpers.build_prog_writer())
    hv, app14 = _layout(case.layout)
    n_c = len(hv)
    for p, (bh, bw) in zip(case.planes, geometry(case.layout, case.w, case.h)[2]):
        assert p.shape == (bh, bw, 64), (case.name, p.shape, bh, bw)
    ptrs = (C.c_void_p * n_c)(*[p.ctypes.data for p in case.planes])
    hs, vs = (C.c_int * n_c)(*[a for a, _ in hv]), (C.c_int * n_c)(*[b for _, b in hv])
    q8 = np.where(case.qt > 255, 1, case.qt).astype(np.uint8)  # placeholders where the real entry needs sixteen bits
    cap = 8192 + sum(p.size for p in case.planes) * 4
    out = np.empty(cap, np.uint8)
    if case.progressive is None:
        L.pw_write_baseline_ex.restype = C.c_long
        L.pw_write_baseline_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, helpers.P_INT, helpers.P_INT, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long]
        n = L.pw_write_baseline_ex(ptrs, n_c, case.w, case.h, hs, vs, q8.ctypes.data_as(C.c_void_p), int(case.restart), int(app14), out.ctypes.data_as(C.c_void_p), cap)
    else:
        assert app14 < 0 and not case.restart
        L.pw_write_progressive.restype = C.c_long
        L.pw_write_progressive.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, helpers.P_INT, helpers.P_INT, C.c_void_p, C.c_int, C.c_void_p, C.c_long]
        n = L.pw_write_progressive(ptrs, n_c, case.w, case.h, hs, vs, q8.ctypes.data_as(C.c_void_p), int(case.progressive), out.ctypes.data_as(C.c_void_p), cap)
    assert 0 < n <= cap, (case.name, n)
    data = out[:n].tobytes()
    return sixteen_bit_tables(data, case.qt) if case.sixteen_bit else data


# ---------------------------------------------------------------- wavefronts of the kernels that classify

def wave_members(path, comp, bh, bw, luma_h=1, luma_v=1):
    """The blocks (by, bx) of every wavefront that transforms component `comp` in kernel family `path`, read off the kernels
    (mij_kernels.h): k_idct_planes, k_fused_grey and k_fused1x1c give a lane block L = first + lane of the plane in raster order, whole
    plane, 64 at a time; the band kernels (fused_band: 4:2:0 and 4:4:0; fused422) go MCU row by MCU row, luma as the luma_v block rows of
    the MCU row back to back, chroma one block row, each cut into wavefronts of 64 -- a new wavefront starts with every MCU row."""
    waves = []
    if path in (2, 5, 7, 3):
        L = np.arange(bh * bw)
        for s in range(0, bh * bw, 64):
            waves.append((L[s:s + 64] // bw, L[s:s + 64] % bw))
        return waves
    rows_per_mcu = luma_v if comp == 0 else 1
    for m in range(bh // rows_per_mcu):
        i = np.arange(rows_per_mcu * bw)
        by, bx = rows_per_mcu * m + i // bw, i % bw
        for s in range(0, i.size, 64):
            waves.append((by[s:s + 64], bx[s:s + 64]))
    return waves


def expected_class_counts(case, path, compact, wide):
    """[DC only, 2x2, 4x4, full] wavefronts of one launch, from the picture's planes and the kernel's geometry alone.  A wavefront takes
    the widest class among its blocks; compact planes make an escaped block class 3 (its flag is part of the test, block_class_b8), int16
    planes classify by extent alone (block_class_i16); a WIDE picture runs the full transform throughout."""
    hv, _ = LAYOUTS[case.layout]
    counts = [0, 0, 0, 0]
    for c, nat in enumerate(case.quantised()):
        cls = M.block_class(nat)
        if compact:
            cls = np.where(M.escaped(nat), 3, cls)
        if wide:
            cls = np.full_like(cls, 3)
        for by, bx in wave_members(path, c, nat.shape[0], nat.shape[1], hv[0][0], hv[0][1]):
            counts[int(cls[by, bx].max())] += 1
    return counts


# ---------------------------------------------------------------- pieces

def _tame(planes, seed=0):
    """small DC everywhere and a few small AC terms in some blocks: L1 far below the limit, everything inside a byte"""
    for c, p in enumerate(planes):
        bh, bw, _ = p.shape
        i = np.arange(bh * bw).reshape(bh, bw) + 17 * c + seed
        p[:, :, 0] = (i * 7) % 41 - 20
        p[:, :, 1] = np.where(i % 3 == 0, (i % 9) - 4, 0)
        p[:, :, 2] = np.where(i % 4 == 1, 3 - (i % 7), 0)
        p[:, :, 4] = np.where(i % 5 == 2, 2, 0)
    return planes


ROW0_W = M.first_pass_weights()[0]  # weights of a column's eight inputs in first-pass output row 0: 4096, 5683, ...


def strong_forms():
    """(name, zigzag block of 64 quantised values, tables or None) with L1 exactly `total` for total in 5903, 5904, 5905 -- see the issue's list"""
    out = []
    for total in (5903, 5904, 5905):
        for col in range(8):  # everything on natural row 1 of column `col`: the weight-5683 input of that column's first pass
            for sign in (1, -1):
                b = np.zeros(64, np.int64)
                b[M.ZZ_OF_NAT[8 + col]] = sign * total
                out.append(("row1col%d%s_%d" % (col, "+" if sign > 0 else "-", total), b, None))
        for sign in (1, -1):
            b = np.zeros(64, np.int64)
            b[0] = sign * total
            out.append(("dc%s_%d" % ("+" if sign > 0 else "-", total), b, None))  # alone among small DC terms: a DC difference of category 13
            out.append(("dcramp%s_%d" % ("+" if sign > 0 else "-", total), b, None))  # l1_case ramps the component's DC terms up to it
            b = np.zeros(64, np.int64)
            b[0], b[2] = -900, sign * (total - 900)
            out.append(("dc-900_ac%s_%d" % ("+" if sign > 0 else "-", total), b, None))
            b = np.zeros(64, np.int64)  # ... and with the rest on the last position a block has: a long code right at the block's end
            b[0], b[63] = 900, sign * (total - 900)
            out.append(("dc900_last%s_%d" % ("+" if sign > 0 else "-", total), b, None))
        # spread over all 63 AC terms with the signs of first-pass output row 0's weights: the block that makes the most of its L1 there
        nat = np.zeros((8, 8), np.int64)
        share, extra = divmod(total, 63)
        k = 0
        for r in range(8):
            for c in range(8):
                if r or c:
                    nat[r, c] = (share + (1 if k < extra else 0)) * (1 if ROW0_W[r] >= 0 else -1)
                    k += 1
        out.append(("spread63_%d" % total, M.nat_to_zz(nat), None))
        # only coefficients inside a byte, -128 among them, under an 8-bit table with entries above one
        q = np.array([1 + (k % 7) for k in range(64)] * 2, np.int64)
        b = np.zeros(64, np.int64)
        b[1] = -128
        rem = total - 128 * int(q[1])
        for k in list(range(2, 63)) + [63]:
            if k % 7 == 0 and k != 63:
                continue
            v = min(127, rem // int(q[k]))
            b[k] = v if k & 1 else -v
            rem -= v * int(q[k])
        for k in range(7, 63, 7):
            v = min(127, rem)
            b[k] = -v
            rem -= v
        assert rem == 0 and np.abs(b).max() <= 128
        out.append(("bytes_q7_%d" % total, b, q))
        # products that wrap: 257 * 255 = 65535 -> (short) -1, and the other sign -> +1; the rest on a position whose quantiser is one
        for sign in (1, -1):
            q = ONES.copy()
            q[5] = q[64 + 5] = 255
            b = np.zeros(64, np.int64)
            b[5], b[2] = sign * 257, -sign * (total - 1)
            out.append(("wrap%s_%d" % ("+" if sign > 0 else "-", total), b, q))
        # a 16-bit table: 19 * 300 = 5700 and the rest on a quantiser of one; and one coefficient of one under a quantiser of `total`
        q = ONES.copy()
        q[3] = q[64 + 3] = 300
        b = np.zeros(64, np.int64)
        b[3], b[1] = -19, total - 5700
        out.append(("q300_%d" % total, b, q))
        q = ONES.copy()
        q[9] = q[64 + 9] = total
        q[0] = q[64] = 257
        b = np.zeros(64, np.int64)
        b[9] = -1
        out.append(("q%d_times_one" % total, b, q))
    # exactly -32768, from either side, and a product far beyond int16 that wraps back to something small
    for name, coef, qq in (("m32768_a", -16384, 2), ("m32768_b", 16384, 2), ("m32768_c", -128, 256), ("wrap_small", 1285, 51)):
        q = ONES.copy()
        q[2] = q[64 + 2] = qq
        b = np.zeros(64, np.int64)
        b[2] = coef
        out.append((name, b, q))
    return out


def _first_pass_peak(b_zz, q):
    return int(np.abs(M.first_pass(M.zz_to_nat(M.dequant(b_zz, q[:64])))).max())


# ---------------------------------------------------------------- the families

SIZE_ONE = {"420": (1040, 32), "440": (520, 32), "422": (1040, 16), "444": (200, 24), "grey": (200, 24), "411": (800, 24), "rgb": (200, 24),
            "cmyk": (200, 24), "ycck": (200, 24)}
EDGE_POSITIONS = [int(M.ZZ_OF_NAT[8 * r + c]) for r, c in ((1, 1), (0, 2), (2, 0), (3, 3), (0, 4), (4, 0), (7, 7))]


def one_position(layout, p, escaped, size=None):
    """every block of every component: a small DC and zigzag position p only, magnitude and sign varying per block; `escaped`: two blocks of
    three hold a value beyond a byte.  Two MCU rows or more, every component with full wavefronts and a partial last one."""
    w, h = size or SIZE_ONE[layout]
    planes = blank(layout, w, h)
    for c, pl in enumerate(planes):
        bh, bw, _ = pl.shape
        i = np.arange(bh * bw).reshape(bh, bw) + 5 * c
        pl[:, :, 0] = (i * 7) % 41 - 20
        small = 1 + (i * 5) % 128                       # 1..128
        small = np.where(i & 1, -small, np.minimum(small, 127))
        big = (128 + (i * 37) % 900) * np.where(i & 2, -1, 1)
        pl[:, :, p] = np.where((i % 3 != 0) & bool(escaped), big, small)
    return Case("one_%s_p%d_%s_%dx%d" % (layout, p, "esc" if escaped else "byte", w, h), "one", layout, w, h, planes)


ODD_POS = {1: [(1, 1), (0, 1), (1, 0), (1, 1), (1, 0)], 2: [(3, 3), (0, 2), (2, 0), (3, 0), (2, 2)], 3: [(7, 7), (0, 4), (4, 0), (5, 2), (3, 4)]}


def odd_lane(layout, cls, place, size=None):
    """every component DC-only except ONE block of class `cls`: in component place % ncomp, lane 0 / 31 / 32 / 63 of a full wavefront
    (place 0..3) or the last lane of the partial last wavefront (place 4) of the picture's own kernel family"""
    w, h = size or SIZE_ONE[layout]
    planes = blank(layout, w, h)
    hv, _ = LAYOUTS[layout]
    for c, pl in enumerate(planes):
        bh, bw, _ = pl.shape
        i = np.arange(bh * bw).reshape(bh, bw) + 3 * c
        pl[:, :, 0] = (i * 11) % 61 - 30
    comp = place % len(planes)
    bh, bw, _ = planes[comp].shape
    waves = wave_members(PATH_OF[layout], comp, bh, bw, hv[0][0], hv[0][1])
    full = [wv for wv in waves if wv[0].size == 64] or waves   # a picture narrower than a wavefront has partial ones only
    part = [wv for wv in waves if wv[0].size < 64] or waves
    if place < 4:
        wv = full[(place + cls) % len(full)]
        lane = min((0, 31, 32, 63)[place], wv[0].size - 1)
    else:
        wv = part[-1]
        lane = wv[0].size - 1
    r, c2 = ODD_POS[cls][place]
    by, bx = int(wv[0][lane]), int(wv[1][lane])
    planes[comp][by, bx, M.ZZ_OF_NAT[8 * r + c2]] = -3 if place & 1 else 2
    return Case("odd_%s_c%d_place%d_%dx%d" % (layout, cls, place, w, h), "odd", layout, w, h, planes, strong=(comp, by, bx))


def edge_pairs(layout, size=None):
    """blocks on either side of each class edge side by side: natural (1,1) | (0,2) | (2,0) | (3,3) | (0,4) | (4,0) | (7,7), one position
    per block, cycling along the plane -- every wavefront mixes classes 1, 2 and 3"""
    w, h = size or SIZE_ONE[layout]
    planes = blank(layout, w, h)
    for c, pl in enumerate(planes):
        bh, bw, _ = pl.shape
        i = np.arange(bh * bw).reshape(bh, bw)
        pl[:, :, 0] = (i * 13) % 51 - 25
        for k, p in enumerate(EDGE_POSITIONS):
            pl[:, :, p] = np.where((i + c) % 7 == k, np.where(i & 1, -1 - (i % 100), 1 + (i % 90)), 0)
    return Case("edges_%s_%dx%d" % (layout, w, h), "edges", layout, w, h, planes)


# a width for each form of the band kernels (mij_runtime.hip, band_form / band_segments, 160 KiB of LDS): one, two, four, eight, sixteen
# waves per workgroup, and column segments (4:2:0 beyond 5840 pixels, 4:4:0 beyond 4300).  The form launched is not visible through the
# binding: it follows from the width.
BAND_WIDTHS = {"420": (336, 880, 1040, 2320, 3000, 5856), "440": (520, 1600, 4312), "422": (336, 880, 1040, 3424, 5136)}
BAND_HEIGHT = {"420": 32, "440": 32, "422": 16}
SEG_WIDTH = {"420": 5840, "440": 4300}


def edge_cases(layout, size=None):
    """the class-edge pictures of one layout and size: the seven edge positions alone (inside a byte and beyond), the pairs, one odd lane"""
    cases = [one_position(layout, p, esc, size) for p in EDGE_POSITIONS for esc in (False, True)]
    cases.append(edge_pairs(layout, size))
    cases += [odd_lane(layout, cls, place, size) for cls in (1, 2, 3) for place in range(5)]
    return cases


SIZE_L1 = {"420": (72, 40), "444": (40, 24), "422": (72, 24), "grey": (40, 24), "440": (40, 40), "411": (72, 24), "rgb": (40, 24), "cmyk": (40, 24),
           "ycck": (40, 24)}


def l1_case(layout, form, comp=0, where="mid", restart=0, progressive=None, escaped_neighbour=False, size=None):
    """a tame picture with one strong block (form = (name, zigzag values, tables)) in component `comp` at `where`:
    first / last / mid block of the plane, "pad": in the MCU padding beyond the picture's edge, (by, bx): there"""
    name, b, q = form
    w, h = size or SIZE_L1[layout]
    planes = _tame(blank(layout, w, h), seed=len(name))
    bh, bw, _ = planes[comp].shape
    if where == "first":
        by, bx = 0, 0
    elif where == "last":
        by, bx = bh - 1, bw - 1
    elif where == "mid":
        by, bx = bh // 2, bw // 2 - 1
    elif where == "pad":
        hv, _ = LAYOUTS[layout]
        hmax, vmax = max(a for a, _ in hv), max(v for _, v in hv)
        real_w = ((w * hv[comp][0] + hmax - 1) // hmax + 7) // 8
        real_h = ((h * hv[comp][1] + vmax - 1) // vmax + 7) // 8
        assert real_w < bw or real_h < bh, ("no MCU padding in this component", layout, comp)
        by, bx = (1, bw - 1) if real_w < bw else (bh - 1, 1)
    else:
        by, bx = where
    if name.startswith("dcramp"):
        # the component's other DC terms rise to 4000 in steps a conforming stream can code (DC differences of category 11 at most), so that
        # the strong block's own difference is one too; their L1 stays far below the limit
        _, oy, ox = scan_order(layout, w, h, comp)
        sign = 1 if b[0] > 0 else -1
        planes[comp][oy, ox, 0] += sign * np.minimum(4000, 1900 * (np.arange(oy.size) + 1))
    planes[comp][by, bx] = b
    if escaped_neighbour:  # a block beyond a byte elsewhere in the strong block's tile of 64: the walk's pack kernel leaves its byte-only sum
        oy, ox = (by, bx - 1) if bx else (by, bx + 1)
        assert (oy * bw + ox) // 64 == (by * bw + bx) // 64
        planes[comp][oy, ox, 6] = 200
    tag = "%s_%s_c%d_%s%s%s%s" % (layout, name, comp, where if isinstance(where, str) else "at%d_%d" % where, "_rst%d" % restart if restart else "",
                                  "_prog%d" % progressive if progressive is not None else "", "_escnb" if escaped_neighbour else "")
    return Case("l1_" + tag, "l1", layout, w, h, planes, qt=q, restart=restart, progressive=progressive, strong=(comp, by, bx))


def l1_family(layout, progressive=None):
    """the L1-limit family of one layout (baseline, or the progressive twins with `progressive` = the writer's script)"""
    forms = strong_forms()
    by_name = {f[0]: f for f in forms}
    ncomp = len(LAYOUTS[layout][0])
    out = [l1_case(layout, f, progressive=progressive) for f in forms]
    if progressive is None:
        for total in (5903, 5904, 5905):
            out.append(l1_case(layout, by_name["bytes_q7_%d" % total], escaped_neighbour=True))
            out.append(l1_case(layout, by_name["spread63_%d" % total], escaped_neighbour=True))
    # placements: first, last, MCU padding, either side of a restart marker, every component in turn
    for total in (5903, 5904, 5905):
        f = by_name["row1col0%s_%d" % ("+" if total & 1 else "-", total)]
        g = by_name["dc-900_ac+_%d" % total]
        for comp in range(ncomp):
            out.append(l1_case(layout, f, comp, "first", progressive=progressive))
            out.append(l1_case(layout, g, comp, "last", progressive=progressive))
        geo = geometry(layout, *SIZE_L1[layout])
        if layout in ("420", "422", "440", "411"):
            # (a progressive file keeps only the DC term of a padding block)
            out.append(l1_case(layout, f if progressive is None else by_name["dc%s_%d" % ("+" if total & 1 else "-", total)], 0, "pad", progressive=progressive))
        if progressive is None:
            # restart interval of two MCUs: the last block of MCU 1 (last before RST0) and the first block of MCU 2 (first after it)
            mcu_x = geo[0]
            hv = LAYOUTS[layout][0]
            last_c = ncomp - 1
            m1x, m1y = 1 % mcu_x, 1 // mcu_x
            out.append(l1_case(layout, g, last_c, (m1y * hv[last_c][1] + hv[last_c][1] - 1, m1x * hv[last_c][0] + hv[last_c][0] - 1), restart=2))
            m2x, m2y = 2 % mcu_x, 2 // mcu_x
            out.append(l1_case(layout, f, 0, (m2y * hv[0][1], m2x * hv[0][0]), restart=2))
    return out


def dc_sweep(layout, neighbour_class):
    """DC-only blocks whose dc * q0 runs from below the clamp at 0 to above the clamp at 255 in steps of one (component 0: -1040 .. 1040 along the
    plane and back; the others: a stride of four, and both clamp regions densely); neighbour_class 1 / 2 / 3: lane 5 of every 64 blocks carries one AC
    term of that class next to them (0: none, every wavefront is class 0)"""
    w, h = {"420": (512, 272), "444": (512, 264), "422": (512, 136), "grey": (512, 264), "440": (256, 528), "411": (1024, 136), "rgb": (512, 264),
            "cmyk": (512, 264), "ycck": (512, 264)}[layout]
    planes = blank(layout, w, h)
    for c, pl in enumerate(planes):
        bh, bw, _ = pl.shape
        i = np.arange(bh * bw).reshape(bh, bw)
        # up and down again, so that no DC difference is larger than a conforming stream's (the scan visits a 4:2:0 MCU's luma blocks in
        # two rows: still neighbours)
        tri = lambda t: np.where(t % 4160 <= 2080, t % 4160, 4160 - t % 4160) - 1040
        if c == 0 or bh * bw >= 2081:
            v = tri(i)
        elif c == 1:
            v = tri(4 * i)
        else:
            dense = np.concatenate([np.arange(-1040, -899), np.arange(900, 1041)])
            dense = np.concatenate([dense, dense[::-1]])
            v = dense[i % dense.size]
        pl[:, :, 0] = v
        if neighbour_class:
            r, cc = ODD_POS[neighbour_class][c % 5]
            pl[:, :, M.ZZ_OF_NAT[8 * r + cc]] = np.where(i % 64 == 5, 1, 0)
    return Case("dc_%s_n%d" % (layout, neighbour_class), "dc", layout, w, h, planes)


GRID = [0, 1, 32, 64, 96, 127, 128, 129, 160, 192, 224, 254, 255]


def colour_grid(layout):
    """flat blocks whose samples (Y, Cb, Cr) run over all of GRID^3: every clamp of the colour row at both ends.  A flat block of sample s
    has DC 8 s - 1024.  4:4:4 and the 1x1 colour layouts: one block per triple (the fourth plane of CMYK / YCCK: the first reversed);
    4:2:0: one MCU per chroma pair and four luma values."""
    n = len(GRID)
    g = np.array(GRID)
    if layout == "420":
        w, h = 16 * 52, 16 * 13
        planes = blank(layout, w, h)
        m = np.arange(52 * 13).reshape(13, 52)          # MCU index: chroma pair m // 4 (169 pairs x 4 luma quadruples)
        pair, quad = m // 4, m % 4
        planes[1][:, :, 0] = 8 * g[pair // n] - 1024
        planes[2][:, :, 0] = 8 * g[pair % n] - 1024
        for dy in range(2):
            for dx in range(2):
                planes[0][dy::2, dx::2, 0] = 8 * g[(4 * quad + 2 * dy + dx) % n] - 1024
    else:
        w, h = 8 * 169, 8 * 13
        planes = blank(layout, w, h)
        t = np.arange(n ** 3).reshape(13, 169)
        planes[0][:, :, 0] = 8 * g[t // (n * n)] - 1024
        planes[1][:, :, 0] = 8 * g[(t // n) % n] - 1024
        planes[2][:, :, 0] = 8 * g[t % n] - 1024
        if len(planes) == 4:
            planes[3][:, :, 0] = planes[0][::-1, ::-1, 0]
    return Case("colour_%s" % layout, "colour", layout, w, h, planes)


# ---------------------------------------------------------------- where a block lies in its entropy-coded segment

def block_bit_ranges(data):
    """A plain baseline Huffman walk over a one-scan stream without restart markers: -> ([(first bit, end bit) of every block in scan
    order], bits of the segment), in bits of the UNSTUFFED entropy-coded segment (the GPU walk cuts the unstuffed stream into subsequences)."""
    data = bytes(data)
    tabs, comps, i = {}, [], 2
    while True:
        assert data[i] == 0xFF
        m, n = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        seg = data[i + 4:i + 2 + n]
        if m == 0xC4:
            j = 0
            while j < len(seg):
                tc_th, counts = seg[j], seg[j + 1:j + 17]
                vals = seg[j + 17:j + 17 + sum(counts)]
                code, k, lut = 0, 0, {}
                for ln in range(1, 17):
                    for _ in range(counts[ln - 1]):
                        lut[(ln, code)] = vals[k]
                        code += 1
                        k += 1
                    code <<= 1
                tabs[tc_th] = lut
                j += 17 + len(vals)
        elif m == 0xC0:
            comps = [(seg[6 + 3 * c + 1] >> 4, seg[6 + 3 * c + 1] & 15) for c in range(seg[5])]
            height, width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
        elif m == 0xDD:
            raise AssertionError("restart intervals are not walked here")
        elif m == 0xDA:
            sel = [seg[1 + 2 * c + 1] for c in range(seg[0])]
            i += 2 + n
            break
        i += 2 + n
    s, e = helpers.entropy_ranges(data)[0]
    assert s == i
    raw = data[s:e].replace(b"\xff\x00", b"\xff")
    bits = np.unpackbits(np.frombuffer(raw, np.uint8))
    hmax, vmax = max(a for a, _ in comps), max(b for _, b in comps)
    nmcu = ((width + 8 * hmax - 1) // (8 * hmax)) * ((height + 8 * vmax - 1) // (8 * vmax))
    pos, out = 0, []

    def sym(lut):
        nonlocal pos
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | int(bits[pos])
            pos += 1
            if (ln, code) in lut:
                return lut[(ln, code)]
        raise AssertionError("bad code")

    for _ in range(nmcu):
        for c, (hh, vv) in enumerate(comps):
            for _b in range(hh * vv):
                start = pos
                cat = sym(tabs[sel[c] >> 4])  # (not pos += sym(...): the walk moves pos itself)
                pos += cat
                k = 1
                while k < 64:
                    rs = sym(tabs[0x10 | (sel[c] & 15)])
                    if rs == 0:
                        break
                    if rs == 0xF0:
                        k += 16
                        continue
                    k += (rs >> 4) + 1
                    pos += rs & 15
                out.append((start, pos))
    return out, 8 * len(raw)


SIZE_STRADDLE = {"420": (136, 72), "444": (72, 40), "422": (136, 40), "grey": (136, 72), "440": (72, 72), "411": (136, 40), "rgb": (72, 40)}


def straddle_case(layout, form, comp=0):
    """-> (case, bits): the strong block placed (first place in raster order that does it) so that it begins in one subsequence of `bits`
    bits (1024 or more) and ends in a later one"""
    bh, bw = geometry(layout, *SIZE_STRADDLE[layout])[2][comp]
    for by in range(bh):
        for bx in range(1, bw):
            case = l1_case(layout, form, comp, (by, bx), size=SIZE_STRADDLE[layout])
            bits = straddling_bits(case, (1024, 2048))
            if bits:
                return case, bits
    raise AssertionError("no place straddles")


def straddling_bits(case, choices=(1024, 1280, 1536, 2048, 3072)):
    """a subsequence length (>= 1024 bits) at which the case's strong block begins in one subsequence and ends in a later one, or None"""
    ranges, _ = block_bit_ranges(case.stream())
    hv, _ = LAYOUTS[case.layout]
    comp, by, bx = case.strong
    mcu_x = geometry(case.layout, case.w, case.h)[0]
    per = [a * b for a, b in hv]
    my, mx = by // hv[comp][1], bx // hv[comp][0]
    idx = (my * mcu_x + mx) * sum(per) + sum(per[:comp]) + (by % hv[comp][1]) * hv[comp][0] + bx % hv[comp][0]
    s, e = ranges[idx]
    for bits in choices:
        if s // bits != (e - 1) // bits:
            return bits
    return None


def straddle_cases():
    """-> [(case, bits)]: the spread and the byte-only strong block at each total, in every layout the GPU walk serves"""
    forms = {f[0]: f for f in strong_forms()}
    return [straddle_case(layout, forms[form % total]) for layout in GPU_WALK_LAYOUTS for total in (5903, 5904, 5905) for form in ("spread63_%d", "bytes_q7_%d")]


def everything():
    """every case test_gpu_coef_contract.py sends to the GPU (test_coef_contract_host.py decodes them all in the oracle, twice)"""
    cases = []
    for layout in LAYOUTS:
        cases += l1_family(layout)
        cases += edge_cases(layout)
        cases += [dc_sweep(layout, n) for n in range(4)]
        cases += [one_position(layout, p, esc) for p in range(1, 64) for esc in (False, True)]
    for layout in ("420", "444", "422", "grey"):
        for script in (0, 1):
            cases += l1_family(layout, progressive=script)
    for layout in BAND_WIDTHS:
        for w in BAND_WIDTHS[layout]:
            if (w, BAND_HEIGHT[layout]) != SIZE_ONE[layout]:
                cases += edge_cases(layout, (w, BAND_HEIGHT[layout]))
    cases += [colour_grid(l) for l in ("444", "420", "rgb", "cmyk", "ycck")]
    cases += [c for c, _ in straddle_cases()]
    seen, out = set(), []
    for c in cases:  # the edge positions are among the 63: once is enough
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    return out
