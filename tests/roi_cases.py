"""What the region-of-interest tests share (test_gpu_roi.py, test_gpu_roi_seams.py, test_roi_host.py): the dense pictures and
their whole-picture decodes, the paint-and-compare run of one batch, and -- for the seam tests -- the window lists with the number of work
items the planner (mij_runtime.hip: plan_decode, push_region_bands, push_window) has to cut each of them into.  The item counts are
restated here from the planner's rules, not read from it: a planner that stops cutting a region fails the count, one that cuts it onto
wrong pixels fails the comparison.

The rules (units: MCUs of the band kernels, 8 x 8 blocks of the 1 x 1 kernels, MCUs at the scale -- luma blocks in the luma-only form -- of
the reduced-size kernels):
    4:2:0, 4:4:0    ceil(rows / per) bands x ceil(columns / fit) column segments; per = MIJ_BAND_ROWS, 4 when unset; fit = FIT[layout]
    4:2:2           ceil(rows / 8) bands at the picture's width, whatever MIJ_BAND_ROWS says
    windowed        ceil(units / 256)
"""
import ctypes as C

import numpy as np

import coef_cases as CC
import orient_model as om
import scaled_model as SM

MB = 1 << 20
# full-size MCU in pixels per layout
MCU = {"420": (16, 16), "422": (16, 8), "440": (8, 16), "444": (8, 8), "grey": (8, 8), "cmyk": (8, 8), "411": (32, 8)}

# LDS bytes per MCU column of the band kernels (mij_runtime.hip, LDS_COL_420 / LDS_COL_440: luma, two chroma blocks, the chroma halo rows and the
# row sums) and the MCU columns of one column segment: two workgroups of a segment and its two halo columns share a CU's 160 KiB
# (band_segments): 163840 // (2 * 448) - 2 = 180 for 4:2:0, 163840 // (2 * 304) - 2 = 267 for 4:4:0
LDS_BYTES = 160 * 1024
LDS_COL = {"420": 16 * 16 + 2 * 8 * 8 + 2 * 16 + 4 * 8, "440": 16 * 8 + 2 * 8 * 8 + 2 * 8 + 4 * 8}
FIT = {k: LDS_BYTES // (2 * v) - 2 for k, v in LDS_COL.items()}

_cache = {}


def dense(layout, size, seed=0):
    """every position of every block in use: small values, a DC ramp, and every seventh block with values beyond a byte (escaped)"""
    k = ("dense", layout, size, seed)
    if k not in _cache:
        w, h = size
        r = np.random.default_rng(1000 * seed + w * 7 + h)
        planes = CC.blank(layout, w, h)
        for pl in planes:
            bh, bw, _ = pl.shape
            pl[:] = r.integers(-9, 10, pl.shape)
            pl[:, :, 0] = r.integers(-300, 301, (bh, bw))
            i = np.arange(bh * bw).reshape(bh, bw)
            pl[:, :, 1:6] += np.where((i % 7 == 3)[:, :, None], r.integers(-700, 701, (bh, bw, 5)), 0).astype(np.int16)
        _cache[k] = CC.Case("roi_%s_%dx%d_%d" % (layout, w, h, seed), "dense", layout, w, h, planes)
    return _cache[k]


def want(oracle, case, req, s=1):
    """the whole-picture decode: computed once per (case, channels, scale), shared, never changed"""
    k = ("want", case.name, req, s)
    if k not in _cache:
        if s == 1:
            kind, px, _ = oracle.load(case.stream(), req)
            assert kind == "ok", case.name
        else:
            px = SM.scaled_picture(case.dequantised(), case.layout, (case.w, case.h), s, req)
        px.setflags(write=False)
        _cache[k] = px
    return _cache[k]


_hip = []


def hip():
    """the HIP runtime this process has already loaded"""
    if not _hip:
        with open("/proc/self/maps") as f:
            path = next(ln.split()[-1] for ln in f if "libamdhip64" in ln)
        h = C.CDLL(path)
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.append(h)
    return _hip[0]


def paint(ica, b, slot, nbytes, seed):
    """fills the slot's output region on the device with a byte pattern; -> the pattern"""
    L = ica.lib()
    L.mij_batch_device_out.restype = C.c_void_p
    L.mij_batch_device_out.argtypes = [C.c_void_p, C.c_int]
    pat = np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
    dst = L.mij_batch_device_out(b._h, int(slot))
    assert dst
    assert hip().hipMemcpy(C.c_void_p(dst), pat.ctypes.data_as(C.c_void_p), nbytes, 1) == 0
    assert hip().hipDeviceSynchronize() == 0
    return pat


def read_back(ica, b, slot, shape):
    """the slot's output region as it is on the device, for a slot that mij_batch_fetch refuses (a skipped one)"""
    L = ica.lib()
    L.mij_batch_device_out.restype = C.c_void_p
    L.mij_batch_device_out.argtypes = [C.c_void_p, C.c_int]
    out = np.empty(shape, np.uint8)
    src = L.mij_batch_device_out(b._h, int(slot))
    assert src
    assert hip().hipDeviceSynchronize() == 0
    assert hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(src), out.size, 2) == 0
    return out


def bound(path, win, W, H, mw, mh):
    """the contract's bound on the decoded rectangle, as (x0, y0, x1, y1), for the kernel family the slot took (mij_batch_slot_path): the
    region rounded out to MCUs, one MCU more on each side, clipped; 4:2:2 band kernel (4): rows only; two-pass (2): the whole picture"""
    x0, y0, w, h = win
    if path == 2:
        return (0, 0, W, H)
    bx0, bx1 = max(0, x0 // mw * mw - mw), min(W, -(-(x0 + w) // mw) * mw + mw)
    by0, by1 = max(0, y0 // mh * mh - mh), min(H, -(-(y0 + h) // mh) * mh + mh)
    return (0, by0, W, by1) if path == 4 else (bx0, by0, bx1, by1)


def stored_window(sw, sh, o, crop):
    """the rectangle of the sw x sh stored picture that a crop (x0, y0, w, h) of the displayed picture (orientation o) reads, found by
    orienting a picture of pixel indices: independent of the runtime's mapping"""
    idx = np.arange(sw * sh, dtype=np.int64).reshape(sh, sw)
    x0, y0, w, h = crop
    sub = om.orient(idx, o)[y0:y0 + h, x0:x0 + w]
    assert sub.shape == (h, w)
    rows, cols = sub // sw, sub % sw
    return int(cols.min()), int(rows.min()), int(cols.max() - cols.min() + 1), int(rows.max() - rows.min() + 1)


def rounded_out(win, sw, sh, uw, uh, rows_only):
    """the window rounded out to units of uw x uh stored pixels and clipped; rows_only: at the picture's width (4:2:2 band kernel)"""
    x0, y0, w, h = win
    rx0, rx1 = (0, sw) if rows_only else (x0 // uw * uw, min(sw, -(-(x0 + w) // uw) * uw))
    ry0, ry1 = y0 // uh * uh, min(sh, -(-(y0 + h) // uh) * uh)
    return rx0, ry0, rx1 - rx0, ry1 - ry0


def unit_px(layout, req, s):
    """the lane unit of the family a (layout, channels, scale) slot takes, in stored pixels: (width, height, rows only), or None for the
    two-pass path, which has no windowed form (mij_runtime.hip, classify and apply_region)"""
    if s > 1:  # reduced-size: MCUs at the scale; luma blocks when only the luma is asked for
        n = 8 // s
        return (n * (2 if req >= 3 and layout in ("420", "422") else 1), n * (2 if req >= 3 and layout == "420" else 1), False)
    if req < 3:  # the grey kernel over the luma plane, where that plane has the picture's resolution
        return (8, 8, False) if layout != "cmyk" else None
    if layout == "411":
        return None
    return MCU[layout] + (layout == "422",)


def expected_path(layout, req, s):
    """mij_batch_slot_path of a slot without force_generic"""
    return 8 if s > 1 else 5 if req < 3 and layout != "cmyk" else CC.PATH_OF[layout] if req >= 3 else 2


def expected_items(layout, req, s, size, win, band_rows=0):
    """work items of a slot with region `win` (x0, y0, w, h in stored pixels; None: no region) on a `size` picture, by the rules in this
    module's docstring.  Slots without a region in force: one item per 256 blocks (1 x 1 kernels) or per 256 units (reduced-size), per four
    picture rows (two-pass, MIJ_RESAMPLE_ROWS), ceil(MCU rows / 8) (4:2:2); 4:2:0 and 4:4:0 only with MIJ_BAND_ROWS set, as
    ceil(MCU rows / MIJ_BAND_ROWS) -- left alone, their band count follows the device's CU count (auto_bands)."""
    W, H = -(-size[0] // s), -(-size[1] // s)
    u = unit_px(layout, req, s)
    if u is None:
        return -(-H // 4)
    uw, uh, rows_only = u
    ux, uy = -(-W // uw), -(-H // uh)
    if win is None:
        x0, y0, x1, y1 = 0, 0, ux, uy
    else:
        x0, y0, x1, y1 = win[0] // uw, win[1] // uh, -(-(win[0] + win[2]) // uw), -(-(win[1] + win[3]) // uh)
    if rows_only:
        x0, x1 = 0, ux
    whole = (x0, y0, x1, y1) == (0, 0, ux, uy)  # the planner drops such a region
    cols, rows = x1 - x0, y1 - y0
    if s == 1 and req >= 3 and layout in ("420", "440"):
        if whole:
            assert band_rows > 0, "the band count of a slot without a region follows the device"
            return -(-rows // band_rows)
        return -(-rows // (band_rows or 4)) * -(-cols // FIT[layout])
    if s == 1 and req >= 3 and layout == "422":
        return -(-rows // 8)
    return -(-cols * rows // 256)


def units_needed(layout, req, s, size, win):
    """(units the window needs, units that hold pixels of the picture), in the family's lane units, columns counted for every family"""
    W, H = -(-size[0] // s), -(-size[1] // s)
    uw, uh, _ = unit_px(layout, req, s) or (8, 8, False)  # two-pass: counted in blocks
    return ((-(-(win[0] + win[2]) // uw) - win[0] // uw) * (-(-(win[1] + win[3]) // uh) - win[1] // uh), -(-W // uw) * -(-H // uh))


def check_slot(b, sl, case, req, s, win, pat, px, t, whole_rect=False, items=None):
    """one slot after launch: the assertions of run_windows; win None: a slot without a region, which has to come out whole"""
    H, W, n = px.shape
    mw, mh = MCU[case.layout][0] // s, MCU[case.layout][1] // s
    assert b.out_size(sl) == (W, H), t
    got = b.fetch(sl)
    rx, ry, rw, rh = rect = b.roi_rect(sl)
    path = b.slot_path(sl)
    if win is None:
        assert rect == (0, 0, W, H) and path == expected_path(case.layout, req, s), t + (rect, path)
        assert np.array_equal(got, px), t + ("whole",)
        if items is not None:
            assert b.work_items(sl) == items, t + ("work items", b.work_items(sl), items)
        return rect, got
    x0, y0, w, h = win
    assert np.array_equal(got[y0:y0 + h, x0:x0 + w], px[y0:y0 + h, x0:x0 + w]), t + ("inside", rect)
    outside = np.ones((H, W), bool)
    outside[ry:ry + rh, rx:rx + rw] = False
    assert np.array_equal(got[outside], pat[outside]), t + ("outside", rect, int((got[outside] != pat[outside]).sum()))
    # the decoded rectangle: contains the region, and obeys the bound
    assert rx <= x0 and ry <= y0 and rx + rw >= x0 + w and ry + rh >= y0 + h, t + (rect,)
    assert path == expected_path(case.layout, req, s), t + (path,)
    bx0, by0, bx1, by1 = bound(path, win, W, H, mw, mh)
    assert bx0 <= rx and by0 <= ry and rx + rw <= bx1 and ry + rh <= by1, t + (rect, (bx0, by0, bx1, by1))
    if path in (2, 4):  # no column form: the picture's width; two-pass: the whole picture
        assert rx == 0 and rw == W, t + (rect,)
    if path == 2 or win == (0, 0, W, H):
        assert rect == (0, 0, W, H) and np.array_equal(got, px), t + (rect,)
    if whole_rect:  # what is built rounds out only; and every seam inside the decoded rectangle is exact: the whole rectangle is the plain decode
        u = unit_px(case.layout, req, s)
        assert rect == ((0, 0, W, H) if u is None else rounded_out(win, W, H, *u)), t + (rect,)
        bad = got[ry:ry + rh, rx:rx + rw] != px[ry:ry + rh, rx:rx + rw]
        assert not bad.any(), t + ("rectangle", rect, "rows", sorted({int(v) + ry for v in np.nonzero(bad)[0]})[:24], "differing bytes", int(bad.sum()))
    if items is not None:
        assert b.work_items(sl) == items, t + ("work items", b.work_items(sl), items, rect)
    return rect, got


def run_windows(ica, ctx, oracle, case, req, fmt, s, wins, producer="host", tag=(), whole_rect=False, items=None):
    """one batch, one slot per window: upload, paint, launch, fetch; -> [(window, rect, picture)].  whole_rect: the decoded rectangle is the
    window rounded out to the family's unit and equals the whole-picture decode throughout; items: the work items of each slot
    (mij_batch_slot_work_items), one number per window"""
    b = ica.Batch(ctx, len(wins), 64 * MB, 64 * MB, 128 * MB)
    try:
        b.set_coef_format(fmt)
        if producer == "walk":
            b.entropy_reserve(16 * MB)
            slots = []
            for _ in wins:
                st, sl = b.add_jpeg_stream(case.stream(), req)
                assert st == 1, case.name
                slots.append(sl)
            for sl in b.entropy_run():  # a stream the walk hands back: the host walk redoes it
                b.fallback_prepare(sl)
                d2, _ = ica.HostDecoder.decode(case.stream(), req, out=b.staging(sl))
                if d2.flags:
                    b.set_flags(sl, d2.flags)
        else:
            slots = [b.add_jpeg(case.stream(), req) for _ in wins]
        for sl, win in zip(slots, wins):
            if s > 1:
                b.set_scale(sl, s)
            b.set_roi(sl, *win)
        b.upload()
        b.wait()
        px = want(oracle, case, req, s)
        pats = [paint(ica, b, sl, px.size, 17 + i).reshape(px.shape) for i, sl in enumerate(slots)]
        b.launch()
        b.wait()
        res = []
        for i, (sl, win, pat) in enumerate(zip(slots, wins, pats)):
            t = (case.name, "req %d" % req, fmt, "s %d" % s, producer, win) + tuple(tag)
            rect, got = check_slot(b, sl, case, req, s, win, pat, px, t, whole_rect, None if items is None else items[i])
            res.append((win, rect, got))
        return res
    finally:
        b.close()


# ------------------------------------------------------------------ the seam cases (test_gpu_roi_seams.py; checked on the host by test_roi_host.py)

class Win:
    """one window of a seam case: the rectangle in stored pixels, the channels and scale it is asked for at, and whether its name says that
    it crosses a seam between work items"""

    def __init__(self, name, win, req=3, s=1, seam=True):
        self.name, self.win, self.req, self.s, self.seam = name, tuple(int(v) for v in win), req, s, seam

    def __repr__(self):
        return "Win(%s %s req %d s %d)" % (self.name, self.win, self.req, self.s)


# A. band seams: layout -> picture size; the last MCU row of 4:2:0 holds 8 pixel rows, that of 4:2:2 holds 4
BAND_PICTURES = {"420": (48, 168), "440": (24, 168), "422": (48, 164)}
BAND_ROWS_ENV = (None, "1", "2", "3", "5")


def band_windows(layout, band_rows=0):
    """one window per pair a <= b of first and last MCU row (4:2:2: the pairs of 1, 8, 9, 16 or 17 rows and those that reach the last row), in
    the middle MCU column.  b > a: from the last pixel row of MCU row a to the first of MCU row b, a pixel inside the column on either side
    -- the rounding out does the rest; a == b: the whole MCU.  `seam`: more than one band at this band height.
    (4:2:2 decodes at the picture's width, so its window over all 21 MCU rows is a region the planner drops; the count rule is the same.)"""
    W, H = BAND_PICTURES[layout]
    mw, mh = MCU[layout]
    ny = -(-H // mh)
    assert W == 3 * mw
    out = []
    for a in range(ny):
        for b in range(a, ny):
            if layout == "422" and b - a + 1 not in (1, 8, 9, 16, 17) and b != ny - 1:
                continue
            win = (mw, a * mh, mw, min(mh, H - a * mh)) if a == b else (mw + 1, a * mh + mh - 1, mw - 2, (b - a - 1) * mh + 2)
            n = expected_items(layout, 3, 1, (W, H), win, band_rows)
            out.append(Win("rows%d-%d" % (a, b), win, seam=n > 1))
    return out


# B. bands x segments: layout -> (picture size, window widths in MCU columns from column 5, over MCU rows 1..6: two bands).  One segment takes
# FIT columns: 180 of 4:2:0 (LDS_COL 448 bytes), 267 of 4:4:0 (304 bytes); a wider window is cut in two
SEGMENT_PICTURES = {"420": ((3200, 112), (180, 181, 190)), "440": ((2400, 112), (266, 267, 268, 280))}


def segment_windows(layout):
    (W, H), widths = SEGMENT_PICTURES[layout]
    mw, mh = MCU[layout]
    return [Win("cols%d" % n, (5 * mw + 5, mh + 3, n * mw - 8, 5 * mh - 6)) for n in widths]


# C. the windowed 1 x 1 kernels past 256 units: name -> (layout, size, channels to ask for, windows (w, h, first column, first row) in blocks).
# Every first column is odd.  64 x 5: each wave lies in one window row; 65 x 4: the last item holds four lanes; the others: items that begin
# in the middle of a row.  The 70-block window of the grey picture ends in its partial last block column, the 64 x 5 one in its partial last row.
BLOCK_PICTURES = {
    "444": ("444", (1024, 48), (3, 4, 1), ((64, 5, 3, 1), (65, 4, 1, 1), (70, 5, 57, 0), (100, 6, 5, 0), (127, 6, 1, 0))),
    "grey": ("grey", (1030, 44), (3, 4, 1), ((64, 5, 3, 1), (65, 4, 1, 1), (70, 5, 59, 0), (100, 6, 5, 0), (127, 6, 1, 0))),
    "luma420": ("420", (1024, 48), (1,), ((64, 5, 3, 1), (65, 4, 1, 1), (70, 5, 57, 0), (100, 6, 5, 0), (127, 6, 1, 0))),
    "cmyk": ("cmyk", (560, 40), (3, 4, 1), ((69, 5, 1, 0),)),
}


def unit_window(W, H, uw, uh, n_x, n_y, x, y):
    """units -> stored pixels: from one pixel inside the first unit to one pixel short of the last unit's end (units of one pixel: the
    unit), clipped to the picture"""
    x0, y0 = x * uw + (uw > 1), y * uh + (uh > 1)
    x1, y1 = max(x0 + 1, min(W, (x + n_x) * uw - (uw > 1))), max(y0 + 1, min(H, (y + n_y) * uh - (uh > 1)))
    assert x1 <= W and y1 <= H
    return (x0, y0, x1 - x0, y1 - y0)


def block_windows(name, req):
    """CMYK asked for with one channel takes the two-pass path, which drops the region: one item per four picture rows"""
    layout, (W, H), reqs, wins = BLOCK_PICTURES[name]
    assert req in reqs
    return [Win("%dx%d" % (w, h), unit_window(W, H, 8, 8, w, h, x, y), req=req, seam=not (layout == "cmyk" and req < 3)) for w, h, x, y in wins]


# D. the windowed reduced-size kernels past 256 units: 40 x 30 MCUs with a partial last column and row.  Windows (w, h, first column, first row) in
# MCUs at the scale, first columns and rows odd so that the pixel offsets are; the last reaches the partial last column and the last row
SCALED_PICTURES = {"420": (637, 477), "422": (637, 237), "444": (317, 237), "grey": (317, 237)}
SCALED_WINDOWS = ((33, 17, 3, 5), (37, 7, 1, 11), (1, 30, 7, 0), (21, 15, 19, 15))
SCALED_LUMA_WINDOW = (70, 9, 5, 11)  # 4:2:0 asked for with one channel: luma blocks on an 80 x 60 grid


def scaled_windows(layout, s, req):
    W, H = SCALED_PICTURES[layout]
    sw, sh = -(-W // s), -(-H // s)
    uw, uh, _ = unit_px(layout, req, s)
    if req < 3:
        assert layout == "420"
        w, h, x, y = SCALED_LUMA_WINDOW
        return [Win("luma%dx%d" % (w, h), unit_window(sw, sh, uw, uh, w, h, x, y), req=req, s=s)]
    return [Win("%dx%d" % (w, h), unit_window(sw, sh, uw, uh, w, h, x, y), req=req, s=s, seam=w * h > 256) for w, h, x, y in SCALED_WINDOWS]


# E. one launch, many kinds: (name, layout, size, scale, window or None, kind).  kind "skip": flagged MIJ_FLAG_SKIP after it got its slot; "clone": of the
# entry before it, and like every clone without a region.  Every region is different.  MIJ_BAND_ROWS is 4 in this test, so that the band
# count of the 4:2:0 slots without a region does not follow the device's CU count
def mixed_slots():
    return [
        ("skipped", "420", BAND_PICTURES["420"], 1, None, "skip"),
        ("420 whole", "420", BAND_PICTURES["420"], 1, None, "plain"),
        ("420 two bands", "420", BAND_PICTURES["420"], 1, (17, 2 * 16 + 15, 14, 4 * 16 + 2), "plain"),
        ("420 clone", "420", BAND_PICTURES["420"], 1, None, "clone"),
        ("444 two items", "444", (1024, 48), 1, unit_window(1024, 48, 8, 8, 64, 5, 3, 1), "plain"),
        ("444 whole", "444", (1024, 48), 1, None, "plain"),
        ("grey window", "grey", (1030, 44), 1, unit_window(1030, 44, 8, 8, 70, 5, 59, 0), "plain"),
        ("cmyk window", "cmyk", (560, 40), 1, unit_window(560, 40, 8, 8, 69, 5, 1, 0), "plain"),
        ("422 region", "422", BAND_PICTURES["422"], 1, (17, 3 * 8 + 7, 14, 8 * 8 + 2), "plain"),
        ("440 region", "440", BAND_PICTURES["440"], 1, (9, 1 * 16 + 15, 6, 7 * 16 + 2), "plain"),
        ("420 half size window", "420", SCALED_PICTURES["420"], 2, unit_window(319, 239, 8, 8, 33, 17, 3, 5), "plain"),
        ("444 quarter size whole", "444", SCALED_PICTURES["444"], 4, None, "plain"),
        ("411 region", "411", (77, 45), 1, (33, 9, 30, 20), "plain"),
    ]


# F. tensor path with tall crops
TENSOR_PICTURES = (("420", (640, 480)), ("422", (640, 240)), ("444", (320, 240)))


def rrc_windows(rng, W, H, n):
    """n windows of torchvision's RandomResizedCrop sampler on a W x H frame: 0.08 .. 1 of the area, ratio 3/4 .. 4/3 log-uniform (as in
    test_gpu_tensor_resize.py)"""
    out = []
    for _ in range(n):
        while True:
            area = W * H * rng.uniform(0.08, 1.0)
            ratio = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
            w, h = int(round(np.sqrt(area * ratio))), int(round(np.sqrt(area / ratio)))
            if 0 < w <= W and 0 < h <= H:
                break
        out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return out


def tensor_crops(o, s, sized, n=12):
    """-> per picture of TENSOR_PICTURES, n crops of its displayed frame (orientation o, reduced by s).  sized: each picture's own sampled
    windows, for a resized request; else one sampled size for the whole call -- an unresized request's tensor has one shape -- taken from
    the smallest displayed frame and placed in each picture at sampled offsets"""
    rng = np.random.default_rng(1000 * o + 10 * s + int(sized))
    frames = []
    for _, (W, H) in TENSOR_PICTURES:
        sw, sh = -(-W // s), -(-H // s)
        frames.append((sh, sw) if o >= 5 else (sw, sh))
    if sized:
        return [rrc_windows(rng, dw, dh, n) for dw, dh in frames]
    (_, _, w, h), = rrc_windows(rng, min(f[0] for f in frames), min(f[1] for f in frames), 1)
    return [[(int(rng.integers(0, dw - w + 1)), int(rng.integers(0, dh - h + 1)), w, h) for _ in range(n)] for dw, dh in frames]


def every_seam_case():
    """-> [(group, case name, layout, size, Win, band_rows, expected items)] of groups A to D, for the host checks"""
    out = []
    for layout, size in BAND_PICTURES.items():
        for env in BAND_ROWS_ENV:
            per = int(env or 0)
            for w in band_windows(layout, per):
                out.append(("A", "%s rows=%s" % (layout, env), layout, size, w, per, expected_items(layout, 3, 1, size, w.win, per)))
    for layout, (size, _) in SEGMENT_PICTURES.items():
        for w in segment_windows(layout):
            out.append(("B", layout, layout, size, w, 0, expected_items(layout, 3, 1, size, w.win)))
    for name, (layout, size, reqs, _) in BLOCK_PICTURES.items():
        for req in reqs:
            for w in block_windows(name, req):
                out.append(("C", name, layout, size, w, 0, expected_items(layout, req, 1, size, w.win)))
    for layout, size in SCALED_PICTURES.items():
        for s in (2, 4, 8):
            for req in (3, 4) + ((1,) if layout == "420" else ()):
                for w in scaled_windows(layout, s, req):
                    out.append(("D", layout, layout, size, w, 0, expected_items(layout, req, s, size, w.win)))
    return out


def every_picture():
    """(layout, size, seed) of every dense picture test_gpu_roi_seams.py sends to the GPU"""
    pics = [(lay, size, 0) for lay, size in BAND_PICTURES.items()]
    pics += [(lay, size, 0) for lay, (size, _) in SEGMENT_PICTURES.items()]
    pics += [(lay, size, 0) for lay, size, _, _ in BLOCK_PICTURES.values()]
    pics += [(lay, size, 0) for lay, size in SCALED_PICTURES.items()]
    pics += [(lay, size, 0) for _, lay, size, _, _, _ in mixed_slots()]
    pics += [(lay, size, seed) for lay, size in TENSOR_PICTURES for seed in (3, 4)]
    return sorted(set(pics))
