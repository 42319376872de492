"""Pictures chosen sample by sample, MCU padding included (test_upsample_host.py, test_gpu_upsample.py).

An encoder fills the MCU padding with copies of the edge samples, so a kernel that reads chroma column wc = ceil(W / hs) or chroma row
comp.y where the reference clamps to the one before gets the same byte and passes every encoder-made picture.  Here every sample of
every padded plane is the generator's: from_samples() turns planes of samples into the coefficient planes of a coef_cases.Case (a float
forward DCT, rounded), and the stream is written from those.  What a decoder has to make of the stream is said by the coefficients
(upsample_model.picture), not by the samples meant -- rounding moves a sample by one or two.

Also here: the band kernels' forms restated from the LDS arithmetic (mij_runtime.hip: band_form, band_segments), for the tests that
assert the form of every slot (Batch.slot_kernel)."""
import numpy as np

import coef_cases as CC
import idct_model as M

# the layouts of tests/golden/make_golden_r2b.py that upsample and coef_cases does not have: 4:1:0, h2v4, h1v4, RGB-tagged 4:2:0, YCCK and
# CMYK with sub-sampled components 1 and 2, a fourth component below full resolution, luma below the chroma resolution; and four-component
# YCbCr for its colour branch
CC.EXTRA_LAYOUTS.update({
    "410": ([(4, 2), (1, 1), (1, 1)], -1), "h2v4": ([(2, 4), (1, 1), (1, 1)], -1), "h1v4": ([(1, 4), (1, 1), (1, 1)], -1),
    "rgb420": ([(2, 2), (1, 1), (1, 1)], 0), "ycck420": ([(2, 2), (1, 1), (1, 1), (2, 2)], 2), "cmyk422": ([(2, 1), (1, 1), (1, 1), (2, 1)], 0),
    "ycck_k": ([(2, 2), (1, 1), (1, 1), (1, 1)], 2), "lumasub": ([(1, 1), (2, 2), (2, 2)], -1), "ycca": ([(1, 1)] * 4, 1),
})
LAYOUTS = CC.all_layouts()
FAMILIES = ("noise", "stripes_h", "stripes_v", "poison")


def factors(layout):
    hv, _ = LAYOUTS[layout]
    return hv, max(h for h, _ in hv), max(v for _, v in hv)


def mcu_px(layout):
    _, hmax, vmax = factors(layout)
    return 8 * hmax, 8 * vmax


def kinds(layout):
    """the reference's resampler per component (upsample_model.kind_of)"""
    import upsample_model as U
    hv, hmax, vmax = factors(layout)
    return [U.kind_of(hmax // h, vmax // v) for h, v in hv]


# the orthonormal 8-point DCT-II: with it the DC term of a block is 8 * (mean - 128)
_x, _u = np.arange(8)[None, :], np.arange(8)[:, None]
DCT = np.where(_u == 0, np.sqrt(1 / 8.0), np.sqrt(2 / 8.0) * np.cos((2 * _x + 1) * _u * np.pi / 16))


def from_samples(layout, w, h, planes, name, family, wide=False):
    """one padded uint8 plane [bh * 8, bw * 8] per component -> a coef_cases.Case with all-ones quantisation tables: forward DCT per block,
    rounded, DC clipped to -1024 .. 1016 and AC to +-1023 (what the writer's Huffman tables can code).  wide: six terms of +-1000 at the end
    of component 0's first block on top, which takes that block's L1 past MIJ_BLOCK_L1_LIMIT and the picture to the WIDE kernels."""
    out = []
    for p, (bh, bw) in zip(planes, CC.geometry(layout, w, h)[2]):
        assert p.shape == (bh * 8, bw * 8) and p.dtype == np.uint8, (layout, p.shape, bh, bw)
        b = p.astype(np.float64).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128.0
        c = np.rint(DCT @ b @ DCT.T).astype(np.int64)
        zz = M.nat_to_zz(c)
        zz[..., 0] = np.clip(zz[..., 0], -1024, 1016)
        zz[..., 1:] = np.clip(zz[..., 1:], -1023, 1023)
        out.append(zz.astype(np.int16))
    if wide:
        out[0][0, 0, 58:64] = [1000, -1000, 1000, -1000, 1000, -1000]
    return CC.Case(name, family, layout, w, h, out)


def _effective(layout, w, h):
    """per component: (effective columns ceil(W * h / h_max), effective rows comp.y, padded rows, padded columns)"""
    hv, hmax, vmax = factors(layout)
    return [((w * hh + hmax - 1) // hmax, (h * vv + vmax - 1) // vmax, bh * 8, bw * 8) for (hh, vv), (bh, bw) in zip(hv, CC.geometry(layout, w, h)[2])]


def _inverse_of_edge(inner, rows, cols):
    """the effective area `inner`, and in the padding 255 - the nearest effective sample: the inverse of what an encoder replicates there"""
    eh, ew = inner.shape
    y, x = np.minimum(np.arange(rows), eh - 1), np.minimum(np.arange(cols), ew - 1)
    p = inner[y[:, None], x[None, :]].astype(np.int64)
    pad = (np.arange(rows) >= eh)[:, None] | (np.arange(cols) >= ew)[None, :]
    return np.where(pad, 255 - p, p).astype(np.uint8)


_cache = {}


# the seed every test takes.  Where a blunder is exposed by a single pixel (pictures one row high, one column wide), noise shows it with a
# chance of a few thousand to one against; under seed 0 one of the 729 such checks of test_upsample_host.py (cmyk422 35 x 1, where a small K
# hides a one-level step in C) came out level, under seeds 1 to 4 none
SEED = 1


def make(family, layout, w, h, seed=SEED, wide=False):
    """noise      every sample of every component uniform in 0..255, padding included
    stripes_h  every sub-sampled component 16 / 240 in turn along its rows (the others 128); the padding holds the inverse of the nearest
               effective sample, so column wc (and row comp.y) is the opposite of what the reference's clamp gives
    stripes_v  the same down the columns
    poison     every component a ramp around 128 over its effective area (x < ceil(W * h / h_max), y < comp.y); every padding sample is 0 in
               components 0 and 2, 255 in components 1 and 3"""
    k = (family, layout, w, h, seed, wide)
    if k in _cache:
        return _cache[k]
    r = np.random.default_rng([FAMILIES.index(family), seed, w, h] + [ord(ch) for ch in layout])
    hv, hmax, vmax = factors(layout)
    planes = []
    for c, (ew, eh, rows, cols) in enumerate(_effective(layout, w, h)):
        y, x = np.arange(eh)[:, None], np.arange(ew)[None, :]
        sub = hv[c] != (hmax, vmax)
        if family == "noise":
            p = r.integers(0, 256, (rows, cols), dtype=np.uint8)
        elif family in ("stripes_h", "stripes_v"):
            t = (x + 0 * y) if family == "stripes_h" else (y + 0 * x)
            inner = np.where((t + c + seed) & 1, 240, 16) if sub else np.full((eh, ew), 128)
            p = _inverse_of_edge(inner.astype(np.uint8), rows, cols) if sub else np.full((rows, cols), 128, np.uint8)
        else:
            p = np.full((rows, cols), 255 if c & 1 else 0, np.uint8)
            p[:eh, :ew] = 128 + (7 * x + 11 * y + 5 * c + seed) % 29 - 14
        planes.append(p)
    name = "%s_%s_%dx%d_s%d%s" % (family, layout, w, h, seed, "_wide" if wide else "")
    if len(_cache) > 4096:
        _cache.clear()
    _cache[k] = from_samples(layout, w, h, planes, name, family, wide)
    return _cache[k]


# ---------------------------------------------------------------- sizes

def nine(m):
    """the nine kinds of extent along an axis whose MCU is m pixels"""
    return sorted({1, 2, m - 1, m, m + 1, 2 * m - 1, 2 * m, 2 * m + 1, 2 * m + 3})


def sweep_sizes(layout):
    """every W in 1 .. 2 mw + 3 at the nine heights, and every H in 1 .. 2 mh + 3 at the nine widths"""
    mw, mh = mcu_px(layout)
    s = {(w, h) for w in range(1, 2 * mw + 4) for h in nine(mh)} | {(w, h) for h in range(1, 2 * mh + 4) for w in nine(mw)}
    return sorted(s)


def corner_sizes(layout):
    mw, mh = mcu_px(layout)
    return [(w, h) for w in nine(mw) for h in nine(mh)]


# ---------------------------------------------------------------- the band kernels' forms, from the LDS arithmetic

LDS_BYTES = 160 * 1024                      # max_dyn_lds: a CU's LDS
ONE_WAVE_COLS, TWO_WAVE_COLS = 24, 56
BAND_MCU_W = {"420": 16, "422": 16, "440": 8}


def lds_row(layout, cols):
    """LDS of a row of `cols` MCUs: 448 B per column for 4:2:0 (luma 16 x 16, two chroma blocks, two chroma halo rows of 16, four row sums of
    8), 304 B for 4:4:0 (luma 16 x 8, halo rows of 8), 256 B and 16 for 4:2:2"""
    return {"420": 448 * cols, "440": 304 * cols, "422": 256 * cols + 16}[layout]


def band_form(layout, cols):
    """-> (kernel family as Batch.slot_kernel names it, column segments).  The form follows the workgroups of the row's LDS that fit a CU:
    three or more: base (t up to ONE_WAVE_COLS columns and s up to TWO_WAVE_COLS in 4:2:0 and 4:2:2), two: w, one: x (4:4:0: w); none:
    column segments (c) in 4:2:0 and 4:4:0, of which two with two halo columns each have to fit; 4:2:2 goes to the two-pass path."""
    lds = lds_row(layout, cols)
    if lds > LDS_BYTES:
        if layout == "422":
            return ("MK_RS_FAST+RS_H2" if cols * 16 % 4 == 0 else "MK_RESAMPLE"), 1
        fit = LDS_BYTES // (2 * lds_row(layout, 1)) - 2
        return "MK_%sC" % layout, -(-cols // fit)
    if layout == "440":
        return ("MK_440W" if 3 * lds > LDS_BYTES else "MK_440"), 1
    if 2 * lds > LDS_BYTES:
        return "MK_%sX" % layout, 1
    if 3 * lds > LDS_BYTES:
        return "MK_%sW" % layout, 1
    return "MK_%s%s" % (layout, "T" if cols <= ONE_WAVE_COLS else "S" if cols <= TWO_WAVE_COLS else ""), 1


def form_ranges(layout):
    """[(form, c_lo, c_hi)]: the MCU columns each single-workgroup form of the layout serves, found by walking band_form"""
    out, c = [], 1
    while True:
        form, _ = band_form(layout, c)
        if form.endswith("C") or "RS" in form or form == "MK_RESAMPLE":
            return out
        hi = c
        while band_form(layout, hi + 1)[0] == form:
            hi += 1
        out.append((form, c, hi))
        c = hi + 1


def band_widths(layout, form):
    """the widths the band tests take for a form: all mw widths of its widest MCU-column count (a full residue sweep at the upper switch) and
    the first four of its narrowest"""
    mw = BAND_MCU_W[layout]
    lo, hi = next((a, b) for f, a, b in form_ranges(layout) if f == form)
    return sorted(set(range(mw * (hi - 1) + 1, mw * hi + 1)) | set(range(mw * (lo - 1) + 1, mw * (lo - 1) + 5)))


# ---------------------------------------------------------------- the kernel a slot takes (mij_runtime.hip: classify, resample_fast_kind)

def fast_kind(layout, w, req, force_generic=1):
    """pass 2 of the two-pass path: the resampler k_resample_fast is compiled for, or MK_RESAMPLE (k_resample_color) -- three or four
    channels, W % 4 == 0, components 0 (and 3 of CMYK / YCCK) at full resolution, components 1 and 2 sharing factors"""
    hv, hmax, vmax = factors(layout)
    app14 = LAYOUTS[layout][1]
    if force_generic >= 2 or req not in (3, 4) or w % 4 or len(hv) < 3 or hv[0] != (hmax, vmax) or hv[1] != hv[2]:
        return "MK_RESAMPLE"
    if len(hv) == 4 and app14 in (0, 2) and hv[3] != (hmax, vmax):
        return "MK_RESAMPLE"
    hs, vs = hmax // hv[1][0], vmax // hv[1][1]
    rs = {1: "RS_V2" if vs == 2 else "RS_ROW1", 2: {1: "RS_H2", 2: "RS_HV2"}.get(vs, "RS_GEN2"), 4: "RS_GEN4"}.get(hs)
    return "MK_RS_FAST+" + rs if rs else "MK_RESAMPLE"


def expected_kernel(layout, w, req, force_generic=0):
    """-> (family, column segments) of a whole-size slot, as Batch.slot_kernel reports it"""
    hv, hmax, vmax = factors(layout)
    app14 = LAYOUTS[layout][1]
    ycc3 = len(hv) == 3 and app14 != 0
    if not force_generic:
        chroma_1x1 = ycc3 and req >= 3 and hv[1] == hv[2] == (1, 1)
        if chroma_1x1 and hv[0] == (2, 2):
            return band_form("420", -(-w // 16))
        if len(hv) == 1 or (ycc3 and req < 3 and hv[0] == (hmax, vmax)):
            return "MK_GREY", 1
        if chroma_1x1 and hv[0] == (2, 1) and lds_row("422", -(-w // 16)) <= LDS_BYTES:
            return band_form("422", -(-w // 16))
        if chroma_1x1 and hv[0] == (1, 2):
            return band_form("440", -(-w // 8))
        if req >= 3 and all(f == (1, 1) for f in hv):
            if ycc3 or (len(hv) == 4 and app14 not in (0, 2)):
                return "MK_444", 1
            return "MK_1X1C", 1
    return fast_kind(layout, w, req, force_generic or 1), 1
