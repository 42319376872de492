"""Chroma upsampling on the GPU at sample level: every kernel that chooses a neighbour, a near and a far row, and a clamp at the picture's
right and bottom edges (fused_band in its forms t, s, base, w, x and c, fused422_band, k_resample_fast's six kinds, k_resample_color)
against tests/upsample_model.py, bit for bit, on pictures whose MCU padding is NOT a copy of the edge (tests/sample_cases.py).  That the
model is the reference's answer, and that these pictures show a kernel reading column wc or row comp.y where an encoder-made picture of
the same size does not, is test_upsample_host.py's part.  The kernel every slot took is asserted through Batch.slot_kernel from the
rules restated in sample_cases, so a switch between two forms cannot move unnoticed."""
import ctypes as C

import numpy as np
import pytest

import coef_cases as CC
import sample_cases as S
import upsample_model as U
from roi_cases import paint, read_back

pytestmark = pytest.mark.gpu

MB = 1 << 20
FORMATS = ("compact", "int16")
_model = {}


def _want(case, n_out):
    """the model's picture of a case: computed once per colour branch (four channels are the three and alpha, two the one and alpha),
    shared, never changed"""
    k = (case.name, n_out >= 3)
    if k not in _model:
        px = U.picture(case, 4 if n_out >= 3 else 2)
        px.setflags(write=False)
        assert (px[..., -1] == 255).all()
        _model[k] = px
    px = _model[k]
    return px if n_out in (2, 4) else px[..., :-1]


def _run(ica, ctx, cases, req, fmt, force_generic=0, walk=False, launches=1):
    """one batch of all cases: decode, paint the whole out arena, launch, read the arena back; every slot against the model, every byte
    behind a picture up to its 256-byte rounding still paint.  -> [(kernel, variant, segments)] per case"""
    ncoef = sum(p.size for c in cases for p in c.planes)
    out_bytes = sum(-(-c.w * c.h * req // 256) * 256 for c in cases)
    arena = MB + sum(ica.Batch.coef_bytes(ica.HostDecoder.probe(c.stream(), req)) for c in cases)
    b = ica.Batch(ctx, len(cases), arena, arena, out_bytes + MB)
    try:
        b.set_coef_format(fmt)
        if walk:
            b.entropy_reserve(16 * MB + 2 * ncoef)
        if force_generic:
            b.force_generic(force_generic)
        ok, slots, reasons = b.decode_jpegs([c.stream() for c in cases], req, threads=16, gpu_entropy=walk)
        assert ok == len(cases) and sorted(slots) == list(range(len(cases))), [r for r in reasons if r][:3]
        b.upload()
        b.wait()
        L = ica.lib()
        L.mij_batch_out_offset.restype = C.c_size_t
        L.mij_batch_out_offset.argtypes = [C.c_void_p, C.c_int]
        L.mij_batch_out_bytes.restype = C.c_size_t
        L.mij_batch_out_bytes.argtypes = [C.c_void_p]
        assert L.mij_batch_out_bytes(b._h) == out_bytes and L.mij_batch_out_offset(b._h, 0) == 0
        kernels = []
        for n in range(launches):
            pat = paint(ica, b, 0, out_bytes, 29 + n)
            b.launch()
            b.wait()
            got = read_back(ica, b, 0, (out_bytes,))
            kernels = []
            for case, sl in zip(cases, slots):
                tag = (case.name, "req %d" % req, fmt, "generic %d" % force_generic, "walk" if walk else "host", "launch %d" % n)
                want = _want(case, req)
                off, nb = L.mij_batch_out_offset(b._h, sl), want.size
                px = got[off:off + nb].reshape(want.shape)
                kernels.append(b.slot_kernel(sl))
                assert b.slot_coef_bytes(sl) == (1 if fmt == "compact" else 0), tag
                assert bool(kernels[-1][1] & 2) == case.needs_wide() or "RS" in kernels[-1][0] or kernels[-1][0] == "MK_RESAMPLE", tag + kernels[-1]
                if not np.array_equal(px, want):
                    bad = np.argwhere((px != want).any(axis=2))
                    raise AssertionError(tag + kernels[-1] + ("%d pixels differ" % len(bad), "rows", sorted(set(bad[:, 0].tolist()))[:8], "columns",
                                                              sorted(set(bad[:, 1].tolist()))[:16]))
                end = -(-nb // 256) * 256
                assert np.array_equal(got[off + nb:off + end], pat[off + nb:off + end]), tag + ("bytes behind the picture were written",)
        return kernels
    finally:
        b.close()


def _small_cases(layout):
    """the host test's size lists: noise at every sweep size, the other families at the corner sizes, and one WIDE picture of each family"""
    mw, mh = S.mcu_px(layout)
    cases = [S.make("noise", layout, w, h) for w, h in S.sweep_sizes(layout)]
    cases += [S.make(f, layout, w, h) for f in ("stripes_h", "stripes_v", "poison") for w, h in S.corner_sizes(layout)]
    cases += [S.make(f, layout, 2 * mw + 3, mh + 1, wide=True) for f in S.FAMILIES]
    cases += [S.make("noise", layout, 2 * mw, 2 * mh, wide=True)]
    return cases


# ------------------------------------------------------------------ 1. the small sweep

@pytest.mark.parametrize("req", (1, 2, 3, 4))
@pytest.mark.parametrize("layout", list(S.LAYOUTS))
def test_small_sweep(ica, gpu_ctx, layout, req):
    """every size kind of the layout in one batch per combination of force_generic 0 / 1 / 2 and plane format (host walk), the kernel of
    every slot as classify and resample_fast_kind prescribe: with force_generic 1 every W % 4 == 0 picture of three or four channels on
    its RS_* kind and every other one on k_resample_color"""
    cases = _small_cases(layout)
    seen = set()
    for fg in (0, 1, 2):
        for fmt in FORMATS:
            kernels = _run(ica, gpu_ctx, cases, req, fmt, force_generic=fg)
            for case, (kind, var, nseg) in zip(cases, kernels):
                assert (kind, nseg) == S.expected_kernel(layout, case.w, req, fg), (case.name, req, fg, kind)
                seen.add((fg, kind))
    if req >= 3 and len(S.LAYOUTS[layout][0]) >= 3:
        fast = S.fast_kind(layout, 4, req)
        assert {k for f, k in seen if f == 1} == {fast, "MK_RESAMPLE"} and {k for f, k in seen if f == 2} == {"MK_RESAMPLE"}, seen


@pytest.mark.parametrize("layout", CC.GPU_WALK_LAYOUTS)
def test_small_sweep_gpu_walk(ica, gpu_ctx, layout):
    """the same pictures with the coefficient planes written by the GPU Huffman walk (three channels, compact planes)"""
    _run(ica, gpu_ctx, _small_cases(layout), 3, "compact", walk=True)


# ------------------------------------------------------------------ 2. the band forms, at both ends of each form's range of MCU columns

def _band_cases(layout, form, height):
    ws = S.band_widths(layout, form)
    return [S.make("noise", layout, w, height) for w in ws] + [S.make("poison", layout, ws[-1], height)]


def _forms():
    return [(layout, form) for layout in ("420", "422", "440") for form, _, _ in S.form_ranges(layout)]


@pytest.mark.parametrize("height", (17, 40))
@pytest.mark.parametrize("band_rows", (None, 1, 2))
@pytest.mark.parametrize("layout,form", _forms())
def test_band_forms(ica, gpu_ctx, monkeypatch, layout, form, band_rows, height):
    """all mw widths of the form's last MCU column (every residue of W at the upper switch; the next column takes the next form) and the
    first four widths of its first column; noise, and poison at the widest; three and four channels, both plane formats; MIJ_BAND_ROWS
    unset (the device's own band count), 1 and 2 (a band seam behind every, and every other, MCU row)"""
    if band_rows:
        monkeypatch.setenv("MIJ_BAND_ROWS", str(band_rows))  # read when the batch is created
    else:
        monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    cases = _band_cases(layout, form, height)
    assert len(cases) == S.BAND_MCU_W[layout] + 4 + 1
    for req in (3, 4):
        for fmt in FORMATS:
            for case, (kind, var, nseg) in zip(cases, _run(ica, gpu_ctx, cases, req, fmt)):
                assert (kind, nseg) == (form, 1), (case.name, kind, nseg)
                assert var == (4 if req == 4 else 0) | (1 if fmt == "compact" else 0), (case.name, var)


def test_422_beyond_the_band_kernel(ica, gpu_ctx):
    """one MCU column more than the widest 4:2:2 band (640: the row no longer fits a CU's LDS): the two-pass path"""
    cases = [S.make("noise", "422", 16 * 639 + 1, 17), S.make("noise", "422", 16 * 640, 17)]
    for req in (3, 4):
        kernels = _run(ica, gpu_ctx, cases, req, "compact")
        assert [k[0] for k in kernels] == ["MK_RESAMPLE", "MK_RS_FAST+RS_H2"], kernels


# ------------------------------------------------------------------ 3. column segments

SEGMENTS = {  # layout -> [(MCU columns, segments, full residue sweep)]: on FIT = 180 / 267 columns per segment (roi_cases.FIT)
    "420": ((366, 3, False), (367, 3, True), (368, 3, False), (541, 4, False)),
    "440": ((539, 3, False), (540, 3, False), (541, 3, True), (802, 4, False)),
}


@pytest.mark.parametrize("height", (17, 40))
@pytest.mark.parametrize("layout,cols,nseg,full", [(l,) + t for l, ts in SEGMENTS.items() for t in ts])
def test_column_segments(ica, gpu_ctx, monkeypatch, layout, cols, nseg, full, height):
    """form c: the first MCU-column counts beyond a CU's LDS (three segments, split unevenly where the count is no multiple of three: the
    full residue sweep is at such a count) and the first count of four segments; noise, stripes_h (every seam column the opposite of both its neighbours) and poison; the segment
    count asserted; both producers for compact planes"""
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    mw = S.BAND_MCU_W[layout]
    assert S.band_form(layout, cols) == ("MK_%sC" % layout, nseg) and (cols % nseg != 0 or not full)
    ws = range(mw * (cols - 1) + 1, mw * cols + 1) if full else (mw * (cols - 1) + 1, mw * (cols - 1) + 2, mw * cols - 1, mw * cols)
    cases = [S.make("noise", layout, w, height) for w in ws]
    cases += [S.make(f, layout, w, height) for f in ("stripes_h", "poison") for w in (ws[0], ws[-1])]
    for req, fmt, walk in ((3, "compact", False), (4, "int16", False), (3, "compact", True), (4, "compact", False), (3, "int16", False)):
        for case, (kind, var, n) in zip(cases, _run(ica, gpu_ctx, cases, req, fmt, walk=walk)):
            assert (kind, n) == ("MK_%sC" % layout, nseg), (case.name, kind, n)


@pytest.mark.parametrize("band_rows", (1, 2))
def test_column_segments_band_seams(ica, gpu_ctx, monkeypatch, band_rows):
    """segments x bands: the uneven three-segment split with a band seam behind every (every other) MCU row"""
    monkeypatch.setenv("MIJ_BAND_ROWS", str(band_rows))
    for layout, cols in (("420", 367), ("440", 541)):
        mw = S.BAND_MCU_W[layout]
        cases = [S.make(f, layout, w, 40) for f in ("noise", "stripes_h", "stripes_v") for w in (mw * cols - 3, mw * cols)]
        for req, fmt in ((3, "compact"), (4, "int16")):
            assert all(k[0] == "MK_%sC" % layout and k[2] == 3 for k in _run(ica, gpu_ctx, cases, req, fmt))


# ------------------------------------------------------------------ 4. every form in one launch

def test_every_form_in_one_batch_launched_twice(ica, gpu_ctx, monkeypatch):
    """one picture of every form of every band layout, column segments and the two-pass kinds among them, in a single launch; launched
    twice into a freshly painted arena, every slot against the model after each"""
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    cases, want = [], []
    for layout, form in _forms():
        _, lo, hi = next(t for t in S.form_ranges(layout) if t[0] == form)
        cases.append(S.make("noise", layout, S.BAND_MCU_W[layout] * hi - 5, 40))
        want.append((form, 1))
    for layout, ts in SEGMENTS.items():
        cases.append(S.make("noise", layout, S.BAND_MCU_W[layout] * next(c for c, _, full in ts if full) - 3, 17))
        want.append(("MK_%sC" % layout, 3))
    for layout in ("411", "410", "h2v4", "h1v4", "rgb420", "cmyk422", "ycck_k", "lumasub", "444", "ycck"):
        for w in (36, 37):
            cases.append(S.make("poison", layout, w, 19))
            want.append(S.expected_kernel(layout, w, 3))
    for req in (3, 4):
        kernels = _run(ica, gpu_ctx, cases, req, "compact", launches=2)
        assert [(k, n) for k, _, n in kernels] == want
