"""Plane output on the GPU (mij_batch_set_out_planes, k_planes_out; TensorDecoder.decode_ycbcr): every case byte for byte against the
model (planes_out_model.py).  Every destination is cut out of a larger sentinel-filled buffer, and the WHOLE buffer is compared: the
sample addresses hold the model's samples and every other byte still holds the sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

import coef_cases as CC
import planes_out_cases as POC
import planes_out_model as PM

pytestmark = pytest.mark.gpu

MIJ_E_ARG, MIJ_E_STATE = -2, -5
SENT = 0xA7
MB = 1 << 20


def up(v, a):
    return -(-v // a) * a


# ------------------------------------------------------------------ destination views: {component: (byte offset, row pitch, x pitch)}

def view_planar(rects, phase=False):
    """contiguous planes on 8-byte boundaries with pitches that are multiples of 8: the fast form.  phase: each plane starts sx0 % 8 bytes
    behind a boundary, which is where a window that starts inside a block leaves its blocks' rows aligned"""
    out, off = {}, 8
    for c, (x0, _, w, h) in sorted(rects.items()):
        rp = up(w, 8)
        out[c] = (off + (x0 % 8 if phase else 0), rp, 1)
        off = up(off + rp * h + 24, 8)
    return out


def view_cut(rects):
    """planes_cases.views' "cut": an odd offset inside a larger array with a wider pitch: the general form"""
    out, off = {}, 8
    for c, (_, _, w, h) in sorted(rects.items()):
        rp = w + 9
        out[c] = (off + 2 * rp + 3, rp, 1)
        off = up(off + (h + 5) * rp, 8)
    return out


def view_nv(rects, swap=False, pad=0, odd=False):
    """Y contiguous, Cb and Cr interleaved (nv12; swap: nv21; pad: a wider pitch; odd: the pair at an odd address)"""
    assert rects[1] == rects[2]
    _, _, w, h = rects[0]
    _, _, cw, ch = rects[1]
    base = up(8 + up(w, 8) * h + 24, 16) + (1 if odd else 0)
    rp = 2 * cw + pad
    return {0: (8, up(w, 8), 1), 1: (base + (1 if swap else 0), rp, 2), 2: (base + (0 if swap else 1), rp, 2)}


def view_packed(rects):
    """packed YCbCr of a 4:4:4 picture: x_pitch 3"""
    _, _, w, _ = rects[0]
    return {c: (8 + c, 3 * w + 5, 3) for c in rects}


def extent(spec, rect):
    off, rp, xp = spec
    return off + (rect[3] - 1) * rp + (rect[2] - 1) * xp + 1


class Job:
    """one slot's request: where its planes go inside a buffer of its own, and what the buffer must hold afterwards"""

    def __init__(self, planes, w, h, hv, view, window=None, comps=None, tag=""):
        self.comps = list(range(len(planes))) if comps is None else list(comps)
        self.rects = {c: PM.rect(w, h, hv, c, window) for c in self.comps}
        self.specs = view(self.rects)
        self.window, self.tag = window, tag
        n = up(max(extent(self.specs[c], self.rects[c]) for c in self.comps) + 40, 16)
        self.want = np.full(n, SENT, np.uint8)
        for c, part in PM.window_of(planes, w, h, hv, window, self.comps).items():
            off, rp, xp = self.specs[c]
            ys, xs = np.mgrid[0:part.shape[0], 0:part.shape[1]]
            self.want[off + ys * rp + xs * xp] = part
        self.buf = torch.full((n,), SENT, dtype=torch.uint8, device="cuda:0")

    def request(self, ncomp=4):
        p = self.buf.data_ptr()
        return [(p + self.specs[c][0], self.specs[c][1], self.specs[c][2]) if c in self.specs else None for c in range(ncomp)]

    def check(self, what):
        got = self.buf.cpu().numpy()
        bad = np.nonzero(got != self.want)[0]
        assert bad.size == 0, "%s %s: %d bytes differ, first at %d (got %d, want %d)" % (what, self.tag, bad.size, bad[0], got[bad[0]], self.want[bad[0]])


def run_jobs(ica, ctx, stream, jobs, fmt="compact", producer="host"):
    """one batch, one slot per job; -> [(work items, kernel name, path, flags)] per slot"""
    b = ica.Batch(ctx, len(jobs), 24 * MB, 24 * MB, 24 * MB)
    try:
        b.set_coef_format(fmt)
        if producer == "host":
            slots = [b.add_jpeg(stream, 0) for _ in jobs]
        else:
            ok, slots, why = b.decode_jpegs([stream] * len(jobs), 0, threads=4)
            assert ok == len(jobs), why
        for sl, job in zip(slots, jobs):
            b.set_out_planes(sl, job.request(), job.window)
            for c in job.comps:
                assert b.plane_rect(sl, c) == job.rects[c], (job.tag, c)
        torch.cuda.synchronize()
        b.submit()
        b.wait()
        info = [(b.work_items(sl), b.slot_kernel(sl)[0], b.slot_path(sl), b.slot_flags(sl), b.slot_escapes(sl) if fmt == "compact" else None) for sl in slots]
        L = ica.lib()
        tmp = np.empty(16, np.uint8)
        for sl in slots:  # a plane slot decodes no pixels
            assert L.mij_batch_fetch(b._h, sl, tmp.ctypes.data_as(C.c_void_p), C.c_size_t(0)) == MIJ_E_STATE
        return info
    finally:
        b.close()


def views_for(layout, size):
    v = [("planar", view_planar), ("cut", view_cut)]
    if len(POC.hv_of(layout)) == 3:
        v += [("nv12", view_nv), ("nv21", lambda r: view_nv(r, swap=True)), ("nv12_pitched", lambda r: view_nv(r, pad=8)), ("nv12_odd", lambda r: view_nv(r, odd=True))]
    if layout == "444":
        v.append(("packed", view_packed))
    return v


# ------------------------------------------------------------------ 1. layouts, sizes, destination views

@pytest.mark.parametrize("layout", POC.LAYOUTS)
def test_layouts_sizes_and_views(ica, gpu_ctx, oracle, layout):
    hv = POC.hv_of(layout)
    for size in POC.SIZES:
        case = POC.picture(layout, size)
        planes = POC.planes_of(oracle, case)
        jobs = [Job(planes, size[0], size[1], hv, view, tag="%s %s %s" % (layout, size, name)) for name, view in views_for(layout, size)]
        info = run_jobs(ica, gpu_ctx, case.stream(), jobs)
        for job, (items, kind, path, _, _) in zip(jobs, info):
            job.check("whole picture")
            assert kind == "MK_PLANES_OUT" and path == 9, (job.tag, kind, path)
            blocks = [-(-job.rects[c][2] // 8) * -(-job.rects[c][3] // 8) for c in job.comps]
            paired = "nv" in job.tag and "odd" not in job.tag
            assert items == sum(-(-n // 256) for n in (blocks[:2] if paired else blocks)), (job.tag, items)


# ------------------------------------------------------------------ 2. windows

@pytest.mark.parametrize("layout", ("420", "422"))
def test_windows(ica, gpu_ctx, oracle, layout):
    w, h = POC.BIG
    hv = POC.hv_of(layout)
    case = POC.picture(layout, POC.BIG)
    planes = POC.planes_of(oracle, case)
    wins = [(0, 0, w, h), (w - 1, h - 1, 1, 1), (6, 10, 101, 37), (200, 0, 67, 69), (0, 40, 267, 29), (160, 32, 107, 37), (16, 16, 64, 32), (2, 2, 3, 3)]
    jobs = []
    for win in wins:
        assert PM.on_grid(w, h, hv, win, (0, 1, 2)) or layout == "422" and win[0] % 2 == 0
        for name, view in (("planar", view_planar), ("phase", lambda r: view_planar(r, phase=True)), ("cut", view_cut), ("nv12", view_nv), ("nv21", lambda r: view_nv(r, swap=True))):
            jobs.append(Job(planes, w, h, hv, view, window=win, tag="%s %s %s" % (layout, win, name)))
    run_jobs(ica, gpu_ctx, case.stream(), jobs)
    for job in jobs:
        job.check("window")
    # the corner sample of luma alone: one block, one work item
    job = Job(planes, w, h, hv, view_cut, window=(w - 1, h - 1, 1, 1), comps=[0], tag="corner luma")
    (items, _, _, _, _), = run_jobs(ica, gpu_ctx, case.stream(), [job])
    job.check("window")
    assert items == 1


# ------------------------------------------------------------------ 3. coefficient forms and producers

def wide_case(layout):
    return next(c for c in CC.l1_family(layout) if c.needs_wide())


@pytest.mark.parametrize("fmt", ("compact", "int16"))
def test_coefficient_forms(ica, gpu_ctx, oracle, fmt):
    for layout in ("420", "444"):
        hv = POC.hv_of(layout)
        wc = wide_case(layout)
        planes = POC.planes_of(oracle, wc)
        jobs = [Job(planes, wc.w, wc.h, hv, v, tag="wide %s %s %s" % (layout, fmt, n)) for n, v in (("planar", view_planar), ("nv12", view_nv), ("cut", view_cut))]
        info = run_jobs(ica, gpu_ctx, wc.stream(), jobs, fmt)
        for job, (_, _, _, flags, _) in zip(jobs, info):
            job.check("wide")
            assert flags & 1, "the strong case must take the wide IDCT"
    dc = POC.picture("420", (77, 45), seed=2)  # roi_cases.dense: every seventh block escaped
    planes = POC.planes_of(oracle, dc)
    jobs = [Job(planes, 77, 45, POC.hv_of("420"), v, tag="dense %s %s" % (fmt, n)) for n, v in (("planar", view_planar), ("nv21", lambda r: view_nv(r, swap=True)))]
    info = run_jobs(ica, gpu_ctx, dc.stream(), jobs, fmt)
    for job, (_, _, _, flags, esc) in zip(jobs, info):
        job.check("dense")
        assert not flags & 1 and (esc is None or esc > 0)


def test_progressive_file(ica, gpu_ctx, oracle, golden):
    data = golden.jpg("prog_420_23x41")
    planes, (w, h, hv, prog) = POC.stream_planes(oracle, data)
    assert prog and (w, h) == (23, 41)
    jobs = [Job(planes, w, h, hv, v, tag="prog %s" % n) for n, v in (("planar", view_planar), ("cut", view_cut), ("nv12", view_nv))]
    run_jobs(ica, gpu_ctx, data, jobs)
    for job in jobs:
        job.check("progressive")


def test_planes_of_the_gpu_walk_at_1080p(ica, gpu_ctx, oracle):
    """a 1080p file through the default front end: the Huffman walk on the GPU made the coefficient planes"""
    data = ica.synth_jpeg(1920, 1080, seed=5, quality=90)
    planes, (w, h, hv, _) = POC.stream_planes(oracle, data)
    jobs = [Job(planes, w, h, hv, view_planar, tag="1080p planar"), Job(planes, w, h, hv, view_nv, tag="1080p nv12")]
    info = run_jobs(ica, gpu_ctx, data, jobs, producer="front end")
    for job in jobs:
        job.check("1080p")
    assert info[0][0] == -(-240 * 135 // 256) + 2 * -(-120 * 68 // 256) and info[1][0] == -(-240 * 135 // 256) + -(-120 * 68 // 256)


# ------------------------------------------------------------------ 4. luma only

def test_luma_only_queues_no_chroma(ica, gpu_ctx, oracle):
    w, h = POC.BIG
    for layout in ("420", "444"):
        case = POC.picture(layout, POC.BIG)
        planes = POC.planes_of(oracle, case)
        jobs = [Job(planes, w, h, POC.hv_of(layout), view_planar, comps=[0], tag="luma %s" % layout),
                Job(planes, w, h, POC.hv_of(layout), view_cut, comps=[0], window=(16, 8, 100, 40), tag="luma window %s" % layout)]
        info = run_jobs(ica, gpu_ctx, case.stream(), jobs)
        for job in jobs:
            job.check("luma only")
        assert info[0][0] == -(-(34 * 9) // 256) == 2 and info[1][0] == -(-(-(-116 // 8) - 2) * 5 // 256) == 1


# ------------------------------------------------------------------ 5. a plane slot among other slots

def test_mixed_batch(ica, gpu_ctx, oracle):
    case = POC.picture("420", (77, 45), seed=2)
    planes = POC.planes_of(oracle, case)
    kind, px, _ = oracle.load(case.stream(), 3)
    assert kind == "ok"
    res = {}
    for with_planes in (False, True):
        b = ica.Batch(gpu_ctx, 3, 8 * MB, 8 * MB, 8 * MB)
        try:
            first = b.add_jpeg(case.stream(), 3)
            job = None
            if with_planes:
                job = Job(planes, 77, 45, POC.hv_of("420"), view_nv, tag="mixed")
                b.set_out_planes(b.add_jpeg(case.stream(), 0), job.request())
            last = b.add_jpeg(case.stream(), 3)
            dst = torch.full((45 * 77 * 3 + 64,), SENT, dtype=torch.uint8, device="cuda:0")
            b.set_out_tensor(last, dst.data_ptr() + 32, "u8", "HWC", 0, 0, 77, 45, 77 * 3)
            torch.cuda.synchronize()
            b.submit()
            b.wait()
            res[with_planes] = (b.fetch(first), b.fetch(last), dst.cpu().numpy())
            if job:
                job.check("mixed batch")
        finally:
            b.close()
    for a, c in zip(res[False], res[True]):
        assert np.array_equal(a, c)
    assert np.array_equal(res[True][0], px) and np.array_equal(res[True][2][32:32 + px.size].reshape(px.shape), px)
    assert (res[True][2][:32] == SENT).all() and (res[True][2][32 + px.size:] == SENT).all()


# ------------------------------------------------------------------ 6. refusals

def _hip():
    paths = {ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


def test_refusals(ica, gpu_ctx, oracle):
    L = ica.lib()
    L.mij_batch_set_out_planes.argtypes = [C.c_void_p, C.c_int, C.POINTER(ica.OutPlanes)]
    L.mij_batch_set_scale.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.mij_batch_set_roi.argtypes = [C.c_void_p] + [C.c_int] * 5
    L.mij_batch_set_roi_auto.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.mij_batch_set_out_tensor.argtypes = [C.c_void_p, C.c_int, C.POINTER(ica.OutTensor), C.c_void_p]
    L.mij_batch_set_out_f32.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mij_batch_fetch_f32.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.mij_batch_slot_plane_rect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int * 4)]
    W, H = 64, 48
    case = POC.picture("420", (W, H))
    planes = POC.planes_of(oracle, case)
    b = ica.Batch(gpu_ctx, 8, 8 * MB, 8 * MB, 8 * MB)
    slots = [b.add_jpeg(case.stream(), 3) for _ in range(6)]
    buf = torch.full((W * H * 2 + 64,), SENT, dtype=torch.uint8, device="cuda:0")
    other = torch.full((W * H * 2 + 64,), SENT, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    yp, cbp, crp = p, p + W * H, p + W * H + (W // 2) * (H // 2)

    def req(slot=0, pl=None, win=(0, 0, 0, 0), reserved=(0, 0)):
        r = ica.OutPlanes()
        for c, e in enumerate(pl if pl is not None else [(yp, W, 1), (cbp, W // 2, 1), (crp, W // 2, 1)]):
            if e is not None:
                r.planes[c] = ica.OutPlane(C.c_void_p(e[0]), e[1], e[2])
        r.x0, r.y0, r.w, r.h = win
        r.reserved[0], r.reserved[1] = reserved
        return L.mij_batch_set_out_planes(b._h, slot, C.byref(r))

    full = [(yp, W, 1), (cbp, W // 2, 1), (crp, W // 2, 1)]
    assert req() == 0
    # windows
    assert req(win=(1, 0, W, H)) == MIJ_E_ARG and req(win=(0, 1, W, H)) == MIJ_E_ARG          # leaves the picture
    assert req(win=(0, 0, 0, 8)) == MIJ_E_ARG and req(win=(0, 0, 8, -1)) == MIJ_E_ARG and req(win=(-2, 0, 8, 8)) == MIJ_E_ARG
    assert req(win=(1, 0, 8, 8)) == MIJ_E_ARG and req(win=(0, 3, 8, 8)) == MIJ_E_ARG          # off the chroma grid
    assert req(pl=[(yp, W, 1)], win=(1, 3, 8, 8)) == 0 and req() == 0                          # ... which luma alone does not have
    assert req(pl=[None, None, None]) == MIJ_E_ARG                                             # no wanted component
    assert req(pl=full + [(yp, W, 1)]) == MIJ_E_ARG                                            # a fourth plane of a three-component file
    assert req(pl=[(yp, 0, 1), None, None]) == MIJ_E_ARG and req(pl=[(yp, W, 0), None, None]) == MIJ_E_ARG
    assert req(pl=[(yp, -W, 1), None, None]) == MIJ_E_ARG and req(pl=[(yp, W, -1), None, None]) == MIJ_E_ARG
    assert req(pl=[(yp, W - 1, 1), None, None]) == MIJ_E_ARG                                   # rows overlap
    assert req(pl=[(yp, 2 * W - 2, 2), None, None]) == MIJ_E_ARG and req(pl=[(yp, 2 * W - 1, 2), None, None]) == 0 and req() == 0
    assert req(pl=[(yp, 1, 1), None, None], win=(0, 0, 1, H)) == 0 and req() == 0               # one column: rows one byte apart do not overlap
    host = np.full(W * H, SENT, np.uint8)
    assert req(pl=[(host.ctypes.data, W, 1), None, None]) == MIJ_E_ARG                         # host memory
    assert req(pl=[(1 << 47, W, 1), None, None]) == MIJ_E_ARG                                  # no allocation at all
    assert req(reserved=(0, 1)) == MIJ_E_ARG and req(reserved=(7, 0)) == MIJ_E_ARG
    assert req(slot=17) == MIJ_E_ARG
    hip = _hip()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    dp = C.c_void_p()
    assert hip.hipMalloc(C.byref(dp), W * H) == 0
    try:
        assert req(slot=5, pl=[(dp.value + 1, W, 1), None, None]) == MIJ_E_ARG                 # one byte past the end of the allocation
        assert req(slot=5, pl=[(dp.value, W, 1), None, None]) == 0                              # ... and exactly inside
        assert req(slot=5, pl=[(other.data_ptr(), W, 1)]) == 0                                  # (replaced: the allocation is freed below)
    finally:
        hip.hipFree(dp)
    # a refused request keeps the earlier one; asking again replaces it
    assert req(slot=1, pl=[(other.data_ptr() + 8, W, 1), None, None]) == 0
    assert req(slot=1) == 0 and req(slot=1, win=(1, 0, 8, 8)) == MIJ_E_ARG
    # the two kinds of request, in both orders
    tdst = torch.full((8 * 8 * 3,), SENT, dtype=torch.uint8, device="cuda:0")
    t = ica.OutTensor(C.c_void_p(tdst.data_ptr()), 0, 0, 0, 0, 8, 8, 0, 0, 24, 0)
    assert L.mij_batch_set_out_tensor(b._h, 0, C.byref(t), None) == MIJ_E_STATE
    lut = np.zeros(3 * 256, np.float32)
    assert L.mij_batch_set_out_f32(b._h, 0, lut.ctypes.data_as(C.c_void_p)) == MIJ_E_STATE
    assert L.mij_batch_set_out_tensor(b._h, 2, C.byref(t), None) == 0 and req(slot=2) == MIJ_E_STATE
    # scale and region, in both orders
    assert L.mij_batch_set_scale(b._h, 0, 2) == MIJ_E_STATE and L.mij_batch_set_scale(b._h, 0, 1) == 0
    assert L.mij_batch_set_roi(b._h, 0, 0, 0, 16, 16) == MIJ_E_STATE and L.mij_batch_set_roi_auto(b._h, 0, 1) == MIJ_E_STATE
    assert L.mij_batch_set_scale(b._h, 3, 2) == 0 and req(slot=3) == MIJ_E_STATE
    assert L.mij_batch_set_roi(b._h, 4, 0, 0, 16, 16) == 0 and req(slot=4) == MIJ_E_STATE
    # a skipped slot
    flags = b.slot_flags(5)
    b.set_flags(5, flags | 2)
    assert req(slot=5) == MIJ_E_STATE
    r4 = (C.c_int * 4)()
    assert L.mij_batch_slot_plane_rect(b._h, 0, 1, C.byref(r4)) == 0 and tuple(r4) == (0, 0, W // 2, H // 2)
    assert L.mij_batch_slot_plane_rect(b._h, 0, 3, C.byref(r4)) == MIJ_E_ARG and L.mij_batch_slot_plane_rect(b._h, 2, 0, C.byref(r4)) == MIJ_E_STATE
    torch.cuda.synchronize()
    b.submit()
    b.wait()
    assert req() == MIJ_E_STATE                                                                # after upload
    tmp = np.empty(W * H * 3, np.uint8)
    f32 = np.empty(W * H * 3, np.float32)
    for sl in (0, 1):
        assert L.mij_batch_fetch(b._h, sl, tmp.ctypes.data_as(C.c_void_p), C.c_size_t(tmp.size)) == MIJ_E_STATE
        assert L.mij_batch_fetch_f32(b._h, sl, f32.ctypes.data_as(C.c_void_p), C.c_size_t(f32.size)) == MIJ_E_STATE
    assert b.fetch_coef(0).size > 0 and np.array_equal(b.fetch_coef(0), b.fetch_coef(2))       # the coefficient planes are still served
    # slots 0 and 1 both asked for the whole picture at the same addresses last; nothing else of buf was written, nor anything of `other`
    want = np.full(buf.numel(), SENT, np.uint8)
    want[:W * H] = planes[0].reshape(-1)
    want[W * H:W * H + (W // 2) * (H // 2)] = planes[1].reshape(-1)
    want[W * H + (W // 2) * (H // 2):W * H + 2 * (W // 2) * (H // 2)] = planes[2].reshape(-1)
    assert np.array_equal(buf.cpu().numpy(), want)
    assert bool((other == SENT).all()) and (host == SENT).all()
    # reset forgets the request: the slot decodes pixels again
    b.reset()
    sl = b.add_jpeg(case.stream(), 3)
    b.submit()
    b.wait()
    assert np.array_equal(b.fetch(sl), oracle.load(case.stream(), 3)[1])
    b.close()


# ------------------------------------------------------------------ 7. TensorDecoder.decode_ycbcr

def np_of(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def dec(ica):
    d = ica.TensorDecoder("cuda:0")
    yield d
    d.close()


def test_decode_ycbcr_formats_and_sizes(ica, dec, oracle, golden):
    cases = [POC.picture("420", (33, 17)), POC.picture("444", (17, 9)), POC.picture("grey", (33, 17)), POC.picture("422", POC.BIG), POC.picture("440", (8, 8)),
             POC.picture("411", (33, 17)), POC.picture("cmyk", (17, 9))]
    datas = [c.stream() for c in cases]
    datas[2:2] = [golden.jpg("trunc_noeoi"), golden.jpg("garbage")]  # header fine and stream rejected; no header at all
    cases[2:2] = [None, None]
    names = ["420", "444", None, None, "grey", "422", "440", "h4v1", None]
    for fmt in ("planar", "nv12", "nv21"):
        pics, why = dec.decode_ycbcr(datas, format=fmt)
        assert dec.last_subsampling == names
        for i, (case, pic) in enumerate(zip(cases, pics)):
            if names[i] is None:
                assert pic is None and why[i], (fmt, i)
                continue
            assert why[i] is None
            want = POC.planes_of(oracle, case)
            if len(want) == 1:
                assert isinstance(pic, torch.Tensor) and np.array_equal(np_of(pic), want[0])
                continue
            if fmt == "nv12":
                y, pair = pic
                assert pair.shape == want[1].shape + (2,) and pair.is_contiguous()
                got = [y, pair[:, :, 0], pair[:, :, 1]]
            else:
                got = list(pic)
                if fmt == "nv21":  # one buffer, NV21 in memory
                    assert got[2].data_ptr() + 1 == got[1].data_ptr() and got[1].stride() == got[2].stride() == (2 * want[1].shape[1], 2)
            for g, wv in zip(got, want):
                assert g.dtype == torch.uint8 and np.array_equal(np_of(g), wv), (fmt, i)


def test_decode_ycbcr_luma_crops_and_out(ica, dec, oracle):
    a, g = POC.picture("420", POC.BIG), POC.picture("grey", (33, 17))
    pa = POC.planes_of(oracle, a)
    hv = POC.hv_of("420")
    pics, why = dec.decode_ycbcr([a.stream(), g.stream()], luma_only=True)
    assert why == [None, None] and np.array_equal(np_of(pics[0]), pa[0]) and np.array_equal(np_of(pics[1]), POC.planes_of(oracle, g)[0])
    win = (6, 10, 101, 37)
    pics, why = dec.decode_ycbcr([a.stream(), g.stream()], crops=[win, None], format="nv12")
    part = PM.window_of(pa, 267, 69, hv, win)
    assert np.array_equal(np_of(pics[0][0]), part[0]) and np.array_equal(np_of(pics[0][1][:, :, 0]), part[1]) and np.array_equal(np_of(pics[0][1][:, :, 1]), part[2])
    with pytest.raises(ValueError):
        dec.decode_ycbcr([a.stream()], crops=[(7, 10, 8, 8)])
    # out=: strided views of larger sentinel-filled tensors
    big = [torch.full((s[0] + 6, 2 * s[1] + 10), SENT, dtype=torch.uint8, device="cuda:0") for s in (p.shape for p in pa)]
    views = tuple(bg[3:3 + p.shape[0], 5:5 + 2 * p.shape[1]:2] for bg, p in zip(big, pa))
    assert views[0].stride() == (2 * 267 + 10, 2)
    pics, why = dec.decode_ycbcr([a.stream()], out=[views])
    assert pics[0] is views and why == [None]
    for bg, p in zip(big, pa):
        want = np.full(tuple(bg.shape), SENT, np.uint8)
        want[3:3 + p.shape[0], 5:5 + 2 * p.shape[1]:2] = p
        assert np.array_equal(np_of(bg), want)
    with pytest.raises(ValueError):  # rows that share memory
        dec.decode_ycbcr([g.stream()], out=[torch.zeros((1, 33), dtype=torch.uint8, device="cuda:0").expand(17, 33)])


def test_round_trip_through_encode_ycbcr(ica, dec):
    """the planes go into TensorEncoder.encode_ycbcr as they come out, and the stream has the source's size and factors"""
    enc = ica.TensorEncoder()
    layouts = ("420", "422", "440", "444", "grey")
    datas = [POC.picture(l, (33, 17) if l != "420" else POC.BIG).stream() for l in layouts]
    for fmt in ("planar", "nv12"):
        pics, why = dec.decode_ycbcr(datas, format=fmt)
        assert why == [None] * len(datas) and dec.last_subsampling == list(layouts)
        streams = enc.encode_ycbcr(pics, subsampling=dec.last_subsampling, quality=90)
        for src, out in zip(datas, streams):
            d0, d1 = ica.HostDecoder.probe(src), ica.HostDecoder.probe(out)
            assert (d1.width, d1.height, d1.ncomp) == (d0.width, d0.height, d0.ncomp)
            assert [(d1.comp[c].h, d1.comp[c].v) for c in range(d1.ncomp)] == [(d0.comp[c].h, d0.comp[c].v) for c in range(d0.ncomp)]
        # and once more around: the second generation's planes are decodable and of the same shapes
        again, why = dec.decode_ycbcr(streams, format=fmt)
        assert why == [None] * len(datas)
        for p, q in zip(pics, again):
            ps, qs = ([p] if isinstance(p, torch.Tensor) else list(p)), ([q] if isinstance(q, torch.Tensor) else list(q))
            assert [tuple(t.shape) for t in ps] == [tuple(t.shape) for t in qs]
