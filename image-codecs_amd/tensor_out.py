"""Batch decode straight into device tensors: crop window, flips, layout and per-channel normalisation done by k_out_tensor
(mij_batch_set_out_tensor) behind the decode kernels, written into memory the caller's torch tensor owns.

Importing this module imports torch; ``import image_codecs_amd`` alone does not (TensorDecoder and tensor_tables are loaded
from here on first use)."""
import torch

from .binding import FILTERS, Batch, Context, HostDecoder, MijError, exif_orientation, MIJ_DT_U8, MIJ_DT_F16, MIJ_DT_BF16, MIJ_DT_F32, MIJ_LAYOUT_HWC, MIJ_LAYOUT_CHW, MIJ_ARITH_LIBJPEG

_DT = {torch.uint8: MIJ_DT_U8, torch.float16: MIJ_DT_F16, torch.bfloat16: MIJ_DT_BF16, torch.float32: MIJ_DT_F32}
_BITS = {torch.uint8: torch.uint8, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}


def tensor_tables(n_out, dtype, mean=None, std=None):
    """[n_out, 256] tables of dtype on the CPU: the value table[c][v] that channel c's byte v becomes.  The contract:
    ((torch.arange(256, dtype=torch.float32) / 255 - mean[c]) / std[c]).to(dtype), with mean / std omitted meaning v / 255, and the
    identity for torch.uint8 (which takes no mean / std)."""
    n_out = int(n_out)
    if dtype not in _DT:
        raise ValueError("dtype must be one of uint8, float16, bfloat16, float32 (got %s)" % (dtype,))
    if dtype == torch.uint8:
        if mean is not None or std is not None:
            raise ValueError("uint8 output takes no mean / std")
        return torch.arange(256, dtype=torch.uint8).repeat(n_out, 1)
    v = torch.arange(256, dtype=torch.float32) / 255
    if mean is None and std is None:
        return v.to(dtype).repeat(n_out, 1)
    mean = _per_channel(mean, n_out, "mean", 0.0)
    std = _per_channel(std, n_out, "std", 1.0)
    return torch.stack([((v - mean[c]) / std[c]).to(dtype) for c in range(n_out)])


def _per_channel(vals, n_out, what, default):
    if vals is None:
        return [default] * n_out
    vals = [float(x) for x in vals]
    if len(vals) != n_out:
        raise ValueError("%s has %d values for %d channels" % (what, len(vals), n_out))
    return vals


def _flags(v, n, what):
    if v is None:
        return [False] * n
    if isinstance(v, bool):
        return [v] * n
    v = [bool(x) for x in v]
    if len(v) != n:
        raise ValueError("%s has %d entries for %d pictures" % (what, len(v), n))
    return v


def _orientations(v, datas):
    """decode's orientation= as one value 1..8 per picture"""
    n = len(datas)
    if v is None:
        return [1] * n
    if isinstance(v, str):
        if v != "exif":
            raise ValueError("orientation must be None, 'exif', 1..8 or one value per picture (got %r)" % (v,))
        return [exif_orientation(d) for d in datas]
    try:
        vals = [v] * n if isinstance(v, int) else list(v)
    except TypeError:
        raise ValueError("orientation must be None, 'exif', 1..8 or one value per picture (got %r)" % (v,)) from None
    if len(vals) != n:
        raise ValueError("orientation has %d values for %d pictures" % (len(vals), n))
    for o in vals:
        if isinstance(o, bool) or not isinstance(o, int) or not 1 <= o <= 8:
            raise ValueError("an orientation is an int 1..8 (got %r)" % (o,))
    return vals


def _reduces(v, n):
    """decode's reduce= as "auto" or one denominator 1, 2, 4 or 8 per picture"""
    if v is None:
        return [1] * n
    if isinstance(v, str):
        if v != "auto":
            raise ValueError("reduce must be None, 1, 2, 4, 8, 'auto' or one value per picture (got %r)" % (v,))
        return "auto"
    try:
        vals = [v] * n if isinstance(v, int) else list(v)
    except TypeError:
        raise ValueError("reduce must be None, 1, 2, 4, 8, 'auto' or one value per picture (got %r)" % (v,)) from None
    if len(vals) != n:
        raise ValueError("reduce has %d values for %d pictures" % (len(vals), n))
    for s in vals:
        if isinstance(s, bool) or not isinstance(s, int) or s not in (1, 2, 4, 8):
            raise ValueError("a reduce denominator is 1, 2, 4 or 8 (got %r)" % (s,))
    return vals


def reducible(d):
    """Whether mij_batch_set_scale takes a picture with descriptor d at a denominator above 1 (include/mij.h): one component, or
    three-component YCbCr whose luma has the picture's resolution with 4:4:4, 4:2:0 or 4:2:2 chroma."""
    if d.ncomp == 1 and d.color == 0:
        return True
    if d.ncomp != 3 or d.color not in (0, 1) or (d.color == 0 and d.n_out >= 3):
        return False
    if (d.comp[0].h, d.comp[0].v) != (d.h_max, d.v_max) or any((d.comp[c].h, d.comp[c].v) != (1, 1) for c in (1, 2)):
        return False
    return (d.h_max, d.v_max) in ((1, 1), (2, 2), (2, 1))


ARITHMETICS = ("stb", "libjpeg")


def libjpeg_decodable(d):
    """Whether mij_batch_set_arith takes a picture with descriptor d for libjpeg's arithmetic (include/mij.h, LIBJPEG ARITHMETIC): one
    component, or three-component YCbCr whose luma has the picture's resolution with 4:4:4, 4:2:2, 4:4:0 or 4:2:0 chroma."""
    if d.ncomp == 1 and d.color == 0:
        return True
    if d.ncomp != 3 or d.color not in (0, 1) or (d.color == 0 and d.n_out >= 3):
        return False
    if (d.comp[0].h, d.comp[0].v) != (d.h_max, d.v_max) or (d.comp[1].h, d.comp[1].v) != (d.comp[2].h, d.comp[2].v):
        return False
    if d.h_max % d.comp[1].h or d.v_max % d.comp[1].v:
        return False
    return (d.h_max // d.comp[1].h, d.v_max // d.comp[1].v) in _SUBSAMPLINGS


def auto_reduce(w, h, out_w, out_h):
    """The largest denominator at which a w x h picture, reduced, is still at least out_w x out_h: never upsample from a reduced picture"""
    for s in (8, 4, 2):
        if -(-w // s) >= out_w and -(-h // s) >= out_h:
            return s
    return 1


_SUBSAMPLINGS = {(1, 1): "444", (2, 1): "422", (1, 2): "440", (2, 2): "420"}
YCBCR_FORMATS = ("planar", "nv12", "nv21")


def ycbcr_subsampling(d):
    """A descriptor's sampling as TensorEncoder.encode_ycbcr names it -- "444", "422", "440", "420" or "grey" -- where the file is one of
    those five (chroma at 1 x 1 under the luma factors); "h{H}v{V}" of the luma factors for anything else (4:1:1: "h4v1")."""
    if d.ncomp == 1:
        return "grey"
    lh, lv = d.comp[0].h, d.comp[0].v
    plain = (lh, lv) == (d.h_max, d.v_max) and all((d.comp[c].h, d.comp[c].v) == (1, 1) for c in range(1, d.ncomp))
    return _SUBSAMPLINGS[(lh, lv)] if plain and (lh, lv) in _SUBSAMPLINGS else "h%dv%d" % (lh, lv)


def plane_windows(d, win, comps):
    """(x0, y0, w, h) of the picture window `win` in the samples of each component of comps (include/mij.h, PLANE OUTPUT); ValueError for
    a window off the grid of one of them"""
    x0, y0, w, h = win
    out = []
    for c in comps:
        ch, cv = d.comp[c].h, d.comp[c].v
        if (x0 * ch) % d.h_max or (y0 * cv) % d.v_max:
            raise ValueError("crop %s starts off the sample grid of component %d (x0 a multiple of %d / %d, y0 of %d / %d)" % (win, c, d.h_max, ch, d.v_max, cv))
        sx0, sy0 = x0 * ch // d.h_max, y0 * cv // d.v_max
        out.append((sx0, sy0, -(-(x0 + w) * ch // d.h_max) - sx0, -(-(y0 + h) * cv // d.v_max) - sy0))
    return out


def _pitches(t, what):
    """(row pitch, sample pitch) in bytes of a 2-D uint8 tensor; the stride of an axis of one element addresses nothing"""
    rp, xp = t.stride(0), t.stride(1)
    if (t.shape[0] > 1 and rp < 1) or (t.shape[1] > 1 and xp < 1):
        raise ValueError("%s has strides %s: planes need positive strides" % (what, tuple(t.stride())))
    return (rp if rp >= 1 else 1), (xp if xp >= 1 else 1)


def _one_hip_runtime():
    """torch and the library must share one HIP runtime, or torch's allocations are unknown to the library (which then refuses them).
    They do when torch is imported before the library is first loaded; loaded the other way round, torch brings its own copy."""
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    if len(paths) > 1:
        raise RuntimeError("two HIP runtimes in this process (%s): import torch before the first call into image_codecs_amd" % ", ".join(sorted(paths)))


class TensorDecoder:
    """Decodes batches of JPEGs into one [N, C, h, w] (layout "CHW") or [N, h, w, C] ("HWC") tensor on a GPU.  Owns a Context and a
    Batch, grown as needed and reused across calls.  decode() is synchronous: it synchronises the device's current torch stream
    before the batch writes the tensor and waits for the batch before it returns."""

    def __init__(self, device=None):
        dev = torch.device("cuda") if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("TensorDecoder needs a GPU device, got %s" % dev)
        self._dev = dev  # without an index: the current device, looked up at first use (argument checks need no device)
        self._ctx = None
        self._batch = None
        self._cap = (0, 0, 0)
        self.last_subsampling = []  # of the last decode_ycbcr: one name per picture, None for a rejected one
        self.last_arithmetic = []  # of the last decode: "stb" or "libjpeg" per picture, None for a rejected one

    @property
    def device(self):
        if self._dev.index is None:
            self._dev = torch.device("cuda", torch.cuda.current_device())
        return self._dev

    def close(self):
        if self._batch is not None:
            self._batch.close()
            self._batch = None
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
        self._cap = (0, 0, 0)

    def _batch_for(self, n, coef, out):
        need = (max(1, n), max(coef, 256), max(out, 256))
        if self._batch is None or any(a > b for a, b in zip(need, self._cap)):
            if self._batch is not None:
                self._batch.close()
                self._batch = None
            if self._ctx is None:
                self._ctx = Context(self.device.index)
            cap = tuple(max(a, b) for a, b in zip(need, self._cap))
            self._batch = Batch(self._ctx, cap[0], cap[1], cap[1], cap[2])
            self._cap = cap
        else:
            self._batch.reset()
        return self._batch

    def decode(self, datas, *, req_comp=3, crops=None, flip_x=None, flip_y=None, layout="CHW", dtype=torch.float16, mean=None, std=None,
               out=None, threads=16, size=None, filter="bilinear", orientation=None, reduce=None, roi=False, arithmetic="stb"):
        """-> (tensor, reasons).  crops: None (the whole picture; every picture the same size) or one (x0, y0, w, h) per picture, all of
        the same w and h.  size: None, or (out_h, out_w): each window is resized to it with filter (box, bilinear, hamming, bicubic or
        lanczos; the exact integer contract of mij_batch_set_out_tensor_resized, Pillow's for one channel, crop first), and windows and
        pictures may then differ in size.  flip_x / flip_y: None, one bool for all, or one per picture (after a resize they reverse the
        resized columns / rows).  The value of channel c's byte v is tensor_tables(C, dtype, mean, std)[c][v].  out: a tensor of the
        right shape and dtype on this device, with any row / plane padding (e.g. a slice of a larger tensor); None allocates one.  A rejected picture leaves its [i] slice untouched (zero in a
        tensor allocated here) and gets its reason in reasons[i]; reasons[i] is None for a decoded one.  orientation: None (the stored
        pictures), "exif" (each file's EXIF Orientation tag), one int 1..8 for all or one per picture: each picture is first turned into
        its displayed picture (include/mij.h, mij_batch_set_out_tensor_oriented), and crops, size and the tensor's shape are in its
        displayed frame.  reduce: None or 1 (full-size decode), 2, 4 or 8 for all pictures or one value per picture: the picture is
        decoded at that fraction of its size straight from its coefficients (mij_batch_set_scale: ceil(W / s) x ceil(H / s)), and crops,
        size and the tensor's shape are in that reduced (and oriented) frame; a picture whose layout has no reduced decode (4:4:0, 4:1:1,
        RGB-tagged, CMYK) is rejected with its reason when s > 1.  "auto" (needs size= and crops=None) takes per picture the largest s at
        which the displayed reduced picture is still at least out_w x out_h -- it never upsamples from a reduced picture -- and 1 for
        layouts without a reduced decode.  roi: False, or True: with crops, every picture decodes only the MCUs its window reads
        (mij_batch_set_roi_auto; the tensor is the same, bit for bit); with crops=None it changes nothing.  arithmetic: "stb" (the
        reference's pixels) or "libjpeg": every picture is decoded with libjpeg's arithmetic (mij_batch_set_arith: ISLOW inverse DCT,
        fancy upsampling, the jdcolor tables), so the pixels under crops, size, orientation and the tables are the ones
        PIL.Image.open(...).convert("RGB") and torchvision.io.decode_jpeg give, byte for byte; it takes no reduce other than None or 1
        (ValueError), and a picture whose layout it does not serve (4:1:1, RGB-tagged, CMYK) is rejected with its reason.
        last_arithmetic[i] names what picture i used (None for a rejected one)."""
        if arithmetic not in ARITHMETICS:
            raise ValueError("arithmetic must be one of %s (got %r)" % (", ".join(ARITHMETICS), arithmetic))
        if arithmetic == "libjpeg" and not (reduce is None or (isinstance(reduce, int) and not isinstance(reduce, bool) and reduce == 1)):
            raise ValueError("arithmetic='libjpeg' has no reduced-size decode: reduce must be None or 1 (got %r)" % (reduce,))
        if not isinstance(roi, bool):
            raise ValueError("roi must be False or True (got %r)" % (roi,))
        datas = list(datas)
        n = len(datas)
        if layout not in ("CHW", "HWC"):
            raise ValueError("layout must be 'CHW' or 'HWC'")
        if dtype not in _DT:
            raise ValueError("dtype must be one of uint8, float16, bfloat16, float32 (got %s)" % (dtype,))
        if not 0 <= int(req_comp) <= 4:
            raise ValueError("req_comp must be 0..4")
        fx, fy = _flags(flip_x, n, "flip_x"), _flags(flip_y, n, "flip_y")
        if dtype == torch.uint8 and (mean is not None or std is not None):
            raise ValueError("uint8 output takes no mean / std")
        if crops is not None and len(crops) != n:
            raise ValueError("crops has %d windows for %d pictures" % (len(crops), n))
        if filter not in FILTERS:
            raise ValueError("filter must be one of %s (got %r)" % (", ".join(FILTERS), filter))
        orients = _orientations(orientation, datas)
        scales = _reduces(reduce, n)
        if scales == "auto" and (size is None or crops is not None):
            raise ValueError("reduce='auto' needs size= and crops=None")
        if size is not None:
            try:
                size = tuple(int(v) for v in size)
            except TypeError:
                raise ValueError("size is (out_h, out_w), got %r" % (size,)) from None
            if len(size) != 2 or not all(1 <= v <= 16384 for v in size):
                raise ValueError("size is (out_h, out_w), each 1..16384, got %r" % (size,))
        # headers only: sizes, channels and arena needs, before any device call
        descs, reasons = [], [None] * n
        for i, d in enumerate(datas):
            try:
                descs.append(HostDecoder.probe(d, req_comp))
            except MijError as e:
                descs.append(None)
                reasons[i] = str(e)
        ok = [d for d in descs if d is not None]
        # displayed sizes: orientations 5..8 swap the axes
        dsz = [None if d is None else ((d.height, d.width) if orients[i] >= 5 else (d.width, d.height)) for i, d in enumerate(descs)]
        if scales == "auto":
            scales = [1 if z is None or not reducible(descs[i]) else auto_reduce(z[0], z[1], size[1], size[0]) for i, z in enumerate(dsz)]
        refused = {}  # pictures asked for at a reduced size their layout does not have: decoded, but not written
        for i, d in enumerate(descs):
            if d is not None and scales[i] > 1 and not reducible(d):
                refused[i] = "no reduced-size decode for this layout (%d components, colour mode %d, luma %dx%d of %dx%d)" % (
                    d.ncomp, d.color, d.comp[0].h, d.comp[0].v, d.h_max, d.v_max)
            elif d is not None and arithmetic == "libjpeg" and not libjpeg_decodable(d):
                refused[i] = "no decode with libjpeg's arithmetic for this layout (%d components, colour mode %d, luma %dx%d of %dx%d)" % (
                    d.ncomp, d.color, d.comp[0].h, d.comp[0].v, d.h_max, d.v_max)
        dsz = [None if z is None or i in refused else (-(-z[0] // scales[i]), -(-z[1] // scales[i])) for i, z in enumerate(dsz)]
        chans = {d.n_out for d in ok}
        if len(chans) > 1:
            raise ValueError("pictures decode to different channel counts %s (pass req_comp)" % sorted(chans))
        if crops is None:
            sizes = {z for z in dsz if z is not None}
            if len(sizes) > 1 and size is None:
                raise ValueError("pictures of different sizes %s need crops" % sorted(sizes))
            wins = [None if z is None else (0, 0, z[0], z[1]) for z in dsz]
        else:
            wins = [tuple(int(v) for v in c) for c in crops]
            if any(len(c) != 4 for c in wins):
                raise ValueError("a crop is (x0, y0, w, h)")
            if len({c[2:] for c in wins}) > 1 and size is None:
                raise ValueError("crop windows of different sizes %s" % sorted({c[2:] for c in wins}))
            for i, (c, z) in enumerate(zip(wins, dsz)):
                if c[2] < 1 or c[3] < 1 or c[0] < 0 or c[1] < 0 or (z is not None and (c[0] + c[2] > z[0] or c[1] + c[3] > z[1])):
                    raise ValueError("crop %s of picture %d outside its %dx%d picture" % (c, i, z[0] if z else 0, z[1] if z else 0))
        whs = {c[2:] for i, c in enumerate(wins) if c is not None and i not in refused} if size is None else {(size[1], size[0])}
        C = req_comp if req_comp else (chans.pop() if chans else None)
        if out is not None:
            if out.dim() != 4:
                raise ValueError("out must have 4 dimensions")
            C = C or (out.shape[1] if layout == "CHW" else out.shape[3])
            oh, ow = (out.shape[2], out.shape[3]) if layout == "CHW" else (out.shape[1], out.shape[2])
            whs.add((ow, oh))
        if not whs or C is None:
            raise ValueError("no decodable picture to size the tensor (pass out)")
        if len(whs) > 1:
            raise ValueError("window sizes %s differ from out" % sorted(whs))
        w, h = whs.pop()
        tables = None if dtype == torch.uint8 else tensor_tables(C, dtype, mean, std)
        shape = (n, C, h, w) if layout == "CHW" else (n, h, w, C)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self.device)
            fresh = True
        else:
            fresh = False
            if out.device != self.device:
                raise ValueError("out is on %s, the decoder on %s" % (out.device, self.device))
            if tuple(out.shape) != shape or out.dtype != dtype:
                raise ValueError("out is %s %s, %s %s expected" % (tuple(out.shape), out.dtype, shape, dtype))
        st = out.stride()
        if layout == "CHW":
            ok_strides = (n < 2 or st[0] >= 0) and (w < 2 or st[3] == 1) and st[2] >= 0 and st[1] >= 0
            row_pitch, plane_pitch = st[2], st[1]
        else:
            ok_strides = (n < 2 or st[0] >= 0) and (C < 2 or st[3] == 1) and (w < 2 or st[2] == C) and st[1] >= 0
            row_pitch, plane_pitch = st[1], 0
        if not ok_strides:
            raise ValueError("out strides %s: %s needs unit-stride channels / pixels" % (st, layout))
        self.last_arithmetic = [None] * n
        if n == 0:
            return out, reasons
        _one_hip_runtime()
        cb = sum(Batch.coef_bytes(d) for d in ok)
        ob = sum(Batch.out_bytes(d) for d in ok)
        b = self._batch_for(n, cb, ob)
        _, slots, why = b.decode_jpegs(datas, req_comp, threads=int(threads))
        es = out.element_size()
        tb = None if tables is None else tables.contiguous().view(_BITS[dtype]).numpy()
        for i, sl in enumerate(slots):
            if sl < 0:
                reasons[i] = why[i] or reasons[i] or "rejected"
                continue
            if i in refused:
                reasons[i] = refused[i]
                continue
            if descs[i] is not None:
                b.descs[sl] = descs[i]  # already probed: spares set_out_tensor a second header parse
            if scales[i] > 1:
                try:
                    b.set_scale(sl, scales[i])
                except MijError as e:  # a marker behind the header changed the colour branch
                    reasons[i] = str(e)
                    continue
            if arithmetic == "libjpeg":
                try:
                    b.set_arith(sl, MIJ_ARITH_LIBJPEG)
                except MijError as e:  # a marker behind the header changed the colour branch
                    reasons[i] = str(e)
                    continue
            self.last_arithmetic[i] = arithmetic
            x0, y0 = wins[i][0], wins[i][1]
            lay = MIJ_LAYOUT_CHW if layout == "CHW" else MIJ_LAYOUT_HWC
            if size is None:
                b.set_out_tensor(sl, out.data_ptr() + i * st[0] * es, _DT[dtype], lay, x0, y0, w, h, row_pitch, plane_pitch, fx[i], fy[i], tb,
                                 orientation=orients[i])
            else:
                b.set_out_tensor_resized(sl, out.data_ptr() + i * st[0] * es, _DT[dtype], lay, x0, y0, wins[i][2], wins[i][3], w, h, row_pitch,
                                         plane_pitch, fx[i], fy[i], tb, filter, orientation=orients[i])
            if roi and crops is not None:
                b.set_roi_auto(sl)
        torch.cuda.current_stream(self.device).synchronize()
        b.submit()
        b.wait()
        if fresh:
            for i, r in enumerate(reasons):
                if r is not None:
                    out[i].zero_()
        return out, reasons

    def decode_ycbcr(self, datas, *, format="planar", luma_only=False, crops=None, out=None, threads=16):
        """-> (pictures, reasons): the Y, Cb and Cr samples of each JPEG as the file stores them, at their own resolutions -- no chroma
        upsampling, no colour conversion, no RGB in between (include/mij.h, PLANE OUTPUT; k_planes_out).  pictures[i] is what
        TensorEncoder.encode_ycbcr takes, uint8 tensors on this device:
            format "planar"  (Y, Cb, Cr), three 2-D tensors (I420 for a 4:2:0 file)
            format "nv12"    (Y, CbCr) with CbCr of shape [ch, cw, 2], Cb and Cr interleaved in memory
            format "nv21"    (Y, Cb, Cr) where Cb and Cr are the two strided slices [:, :, 1] and [:, :, 0] of one [ch, cw, 2] buffer, which
                             is NV21 in memory (torch has no view that reverses an axis)
        and Y alone for a grey file or with luma_only=True, which transforms no chroma block at all.  A rejected picture is None with
        its reason in reasons[i].  Pictures may differ in size and sampling; Y is H x W, Cb and Cr are ceil(H * v_c / v_max) x
        ceil(W * h_c / h_max).  last_subsampling[i] names the file's sampling as encode_ycbcr names it ("444", "422", "440", "420",
        "grey"; "h{H}v{V}" of the luma factors for other files, None for a rejected picture), so that
        enc.encode_ycbcr(pictures, subsampling=dec.last_subsampling) takes the result as it is.
        crops: None, or one (x0, y0, w, h) in picture coordinates or None per picture; every wanted component then receives the samples
        its part of the window holds (Batch.plane_rect).  x0 and y0 lie on the grid of every wanted component (4:2:0: even); an
        off-grid window is a ValueError.  out: None, or one entry per picture in the shapes above (None for pictures to allocate), with
        any positive strides; a picture written into out[i] is out[i].  Planes allocated here are slices of one tensor per plane and
        group of equally shaped pictures (three allocations for a batch of equal 4:2:0 pictures), so a kept picture keeps its group's
        memory alive; .clone() what outlives the batch.
        Served here: grey and YCbCr files.  RGB-tagged, CMYK, YCCK and other four-component files are rejected per picture with a
        reason (mij_batch_set_out_planes serves them: their planes are their stored components)."""
        datas = list(datas)
        n = len(datas)
        if format not in YCBCR_FORMATS:
            raise ValueError("format must be one of %s (got %r)" % (", ".join(YCBCR_FORMATS), format))
        if not isinstance(luma_only, bool):
            raise ValueError("luma_only must be a bool (got %r)" % (luma_only,))
        if crops is not None:
            crops = list(crops)
            if len(crops) != n:
                raise ValueError("crops has %d windows for %d pictures" % (len(crops), n))
            crops = [None if c is None else tuple(int(v) for v in c) for c in crops]
            if any(c is not None and len(c) != 4 for c in crops):
                raise ValueError("a crop is (x0, y0, w, h)")
        if out is not None:
            out = list(out)
            if len(out) != n:
                raise ValueError("out has %d entries for %d pictures" % (len(out), n))
        # headers only: geometry, shapes and arena needs, before any device call
        descs, reasons = [], [None] * n
        for i, data in enumerate(datas):
            try:
                d = HostDecoder.probe(data, 0)
            except MijError as e:
                d, reasons[i] = None, str(e)
            if d is not None and not ((d.ncomp == 1 and d.color == 0) or (d.ncomp == 3 and d.color == 1)):
                reasons[i] = "not a grey or YCbCr file (%d components, colour mode %d): its planes are served by mij_batch_set_out_planes only" % (d.ncomp, d.color)
                d = None
            descs.append(d)
        plans = [None] * n  # per picture: (components, their windows, picture window or None)
        for i, d in enumerate(descs):
            if d is None:
                continue
            comps = [0] if (luma_only or d.ncomp == 1) else [0, 1, 2]
            win = (0, 0, d.width, d.height) if crops is None or crops[i] is None else crops[i]
            if win[2] < 1 or win[3] < 1 or win[0] < 0 or win[1] < 0 or win[0] + win[2] > d.width or win[1] + win[3] > d.height:
                raise ValueError("crop %s of picture %d outside its %dx%d picture" % (win, i, d.width, d.height))
            rects = plane_windows(d, win, comps)
            if len(comps) == 3 and format != "planar" and rects[1] != rects[2]:
                reasons[i], descs[i] = "Cb and Cr differ in sampling: no %s" % format, None
                continue
            plans[i] = (comps, rects, None if crops is None or crops[i] is None else win)
        pictures, views = [None] * n, [None] * n
        for i, plan in enumerate(plans):  # the caller's tensors first: every ValueError comes before the first allocation on the device
            if plan is None or out is None or out[i] is None:
                continue
            comps, rects, _ = plan
            shapes = [(r[3], r[2]) for r in rects]
            given = out[i]
            parts = [given] if isinstance(given, torch.Tensor) else list(given)
            if len(parts) == 2 and len(comps) == 3 and isinstance(parts[1], torch.Tensor) and parts[1].dim() == 3 and parts[1].shape[2] == 2:
                parts = [parts[0], parts[1][:, :, 0], parts[1][:, :, 1]]
            if len(parts) != len(comps):
                raise ValueError("out[%d] has %d planes, %d expected" % (i, len(parts), len(comps)))
            for k, (t, s) in enumerate(zip(parts, shapes)):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or tuple(t.shape) != s:
                    raise ValueError("out[%d] plane %d is %s, uint8 %s expected" % (i, k, "%s %s" % (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t), s))
                _pitches(t, "plane %d of out[%d]" % (k, i))
                if t.device.type != "cuda" or (self._dev.index is not None and t.device != self._dev):
                    raise ValueError("out[%d] plane %d is on %s, the decoder on %s" % (i, k, t.device, self._dev))
            pictures[i], views[i] = given, parts
        # the pictures to allocate, by shape: one tensor per plane and group of equal pictures, whose slices the pictures are (a batch
        # of 256 equal pictures is three allocations, not 768)
        groups = {}
        for i, plan in enumerate(plans):
            if plan is not None and views[i] is None:
                groups.setdefault(tuple((r[3], r[2]) for r in plan[1]), []).append(i)
        for shapes, members in groups.items():
            g = len(members)
            ys = torch.empty((g,) + shapes[0], dtype=torch.uint8, device=self.device).unbind(0)
            if len(shapes) == 1:
                for k, i in enumerate(members):
                    pictures[i], views[i] = ys[k], [ys[k]]
            elif format == "planar":
                cbs, crs = (torch.empty((g,) + s, dtype=torch.uint8, device=self.device).unbind(0) for s in shapes[1:])
                for k, i in enumerate(members):
                    pictures[i] = (ys[k], cbs[k], crs[k])
                    views[i] = list(pictures[i])
            else:
                pairs = torch.empty((g,) + shapes[1] + (2,), dtype=torch.uint8, device=self.device)
                lo, hi = pairs[..., 0].unbind(0), pairs[..., 1].unbind(0)
                for k, (i, pair) in enumerate(zip(members, pairs.unbind(0))):
                    if format == "nv12":
                        pictures[i], views[i] = (ys[k], pair), [ys[k], lo[k], hi[k]]
                    else:
                        pictures[i] = (ys[k], hi[k], lo[k])
                        views[i] = list(pictures[i])
        triples = [None if v is None else [(t,) + _pitches(t, "plane %d of picture %d" % (k, i)) for k, t in enumerate(v)] for i, v in enumerate(views)]
        self.last_subsampling = [None if d is None else ycbcr_subsampling(d) for d in descs]
        ok = [d for d in descs if d is not None]
        if not ok:
            return pictures, reasons
        _one_hip_runtime()
        b = self._batch_for(n, sum(Batch.coef_bytes(d) for d in ok), sum(Batch.out_bytes(d) for d in ok))
        good = [i for i, d in enumerate(descs) if d is not None]
        _, slots, why = b.decode_jpegs([datas[i] for i in good], 0, threads=int(threads))
        asked = 0
        for k, (i, sl) in enumerate(zip(good, slots)):
            if sl < 0:
                reasons[i], pictures[i], self.last_subsampling[i] = why[k] or "rejected", None, None
                continue
            b.descs[sl] = descs[i]
            try:
                b.set_out_planes(sl, [(t.data_ptr(), rp, xp) for t, rp, xp in triples[i]], plans[i][2])
                asked += 1
            except MijError as e:  # a marker behind the header changed what the file is
                reasons[i], pictures[i], self.last_subsampling[i] = str(e), None, None
        if asked:
            torch.cuda.current_stream(self.device).synchronize()
            b.submit()
            b.wait()
        return pictures, reasons
