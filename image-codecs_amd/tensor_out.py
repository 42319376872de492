"""Batch decode straight into device tensors: crop window, flips, layout and per-channel normalisation done by k_out_tensor
(mij_batch_set_out_tensor) behind the decode kernels, written into memory the caller's torch tensor owns.

Importing this module imports torch; ``import image_codecs_amd`` alone does not (TensorDecoder and tensor_tables are loaded
from here on first use)."""
import torch

from .binding import FILTERS, Batch, Context, HostDecoder, MijError, exif_orientation, MIJ_DT_U8, MIJ_DT_F16, MIJ_DT_BF16, MIJ_DT_F32, MIJ_LAYOUT_HWC, MIJ_LAYOUT_CHW

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


def auto_reduce(w, h, out_w, out_h):
    """The largest denominator at which a w x h picture, reduced, is still at least out_w x out_h: never upsample from a reduced picture"""
    for s in (8, 4, 2):
        if -(-w // s) >= out_w and -(-h // s) >= out_h:
            return s
    return 1


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
               out=None, threads=16, size=None, filter="bilinear", orientation=None, reduce=None, roi=False):
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
        (mij_batch_set_roi_auto; the tensor is the same, bit for bit); with crops=None it changes nothing."""
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
