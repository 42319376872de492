"""JPEG streams straight from device tensors: the encoder's slots read caller-owned device memory (mij_enc_add_device, a gather
kernel in place of the host copy), and the Huffman stage runs on the GPU too (mij_enc_stream_reserve), so only finished streams
cross PCIe.  The counterpart of TensorDecoder: encode() takes uint8 pictures, encode_normalized() the float16 / bfloat16 / float32
tensors a model works on, de-normalised inside the gather kernel (mij_enc_add_device_float).

Importing this module imports torch; ``import image_codecs_amd`` alone does not (TensorEncoder is loaded from here on first use)."""
import ctypes as C
import math

import torch

from .binding import (Context, Encoder, InConvert, InTensor, WritePlan, emit_jpeg, emit_transcoded, lib, sampled_plan, sampling_factors,
                      sampling_name, _qtable_pair, plane_sampling, planes_plan, split_planes, video_range_convert, MIJ_LAYOUT_HWC, MIJ_LAYOUT_CHW, MIJ_DT_F16, MIJ_DT_BF16, MIJ_DT_F32,
                      MIJ_ARITH_LIBJPEG, ARITHMETICS, libjpeg_reframe)
from .tensor_out import _one_hip_runtime

# one launch takes at most this many pictures / bytes of pixel arena; larger calls are cut into chunks
MAX_SLOTS = 4096
MAX_PIXEL_BYTES = 2 << 30


def _plan(w, h, c, quality):
    p = WritePlan()
    L = lib()
    L.mjw_plan_init.argtypes = [C.POINTER(WritePlan), C.c_int, C.c_int, C.c_int, C.c_int]
    if not L.mjw_plan_init(C.byref(p), int(w), int(h), int(c), int(quality)):
        raise ValueError("picture %dx%d with %d channels is refused by the writer" % (w, h, c))
    return p


def _align(v, a):
    return (v + a - 1) // a * a


_FLOAT_DT = {torch.float16: MIJ_DT_F16, torch.bfloat16: MIJ_DT_BF16, torch.float32: MIJ_DT_F32}


def _numbers(vals, what):
    if vals is None:
        return None
    try:
        return [float(x) for x in vals]
    except TypeError:
        raise ValueError("%s must be None or a sequence of numbers, one per channel" % what) from None


def denorm_scale_bias(n, mean=None, std=None):
    """-> (scale, bias), n float32 values each (as Python floats): scale[c] = float32(255.0 * std[c]), bias[c] = float32(255.0 *
    mean[c]), the products taken in Python doubles; mean / std omitted mean 0 / 1, tensor_tables' convention.  ValueError for a wrong
    number of values, a std of 0 and anything that is not finite as a float32."""
    out = []
    for vals, what, default in ((_numbers(std, "std"), "std", 1.0), (_numbers(mean, "mean"), "mean", 0.0)):
        if vals is None:
            vals = [default] * n
        if len(vals) != n:
            raise ValueError("%s has %d values for %d channels" % (what, len(vals), n))
        f = [C.c_float(255.0 * v).value for v in vals]
        if not all(math.isfinite(v) for v in f):
            raise ValueError("%s %r: a value is not finite as a float32 once multiplied by 255" % (what, vals))
        if what == "std" and 0.0 in f:
            raise ValueError("std %r holds a 0 (as a float32 once multiplied by 255)" % (vals,))
        out.append(f)
    return out[0], out[1]


def _restart_values(v, n, name):
    """restart_rows= / restart_mcus= as one int >= 0 per picture (None is 0: none)"""
    what = name + " must be None, an int >= 0 or one of those per picture (got %r)"
    if v is None or (isinstance(v, int) and not isinstance(v, bool)):
        vals = [v] * n
    else:
        if isinstance(v, (str, bytes, torch.Tensor)):
            raise ValueError(what % (v,))
        try:
            vals = list(v)
        except TypeError:
            raise ValueError(what % (v,)) from None
        if len(vals) != n:
            raise ValueError("%s has %d values for %d pictures" % (name, len(vals), n))
    for x in vals:
        if not (x is None or (isinstance(x, int) and not isinstance(x, bool) and x >= 0)):
            raise ValueError(what % (x,))
    return [0 if x is None else x for x in vals]


def _sampling_values(v, n):
    """subsampling= as one name or None per picture"""
    if v is None or isinstance(v, str):
        vals = [v] * n
    else:
        if isinstance(v, (bytes, torch.Tensor)):
            raise ValueError("subsampling must be None, a sampling name or one of those per picture (got %r)" % (v,))
        try:
            vals = list(v)
        except TypeError:
            raise ValueError("subsampling must be None, a sampling name or one of those per picture (got %r)" % (v,)) from None
        if len(vals) != n:
            raise ValueError("subsampling has %d values for %d pictures" % (len(vals), n))
    for x in vals:
        sampling_factors(x)  # ValueError for an unknown name
    return vals


def _arith_values(v, n):
    """arithmetic= as one of "stb" / "libjpeg" per picture"""
    what = "arithmetic must be 'stb', 'libjpeg' or one of those per picture (got %r)"
    if isinstance(v, str):
        vals = [v] * n
    else:
        if v is None or isinstance(v, (bytes, torch.Tensor)):
            raise ValueError(what % (v,))
        try:
            vals = list(v)
        except TypeError:
            raise ValueError(what % (v,)) from None
        if len(vals) != n:
            raise ValueError("arithmetic has %d values for %d pictures" % (len(vals), n))
    for x in vals:
        if not isinstance(x, str) or x not in ARITHMETICS:
            raise ValueError(what % (x,))
    return vals


class TensorEncoder:
    """Encodes uint8 pictures that live on a GPU into JPEG byte streams, each exactly what stbi_write_jpg_to_func writes for that
    picture (encode), and float16 / bfloat16 / float32 pictures as the uint8 pictures they de-normalise to (encode_normalized).
    Owns a Context, an Encoder and its emission arena, grown as needed and reused across calls.  Both calls are synchronous: they
    synchronise the device's current torch stream before the encoder reads the tensors and wait for the streams before they
    return.  Slots whose streams do not fit the arena are finished on the host from their data units (last_host_emitted counts
    them) and the arena grows for the next call."""

    def __init__(self, device=None):
        dev = torch.device("cuda") if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("TensorEncoder needs a GPU device, got %s" % dev)
        self._dev = dev  # without an index: the current device, looked up at first use (argument checks need no device)
        self._ctx = None
        self._enc = None
        self._cap = (0, 0, 0)
        self._arena = 0
        self.last_host_emitted = 0
        self.last_restarts = []
        self.last_subsampling = []
        self.last_arithmetic = []

    @property
    def device(self):
        if self._dev.index is None:
            self._dev = torch.device("cuda", torch.cuda.current_device())
        return self._dev

    @property
    def arena_bytes(self):
        return self._arena

    def close(self):
        if self._enc is not None:
            self._enc.close()
            self._enc = None
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
        self._cap = (0, 0, 0)
        self._arena = 0

    def reserve_arena(self, nbytes):
        """Sets the emission arena's size for the next call (tests and measurements; encode() sizes it by itself)."""
        self._arena = max(0, int(nbytes))
        if self._enc is not None:
            self._enc.stream_reserve(self._arena)

    @staticmethod
    def _views(images, layout, floats=False):
        """-> [(tensor, width, height, comp, row_pitch, plane_pitch)], the checks of dtype, shape and strides.  floats: the pictures are
        float16, bfloat16 or float32, all of one dtype (encode_normalized); else uint8."""
        if layout not in ("CHW", "HWC"):
            raise ValueError("layout must be 'CHW' or 'HWC'")
        if isinstance(images, torch.Tensor):
            if images.dim() != 4:
                raise ValueError("a tensor of pictures is 4-D ([N, C, H, W] or [N, H, W, C]), got %d-D" % images.dim())
            images = list(images.unbind(0))
        else:
            images = list(images)
        out = []
        for i, t in enumerate(images):
            if not isinstance(t, torch.Tensor):
                raise ValueError("picture %d is not a tensor" % i)
            if floats:
                if t.dtype not in _FLOAT_DT:
                    raise ValueError("picture %d is %s; encode_normalized takes float16, bfloat16 or float32 pictures (uint8: encode)" % (i, t.dtype))
                if t.dtype != images[0].dtype:
                    raise ValueError("picture %d is %s, picture 0 is %s; one call takes one dtype" % (i, t.dtype, images[0].dtype))
            elif t.dtype != torch.uint8:
                raise ValueError("picture %d is %s; only uint8 pictures are encoded (float pictures: encode_normalized)" % (i, t.dtype))
            if t.dim() == 2:
                h, w = t.shape
                c, rp, pp = 1, t.stride(0), 0
                if w > 1 and t.stride(1) != 1:
                    raise ValueError("picture %d: a grey picture needs unit stride along W" % i)
                out.append((t, w, h, c, rp, pp))
                continue
            if t.dim() != 3:
                raise ValueError("picture %d is %d-D; pictures are 2-D (grey) or 3-D" % (i, t.dim()))
            if layout == "CHW":
                c, h, w = t.shape
                rp, pp = t.stride(1), t.stride(0)
                if w > 1 and t.stride(2) != 1:
                    raise ValueError("picture %d: CHW needs unit stride along W" % i)
            else:
                h, w, c = t.shape
                rp, pp = t.stride(0), 0
                if (w > 1 and t.stride(1) != c) or (c > 1 and t.stride(2) != 1):
                    raise ValueError("picture %d: HWC needs strides (.., C, 1) along W and C" % i)
            if not 1 <= c <= 4:
                raise ValueError("picture %d has %d channels; 1..4 are encoded" % (i, c))
            out.append((t, w, h, c, rp, pp))
        return out

    @staticmethod
    def _placed(views):
        """the checks of where the pictures are and how large, after those of what they are"""
        for i, (t, w, h, _, _, _) in enumerate(views):
            if t.device.type != "cuda":
                raise ValueError("picture %d is on %s, not on a GPU" % (i, t.device))
        for (_, w, h, _, _, _) in views:
            if not (1 <= w <= 65535 and 1 <= h <= 65535):
                raise ValueError("picture size %dx%d outside 1..65535" % (w, h))

    def _encoder_for(self, n, pix, du):
        need = (max(1, n), max(pix, 256), max(du, 256))
        if self._enc is None or any(a > b for a, b in zip(need, self._cap)):
            if self._enc is not None:
                self._enc.close()
                self._enc = None
            if self._ctx is None:
                self._ctx = Context(self.device.index)
            cap = tuple(max(a, b) for a, b in zip(need, self._cap))
            self._enc = Encoder(self._ctx, cap[0], cap[1], cap[2], stage_bytes=0)
            self._cap = cap
            if self._arena:
                self._enc.stream_reserve(self._arena)
        else:
            self._enc.reset()
        return self._enc

    def encode(self, images, *, quality=90, layout="CHW", flip_vertically=False, optimize=False, restart_rows=None, restart_mcus=None,
               progressive=False, subsampling=None, qtables=None, arithmetic="stb"):
        """quality: 1..100, or 0 for the default 90, as stbi_write_jpg takes it.  images: a 4-D uint8 tensor on the GPU ([N, C, H, W] for layout "CHW", [N, H, W, C] for "HWC") or a sequence of 3-D
        (2-D: grey) uint8 tensors, whose sizes may differ; C is 1..4 (stbi_write_jpg's comp).  Strided views are accepted (unit
        stride along W for CHW; strides C and 1 along W and C for HWC).  -> one bytes object per picture: what
        stbi_write_jpg_to_func(W, H, C, picture, quality) writes (under stbi_flip_vertically_on_write(1) with flip_vertically).
        optimize (a bool): every stream gets Huffman tables built on the GPU from its own symbol statistics -- the same coefficients in
        fewer bytes, what mjw_emit_optimized writes for the picture's data units, whatever the arena's size.
        restart_rows, restart_mcus: None, an int >= 0 or one of those per picture: restart markers after every so many MCU rows, or MCUs
        (an MCU is 16 x 16 pixels up to quality 90 and 8 x 8 above) -- what mjw_emit_restart writes (include/mij_host.h, RESTART
        INTERVALS).  None or 0 means none.  ValueError for both given for one picture and for an interval above 65535 MCUs.
        last_restarts[i] is the interval used, in MCUs.
        progressive (a bool): every stream is written as a progressive one -- what mjw_emit_progressive writes for the picture's data
        units (include/mij_host.h, PROGRESSIVE STREAMS), under per-scan optimal tables whatever optimize says.  ValueError together with
        a restart interval.
        subsampling: None, "444", "422", "440", "420" or "grey", or one of those per picture: the chroma subsampling of the stream, or a
        one-component grey stream (allowed for every C; it codes the luma of the picture) -- what mjh_write_jpg_sampled_to_memory writes
        (include/mij_host.h, SAMPLED ENCODING).  None leaves the choice to the quality as stbi_write_jpg makes it ("420" up to 90, "444"
        above), and naming that choice gives the same bytes.  The MCU, and with it a restart interval, is 8 * lh x 8 * lv pixels.
        last_subsampling[i] is the name each stream used.
        qtables: None or (luma, chroma), 64 ints 1..255 each in zigzag order (quality_tables' convention) in place of the tables of a
        quality; the sampling is then "420" unless subsampling says otherwise.  ValueError for an unknown name, for qtables together
        with a quality other than the default, and for tables that are not 64 values in 1..255.
        arithmetic: "stb" (the default) or "libjpeg", or one of those per picture.  "libjpeg" writes what PIL.Image.save(..., quality=,
        subsampling=), torchvision.io.encode_jpeg and cv2.imencode (libjpeg-turbo) write for the picture, byte for byte -- libjpeg's integer
        colour conversion, chroma filter, forward DCT and quantiser and its framing of the header (include/mij_host.h, LIBJPEG ENCODING);
        optimize, progressive and restart intervals are libjpeg's optimize=, progressive= and restart markers.  Its default subsampling is
        "420" whatever the quality, as libjpeg's is.  It takes C = 1 or 3 and no "440": ValueError otherwise, and for any other value.
        last_arithmetic[i] is what each picture got."""
        return self._encode(images, None, None, quality, layout, flip_vertically, optimize, False, restart_rows, restart_mcus, progressive,
                            subsampling, qtables, arithmetic)

    def encode_normalized(self, images, *, mean=None, std=None, quality=90, layout="CHW", flip_vertically=False, optimize=False,
                          restart_rows=None, restart_mcus=None, progressive=False, subsampling=None, qtables=None, arithmetic="stb"):
        """encode() for the tensors a model works on: images as for encode() -- the same shapes, stride rules and layouts -- but float16,
        bfloat16 or float32, one dtype per call.  The pictures are de-normalised on the GPU, inside the kernel that gathers them
        (mij_enc_add_device_float), by the contract of include/mij.h: for element x of channel c
            t = float32(x) * scale[c];  t = t + bias[c]   (float32, two roundings, no fused multiply-add)
            u = uint8(rint(min(max(t, 0), 255)))          (round half to even; NaN -> 0, -Inf -> 0, +Inf -> 255)
        with scale[c] = float32(255.0 * std[c]) and bias[c] = float32(255.0 * mean[c]).  -> one bytes object per picture: what encode()
        gives for the uint8 pictures of those u.
        mean / std: None, or one value per channel of the pictures (C values; the alpha of C = 2 or 4 takes a value that is never used).
        Both None: the pictures hold v / 255, tensor_tables' convention; with the mean / std a TensorDecoder.decode was given, its
        tensors come back as the bytes they were made from, for all three dtypes.  A tensor holding 0..255 values is std=[1/255]*C.
        ValueError, before any device is touched, for uint8 or any other non-float dtype, mixed dtypes, a wrong number of mean / std
        values, a std of 0, a value that is not finite, and everything encode() refuses.  restart_rows, restart_mcus, progressive,
        subsampling, qtables, arithmetic: as for encode()."""
        return self._encode(images, mean, std, quality, layout, flip_vertically, optimize, True, restart_rows, restart_mcus, progressive,
                            subsampling, qtables, arithmetic)

    def encode_ycbcr(self, pictures, *, subsampling="420", video_range=False, quality=90, qtables=None, flip_vertically=False, optimize=False,
                     restart_rows=None, restart_mcus=None, progressive=False, arithmetic="stb"):
        """JPEG streams from Y, Cb and Cr PLANES as a video decoder, a camera pipeline or a model holds them: no conversion to RGB and
        back, no second chroma filter -- the samples reach the stream as they lie (include/mij_host.h, PLANE ENCODING) -> one bytes
        object per picture: what mjh_write_jpg_planes_to_memory writes for those planes.
        pictures: a sequence whose entries are (Y, Cb, Cr), three 2-D uint8 tensors on the GPU with any strides (I420, 4:2:2, 4:4:4);
        (Y, CbCr) with CbCr of shape [ch, cw, 2] (NV12; for NV21 pass CbCr.flip(-1) or the two strided slices); or Y alone with
        subsampling="grey".  Or one [N, 3, H, W] tensor with subsampling="444".  Y is H x W, Cb and Cr are ceil(H / lv) x ceil(W / lh).
        subsampling: "444", "422", "440", "420" or "grey", one value or one per picture.  It is required knowledge, never guessed from
        the shapes.
        video_range: the planes hold studio-range samples (Y 16..235, chroma 16..240) and are expanded to JFIF's full range on the GPU,
        inside the kernel that gathers them (mjw_video_range's constants, mij_in_convert's arithmetic).  Only the range is converted: the
        colour matrix (BT.601 against BT.709) is not touched.
        quality, qtables, flip_vertically, optimize, restart_rows, restart_mcus, progressive: as for encode(); the MCU, and with it a
        restart interval, is 8 * lh x 8 * lv pixels.  last_subsampling and last_restarts report as they do for encode().
        arithmetic: as for encode(): "libjpeg" gives the planes libjpeg's forward DCT, quantiser, dummy blocks and header -- what Pillow
        writes for a "YCbCr"-mode or "L" picture of those samples; no "440".
        ValueError for plane shapes that do not match, a dtype other than uint8, a tensor that is not on a GPU, an unknown sampling and a
        restart interval together with progressive."""
        if not isinstance(optimize, bool):
            raise ValueError("optimize must be a bool, got %r" % (optimize,))
        if not isinstance(progressive, bool):
            raise ValueError("progressive must be a bool, got %r" % (progressive,))
        if not isinstance(video_range, bool):
            raise ValueError("video_range must be a bool, got %r" % (video_range,))
        if isinstance(quality, bool) or not isinstance(quality, int) or not 0 <= quality <= 100:
            raise ValueError("quality must be an int in 0..100 (0: stbi_write_jpg's default, 90), got %r" % (quality,))
        if qtables is not None:
            if quality not in (0, 90):
                raise ValueError("qtables replace the tables of a quality: give one of the two (quality=%r)" % (quality,))
            qtables = _qtable_pair(qtables)
            qtables = (list(qtables[0]), list(qtables[1]))
        if isinstance(pictures, torch.Tensor):
            if pictures.dim() != 4 or pictures.shape[1] != 3:
                raise ValueError("a tensor of pictures is [N, 3, H, W] (with subsampling='444'), got %s" % (tuple(pictures.shape),))
            pictures = [tuple(p.unbind(0)) for p in pictures.unbind(0)]
        else:
            pictures = list(pictures)
        if subsampling is None:
            plane_sampling(None)  # ValueError: the sampling is required
        samplings = _sampling_values(subsampling, len(pictures))
        for sm in samplings:
            plane_sampling(sm)
        ariths = _arith_values(arithmetic, len(pictures))
        for sm, ar in zip(samplings, ariths):
            if ar == "libjpeg" and sm == "440":
                raise ValueError("arithmetic 'libjpeg' does not serve subsampling '440'")
        pics = []
        for i, (pic, sm) in enumerate(zip(pictures, samplings)):
            for t in ([pic] if isinstance(pic, torch.Tensor) else list(pic)):
                if not isinstance(t, torch.Tensor):
                    raise ValueError("picture %d: a plane is not a tensor" % i)
                if t.dtype != torch.uint8:
                    raise ValueError("picture %d: a plane is %s; planes hold uint8 samples" % (i, t.dtype))
            try:
                planes = split_planes(pic, sm)
            except ValueError as e:
                raise ValueError("picture %d: %s" % (i, e)) from None
            pics.append(planes)
        rrows, rmcus = _restart_values(restart_rows, len(pics), "restart_rows"), _restart_values(restart_mcus, len(pics), "restart_mcus")
        if progressive and (any(rrows) or any(rmcus)):
            raise ValueError("restart intervals are not combined with progressive output")
        for i, planes in enumerate(pics):
            for t in planes:
                if t.device.type != "cuda":
                    raise ValueError("picture %d: a plane is on %s, not on a GPU" % (i, t.device))
                if t.device != planes[0].device:
                    raise ValueError("picture %d: its planes are on different devices" % i)
                if any(st == 0 and n > 1 for st, n in zip(t.stride(), t.shape)):
                    raise ValueError("picture %d: a plane has a stride of 0 (an expanded tensor); planes are addressed by pitches > 0" % i)
            h, w = planes[0].shape
            if not (1 <= w <= 65535 and 1 <= h <= 65535):
                raise ValueError("picture size %dx%d outside 1..65535" % (w, h))
        self.last_restarts = restarts = []
        self.last_subsampling = used = []
        self.last_arithmetic = list(ariths)
        if not pics:
            return []
        sizes, plans = [], {}
        for k, planes in enumerate(pics):
            h, w = planes[0].shape
            t = plans.get((w, h, samplings[k]))
            if t is None:
                t = plans[(w, h, samplings[k])] = planes_plan(w, h, samplings[k], quality, qtables)
            if t is None:
                raise ValueError("picture %dx%d is refused by the writer" % (w, h))
            p = t.plan
            used.append(sampling_name(t))
            units = p.mcu_x * p.mcu_y * p.du_per_mcu
            sizes.append((_align(units * 64, 256), _align(units * 128, 256), w * h))
            if rrows[k] and rmcus[k]:
                raise ValueError("picture %d: restart_rows and restart_mcus are two ways to say the same thing: give one" % k)
            ri = rrows[k] * p.mcu_x if rrows[k] else rmcus[k]
            if ri > 65535:
                raise ValueError("picture %d: a restart interval of %d MCUs does not fit the DRI segment (65535 at most)" % (k, ri))
            restarts.append(ri)
        if pics[0][0].device.index is not None and self._dev.index is not None and pics[0][0].device != self._dev:
            raise ValueError("the planes are on %s, the encoder on %s" % (pics[0][0].device, self._dev))
        _one_hip_runtime()
        torch.cuda.current_stream(self.device).synchronize()
        cv = video_range_convert() if video_range else None
        flip = bool(flip_vertically)
        out, host, i = [], 0, 0
        while i < len(pics):
            j, pix = i, 0
            while j < len(pics) and j - i < MAX_SLOTS and (j == i or pix + sizes[j][0] <= MAX_PIXEL_BYTES):
                pix += sizes[j][0]
                j += 1
            if not self._arena:  # a first guess, about 0.75 bytes per pixel; misses grow it
                self._arena = _align(sum(1024 + (px * 3) // 4 for (_, _, px) in sizes[i:j]), 1 << 20)
            enc = self._encoder_for(j - i, sum(s[0] for s in sizes[i:j]), sum(s[1] for s in sizes[i:j]))
            for k in range(i, j):
                planes = pics[k]
                h, w = planes[0].shape
                # a stride of an axis of one element addresses nothing: 0 rows down, 1 sample across
                triples = [(t.data_ptr(), t.stride(0) if t.shape[0] > 1 else 0, t.stride(1) if t.shape[1] > 1 else 1) for t in planes]
                slot = enc.add_device_planes(triples, w, h, samplings[k], quality, qtables, flip=flip, convert=cv)
                if ariths[k] == "libjpeg":
                    enc.set_arith(slot, MIJ_ARITH_LIBJPEG)
                if progressive:
                    enc.set_progressive(slot)
                elif optimize:
                    enc.set_optimize(slot)
                if restarts[k]:
                    enc.set_restart(slot, restarts[k])
            streams, hst = self._run(enc, [True] * (j - i), optimize, progressive, [a == "libjpeg" for a in ariths[i:j]])
            out.extend(streams)
            host += hst
            i = j
        self.last_host_emitted = host
        return out

    def _encode(self, images, mean, std, quality, layout, flip_vertically, optimize, floats, restart_rows=None, restart_mcus=None,
                progressive=False, subsampling=None, qtables=None, arithmetic="stb"):
        if not isinstance(optimize, bool):
            raise ValueError("optimize must be a bool, got %r" % (optimize,))
        if not isinstance(progressive, bool):
            raise ValueError("progressive must be a bool, got %r" % (progressive,))
        if isinstance(quality, bool) or not isinstance(quality, int) or not 0 <= quality <= 100:
            raise ValueError("quality must be an int in 0..100 (0: stbi_write_jpg's default, 90), got %r" % (quality,))
        if qtables is not None:
            if quality not in (0, 90):
                raise ValueError("qtables replace the tables of a quality: give one of the two (quality=%r)" % (quality,))
            qtables = _qtable_pair(qtables)
            qtables = (list(qtables[0]), list(qtables[1]))
        views = self._views(images, layout, floats)
        samplings = _sampling_values(subsampling, len(views))
        ariths = _arith_values(arithmetic, len(views))
        for k, (v, ar) in enumerate(zip(views, ariths)):
            if ar != "libjpeg":
                continue
            if samplings[k] is None:  # libjpeg's default, not the writer's quality-dependent choice
                samplings[k] = "420"
            if samplings[k] == "440":
                raise ValueError("picture %d: arithmetic 'libjpeg' does not serve subsampling '440'" % k)
            if v[3] not in (1, 3):
                raise ValueError("picture %d has %d channels; arithmetic 'libjpeg' takes 1 or 3" % (k, v[3]))
        convs = None
        if floats:  # one InConvert per channel count among the pictures; mean / std are checked even for an empty call
            mean, std = _numbers(mean, "mean"), _numbers(std, "std")
            given = mean if mean is not None else std
            by_c = {c: None for c in ([v[3] for v in views] or [len(given) if given is not None else 1])}
            for c in by_c:
                scale, bias = denorm_scale_bias(c, mean, std)
                by_c[c] = InConvert(_FLOAT_DT[views[0][0].dtype] if views else MIJ_DT_F32, scale, bias)
            convs = [by_c[v[3]] for v in views]
        rrows, rmcus = _restart_values(restart_rows, len(views), "restart_rows"), _restart_values(restart_mcus, len(views), "restart_mcus")
        if progressive and (any(rrows) or any(rmcus)):
            raise ValueError("restart intervals are not combined with progressive output")
        self._placed(views)
        self.last_restarts = restarts = []
        self.last_subsampling = used = []
        self.last_arithmetic = list(ariths)
        if not views:
            return []
        flip = bool(flip_vertically)
        lay = MIJ_LAYOUT_CHW if layout == "CHW" else MIJ_LAYOUT_HWC
        sizes = []
        for (_, w, h, c, _, _) in views:
            k = len(restarts)
            if samplings[k] is None and qtables is None:
                p = _plan(w, h, c, quality)
                pad_w = _align(w, 16 if p.subsample else 8)
                used.append("420" if p.subsample else "444")
            else:  # the sizes of the slot's own sampling: rows of whole MCU columns, mjw_tplan_du_count units
                t = sampled_plan(w, h, c, quality, samplings[k], qtables)
                if t is None:
                    raise ValueError("picture %dx%d with %d channels is refused by the writer" % (w, h, c))
                p = t.plan
                pad_w = _align(w, 8 * t.lh)
                used.append(sampling_name(t))
            sizes.append((_align(pad_w * h * 3, 256), _align(p.mcu_x * p.mcu_y * p.du_per_mcu * 128, 256), w * h))
            if rrows[k] and rmcus[k]:
                raise ValueError("picture %d: restart_rows and restart_mcus are two ways to say the same thing: give one" % k)
            ri = rrows[k] * p.mcu_x if rrows[k] else rmcus[k]
            if ri > 65535:
                raise ValueError("picture %d: a restart interval of %d MCUs does not fit the DRI segment (65535 at most)" % (k, ri))
            restarts.append(ri)
        _one_hip_runtime()
        torch.cuda.current_stream(self.device).synchronize()
        out, host, i = [], 0, 0
        while i < len(views):
            j, pix = i, 0
            while j < len(views) and j - i < MAX_SLOTS and (j == i or pix + sizes[j][0] <= MAX_PIXEL_BYTES):
                pix += sizes[j][0]
                j += 1
            streams, h = self._encode_chunk(views[i:j], sizes[i:j], quality, lay, flip, optimize, convs[i:j] if floats else None, restarts[i:j],
                                            progressive, samplings[i:j], qtables, ariths[i:j])
            out.extend(streams)
            host += h
            i = j
        self.last_host_emitted = host
        return out

    def _encode_chunk(self, views, sizes, quality, lay, flip, optimize, convs=None, restarts=None, progressive=False, samplings=None, qtables=None,
                      ariths=None):
        if not self._arena:  # a first guess, about 0.75 bytes per pixel; misses grow it
            self._arena = _align(sum(1024 + (px * 3) // 4 for (_, _, px) in sizes), 1 << 20)
        enc = self._encoder_for(len(views), sum(s[0] for s in sizes), sum(s[1] for s in sizes))
        for k, (t, w, h, c, rp, pp) in enumerate(views):
            it = InTensor(t.data_ptr(), lay, w, h, c, rp, pp)
            sm = samplings[k] if samplings else None
            slot = (enc.add_device(it, quality, flip, sm, qtables) if convs is None else
                    enc.add_device_float(it, convs[k], quality, flip, sm, qtables))
            if ariths and ariths[k] == "libjpeg":
                enc.set_arith(slot, MIJ_ARITH_LIBJPEG)
            if progressive:
                enc.set_progressive(slot)
            elif optimize:
                enc.set_optimize(slot)
            if restarts and restarts[k]:
                enc.set_restart(slot, restarts[k])
        own = [qtables is not None or bool(samplings and samplings[slot] is not None) for slot in range(len(views))]
        return self._run(enc, own, optimize, progressive, [a == "libjpeg" for a in ariths] if ariths else None)

    def _run(self, enc, own, optimize, progressive, lj=None):
        """upload, launch and bring back the streams of the encoder's slots; own[slot]: the slot has a plan of its own (mij_enc_tplan);
        lj[slot]: it is a libjpeg slot, whose host-finished stream takes libjpeg's framing"""
        enc.upload()
        enc.launch()
        enc.fetch_streams()
        streams, need, host, grow = [], 0, 0, 0
        for slot in range(len(own)):
            data, n = enc.stream(slot)
            if data is None:  # did not fit: its units are still on the device, the host Huffman stage finishes it
                if own[slot]:
                    data = emit_transcoded(enc.tplan(slot), enc.fetch(slot), optimize, restart_mcus=enc.slot_restart(slot), progressive=progressive)
                else:
                    data = emit_jpeg(enc.plan(slot), enc.fetch(slot), optimize, restart_mcus=enc.slot_restart(slot), progressive=progressive)
                if lj and lj[slot]:
                    data = libjpeg_reframe(data)
                host += 1
                if enc.slot_status(slot) == "host flush":  # a progressive slot with a forced flush: the device reported no length
                    n = len(data)
                else:
                    grow += 1
            need += n
            streams.append(data)
        if grow:
            self._arena = _align(need + need // 8, 1 << 20)
            enc.stream_reserve(self._arena)
        return streams, host
