"""JPEG streams straight from device tensors: the encoder's slots read caller-owned device memory (mij_enc_add_device, a gather
kernel in place of the host copy), and the Huffman stage runs on the GPU too (mij_enc_stream_reserve), so only finished streams
cross PCIe.  The counterpart of TensorDecoder.

Importing this module imports torch; ``import image_codecs_amd`` alone does not (TensorEncoder is loaded from here on first use)."""
import ctypes as C

import torch

from .binding import Context, Encoder, InTensor, WritePlan, emit_jpeg, lib, MIJ_LAYOUT_HWC, MIJ_LAYOUT_CHW
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


class TensorEncoder:
    """Encodes uint8 pictures that live on a GPU into JPEG byte streams, each exactly what stbi_write_jpg_to_func writes for that
    picture.  Owns a Context, an Encoder and its emission arena, grown as needed and reused across calls.  encode() is synchronous:
    it synchronises the device's current torch stream before the encoder reads the tensors and waits for the streams before it
    returns.  Slots whose streams do not fit the arena are finished on the host from their data units (last_host_emitted counts
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
    def _views(images, layout):
        """-> [(tensor, width, height, comp, row_pitch, plane_pitch)], every check that needs no device"""
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
            if t.dtype != torch.uint8:
                raise ValueError("picture %d is %s; only uint8 pictures are encoded" % (i, t.dtype))
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
        for i, (t, w, h, _, _, _) in enumerate(out):
            if t.device.type != "cuda":
                raise ValueError("picture %d is on %s, not on a GPU" % (i, t.device))
        for (_, w, h, _, _, _) in out:
            if not (1 <= w <= 65535 and 1 <= h <= 65535):
                raise ValueError("picture size %dx%d outside 1..65535" % (w, h))
        return out

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

    def encode(self, images, *, quality=90, layout="CHW", flip_vertically=False, optimize=False):
        """quality: 1..100, or 0 for the default 90, as stbi_write_jpg takes it.  images: a 4-D uint8 tensor on the GPU ([N, C, H, W] for layout "CHW", [N, H, W, C] for "HWC") or a sequence of 3-D
        (2-D: grey) uint8 tensors, whose sizes may differ; C is 1..4 (stbi_write_jpg's comp).  Strided views are accepted (unit
        stride along W for CHW; strides C and 1 along W and C for HWC).  -> one bytes object per picture: what
        stbi_write_jpg_to_func(W, H, C, picture, quality) writes (under stbi_flip_vertically_on_write(1) with flip_vertically).
        optimize (a bool): every stream gets Huffman tables built on the GPU from its own symbol statistics -- the same coefficients in
        fewer bytes, what mjw_emit_optimized writes for the picture's data units, whatever the arena's size."""
        if not isinstance(optimize, bool):
            raise ValueError("optimize must be a bool, got %r" % (optimize,))
        if isinstance(quality, bool) or not isinstance(quality, int) or not 0 <= quality <= 100:
            raise ValueError("quality must be an int in 0..100 (0: stbi_write_jpg's default, 90), got %r" % (quality,))
        views = self._views(images, layout)
        if not views:
            return []
        flip = bool(flip_vertically)
        lay = MIJ_LAYOUT_CHW if layout == "CHW" else MIJ_LAYOUT_HWC
        sizes = []
        for (_, w, h, c, _, _) in views:
            p = _plan(w, h, c, quality)
            pad_w = _align(w, 16 if p.subsample else 8)
            sizes.append((_align(pad_w * h * 3, 256), _align(p.mcu_x * p.mcu_y * p.du_per_mcu * 128, 256), w * h))
        _one_hip_runtime()
        torch.cuda.current_stream(self.device).synchronize()
        out, host, i = [], 0, 0
        while i < len(views):
            j, pix = i, 0
            while j < len(views) and j - i < MAX_SLOTS and (j == i or pix + sizes[j][0] <= MAX_PIXEL_BYTES):
                pix += sizes[j][0]
                j += 1
            streams, h = self._encode_chunk(views[i:j], sizes[i:j], quality, lay, flip, optimize)
            out.extend(streams)
            host += h
            i = j
        self.last_host_emitted = host
        return out

    def _encode_chunk(self, views, sizes, quality, lay, flip, optimize):
        if not self._arena:  # a first guess, about 0.75 bytes per pixel; misses grow it
            self._arena = _align(sum(1024 + (px * 3) // 4 for (_, _, px) in sizes), 1 << 20)
        enc = self._encoder_for(len(views), sum(s[0] for s in sizes), sum(s[1] for s in sizes))
        for (t, w, h, c, rp, pp) in views:
            slot = enc.add_device(InTensor(t.data_ptr(), lay, w, h, c, rp, pp), quality, flip)
            if optimize:
                enc.set_optimize(slot)
        enc.upload()
        enc.launch()
        enc.fetch_streams()
        streams, need, host = [], 0, 0
        for slot in range(len(views)):
            data, n = enc.stream(slot)
            need += n
            if data is None:  # did not fit: its units are still on the device, the host Huffman stage finishes it
                data = emit_jpeg(enc.plan(slot), enc.fetch(slot), optimize)
                host += 1
            streams.append(data)
        if host:
            self._arena = _align(need + need // 8, 1 << 20)
            enc.stream_reserve(self._arena)
        return streams, host
