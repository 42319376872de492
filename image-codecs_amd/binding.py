"""ctypes bindings over lib/libimagecodecs_mi355x.so (see package docstring).

Nothing here computes pixels: every function forwards to the C-ABI.  The library is loaded
lazily; a missing library raises (no fallback).  Decode calls need a gfx950 GPU and fail with
the library's own reason ("no gpu device") without one.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# eight hardware queues instead of HIP's default four, unless the user chose (see mij_hip_defaults in mij_runtime.hip): must be in
# the environment before the HIP runtime initialises, i.e. before anything in this process touches the GPU
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
LIB_PATH = os.environ.get("MIJ_LIB") or os.path.join(_HERE, "lib", "libimagecodecs_mi355x.so")  # MIJ_LIB: A/B builds

MIJ_FLAG_WIDE_IDCT = 1
COLOR_NAMES = {0: "grey", 1: "ycbcr", 2: "rgb", 3: "cmyk", 4: "ycck", 5: "ycbcra"}

ROWSLOT = (0, 4, 2, 5, 1, 6, 3, 7)  # include/mij.h mij_rowslot


class MijError(RuntimeError):
    pass


class CompDesc(C.Structure):
    _fields_ = [("h", C.c_int32), ("v", C.c_int32), ("tq", C.c_int32), ("x", C.c_int32), ("y", C.c_int32),
                ("bw", C.c_int32), ("bh", C.c_int32)]


class ImageDesc(C.Structure):
    """mij_image_desc (include/mij.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("n_out", C.c_int32),
                ("color", C.c_int32), ("flags", C.c_uint32), ("h_max", C.c_int32), ("v_max", C.c_int32),
                ("mcu_x", C.c_int32), ("mcu_y", C.c_int32), ("comp", CompDesc * 4),
                ("dequant", (C.c_uint16 * 64) * 4)]

    def plane_elems(self, c):
        nblk = self.comp[c].bw * self.comp[c].bh
        return ((nblk + 63) >> 6) << 12

    def coef_elems(self):
        return sum(self.plane_elems(c) for c in range(self.ncomp))


class GpuHuff(C.Structure):
    """mjg_huff (include/mij.h)."""
    _fields_ = [("fast", C.c_uint8 * 512), ("size", C.c_uint8 * 256), ("values", C.c_uint8 * 256), ("maxcode", C.c_uint32 * 18),
                ("delta", C.c_int32 * 18)]


class GpuScan(C.Structure):
    """mjg_scan (include/mij.h): what the GPU entropy stage needs to walk one baseline scan."""
    _fields_ = [("desc", ImageDesc), ("nblocks", C.c_uint32), ("blocks_per_mcu", C.c_uint32), ("blk_comp", C.c_uint8 * 12),
                ("blk_dx", C.c_uint8 * 12), ("blk_dy", C.c_uint8 * 12), ("dc_tab", C.c_uint8 * 4), ("ac_tab", C.c_uint8 * 4),
                ("huff", GpuHuff * 8), ("qz", (C.c_uint16 * 64) * 4), ("n_seg", C.c_uint32), ("restart_mcus", C.c_uint32),
                ("seg_table_off", C.c_uint32), ("reserved", C.c_uint32)]


_lib = None


def _library_stale():
    """True when the .so is missing or older than any source it is built from (csrc/, include/)."""
    if not os.path.exists(LIB_PATH):
        return True
    built = os.path.getmtime(LIB_PATH)
    for d in (os.path.join(_HERE, "csrc"), os.path.join(os.path.dirname(_HERE), "include")):
        for name in os.listdir(d):
            if name.endswith((".c", ".h", ".hip")) or name == "Makefile":
                if os.path.getmtime(os.path.join(d, name)) > built:
                    return True
    return False


def build_library(force=False):
    """Compile the HIP/C sources in csrc/ for gfx950 (hipcc cross-compiles without a GPU).  Rebuilds when the
    library is missing or any file under csrc/ or include/ is newer than it (make decides what to recompile)."""
    if os.environ.get("MIJ_LIB"):
        return LIB_PATH  # an A/B build chosen by the caller: never rebuilt behind its back
    if force or _library_stale():
        subprocess.run(["make", "-C", os.path.join(_HERE, "csrc")] + (["-B"] if force else []), check=True)
    return LIB_PATH


def lib():
    """The loaded shared library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MijError("%s is missing: run `python __graft_entry__.py` (build()) or `make -C image-codecs_amd/csrc`" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    p_int = C.POINTER(C.c_int)
    L.stbi_load_from_memory.restype = C.POINTER(C.c_ubyte)
    L.stbi_load_from_memory.argtypes = [C.c_char_p, C.c_int, p_int, p_int, p_int, C.c_int]
    L.stbi_load.restype = C.POINTER(C.c_ubyte)
    L.stbi_load.argtypes = [C.c_char_p, p_int, p_int, p_int, C.c_int]
    L.stbi_load_16_from_memory.restype = C.POINTER(C.c_ushort)
    L.stbi_load_16_from_memory.argtypes = [C.c_char_p, C.c_int, p_int, p_int, p_int, C.c_int]
    L.stbi_info_from_memory.restype = C.c_int
    L.stbi_info_from_memory.argtypes = [C.c_char_p, C.c_int, p_int, p_int, p_int]
    L.stbi_failure_reason.restype = C.c_char_p
    L.stbi_image_free.argtypes = [C.c_void_p]
    L.stbi_set_flip_vertically_on_load.argtypes = [C.c_int]
    L.stbi_write_jpg_to_func.restype = C.c_int
    L.mij_last_error.restype = C.c_char_p
    L.mij_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mij_ctx_destroy.argtypes = [C.c_void_p]
    L.mij_ctx_info.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, p_int, C.POINTER(C.c_size_t)]
    L.mij_batch_create.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p)]
    L.mij_batch_destroy.argtypes = [C.c_void_p]
    L.mij_batch_reset.argtypes = [C.c_void_p]
    L.mij_image_coef_bytes.restype = C.c_size_t
    L.mij_image_coef_bytes.argtypes = [C.POINTER(ImageDesc)]
    L.mij_image_out_bytes.restype = C.c_size_t
    L.mij_image_out_bytes.argtypes = [C.POINTER(ImageDesc)]
    L.mij_batch_add.argtypes = [C.c_void_p, C.POINTER(ImageDesc)]
    L.mij_batch_add_clone.argtypes = [C.c_void_p, C.c_int]
    L.mij_batch_coef.restype = C.c_void_p
    L.mij_batch_coef.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.mij_batch_set_flags.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.mij_batch_set_color.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.mij_batch_set_coef_format.argtypes = [C.c_void_p, C.c_int]
    L.mij_batch_slot_escapes.argtypes = [C.c_void_p, C.c_int]
    L.mij_batch_slot_coef_bytes.argtypes = [C.c_void_p, C.c_int]
    for name in ("mij_batch_upload", "mij_batch_launch", "mij_batch_submit", "mij_batch_wait", "mij_batch_timer_begin",
                 "mij_batch_timer_end", "mij_batch_image_count"):
        getattr(L, name).argtypes = [C.c_void_p]
    L.mij_batch_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.mij_batch_device_out.restype = C.c_void_p
    L.mij_batch_device_out.argtypes = [C.c_void_p, C.c_int]
    L.mij_batch_timer_elapsed_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mij_batch_hash_out.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    L.mij_batch_slot_path.argtypes = [C.c_void_p, C.c_int]
    L.mij_batch_force_generic.argtypes = [C.c_void_p, C.c_int]
    L.mjh_probe_memory.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(ImageDesc), C.POINTER(C.c_char_p)]
    L.mjh_decode_memory.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(ImageDesc), C.c_void_p, C.c_size_t,
                                    C.POINTER(C.c_char_p)]
    L.mjh_decode_batch.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                   C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
    _lib = L
    return L


def gpu_available():
    """True when the library sees at least one HIP device (no torch involved)."""
    try:
        return lib().mij_device_count() > 0
    except (MijError, OSError):
        return False


# ---------------------------------------------------------------- stb-style surface

def stbi_failure_reason():
    r = lib().stbi_failure_reason()
    return r.decode() if r else None


def stbi_set_flip_vertically_on_load(flag):
    lib().stbi_set_flip_vertically_on_load(int(flag))


def _take(ptr, shape, dtype):
    n = int(np.prod(shape))
    arr = np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype).reshape(shape).copy()
    lib().stbi_image_free(ptr)
    return arr


def stbi_load_from_memory(data, req_comp=0):
    """-> (pixels[h, w, n] uint8, w, h, comp_in_file) or None (see stbi_failure_reason())."""
    x, y, c = C.c_int(), C.c_int(), C.c_int()
    p = lib().stbi_load_from_memory(bytes(data), len(data), C.byref(x), C.byref(y), C.byref(c), int(req_comp))
    if not p:
        return None
    n = req_comp if req_comp else c.value
    return _take(p, (y.value, x.value, n), np.uint8), x.value, y.value, c.value


def stbi_load(filename, req_comp=0):
    x, y, c = C.c_int(), C.c_int(), C.c_int()
    p = lib().stbi_load(os.fsencode(filename), C.byref(x), C.byref(y), C.byref(c), int(req_comp))
    if not p:
        return None
    n = req_comp if req_comp else c.value
    return _take(p, (y.value, x.value, n), np.uint8), x.value, y.value, c.value


def stbi_load_16_from_memory(data, req_comp=0):
    x, y, c = C.c_int(), C.c_int(), C.c_int()
    p = lib().stbi_load_16_from_memory(bytes(data), len(data), C.byref(x), C.byref(y), C.byref(c), int(req_comp))
    if not p:
        return None
    n = req_comp if req_comp else c.value
    cnt = y.value * x.value * n
    arr = np.ctypeslib.as_array(p, shape=(cnt,)).astype(np.uint16).reshape(y.value, x.value, n).copy()
    lib().stbi_image_free(p)
    return arr, x.value, y.value, c.value


# ---- float loaders (convert.c:286-336) and their gamma / scale (convert.c:402-411)

# What stbi_ldr_to_hdr_gamma / _scale last set THROUGH THIS MODULE (the C globals are float): the defaults of ldr_to_hdr_lut() and
# Batch.set_out_f32(lut=None).  The library has no getter, so a value set by C code in the same process is not seen here; pass
# gamma / scale or a table explicitly in that case.  The stbi_loadf* loaders themselves always read the C globals.
_l2h = [np.float32(2.2), np.float32(1.0)]


def stbi_ldr_to_hdr_gamma(gamma):
    lib().stbi_ldr_to_hdr_gamma.argtypes = [C.c_float]
    lib().stbi_ldr_to_hdr_gamma(float(gamma))
    _l2h[0] = np.float32(gamma)


def stbi_ldr_to_hdr_scale(scale):
    lib().stbi_ldr_to_hdr_scale.argtypes = [C.c_float]
    lib().stbi_ldr_to_hdr_scale(float(scale))
    _l2h[1] = np.float32(scale)


def stbi_hdr_to_ldr_gamma(gamma):
    lib().stbi_hdr_to_ldr_gamma.argtypes = [C.c_float]
    lib().stbi_hdr_to_ldr_gamma(float(gamma))


def stbi_hdr_to_ldr_scale(scale):
    lib().stbi_hdr_to_ldr_scale.argtypes = [C.c_float]
    lib().stbi_hdr_to_ldr_scale(float(scale))


def ldr_to_hdr_lut(n_out, gamma=None, scale=None):
    """mjh_ldr_to_hdr_lut: float32 [n_out, 256], the tables of stbi__ldr_to_hdr (gamma / scale None: the values last set through
    this module's stbi_ldr_to_hdr_gamma / _scale -- not ones C code set directly, see _l2h)."""
    L = lib()
    L.mjh_ldr_to_hdr_lut.argtypes = [C.c_int, C.c_float, C.c_float, C.c_void_p]
    out = np.empty((int(n_out), 256), dtype=np.float32)
    L.mjh_ldr_to_hdr_lut(int(n_out), float(_l2h[0] if gamma is None else gamma), float(_l2h[1] if scale is None else scale),
                         out.ctypes.data_as(C.c_void_p))
    return out


def _loadf_result(p, x, y, c, req_comp):
    if not p:
        return None
    n = req_comp if req_comp else c.value
    return _take(p, (y.value, x.value, n), np.float32), x.value, y.value, c.value


def stbi_loadf_from_memory(data, req_comp=0):
    """-> (pixels[h, w, n] float32, w, h, comp_in_file) or None (see stbi_failure_reason())."""
    L = lib()
    L.stbi_loadf_from_memory.restype = C.POINTER(C.c_float)
    L.stbi_loadf_from_memory.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    x, y, c = C.c_int(), C.c_int(), C.c_int()
    p = L.stbi_loadf_from_memory(bytes(data), len(data), C.byref(x), C.byref(y), C.byref(c), int(req_comp))
    return _loadf_result(p, x, y, c, req_comp)


def stbi_loadf(filename, req_comp=0):
    L = lib()
    L.stbi_loadf.restype = C.POINTER(C.c_float)
    L.stbi_loadf.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    x, y, c = C.c_int(), C.c_int(), C.c_int()
    p = L.stbi_loadf(os.fsencode(filename), C.byref(x), C.byref(y), C.byref(c), int(req_comp))
    return _loadf_result(p, x, y, c, req_comp)


def stbi_info_from_memory(data):
    """-> (ok, w, h, comp)"""
    x, y, c = C.c_int(), C.c_int(), C.c_int()
    ok = lib().stbi_info_from_memory(bytes(data), len(data), C.byref(x), C.byref(y), C.byref(c))
    return ok, x.value, y.value, c.value


# ---- the callback / FILE* / file-name variants of the loaders (convert.c:188-211,261-266; image_api.c:74-131)

_READ_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_char), C.c_int)
_SKIP_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int)
_EOF_CB = C.CFUNCTYPE(C.c_int, C.c_void_p)


class IoCallbacks(C.Structure):
    """stbi_io_callbacks (include/image_api.h)."""
    _fields_ = [("read", _READ_CB), ("skip", _SKIP_CB), ("eof", _EOF_CB)]


class _CallbackSource:
    """A byte string behind stbi_io_callbacks whose read() hands out at most `chunk(k)` bytes on its k-th call
    (short reads are legal: the reference refills its 128-byte buffer with whatever comes, common.c:10-26)."""

    def __init__(self, data, chunk=None):
        self.data, self.pos, self.calls = bytes(data), 0, 0
        self.chunk = chunk

        def read(_u, buf, size):
            n = min(size, len(self.data) - self.pos)
            if self.chunk is not None:
                n = min(n, max(1, int(self.chunk(self.calls))))
            self.calls += 1
            C.memmove(buf, self.data[self.pos:self.pos + n], n)
            self.pos += n
            return n

        def skip(_u, n):
            self.pos = min(len(self.data), max(0, self.pos + n))

        def eof(_u):
            return 1 if self.pos >= len(self.data) else 0

        self.cb = IoCallbacks(_READ_CB(read), _SKIP_CB(skip), _EOF_CB(eof))


def stbi_load_from_callbacks(data, req_comp=0, chunk=None):
    """stbi_load_from_callbacks over an in-memory source with (optionally) short reads; result as stbi_load_from_memory."""
    L = lib()
    L.stbi_load_from_callbacks.restype = C.POINTER(C.c_ubyte)
    L.stbi_load_from_callbacks.argtypes = [C.POINTER(IoCallbacks), C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    src = _CallbackSource(data, chunk)
    x, y, c = C.c_int(), C.c_int(), C.c_int()
    p = L.stbi_load_from_callbacks(C.byref(src.cb), None, C.byref(x), C.byref(y), C.byref(c), int(req_comp))
    if not p:
        return None
    n = req_comp if req_comp else c.value
    return _take(p, (y.value, x.value, n), np.uint8), x.value, y.value, c.value


def stbi_loadf_from_callbacks(data, req_comp=0, chunk=None):
    """stbi_loadf_from_callbacks over an in-memory source; result as stbi_loadf_from_memory."""
    L = lib()
    L.stbi_loadf_from_callbacks.restype = C.POINTER(C.c_float)
    L.stbi_loadf_from_callbacks.argtypes = [C.POINTER(IoCallbacks), C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    src = _CallbackSource(data, chunk)
    x, y, c = C.c_int(), C.c_int(), C.c_int()
    p = L.stbi_loadf_from_callbacks(C.byref(src.cb), None, C.byref(x), C.byref(y), C.byref(c), int(req_comp))
    return _loadf_result(p, x, y, c, req_comp)


def stbi_info_from_callbacks(data, chunk=None):
    L = lib()
    L.stbi_info_from_callbacks.argtypes = [C.POINTER(IoCallbacks), C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    src = _CallbackSource(data, chunk)
    x, y, c = C.c_int(), C.c_int(), C.c_int()
    ok = L.stbi_info_from_callbacks(C.byref(src.cb), None, C.byref(x), C.byref(y), C.byref(c))
    return ok, x.value, y.value, c.value


_libc = None


def _c_stdio():
    global _libc
    if _libc is None:
        _libc = C.CDLL(None)
        _libc.fopen.restype = C.c_void_p
        _libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        _libc.fclose.argtypes = [C.c_void_p]
        _libc.ftell.restype = C.c_long
        _libc.ftell.argtypes = [C.c_void_p]
        _libc.fseek.argtypes = [C.c_void_p, C.c_long, C.c_int]
    return _libc


def stbi_load_from_file(filename, req_comp=0, offset=0):
    """fopen + fseek(offset) + stbi_load_from_file + ftell: -> (result as stbi_load_from_memory or None, position the
    FILE* was left at) -- the reference seeks back over what it buffered but did not consume (convert.c:208)."""
    L, libc = lib(), _c_stdio()
    L.stbi_load_from_file.restype = C.POINTER(C.c_ubyte)
    L.stbi_load_from_file.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    f = libc.fopen(os.fsencode(filename), b"rb")
    if not f:
        raise OSError("fopen failed: %s" % filename)
    try:
        libc.fseek(f, offset, 0)
        x, y, c = C.c_int(), C.c_int(), C.c_int()
        p = L.stbi_load_from_file(f, C.byref(x), C.byref(y), C.byref(c), int(req_comp))
        pos = libc.ftell(f)
        if not p:
            return None, pos
        n = req_comp if req_comp else c.value
        return (_take(p, (y.value, x.value, n), np.uint8), x.value, y.value, c.value), pos
    finally:
        libc.fclose(f)


def stbi_loadf_from_file(filename, req_comp=0, offset=0):
    """fopen + fseek(offset) + stbi_loadf_from_file + ftell: -> (result as stbi_loadf_from_memory or None, position the FILE*
    was left at -- wherever reading stopped: the float loader does not seek back, convert.c:331-336)."""
    L, libc = lib(), _c_stdio()
    L.stbi_loadf_from_file.restype = C.POINTER(C.c_float)
    L.stbi_loadf_from_file.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    f = libc.fopen(os.fsencode(filename), b"rb")
    if not f:
        raise OSError("fopen failed: %s" % filename)
    try:
        libc.fseek(f, offset, 0)
        x, y, c = C.c_int(), C.c_int(), C.c_int()
        p = L.stbi_loadf_from_file(f, C.byref(x), C.byref(y), C.byref(c), int(req_comp))
        return _loadf_result(p, x, y, c, req_comp), libc.ftell(f)
    finally:
        libc.fclose(f)


def stbi_info_from_file(filename, offset=0):
    """-> ((ok, w, h, comp), position afterwards): stbi_info_from_file restores the position (image_api.c:85-94)."""
    L, libc = lib(), _c_stdio()
    L.stbi_info_from_file.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    f = libc.fopen(os.fsencode(filename), b"rb")
    if not f:
        raise OSError("fopen failed: %s" % filename)
    try:
        libc.fseek(f, offset, 0)
        x, y, c = C.c_int(), C.c_int(), C.c_int()
        ok = L.stbi_info_from_file(f, C.byref(x), C.byref(y), C.byref(c))
        return (ok, x.value, y.value, c.value), libc.ftell(f)
    finally:
        libc.fclose(f)


def stbi_info(filename):
    L = lib()
    L.stbi_info.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    x, y, c = C.c_int(), C.c_int(), C.c_int()
    ok = L.stbi_info(os.fsencode(filename), C.byref(x), C.byref(y), C.byref(c))
    return ok, x.value, y.value, c.value


def stbi_write_jpg(filename, pixels, quality=90):
    """stbi_write_jpg(filename, ...) (codec/jpeg_write.c:376-388); returns its int result."""
    a = np.ascontiguousarray(pixels, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, comp = a.shape
    L = lib()
    L.stbi_write_jpg.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    return L.stbi_write_jpg(os.fsencode(filename), w, h, comp, a.ctypes.data_as(C.c_void_p), int(quality))


_WRITE_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int)


def stbi_write_jpg_to_memory(pixels, quality=90):
    """stbi_write_jpg_to_func into a bytes object.  pixels: uint8 [h, w, comp] (comp 1..4) or [h, w]."""
    a = np.ascontiguousarray(pixels, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, comp = a.shape
    chunks = []

    def sink(_ctx, data, size):
        chunks.append(C.string_at(data, size))

    cb = _WRITE_CB(sink)
    ok = lib().stbi_write_jpg_to_func(cb, None, C.c_int(w), C.c_int(h), C.c_int(comp), a.ctypes.data_as(C.c_void_p), C.c_int(int(quality)))
    if not ok:
        return None
    return b"".join(chunks)


# ---------------------------------------------------------------- host entropy stage

class HostDecoder:
    """mjh_probe_memory / mjh_decode_memory: marker parse + Huffman walk into tile-layout planes."""

    @staticmethod
    def probe(data, req_comp=0):
        d = ImageDesc()
        why = C.c_char_p()
        ok = lib().mjh_probe_memory(bytes(data), len(data), int(req_comp), C.byref(d), C.byref(why))
        if not ok:
            raise MijError(why.value.decode() if why.value else "decode failed")
        return d

    @staticmethod
    def plane_shapes(desc):
        """-> [(ph, pw), ...]: the shape of every stored component's plane (include/mij.h, PLANE OUTPUT): ceil(W * h_c / h_max) columns
        and ceil(H * v_c / v_max) rows, which are the descriptor's comp[c].x / .y.  Host only."""
        return [(int(desc.comp[c].y), int(desc.comp[c].x)) for c in range(desc.ncomp)]

    @staticmethod
    def decode(data, req_comp=0, out=None):
        """-> (desc, arena int16[coef_elems]) ; `out` may be a preallocated int16 array (e.g. a view of pinned staging)."""
        d = HostDecoder.probe(data, req_comp)
        n = d.coef_elems()
        arena = out if out is not None else np.empty(n, dtype=np.int16)
        if arena.size < n:
            raise MijError("arena too small")
        why = C.c_char_p()
        ok = lib().mjh_decode_memory(bytes(data), len(data), int(req_comp), C.byref(d), arena.ctypes.data_as(C.c_void_p),
                                     C.c_size_t(arena.size), C.byref(why))
        if not ok:
            raise MijError(why.value.decode() if why.value else "decode failed")
        return d, arena


def host_decode_staged(data, req_comp=0, want_compact=True):
    """mjh_decode_memory_fmt into a plain numpy region (no GPU): -> (desc, region bytes).  desc.flags says which format the walk wrote
    (MIJ_FLAG_STAGED_COMPACT = 4, MIJ_FLAG_HAS_ESCAPES = 8); compact regions follow mij_compact_offsets (compact_offsets below)."""
    d = HostDecoder.probe(data, req_comp)
    L = lib()
    L.mjh_decode_memory_fmt.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(ImageDesc), C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_char_p)]
    tiles = [((d.comp[c].bw * d.comp[c].bh) + 63) // 64 for c in range(d.ncomp)]
    region = np.full(sum(tiles) * (4096 + 128 + 4096), 0xA5, dtype=np.uint8)  # poisoned: what the walk does not clear it must not need
    why = C.c_char_p()
    d2 = ImageDesc()
    if not L.mjh_decode_memory_fmt(bytes(data), len(data), int(req_comp), C.byref(d2), region.ctypes.data_as(C.c_void_p), C.c_size_t(region.size), int(bool(want_compact)), C.byref(why)):
        raise MijError(why.value.decode() if why.value else "decode failed")
    return d2, region


def host_decode_rows(data, req_comp=0, want_compact=True):
    """mjh_decode_memory_rows (no GPU): host_decode_staged plus the walk's row-extent table -> (desc, region bytes, classes), classes one
    uint8 per block row, component after component (mij.h, "row-extent table": 0 DC only, 1 inside the 2x2, 2 inside the 4x4, 3 anything
    or unknown)."""
    d = HostDecoder.probe(data, req_comp)
    L = lib()
    L.mjh_decode_memory_rows.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(ImageDesc), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_char_p)]
    tiles = [((d.comp[c].bw * d.comp[c].bh) + 63) // 64 for c in range(d.ncomp)]
    region = np.full(sum(tiles) * (4096 + 128 + 4096), 0xA5, dtype=np.uint8)
    rows = np.full(sum(d.comp[c].bh for c in range(d.ncomp)), 0xA5, dtype=np.uint8)
    why = C.c_char_p()
    d2 = ImageDesc()
    if not L.mjh_decode_memory_rows(bytes(data), len(data), int(req_comp), C.byref(d2), region.ctypes.data_as(C.c_void_p), C.c_size_t(region.size),
                                    int(bool(want_compact)), rows.ctypes.data_as(C.c_void_p), C.c_size_t(rows.size), C.byref(why)):
        raise MijError(why.value.decode() if why.value else "decode failed")
    return d2, region, rows


def compact_offsets(desc):
    """mij_compact_offsets: per component (lo, dc, hi) byte offsets inside an image's region, and the main part's size"""
    tiles = [((desc.comp[c].bw * desc.comp[c].bh) + 63) // 64 for c in range(desc.ncomp)]
    main = sum(t * (4096 + 128) for t in tiles)
    out, m, e = [], 0, main
    for t in tiles:
        out.append((m, m + t * 4096, e))
        m += t * (4096 + 128)
        e += t * 4096
    return out, main


def expand_compact_region(desc, region):
    """compact planes (mij.h) -> the int16 tile-layout arena mjh_decode_memory would have written (the inverse of k_pack_c8)"""
    offs, _ = compact_offsets(desc)
    parts = []
    for c, (lo_o, dc_o, hi_o) in enumerate(offs):
        nt = ((desc.comp[c].bw * desc.comp[c].bh) + 63) // 64
        lo = region[lo_o:lo_o + nt * 4096].reshape(nt, 8, 64, 8)          # [tile, chunk, lane, slot]
        dc = region[dc_o:dc_o + nt * 128].view(np.int16).reshape(nt, 64)
        hi = region[hi_o:hi_o + nt * 4096].reshape(nt, 64, 8, 8)          # [tile, lane, chunk, slot] (64 bytes per block, position order)
        val = lo.view(np.int8).astype(np.int32)
        esc = (lo[:, 0, :, 0] & 1).astype(bool)                            # [tile, lane]
        h = np.where(esc[:, None, :, None], hi.view(np.int8).transpose(0, 2, 1, 3).astype(np.int32), 0)
        val = val + 256 * h
        val[:, 0, :, 0] = dc
        parts.append(val.astype(np.int16).reshape(-1))
    return np.concatenate(parts)


def detile_coefficients(desc, arena):
    """Tile layout -> list of per-component arrays [bh, bw, 8, 8] (natural row, col order), for tests."""
    out = []
    off = 0
    pos = np.empty((8, 8), dtype=np.int64)  # [row, col] -> P
    for r in range(8):
        for c in range(8):
            pos[r, c] = 8 * c + ROWSLOT[r]
    for ci in range(desc.ncomp):
        bw, bh = desc.comp[ci].bw, desc.comp[ci].bh
        n = desc.plane_elems(ci)
        plane = np.asarray(arena[off:off + n]).reshape(-1, 8, 64, 8)  # [tile, chunk, lane, j]
        off += n
        L = np.arange(bw * bh)
        blk = plane[L >> 6, :, L & 63, :]  # [nblk, chunk, j]
        flat = blk.reshape(-1, 64)  # index P = 8*chunk + j
        nat = flat[:, pos.reshape(-1)].reshape(bh, bw, 8, 8)
        out.append(nat)
    return out


# ---------------------------------------------------------------- GPU back end

def _check(rc, what):
    if rc < 0:
        raise MijError("%s: %s" % (what, lib().mij_last_error().decode()))
    return rc


MIJ_DT_U8, MIJ_DT_F16, MIJ_DT_BF16, MIJ_DT_F32 = 0, 1, 2, 3
MIJ_LAYOUT_HWC, MIJ_LAYOUT_CHW = 0, 1
MIJ_ARITH_STB, MIJ_ARITH_LIBJPEG = 0, 1  # mij_batch_set_arith
_DTYPES = {"u8": MIJ_DT_U8, "f16": MIJ_DT_F16, "bf16": MIJ_DT_BF16, "f32": MIJ_DT_F32}
_LAYOUTS = {"HWC": MIJ_LAYOUT_HWC, "CHW": MIJ_LAYOUT_CHW}


class OutTensor(C.Structure):
    """mij_out_tensor (include/mij.h)."""
    _fields_ = [("dst", C.c_void_p), ("dtype", C.c_int32), ("layout", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32),
                ("h", C.c_int32), ("flip_x", C.c_int32), ("flip_y", C.c_int32), ("row_pitch", C.c_int64), ("plane_pitch", C.c_int64)]


MIJ_FILTER_BOX, MIJ_FILTER_BILINEAR, MIJ_FILTER_HAMMING, MIJ_FILTER_BICUBIC, MIJ_FILTER_LANCZOS = 0, 1, 2, 3, 4
FILTERS = {"box": MIJ_FILTER_BOX, "bilinear": MIJ_FILTER_BILINEAR, "hamming": MIJ_FILTER_HAMMING, "bicubic": MIJ_FILTER_BICUBIC,
           "lanczos": MIJ_FILTER_LANCZOS}


class OutResize(C.Structure):
    """mij_out_resize (include/mij.h)."""
    _fields_ = [("out_w", C.c_int32), ("out_h", C.c_int32), ("filter", C.c_int32), ("reserved", C.c_int32)]


def resize_coeffs(n_in, n_out, filter="bilinear"):
    """mjh_resize_coeffs: one axis of the resized tensor output's contract -> (lo, n, k): int32 [n_out], int32 [n_out] and the
    fixed-point taps int32 [n_out, ksize] (k[o, t] for t >= n[o] is zero).  filter: a name of FILTERS or MIJ_FILTER_*."""
    f = FILTERS.get(filter, filter)
    L = lib()
    L.mjh_resize_coeffs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    ks = L.mjh_resize_coeffs(int(n_in), int(n_out), int(f), None, None, 0)
    if ks < 1:
        raise ValueError("mjh_resize_coeffs(%r, %r, %r) refused" % (n_in, n_out, filter))
    lo_n = np.zeros((int(n_out), 2), np.int32)
    k = np.zeros((int(n_out), ks), np.int32)
    got = L.mjh_resize_coeffs(int(n_in), int(n_out), int(f), lo_n.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), k.size)
    assert got == ks
    return lo_n[:, 0].copy(), lo_n[:, 1].copy(), k


def exif_orientation(data):
    """mjh_exif_orientation: the EXIF Orientation tag (1..8) of a JPEG file's bytes; 1 where there is none or it cannot be read."""
    b = bytes(data)
    L = lib()
    L.mjh_exif_orientation.argtypes = [C.c_char_p, C.c_int]
    return int(L.mjh_exif_orientation(b, len(b)))


def exif_set_orientation(data, value):
    """mjh_exif_set_orientation on a copy of a JPEG file's bytes -> (bytes, patched): the entry exif_orientation reads set to value
    (1..8); the same bytes and False where there is no such entry."""
    buf = C.create_string_buffer(bytes(data), len(data))
    L = lib()
    L.mjh_exif_set_orientation.argtypes = [C.c_char_p, C.c_int, C.c_int]
    ok = L.mjh_exif_set_orientation(buf, len(data), int(value))
    return buf.raw, bool(ok)


class Context:
    """mij_ctx: one per (process, device)."""

    def __init__(self, device=-1):
        self._h = C.c_void_p()
        _check(lib().mij_ctx_create(int(device), C.byref(self._h)), "mij_ctx_create")

    def info(self):
        arch = C.create_string_buffer(64)
        cu = C.c_int()
        mem = C.c_size_t()
        _check(lib().mij_ctx_info(self._h, arch, 64, C.byref(cu), C.byref(mem)), "mij_ctx_info")
        return arch.value.decode(), cu.value, mem.value

    def close(self):
        if self._h:
            lib().mij_ctx_destroy(self._h)
            self._h = C.c_void_p()


# the kernel families of a launch plan by index: the MK_* enumeration of mij_runtime.hip, in its order (mij_batch_slot_kernel)
KERNEL_KINDS = (
    "MK_PLANES", "MK_RESAMPLE", "MK_RS_FAST+RS_ROW1", "MK_RS_FAST+RS_V2", "MK_RS_FAST+RS_H2", "MK_RS_FAST+RS_HV2", "MK_RS_FAST+RS_GEN2",
    "MK_RS_FAST+RS_GEN4", "MK_420", "MK_422", "MK_444", "MK_GREY", "MK_440", "MK_420W", "MK_440W", "MK_420X", "MK_420S", "MK_420T", "MK_422W",
    "MK_422X", "MK_422S", "MK_422T", "MK_1X1C", "MK_420C", "MK_440C", "MK_SCALED+SC_Y", "MK_SCALED+SC_444", "MK_SCALED+SC_420",
    "MK_SCALED+SC_422", "MK_444R", "MK_GREYR", "MK_1X1CR", "MK_SCALEDR+SC_Y", "MK_SCALEDR+SC_444", "MK_SCALEDR+SC_420", "MK_SCALEDR+SC_422",
    "MK_PLANES_OUT", "MK_LJ_IDCT", "MK_LJ_COLOR+LJ_11", "MK_LJ_COLOR+LJ_21", "MK_LJ_COLOR+LJ_12", "MK_LJ_COLOR+LJ_22",
)


class OutPlane(C.Structure):
    """mij_out_plane (include/mij.h)."""
    _fields_ = [("dst", C.c_void_p), ("row_pitch", C.c_int64), ("x_pitch", C.c_int64)]


class OutPlanes(C.Structure):
    """mij_out_planes (include/mij.h)."""
    _fields_ = [("planes", OutPlane * 4), ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("reserved", C.c_int32 * 2)]


class Batch:
    """mij_batch: staging + device arenas + stream.  Thin, order-preserving wrapper."""

    def __init__(self, ctx, max_images, stage_bytes, coef_bytes, out_bytes):
        self.ctx = ctx
        self._h = C.c_void_p()
        _check(lib().mij_batch_create(ctx._h, int(max_images), C.c_size_t(stage_bytes), C.c_size_t(coef_bytes), C.c_size_t(out_bytes),
                                      C.byref(self._h)), "mij_batch_create")
        self.descs = []

    @staticmethod
    def coef_bytes(desc):
        return lib().mij_image_coef_bytes(C.byref(desc))

    @staticmethod
    def out_bytes(desc):
        return lib().mij_image_out_bytes(C.byref(desc))

    def add(self, desc):
        slot = _check(lib().mij_batch_add(self._h, C.byref(desc)), "mij_batch_add")
        self.descs.append(desc)
        return slot

    def _desc(self, slot):
        """Descriptor of a slot; slots added by the C-side front ends keep (data, req_comp) until first use, so that
        a pipelined caller does not pay a Python-side header probe per image."""
        d = self.descs[slot]
        if isinstance(d, tuple):
            d = self.descs[slot] = HostDecoder.probe(d[0], d[1])
        return d

    def add_clone(self, src):
        slot = _check(lib().mij_batch_add_clone(self._h, int(src)), "mij_batch_add_clone")
        self.descs.append(self.descs[src])
        return slot

    def stage_region(self, slot):
        """uint8 numpy view over the slot's whole pinned staging region (mij_batch_stage_region: room for either format)"""
        L = lib()
        L.mij_batch_stage_region.restype = C.c_void_p
        L.mij_batch_stage_region.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
        nb = C.c_size_t()
        p = L.mij_batch_stage_region(self._h, int(slot), C.byref(nb))
        if not p:
            raise MijError("mij_batch_stage_region: %s" % L.mij_last_error().decode())
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nb.value,))

    def set_dequant(self, slot, desc):
        """mij_batch_set_dequant: the slot (and its clones) takes comp[].tq and the quantisation tables of desc"""
        L = lib()
        L.mij_batch_set_dequant.argtypes = [C.c_void_p, C.c_int, C.POINTER(ImageDesc)]
        _check(L.mij_batch_set_dequant(self._h, int(slot), C.byref(desc)), "mij_batch_set_dequant")

    def set_flags(self, slot, flags):
        _check(lib().mij_batch_set_flags(self._h, int(slot), int(flags)), "mij_batch_set_flags")
        d = self._desc(slot)
        d.flags = int(flags)

    def staging(self, slot):
        """int16 numpy view over the slot's pinned planes (all components, back to back)."""
        d = self._desc(slot)
        p = lib().mij_batch_coef(self._h, int(slot), 0)
        if not p:
            raise MijError("mij_batch_coef: %s" % lib().mij_last_error().decode())
        n = d.coef_elems()
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int16)), shape=(n,))

    # ---- GPU entropy stage (experimental)
    def entropy_reserve(self, stream_bytes):
        L = lib()
        L.mij_batch_entropy_reserve.argtypes = [C.c_void_p, C.c_size_t]
        _check(L.mij_batch_entropy_reserve(self._h, C.c_size_t(stream_bytes)), "mij_batch_entropy_reserve")
        L.mij_batch_entropy_stage.restype = C.c_void_p
        L.mij_batch_entropy_stage.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        cap = C.c_size_t()
        self._es_base = L.mij_batch_entropy_stage(self._h, C.byref(cap))
        self._es_cap, self._es_used = cap.value, 0

    def add_jpeg_stream(self, data, req_comp=0):
        """mjh_extract_scan + mij_batch_add_stream: -> (status, slot).  status 1: the GPU walks this image;
        2: not a layout the GPU walk takes (nothing added); 0: rejected (reason in .last_reason)."""
        L = lib()
        L.mjh_extract_scan.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(GpuScan), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)]
        L.mij_batch_add_stream.argtypes = [C.c_void_p, C.POINTER(GpuScan), C.c_void_p, C.c_size_t]
        scan, n, why = GpuScan(), C.c_size_t(), C.c_char_p()
        dst = self._es_base + self._es_used
        st = L.mjh_extract_scan(bytes(data), len(data), int(req_comp), C.byref(scan), C.c_void_p(dst), C.c_size_t(self._es_cap - self._es_used), C.byref(n), C.byref(why))
        self.last_reason = why.value.decode() if why.value else None
        if st != 1:
            return st, -1
        slot = _check(L.mij_batch_add_stream(self._h, C.byref(scan), C.c_void_p(dst), n), "mij_batch_add_stream")
        self._es_used += (n.value + 32 + 255) // 256 * 256
        d = ImageDesc()
        C.memmove(C.byref(d), C.byref(scan.desc), C.sizeof(ImageDesc))
        self.descs.append(d)
        return 1, slot

    def entropy_run(self):
        """-> list of slots the host walk must redo."""
        L = lib()
        n = max(1, len(self.descs))
        fb = (C.c_int * n)()
        cnt = C.c_int()
        L.mij_batch_entropy_run.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
        _check(L.mij_batch_entropy_run(self._h, fb, n, C.byref(cnt)), "mij_batch_entropy_run")
        return list(fb[:cnt.value])

    def entropy_anomaly(self, slot):
        """tests: OR of the GPU walk's anomaly words of the slot's scans after entropy_run (0: kept; bits as listed in mij.h)."""
        L = lib()
        L.mij_batch_entropy_anomaly.argtypes = [C.c_void_p, C.c_int]
        return _check(L.mij_batch_entropy_anomaly(self._h, int(slot)), "mij_batch_entropy_anomaly")

    def work_items(self, slot):
        """tests: work items the last upload put on the slot's own family list (mij_batch_slot_work_items); 0 for a skipped slot."""
        L = lib()
        L.mij_batch_slot_work_items.argtypes = [C.c_void_p, C.c_int]
        return _check(L.mij_batch_slot_work_items(self._h, int(slot)), "mij_batch_slot_work_items")

    def slot_kernel(self, slot):
        """tests: what the last upload chose for the slot (mij_batch_slot_kernel): -> (family name from KERNEL_KINDS, variant bits, column
        segments per band); (None, 0, 1) for a skipped slot."""
        L = lib()
        L.mij_batch_slot_kernel.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        kind, var, nseg = C.c_int(), C.c_int(), C.c_int()
        _check(L.mij_batch_slot_kernel(self._h, int(slot), C.byref(kind), C.byref(var), C.byref(nseg)), "mij_batch_slot_kernel")
        return (KERNEL_KINDS[kind.value] if kind.value >= 0 else None), var.value, nseg.value

    def slot_pipelined(self, slot):
        """tests: True when the slot's launch runs the pipelined twin of its band kernel (mij_batch_slot_pipelined)"""
        L = lib()
        L.mij_batch_slot_pipelined.argtypes = [C.c_void_p, C.c_int]
        return bool(_check(L.mij_batch_slot_pipelined(self._h, int(slot)), "mij_batch_slot_pipelined"))

    def slot_marched(self, slot):
        """tests: True when the slot's launch runs the pipelined twin with the marching phase B, k_fused420m (mij_batch_slot_marched)"""
        L = lib()
        L.mij_batch_slot_marched.argtypes = [C.c_void_p, C.c_int]
        return bool(_check(L.mij_batch_slot_marched(self._h, int(slot)), "mij_batch_slot_marched"))

    def slot_row_classes(self, slot):
        """tests: the slot's row-extent table as the next upload sends it (mij_batch_slot_row_classes): one uint8 per block row, component
        after component; all 3 unless the library's own host walk staged the slot (a clone reads its source's)"""
        L = lib()
        L.mij_batch_slot_row_classes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        n = _check(L.mij_batch_slot_row_classes(self._h, int(slot), None, 0), "mij_batch_slot_row_classes")
        out = np.empty(n, dtype=np.uint8)
        _check(L.mij_batch_slot_row_classes(self._h, int(slot), out.ctypes.data_as(C.c_void_p), C.c_size_t(n)), "mij_batch_slot_row_classes")
        return out

    def slot_row_classes_device(self, slot):
        """tests: the packed table the band kernels read, copied back from the device (mij_batch_fetch_row_classes_packed): one uint8 per
        MCU row, two bits a component"""
        L = lib()
        L.mij_batch_fetch_row_classes_packed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        n = _check(L.mij_batch_fetch_row_classes_packed(self._h, int(slot), None, 0), "mij_batch_fetch_row_classes_packed")
        out = np.empty(n, dtype=np.uint8)
        _check(L.mij_batch_fetch_row_classes_packed(self._h, int(slot), out.ctypes.data_as(C.c_void_p), C.c_size_t(n)), "mij_batch_fetch_row_classes_packed")
        return out

    def slot_coef_bytes(self, slot):
        """1 when the slot's coefficients sit in HBM as compact planes (the default), 0 for the int16 tile layout."""
        return lib().mij_batch_slot_coef_bytes(self._h, int(slot))

    def set_coef_format(self, fmt):
        """'compact' (default) or 'int16': the format new coefficient planes of this batch get in HBM."""
        _check(lib().mij_batch_set_coef_format(self._h, {"int16": 0, "compact": 1}[fmt]), "mij_batch_set_coef_format")

    def slot_escapes(self, slot):
        """Blocks of the slot that hold a coefficient outside -128..127 (compact planes only)."""
        return _check(lib().mij_batch_slot_escapes(self._h, int(slot)), "mij_batch_slot_escapes")

    def slot_flags(self, slot):
        L = lib()
        L.mij_batch_slot_flags.restype = C.c_uint32
        L.mij_batch_slot_flags.argtypes = [C.c_void_p, C.c_int]
        return int(L.mij_batch_slot_flags(self._h, int(slot)))

    def pack_ms(self):
        """ms of k_pack_c8 in the last upload, or None when nothing was packed (host-staged compact planes, GPU-walk planes, int16 planes)"""
        L = lib()
        L.mij_batch_pack_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        ms = C.c_float()
        _check(L.mij_batch_pack_ms(self._h, C.byref(ms)), "mij_batch_pack_ms")
        return None if ms.value < 0 else ms.value

    def count_idct_classes(self, on=True):
        """Measurement: make the launches that follow count wavefronts per sparse-block class (clears the counters when switched on)."""
        L = lib()
        L.mij_batch_count_idct_classes.argtypes = [C.c_void_p, C.c_int]
        _check(L.mij_batch_count_idct_classes(self._h, int(bool(on))), "mij_batch_count_idct_classes")

    def idct_class_counts(self):
        """[DC only, inside 2x2, inside 4x4, full] wavefronts since count_idct_classes(True)"""
        L = lib()
        out = (C.c_uint64 * 4)()
        L.mij_batch_idct_class_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        _check(L.mij_batch_idct_class_counts(self._h, out), "mij_batch_idct_class_counts")
        return [int(v) for v in out]

    def entropy_rounds(self):
        L = lib()
        L.mij_batch_entropy_rounds.argtypes = [C.c_void_p]
        return L.mij_batch_entropy_rounds(self._h)

    def fallback_prepare(self, slot):
        _check(lib().mij_batch_fallback_prepare(self._h, int(slot)), "mij_batch_fallback_prepare")

    def fetch_coef(self, slot):
        d = self._desc(slot)
        out = np.empty(d.coef_elems(), dtype=np.int16)
        L = lib()
        L.mij_batch_fetch_coef.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        _check(L.mij_batch_fetch_coef(self._h, int(slot), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size)), "mij_batch_fetch_coef")
        return out

    def add_jpeg(self, data, req_comp=0, stage=None):
        """Host stage of one image straight into a new slot's pinned staging; returns the slot.  stage None: what the batch front ends do
        (mjh_decode_memory_rows: a baseline file is staged as COMPACT planes by the walk itself when the batch's format is compact, no
        pack pass on the device, and the slot takes the walk's row-extent table); "int16": int16 tile-layout staging whatever the file (mjh_decode_memory; compact batches then pack
        it on the device with k_pack_c8 -- the pipeline of rounds 1 and 2, kept for progressive files)."""
        d = HostDecoder.probe(data, req_comp)
        slot = self.add(d)
        L = lib()
        if stage == "int16":
            d2, _ = HostDecoder.decode(data, req_comp, out=self.staging(slot))
        else:
            L.mij_batch_stage_region.restype = C.c_void_p
            L.mij_batch_stage_region.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
            L.mij_batch_coef_format.argtypes = [C.c_void_p]
            rows_fn = hasattr(L, "mjh_decode_memory_rows")  # an A/B library from before the table (MIJ_LIB) stages without one
            if rows_fn:
                L.mjh_decode_memory_rows.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(ImageDesc), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                                     C.POINTER(C.c_char_p)]
                L.mij_batch_set_row_classes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
            else:
                L.mjh_decode_memory_fmt.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(ImageDesc), C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_char_p)]
            nb = C.c_size_t()
            region = L.mij_batch_stage_region(self._h, int(slot), C.byref(nb))
            if not region:
                raise MijError("mij_batch_stage_region: " + L.mij_last_error().decode())
            d2, why = ImageDesc(), C.c_char_p()
            # the walk's row-extent table goes in with the planes it describes, as in the batch front ends (mij.h, "row-extent table")
            rows = np.empty(sum(d.comp[c].bh for c in range(d.ncomp)), dtype=np.uint8)
            compact = int(L.mij_batch_coef_format(self._h) == 1)
            if not (L.mjh_decode_memory_rows(bytes(data), len(data), int(req_comp), C.byref(d2), region, nb, compact, rows.ctypes.data_as(C.c_void_p),
                                             C.c_size_t(rows.size), C.byref(why)) if rows_fn else
                    L.mjh_decode_memory_fmt(bytes(data), len(data), int(req_comp), C.byref(d2), region, nb, compact, C.byref(why))):
                raise MijError("mjh_decode_memory_fmt: %s" % (why.value.decode() if why.value else "failed"))  # either entry point: the text callers match
            if rows_fn:
                _check(L.mij_batch_set_row_classes(self._h, int(slot), rows.ctypes.data_as(C.c_void_p), C.c_size_t(rows.size)), "mij_batch_set_row_classes")
        if d2.flags:
            _check(L.mij_batch_set_flags(self._h, slot, d2.flags), "mij_batch_set_flags")
            d.flags = d2.flags
        if bytes(d2.dequant) != bytes(d.dequant) or any(d2.comp[c].tq != d.comp[c].tq for c in range(d.ncomp)):
            # DQT segments behind SOF: the walk ended with other tables than the frame header saw (mjh_final_dequant)
            self.set_dequant(slot, d2)
            C.memmove(C.byref(d.dequant), C.byref(d2.dequant), C.sizeof(d.dequant))
            for c in range(d.ncomp):
                d.comp[c].tq = d2.comp[c].tq
        if d2.color != d.color:  # a JFIF / Adobe marker behind SOF changed the colour branch (codec/jpeg.c:2244)
            _check(L.mij_batch_set_color(self._h, slot, d2.color), "mij_batch_set_color")
            d.color = d2.color
        return slot

    def decode_jpegs(self, datas, req_comp=0, threads=1, gpu_entropy=None):
        """gpu_entropy None: mjh_decode_batch, the default front end (Huffman walk on the GPU where it applies, host walk
        as the fallback; the batch gets its entropy arena on first use); False: mjh_decode_batch_host (every walk on the
        host threads); True: mjh_decode_batch_gpu (needs entropy_reserve).
        -> (n_ok, slots, reasons); slots[i] < 0 marks a rejected image (reasons[i] says why)."""
        n = len(datas)
        bufs = (C.c_char_p * n)(*[bytes(d) for d in datas])
        lens = (C.c_int * n)(*[len(d) for d in datas])
        slots = (C.c_int * n)()
        reasons = (C.c_char_p * n)()
        first = len(self.descs)
        fn = lib().mjh_decode_batch if gpu_entropy is None else (lib().mjh_decode_batch_gpu if gpu_entropy else lib().mjh_decode_batch_host)
        fn.argtypes = lib().mjh_decode_batch.argtypes
        rc = fn(self._h, bufs, lens, n, int(req_comp), int(threads), slots, reasons)
        if rc < 0:
            raise MijError("mjh_decode_batch: %s" % lib().mij_last_error().decode())
        out_slots = list(slots)
        # mirror the descriptors of the slots the C side added
        self._mirror_slots(datas, req_comp, out_slots, first)
        return rc, out_slots, [r.decode() if r else None for r in reasons]

    def _mirror_slots(self, datas, req_comp, out_slots, first):
        """Mirror the descriptors of the slots the C side added, BY SLOT INDEX: a stream rejected in slot 0 is reported as -1 - 0, which
        reads like a rejected header (no slot), so counting the reported slots would shift every later descriptor by one."""
        for i, sl in enumerate(out_slots):
            real = sl if sl >= 0 else (-1 - sl if sl < -1 else None)
            if real is not None and real >= first:
                while len(self.descs) <= real:
                    self.descs.append(None)
                self.descs[real] = (datas[i], req_comp)  # header probed when somebody asks (fetch, staging)

    def decode_jpegs_gpu_begin(self, datas, req_comp=0, threads=1):
        """mjh_decode_batch_gpu_begin: headers + unstuffing on the host threads, GPU walk queued; returns a job
        to pass to decode_jpegs_gpu_end (which waits for the walk and host-walks what it handed back)."""
        L = lib()
        n = len(datas)
        job = {"datas": datas, "req": req_comp, "first": len(self.descs),
               "bufs": (C.c_char_p * n)(*[bytes(d) for d in datas]), "lens": (C.c_int * n)(*[len(d) for d in datas]),
               "slots": (C.c_int * n)(), "reasons": (C.c_char_p * n)(), "rc": C.c_int()}
        L.mjh_decode_batch_gpu_begin.restype = C.c_void_p
        L.mjh_decode_batch_gpu_begin.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                                 C.POINTER(C.c_char_p), C.POINTER(C.c_int)]
        job["h"] = L.mjh_decode_batch_gpu_begin(self._h, job["bufs"], job["lens"], n, int(req_comp), int(threads), job["slots"], job["reasons"], C.byref(job["rc"]))
        if not job["h"]:
            raise MijError("mjh_decode_batch_gpu_begin: %d %s" % (job["rc"].value, lib().mij_last_error().decode()))
        return job

    def decode_jpegs_gpu_end(self, job):
        L = lib()
        L.mjh_decode_batch_gpu_end.argtypes = [C.c_void_p]
        rc = L.mjh_decode_batch_gpu_end(C.c_void_p(job["h"]))
        if rc < 0:
            raise MijError("mjh_decode_batch_gpu_end: %s" % lib().mij_last_error().decode())
        out_slots = list(job["slots"])
        self._mirror_slots(job["datas"], job["req"], out_slots, job["first"])
        return rc, out_slots, [r.decode() if r else None for r in job["reasons"]]

    def set_flags(self, slot, flags):
        _check(lib().mij_batch_set_flags(self._h, int(slot), int(flags)), "mij_batch_set_flags")

    def force_generic(self, on=True):
        """True / 1: two-pass path for every image; 2: and the run-time-general pass 2; False / 0: default choice."""
        _check(lib().mij_batch_force_generic(self._h, int(on)), "mij_batch_force_generic")

    def upload(self):
        _check(lib().mij_batch_upload(self._h), "mij_batch_upload")

    def launch(self):
        _check(lib().mij_batch_launch(self._h), "mij_batch_launch")

    def submit(self):
        _check(lib().mij_batch_submit(self._h), "mij_batch_submit")

    def wait(self):
        _check(lib().mij_batch_wait(self._h), "mij_batch_wait")

    def set_scale(self, slot, denom):
        """mij_batch_set_scale: decode the slot at 1/denom size (1, 2, 4 or 8) straight from its coefficients; before upload and
        before the slot's tensor request.  Everything that reads the slot's pixels then sees the out_size(slot) picture."""
        L = lib()
        L.mij_batch_set_scale.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _check(L.mij_batch_set_scale(self._h, int(slot), int(denom)), "mij_batch_set_scale")

    def set_arith(self, slot, arith):
        """mij_batch_set_arith: ARITH_LIBJPEG decodes the slot with libjpeg's arithmetic (ISLOW inverse DCT, fancy upsampling, jdcolor
        tables: Pillow's pixels byte for byte), ARITH_STB (the default) with the reference's; before upload."""
        L = lib()
        L.mij_batch_set_arith.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _check(L.mij_batch_set_arith(self._h, int(slot), int(arith)), "mij_batch_set_arith")

    def set_roi(self, slot, x0, y0, w, h):
        """mij_batch_set_roi: only the MCUs that the rectangle (x0, y0, w, h) of the slot's stored picture needs are decoded; the pixels
        inside it are what they are without a region, bytes outside roi_rect(slot) are not written.  w == h == 0 takes it back."""
        L = lib()
        L.mij_batch_set_roi.argtypes = [C.c_void_p] + [C.c_int] * 5
        _check(L.mij_batch_set_roi(self._h, int(slot), int(x0), int(y0), int(w), int(h)), "mij_batch_set_roi")

    def set_roi_auto(self, slot, on=True):
        """mij_batch_set_roi_auto: at upload the slot's region becomes the window its tensor request reads."""
        L = lib()
        L.mij_batch_set_roi_auto.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _check(L.mij_batch_set_roi_auto(self._h, int(slot), int(bool(on))), "mij_batch_set_roi_auto")

    def roi_rect(self, slot):
        """(x0, y0, w, h): the rectangle of the stored picture that the last upload decodes (mij_batch_slot_roi_rect); the whole picture
        for a slot without a region."""
        L = lib()
        L.mij_batch_slot_roi_rect.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int * 4)]
        r = (C.c_int * 4)()
        _check(L.mij_batch_slot_roi_rect(self._h, int(slot), C.byref(r)), "mij_batch_slot_roi_rect")
        return tuple(r)

    def out_size(self, slot):
        """(width, height) of the slot's stored picture: the file's, or the reduced one (mij_batch_slot_out_size)."""
        L = lib()
        L.mij_batch_slot_out_size.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        w, h = C.c_int(), C.c_int()
        _check(L.mij_batch_slot_out_size(self._h, int(slot), C.byref(w), C.byref(h)), "mij_batch_slot_out_size")
        return w.value, h.value

    def fetch(self, slot):
        d = self._desc(slot)
        w, h = self.out_size(slot)
        out = np.empty((h, w, d.n_out), dtype=np.uint8)
        _check(lib().mij_batch_fetch(self._h, int(slot), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size)), "mij_batch_fetch")
        return out

    # ---- float output (mij_batch_set_out_f32): k_out_f32 behind the decode kernels, into a float arena of its own
    @staticmethod
    def out_f32_bytes(desc):
        L = lib()
        L.mij_image_out_f32_bytes.restype = C.c_size_t
        L.mij_image_out_f32_bytes.argtypes = [C.POINTER(ImageDesc)]
        return L.mij_image_out_f32_bytes(C.byref(desc))

    def reserve_out_f32(self, nbytes):
        L = lib()
        L.mij_batch_out_f32_reserve.argtypes = [C.c_void_p, C.c_size_t]
        _check(L.mij_batch_out_f32_reserve(self._h, C.c_size_t(nbytes)), "mij_batch_out_f32_reserve")

    def set_out_f32(self, slot, lut=None):
        """Ask for the slot's pixels as float32 through lut [n_out, 256] (None: the stb table at the gamma and scale last set through
        this module, see ldr_to_hdr_lut)."""
        n = self._desc(slot).n_out
        t = ldr_to_hdr_lut(n) if lut is None else np.ascontiguousarray(lut, dtype=np.float32).reshape(n, 256)
        L = lib()
        L.mij_batch_set_out_f32.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _check(L.mij_batch_set_out_f32(self._h, int(slot), t.ctypes.data_as(C.c_void_p)), "mij_batch_set_out_f32")

    def fetch_f32(self, slot):
        d = self._desc(slot)
        out = np.empty((d.height, d.width, d.n_out), dtype=np.float32)
        L = lib()
        L.mij_batch_fetch_f32.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        _check(L.mij_batch_fetch_f32(self._h, int(slot), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size)), "mij_batch_fetch_f32")
        return out

    def device_out_f32(self, slot):
        """Device address of the slot's floats (None without float output)."""
        L = lib()
        L.mij_batch_device_out_f32.restype = C.c_void_p
        L.mij_batch_device_out_f32.argtypes = [C.c_void_p, C.c_int]
        return L.mij_batch_device_out_f32(self._h, int(slot))

    # ---- tensor output (mij_batch_set_out_tensor): k_out_tensor writes a crop window into device memory the caller owns
    def set_out_tensor(self, slot, dst, dtype, layout, x0, y0, w, h, row_pitch, plane_pitch=0, flip_x=False, flip_y=False, table=None,
                       orientation=1):
        """dst: raw device address; dtype MIJ_DT_* (or "u8", "f16", "bf16", "f32"), layout MIJ_LAYOUT_* (or "HWC", "CHW"); pitches in
        elements; table: n_out*256 elements of dtype as any buffer (e.g. numpy uint16 for f16 / bf16), None only for u8 (identity).
        orientation: 1..8 (EXIF); other than 1, the window is in the displayed picture (mij_batch_set_out_tensor_oriented)."""
        t = OutTensor(C.c_void_p(int(dst)), _DTYPES.get(dtype, dtype), _LAYOUTS.get(layout, layout), int(x0), int(y0), int(w), int(h),
                      int(bool(flip_x)), int(bool(flip_y)), int(row_pitch), int(plane_pitch))
        tb, tp = self._table(slot, t, table)
        L = lib()
        if orientation != 1:
            self._set_oriented(slot, t, None, orientation, tp)
            return
        L.mij_batch_set_out_tensor.argtypes = [C.c_void_p, C.c_int, C.POINTER(OutTensor), C.c_void_p]
        _check(L.mij_batch_set_out_tensor(self._h, int(slot), C.byref(t), tp), "mij_batch_set_out_tensor")

    def _table(self, slot, t, table):
        """-> (buffer, pointer): the caller keeps the buffer alive across the call, which copies the table."""
        if table is None:
            return None, None
        tb = np.ascontiguousarray(table)
        need = 256 * self._desc(slot).n_out * (1, 2, 2, 4)[t.dtype] if 0 <= t.dtype <= 3 else 0
        if tb.nbytes < need:
            raise ValueError("table has %d bytes, %d needed" % (tb.nbytes, need))
        return tb, tb.ctypes.data_as(C.c_void_p)

    def _set_oriented(self, slot, t, r, orientation, tp):
        L = lib()
        L.mij_batch_set_out_tensor_oriented.argtypes = [C.c_void_p, C.c_int, C.POINTER(OutTensor), C.POINTER(OutResize), C.c_int32, C.c_void_p]
        _check(L.mij_batch_set_out_tensor_oriented(self._h, int(slot), C.byref(t), None if r is None else C.byref(r), int(orientation), tp),
               "mij_batch_set_out_tensor_oriented")

    def set_out_tensor_resized(self, slot, dst, dtype, layout, x0, y0, w, h, out_w, out_h, row_pitch, plane_pitch=0, flip_x=False, flip_y=False,
                               table=None, filter="bilinear", orientation=1):
        """mij_batch_set_out_tensor_resized: the window (x0, y0, w, h) resized to out_w x out_h with filter (a name of FILTERS or
        MIJ_FILTER_*), then as set_out_tensor; pitches describe the out_w x out_h extent.  orientation: as set_out_tensor's."""
        t = OutTensor(C.c_void_p(int(dst)), _DTYPES.get(dtype, dtype), _LAYOUTS.get(layout, layout), int(x0), int(y0), int(w), int(h),
                      int(bool(flip_x)), int(bool(flip_y)), int(row_pitch), int(plane_pitch))
        r = OutResize(int(out_w), int(out_h), int(FILTERS.get(filter, filter)), 0)
        tb, tp = self._table(slot, t, table)
        if orientation != 1:
            self._set_oriented(slot, t, r, orientation, tp)
            return
        L = lib()
        L.mij_batch_set_out_tensor_resized.argtypes = [C.c_void_p, C.c_int, C.POINTER(OutTensor), C.POINTER(OutResize), C.c_void_p]
        _check(L.mij_batch_set_out_tensor_resized(self._h, int(slot), C.byref(t), C.byref(r), tp), "mij_batch_set_out_tensor_resized")

    # ---- plane output (mij_batch_set_out_planes): k_planes_out writes the stored components' samples into device memory the caller owns
    def set_out_planes(self, slot, planes, window=None, reserved=(0, 0)):
        """planes: up to four entries in the frame header's component order, each None (not wanted) or (raw device address, row pitch,
        x pitch) in bytes; window: None (the whole picture) or (x0, y0, w, h) in picture coordinates, on the grid of every wanted
        component.  No upsampling and no colour conversion: the samples as the file stores them (include/mij.h, PLANE OUTPUT)."""
        planes = list(planes)
        if len(planes) > 4:
            raise ValueError("at most four planes (got %d)" % len(planes))
        req = OutPlanes()
        for c, pl in enumerate(planes):
            if pl is not None:
                req.planes[c] = OutPlane(C.c_void_p(int(pl[0])), int(pl[1]), int(pl[2]))
        if window is not None:
            req.x0, req.y0, req.w, req.h = (int(v) for v in window)
        req.reserved[0], req.reserved[1] = int(reserved[0]), int(reserved[1])
        L = lib()
        L.mij_batch_set_out_planes.argtypes = [C.c_void_p, C.c_int, C.POINTER(OutPlanes)]
        _check(L.mij_batch_set_out_planes(self._h, int(slot), C.byref(req)), "mij_batch_set_out_planes")

    def plane_rect(self, slot, comp):
        """(x0, y0, w, h) of the window of component `comp` in its own samples, as the slot's plane request has it (mij_batch_slot_plane_rect)"""
        L = lib()
        L.mij_batch_slot_plane_rect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int * 4)]
        r = (C.c_int * 4)()
        _check(L.mij_batch_slot_plane_rect(self._h, int(slot), int(comp), C.byref(r)), "mij_batch_slot_plane_rect")
        return tuple(r)

    def fetch_all_async(self, dst_ptr, dst_bytes):
        """mij_batch_fetch_all_async into a (pinned) host buffer; wait() completes it."""
        L = lib()
        L.mij_batch_fetch_all_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        _check(L.mij_batch_fetch_all_async(self._h, C.c_void_p(dst_ptr), C.c_size_t(dst_bytes)), "mij_batch_fetch_all_async")

    def out_offset(self, slot):
        L = lib()
        L.mij_batch_out_offset.restype = C.c_size_t
        L.mij_batch_out_offset.argtypes = [C.c_void_p, C.c_int]
        return L.mij_batch_out_offset(self._h, int(slot))

    def out_total_bytes(self):
        L = lib()
        L.mij_batch_out_bytes.restype = C.c_size_t
        L.mij_batch_out_bytes.argtypes = [C.c_void_p]
        return L.mij_batch_out_bytes(self._h)

    def hash_out(self, slot):
        h = C.c_uint64()
        _check(lib().mij_batch_hash_out(self._h, int(slot), C.byref(h)), "mij_batch_hash_out")
        return h.value

    def diff_slots(self, pairs):
        """mij_batch_diff_slots: number of 16-byte words in which the device images of the slot pairs differ."""
        L = lib()
        n = len(pairs)
        L.mij_batch_diff_slots.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_uint64)]
        sa = (C.c_int * n)(*[int(p[0]) for p in pairs])
        sb = (C.c_int * n)(*[int(p[1]) for p in pairs])
        out = C.c_uint64()
        _check(L.mij_batch_diff_slots(self._h, sa, sb, n, C.byref(out)), "mij_batch_diff_slots")
        return out.value

    def slot_path(self, slot):
        return lib().mij_batch_slot_path(self._h, int(slot))

    def timer_begin(self):
        _check(lib().mij_batch_timer_begin(self._h), "mij_batch_timer_begin")

    def timer_end(self):
        _check(lib().mij_batch_timer_end(self._h), "mij_batch_timer_end")

    def timer_ms(self):
        ms = C.c_float()
        _check(lib().mij_batch_timer_elapsed_ms(self._h, C.byref(ms)), "mij_batch_timer_elapsed_ms")
        return ms.value

    def reset(self):
        self._es_used = 0
        _check(lib().mij_batch_reset(self._h), "mij_batch_reset")
        self.descs = []

    def close(self):
        if self._h:
            lib().mij_batch_destroy(self._h)
            self._h = C.c_void_p()


def decode_jpegs_multi(batches, datas, req_comp=0, threads=1):
    """mjh_decode_batch_multi: one logical batch sliced over several mij batches (one per device context), host
    walk on a shared pool, every batch submitted as soon as its slice is walked.  -> (n_ok, owner, slots, reasons)."""
    L = lib()
    n, nb = len(datas), len(batches)
    L.mjh_decode_batch_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
    hs = (C.c_void_p * nb)(*[b._h for b in batches])
    bufs = (C.c_char_p * n)(*[bytes(d) for d in datas])
    lens = (C.c_int * n)(*[len(d) for d in datas])
    owner, slots, reasons = (C.c_int * n)(), (C.c_int * n)(), (C.c_char_p * n)()
    rc = L.mjh_decode_batch_multi(hs, nb, bufs, lens, n, int(req_comp), int(threads), owner, slots, reasons)
    if rc < 0:
        raise MijError("mjh_decode_batch_multi: %d %s" % (rc, L.mij_last_error().decode()))
    for i in range(n):
        sl = slots[i]
        real = sl if sl >= 0 else (-1 - sl if sl < -1 else None)
        if real is not None:
            b = batches[owner[i]]
            while len(b.descs) <= real:
                b.descs.append(None)
            b.descs[real] = (datas[i], req_comp)
    return rc, list(owner), list(slots), [r.decode() if r else None for r in reasons]


class PinnedBuffer:
    """mij_host_alloc / mij_host_free: page-locked host memory as a numpy uint8 view."""

    def __init__(self, nbytes):
        L = lib()
        L.mij_host_alloc.restype = C.c_void_p
        L.mij_host_alloc.argtypes = [C.c_size_t]
        L.mij_host_free.argtypes = [C.c_void_p]
        self.ptr = L.mij_host_alloc(C.c_size_t(nbytes))
        if not self.ptr:
            raise MijError("mij_host_alloc(%d) failed" % nbytes)
        self.nbytes = nbytes
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_ubyte)), shape=(nbytes,))

    def close(self):
        if self.ptr:
            self.array = None
            lib().mij_host_free(C.c_void_p(self.ptr))
            self.ptr = None


# ---------------------------------------------------------------- encoder (config 5)

MJW_OPTIMIZE_HUFFMAN = 1


class WritePlan(C.Structure):
    """mjw_plan (include/mij_host.h)."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("comp", C.c_int), ("subsample", C.c_int), ("mcu_x", C.c_int),
                ("mcu_y", C.c_int), ("du_per_mcu", C.c_int), ("ytab", C.c_ubyte * 64), ("ctab", C.c_ubyte * 64),
                ("fdtbl_y", C.c_float * 64), ("fdtbl_c", C.c_float * 64)]

    def du_elems(self):
        return self.mcu_x * self.mcu_y * self.du_per_mcu * 64


def host_transform(pixels, quality=90, flip=False):
    """mjw_plan_init + mjw_transform_host: the writer's data units computed on the HOST
    (int16 [n_du, 64], zigzag order) -- the CPU twin of Encoder, used to check it."""
    a = np.ascontiguousarray(pixels, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, comp = a.shape
    L = lib()
    plan = WritePlan()
    L.mjw_plan_init.argtypes = [C.POINTER(WritePlan), C.c_int, C.c_int, C.c_int, C.c_int]
    L.mjw_transform_host.argtypes = [C.POINTER(WritePlan), C.c_void_p, C.c_int, C.c_void_p]
    if not L.mjw_plan_init(C.byref(plan), w, h, comp, int(quality)):
        return None, None
    du = np.empty(plan.du_elems(), dtype=np.int16)
    L.mjw_transform_host(C.byref(plan), a.ctypes.data_as(C.c_void_p), int(bool(flip)), du.ctypes.data_as(C.c_void_p))
    return plan, du.reshape(-1, 64)


def _restart_mcus(v):
    """a restart interval in MCUs as an int; None means 0 (none)"""
    if v is None:
        return 0
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError("a restart interval is None or an int (got %r)" % (v,))
    return int(v)


def _progressive_flag(v, restart=False):
    """the progressive request as a bool; ValueError for a non-bool and for the request together with a restart interval"""
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("progressive is a bool (got %r)" % (v,))
    if v and restart:
        raise ValueError("restart intervals are not combined with progressive output")
    return bool(v)


def emit_jpeg(plan, du, optimize=False, restart_mcus=None, progressive=False):
    """mjw_emit: headers + Huffman stage over given data units -> bytes.  optimize: mjw_emit_optimized, the same stream with Huffman
    tables built from the units' own symbol statistics.  restart_mcus: mjw_emit_restart, a restart interval of that many MCUs (None or
    0: none, the calls above); None for an interval outside 0..65535.  progressive: mjw_emit_progressive (a WritePlan) or
    mjw_temit_progressive (a TranscodePlan), the multi-scan stream (include/mij_host.h, PROGRESSIVE STREAMS); its tables are always the
    optimal ones, and it takes no restart interval (ValueError)."""
    L = lib()
    ri = _restart_mcus(restart_mcus)
    chunks = []
    cb = _WRITE_CB(lambda _c, data, size: chunks.append(C.string_at(data, size)))
    d = np.ascontiguousarray(du, dtype=np.int16)
    if _progressive_flag(progressive, ri):
        if d.size != plan.du_elems():
            raise ValueError("%d data-unit elements for a picture that has %d" % (d.size, plan.du_elems()))
        t = isinstance(plan, TranscodePlan)
        fn = L.mjw_temit_progressive if t else L.mjw_emit_progressive
        fn.argtypes = [C.POINTER(TranscodePlan if t else WritePlan), C.c_void_p, _WRITE_CB, C.c_void_p]
        return b"".join(chunks) if fn(C.byref(plan), d.ctypes.data_as(C.c_void_p), cb, None) else None
    if ri:
        L.mjw_emit_restart.argtypes = [C.POINTER(WritePlan), C.c_void_p, C.c_uint, C.c_int, _WRITE_CB, C.c_void_p]
        ok = L.mjw_emit_restart(C.byref(plan), d.ctypes.data_as(C.c_void_p), MJW_OPTIMIZE_HUFFMAN if optimize else 0, ri, cb, None)
        return b"".join(chunks) if ok else None
    fn = L.mjw_emit_optimized if optimize else L.mjw_emit
    fn.argtypes = [C.POINTER(WritePlan), C.c_void_p, _WRITE_CB, C.c_void_p]
    ok = fn(C.byref(plan), d.ctypes.data_as(C.c_void_p), cb, None)
    return b"".join(chunks) if ok else None


class TranscodePlan(C.Structure):
    """mjw_tplan (include/mij_host.h): the plan of a lossless transcode -- the source's geometry and tables."""
    _fields_ = [("plan", WritePlan), ("ncomp", C.c_int), ("lh", C.c_int), ("lv", C.c_int)]

    def du_elems(self):
        return self.plan.du_elems()


MJW_COPY_MARKERS = 2
_libc_free = None


def _take_malloced(ptr, n):
    global _libc_free
    if _libc_free is None:
        _libc_free = C.CDLL(None).free
        _libc_free.argtypes = [C.c_void_p]
    data = C.string_at(ptr, n)
    _libc_free(ptr)
    return data


def transcode_plan(desc):
    """mjw_tplan_from_desc -> (TranscodePlan, None), or (None, reason) for a source that is not transcodable."""
    L = lib()
    L.mjw_tplan_from_desc.argtypes = [C.POINTER(TranscodePlan), C.POINTER(ImageDesc), C.POINTER(C.c_char_p)]
    t, why = TranscodePlan(), C.c_char_p()
    if not L.mjw_tplan_from_desc(C.byref(t), C.byref(desc), C.byref(why)):
        return None, (why.value.decode() if why.value else "refused")
    return t, None


def transcode_header(tplan, tables=None):
    """mjw_theader, or mjw_theader_optimized with tables = (bits uint8 [4, 16], vals uint8 [4, 256]) -> bytes"""
    L = lib()
    out = C.create_string_buffer(1024)
    if tables is None:
        L.mjw_theader.restype = C.c_size_t
        L.mjw_theader.argtypes = [C.POINTER(TranscodePlan), C.c_char_p]
        n = L.mjw_theader(C.byref(tplan), out)
    else:
        bits, vals = (np.ascontiguousarray(a, np.uint8) for a in tables)
        assert bits.shape == (4, 16) and vals.shape == (4, 256)
        L.mjw_theader_optimized.restype = C.c_size_t
        L.mjw_theader_optimized.argtypes = [C.POINTER(TranscodePlan), C.c_void_p, C.c_void_p, C.c_char_p]
        n = L.mjw_theader_optimized(C.byref(tplan), bits.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), out)
    return out.raw[:n]


def units_from_region(desc, region, compact):
    """mjw_units_from_region: an image's coefficient region (host_decode_staged) -> int16 [n_du, 64], None when not transcodable."""
    t, _ = transcode_plan(desc)
    if t is None:
        return None
    L = lib()
    L.mjw_units_from_region.argtypes = [C.POINTER(ImageDesc), C.c_void_p, C.c_int, C.c_void_p]
    r = np.ascontiguousarray(region, np.uint8)
    du = np.empty(t.du_elems(), np.int16)
    if not L.mjw_units_from_region(C.byref(desc), r.ctypes.data_as(C.c_void_p), int(bool(compact)), du.ctypes.data_as(C.c_void_p)):
        return None
    return du.reshape(-1, 64)


def units_codable(tplan, du, restart_mcus=None):
    """mjw_tunits_codable -> (True, None) or (False, reason); restart_mcus: mjw_tunits_codable_restart, the DC differences taken against
    predictors that restart every that many MCUs"""
    L = lib()
    ri = _restart_mcus(restart_mcus)
    d = np.ascontiguousarray(du, np.int16)
    if d.size != tplan.du_elems():
        raise ValueError("%d data-unit elements for a picture that has %d" % (d.size, tplan.du_elems()))
    why = C.c_char_p()
    if ri:
        L.mjw_tunits_codable_restart.argtypes = [C.POINTER(TranscodePlan), C.c_void_p, C.c_int, C.POINTER(C.c_char_p)]
        ok = L.mjw_tunits_codable_restart(C.byref(tplan), d.ctypes.data_as(C.c_void_p), ri, C.byref(why))
    else:
        L.mjw_tunits_codable.argtypes = [C.POINTER(TranscodePlan), C.c_void_p, C.POINTER(C.c_char_p)]
        ok = L.mjw_tunits_codable(C.byref(tplan), d.ctypes.data_as(C.c_void_p), C.byref(why))
    return bool(ok), (None if ok else why.value.decode())


class ProgressiveStats(C.Structure):
    """mjw_progressive_stats (include/mij_host.h)."""
    _fields_ = [("forced_run_flushes", C.c_uint32), ("forced_bit_flushes", C.c_uint32), ("longest_run", C.c_uint32), ("most_pending_bits", C.c_uint32)]


def progressive_stats(tplan, du):
    """mjw_tprogressive_stats: what the progressive writer meets in these units -> ProgressiveStats, None when refused"""
    L = lib()
    d = np.ascontiguousarray(du, np.int16)
    if d.size != tplan.du_elems():
        raise ValueError("%d data-unit elements for a picture that has %d" % (d.size, tplan.du_elems()))
    L.mjw_tprogressive_stats.argtypes = [C.POINTER(TranscodePlan), C.c_void_p, C.POINTER(ProgressiveStats)]
    st = ProgressiveStats()
    return st if L.mjw_tprogressive_stats(C.byref(tplan), d.ctypes.data_as(C.c_void_p), C.byref(st)) else None


def emit_transcoded(tplan, du, optimize=False, restart_mcus=None, progressive=False):
    """mjw_temit / mjw_temit_optimized over given units -> bytes, None when the units are not codable.  restart_mcus: mjw_temit_restart.
    progressive: mjw_temit_progressive (no restart interval with it: ValueError)."""
    L = lib()
    ri = _restart_mcus(restart_mcus)
    if _progressive_flag(progressive, ri):
        return emit_jpeg(tplan, du, progressive=True)
    d = np.ascontiguousarray(du, np.int16)
    if d.size != tplan.du_elems():
        raise ValueError("%d data-unit elements for a picture that has %d" % (d.size, tplan.du_elems()))
    chunks = []
    cb = _WRITE_CB(lambda _c, data, size: chunks.append(C.string_at(data, size)))
    if ri:
        L.mjw_temit_restart.argtypes = [C.POINTER(TranscodePlan), C.c_void_p, C.c_uint, C.c_int, _WRITE_CB, C.c_void_p]
        ok = L.mjw_temit_restart(C.byref(tplan), d.ctypes.data_as(C.c_void_p), MJW_OPTIMIZE_HUFFMAN if optimize else 0, ri, cb, None)
        return b"".join(chunks) if ok else None
    fn = L.mjw_temit_optimized if optimize else L.mjw_temit
    fn.argtypes = [C.POINTER(TranscodePlan), C.c_void_p, _WRITE_CB, C.c_void_p]
    return b"".join(chunks) if fn(C.byref(tplan), d.ctypes.data_as(C.c_void_p), cb, None) else None


def restart_interval(tplan, restart_rows=None, restart_mcus=None):
    """mjw_restart_interval: the interval in MCUs of a plan from one given in MCU rows or in MCUs -> (Ri, None), or (None, reason) for both
    given, a negative value or a result above 65535"""
    L = lib()
    L.mjw_restart_interval.argtypes = [C.POINTER(TranscodePlan), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
    ri, why = C.c_int(), C.c_char_p()
    rows, mcus = (min(max(_restart_mcus(v), -1), 1 << 30) for v in (restart_rows, restart_mcus))
    if not L.mjw_restart_interval(C.byref(tplan), rows, mcus, C.byref(ri), C.byref(why)):
        return None, (why.value.decode() if why.value else "refused")
    return ri.value, None


def restart_histogram(plan, du, restart_mcus):
    """mjw_histogram_restart (a WritePlan) or mjw_thistogram_restart (a TranscodePlan) -> uint32 [4, 256], None when refused"""
    L = lib()
    t = isinstance(plan, TranscodePlan)
    fn = L.mjw_thistogram_restart if t else L.mjw_histogram_restart
    fn.argtypes = [C.POINTER(TranscodePlan if t else WritePlan), C.c_void_p, C.c_int, C.c_void_p]
    d = np.ascontiguousarray(du, np.int16)
    if d.size != plan.du_elems():
        raise ValueError("%d data-unit elements for a picture that has %d" % (d.size, plan.du_elems()))
    freq = np.zeros((4, 256), np.uint32)
    if not fn(C.byref(plan), d.ctypes.data_as(C.c_void_p), _restart_mcus(restart_mcus), freq.ctypes.data_as(C.c_void_p)):
        return None
    return freq


def copy_markers(src, stream):
    """mjw_copy_markers: `stream` with the source's APPn and COM segments behind SOI -> (bytes, None) or (None, reason)"""
    L = lib()
    L.mjw_copy_markers.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)]
    src, stream = bytes(src), bytes(stream)
    out, n, why = C.c_void_p(), C.c_size_t(), C.c_char_p()
    if not L.mjw_copy_markers(src, len(src), stream, len(stream), C.byref(out), C.byref(n), C.byref(why)):
        return None, (why.value.decode() if why.value else "refused")
    return _take_malloced(out, n.value), None


def _qtable_pair(tables):
    """(luma, chroma), 64 ints 1..255 each in zigzag order -> two 64-byte strings; ValueError for anything else"""
    what = "qtables must be a (luma, chroma) pair of 64 ints 1..255 each, in zigzag order"
    try:
        pair = [list(t) for t in tables]
    except TypeError:
        raise ValueError(what) from None
    if len(pair) != 2 or any(len(t) != 64 for t in pair):
        raise ValueError(what)
    for t in pair:
        for v in t:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= v <= 255:
                raise ValueError(what + " (got %r)" % (v,))
    return bytes(int(v) for v in pair[0]), bytes(int(v) for v in pair[1])


def quality_tables(quality):
    """mjw_quality_tables: the (luma, chroma) tables the writer uses at quality 1..100, uint8 [64] each in zigzag order; None outside"""
    L = lib()
    L.mjw_quality_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    luma, chroma = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    if not L.mjw_quality_tables(int(quality), luma.ctypes.data_as(C.c_void_p), chroma.ctypes.data_as(C.c_void_p)):
        return None
    return luma, chroma


SAMPLINGS = {"444": (3, 1, 1), "422": (3, 2, 1), "440": (3, 1, 2), "420": (3, 2, 2), "grey": (1, 1, 1)}


def sampling_factors(sampling):
    """a sampling name -> (ncomp, lh, lv) (include/mij_host.h, SAMPLED ENCODING); None -> (0, 0, 0), the writer's own choice;
    ValueError for any other value"""
    if sampling is None:
        return (0, 0, 0)
    if not isinstance(sampling, str) or sampling not in SAMPLINGS:
        raise ValueError("sampling must be None or one of %s (got %r)" % (", ".join(repr(k) for k in SAMPLINGS), sampling))
    return SAMPLINGS[sampling]


def sampling_name(tplan):
    """the name of a TranscodePlan's sampling"""
    key = (1, 1, 1) if tplan.ncomp == 1 else (tplan.ncomp, tplan.lh, tplan.lv)
    return {v: k for k, v in SAMPLINGS.items()}[key]


class EncOpts(C.Structure):
    """mij_enc_opts (include/mij.h)."""
    _fields_ = [("ncomp", C.c_int), ("lh", C.c_int), ("lv", C.c_int), ("luma", C.c_char_p), ("chroma", C.c_char_p)]


def enc_opts(sampling=None, qtables=None):
    """-> an EncOpts, or None when neither is given (the plain calls).  ValueError for an unknown name or bad tables."""
    ncomp, lh, lv = sampling_factors(sampling)
    luma, chroma = (None, None) if qtables is None else _qtable_pair(qtables)
    if not ncomp and luma is None:
        return None
    return EncOpts(ncomp, lh, lv, luma, chroma)


def sampled_plan(width, height, comp, quality=90, sampling=None, qtables=None):
    """mjw_splan_init -> TranscodePlan; None where the writer refuses the picture"""
    L = lib()
    o = enc_opts(sampling, qtables) or EncOpts()
    t = TranscodePlan()
    L.mjw_splan_init.argtypes = [C.POINTER(TranscodePlan), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p]
    if not L.mjw_splan_init(C.byref(t), int(width), int(height), int(comp), int(quality), o.ncomp, o.lh, o.lv, o.luma, o.chroma):
        return None
    return t


def _hwc_u8(pixels):
    a = np.ascontiguousarray(pixels, dtype=np.uint8)
    return a[:, :, None] if a.ndim == 2 else a


def host_transform_sampled(pixels, quality=90, sampling=None, qtables=None, flip=False):
    """mjw_splan_init + mjw_stransform_host: the units of a sampled slot computed on the HOST -> (TranscodePlan, int16 [n_du, 64]); the
    CPU twin of Encoder.add(..., sampling=, qtables=)."""
    a = _hwc_u8(pixels)
    h, w, comp = a.shape
    t = sampled_plan(w, h, comp, quality, sampling, qtables)
    if t is None:
        return None, None
    L = lib()
    L.mjw_stransform_host.argtypes = [C.POINTER(TranscodePlan), C.c_void_p, C.c_int, C.c_void_p]
    du = np.empty(t.du_elems(), dtype=np.int16)
    L.mjw_stransform_host(C.byref(t), a.ctypes.data_as(C.c_void_p), int(bool(flip)), du.ctypes.data_as(C.c_void_p))
    return t, du.reshape(-1, 64)


def write_jpg_sampled_to_memory(pixels, quality=90, sampling=None, qtables=None, flip=False, optimize=False, restart_rows=None, restart_mcus=None,
                                progressive=False):
    """mjh_write_jpg_sampled_to_memory: the host writer with a sampling ("444", "422", "440", "420", "grey"; None: the writer's own) and
    / or (luma, chroma) tables -> bytes, None where it refuses.  restart_rows counts MCU rows of the sampling's own MCU size."""
    a = _hwc_u8(pixels)
    h, w, comp = a.shape
    o = enc_opts(sampling, qtables) or EncOpts()
    rows, mcus = _restart_mcus(restart_rows), _restart_mcus(restart_mcus)
    if rows and mcus:
        raise ValueError("restart_rows and restart_mcus are two ways to say the same thing: give one")
    if rows:
        t = sampled_plan(w, h, comp, quality, sampling, qtables)
        if t is None:
            return None
        mcus = rows * t.plan.mcu_x
    prog = _progressive_flag(progressive, mcus)
    L = lib()
    L.mjh_write_jpg_sampled_to_memory.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                                  C.c_int, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    out, n = C.c_void_p(), C.c_size_t()
    if not L.mjh_write_jpg_sampled_to_memory(a.ctypes.data_as(C.c_void_p), w, h, comp, int(quality), o.ncomp, o.lh, o.lv, o.luma, o.chroma,
                                             int(bool(flip)), MJW_OPTIMIZE_HUFFMAN if optimize else 0, mcus, int(prog), C.byref(out), C.byref(n)):
        return None
    return _take_malloced(out, n.value)


ARITHMETICS = {"stb": MIJ_ARITH_STB, "libjpeg": MIJ_ARITH_LIBJPEG}  # mij_enc_set_arith
ENC_GROUPS = 22  # MIJ_ENC_GROUPS


def libjpeg_plan(width, height, comp, quality=90, sampling=None, qtables=None):
    """mjw_lj_plan_init -> TranscodePlan (include/mij_host.h, LIBJPEG ENCODING); None for what it refuses ("440", comp 2 and 4).  No
    sampling: "420"."""
    L = lib()
    o = enc_opts(sampling, qtables) or EncOpts()
    t = TranscodePlan()
    L.mjw_lj_plan_init.argtypes = [C.POINTER(TranscodePlan), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p]
    if not L.mjw_lj_plan_init(C.byref(t), int(width), int(height), int(comp), int(quality), o.ncomp, o.lh, o.lv, o.luma, o.chroma):
        return None
    return t


def host_transform_libjpeg(pixels, quality=90, sampling=None, qtables=None, flip=False):
    """mjw_lj_plan_init + mjw_lj_transform_host: the units of a libjpeg slot computed on the HOST -> (TranscodePlan, int16 [n_du, 64]);
    (None, None) for what is refused"""
    a = _hwc_u8(pixels)
    h, w, comp = a.shape
    t = libjpeg_plan(w, h, comp, quality, sampling, qtables)
    if t is None:
        return None, None
    L = lib()
    L.mjw_lj_transform_host.argtypes = [C.POINTER(TranscodePlan), C.c_void_p, C.c_int, C.c_void_p]
    du = np.empty(t.du_elems(), dtype=np.int16)
    if not L.mjw_lj_transform_host(C.byref(t), a.ctypes.data_as(C.c_void_p), int(bool(flip)), du.ctypes.data_as(C.c_void_p)):
        return None, None
    return t, du.reshape(-1, 64)


def libjpeg_quantise_all(q):
    """mjw_lj_quantise(x, q) for x = -32768 .. 32768 -> int32 [65537]: the multiply-high quantiser of LIBJPEG ENCODING"""
    L = lib()
    L.mjw_lj_quantise_all.argtypes = [C.c_int, C.c_void_p]
    L.mjw_lj_quantise_all.restype = None
    out = np.empty(65537, np.int32)
    L.mjw_lj_quantise_all(int(q), out.ctypes.data_as(C.c_void_p))
    return out


def libjpeg_reframe(stream):
    """mjw_lj_reframe: a stream of this library's writer in libjpeg's framing (a DQT and a DHT segment per table) -> bytes; None for a
    malformed header"""
    L = lib()
    L.mjw_lj_reframe.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    L.mjw_lj_reframe.restype = C.c_size_t
    data = bytes(stream)
    out = C.create_string_buffer(len(data) + 64)
    n = L.mjw_lj_reframe(data, len(data), out)
    return out.raw[:n] if n else None


def write_jpg_libjpeg_to_memory(pixels, quality=90, sampling=None, qtables=None, flip=False, optimize=False, restart_rows=None, restart_mcus=None,
                                progressive=False):
    """mjh_write_jpg_libjpeg_to_memory: the host twin of arithmetic="libjpeg" -- what Pillow's save(..., quality=, subsampling=) writes for
    these pixels, byte for byte -> bytes, None where it refuses ("440", 2 or 4 channels).  sampling None: "420"."""
    a = _hwc_u8(pixels)
    h, w, comp = a.shape
    o = enc_opts(sampling, qtables) or EncOpts()
    rows, mcus = _restart_mcus(restart_rows), _restart_mcus(restart_mcus)
    if rows and mcus:
        raise ValueError("restart_rows and restart_mcus are two ways to say the same thing: give one")
    if rows:
        t = libjpeg_plan(w, h, comp, quality, sampling, qtables)
        if t is None:
            return None
        mcus = rows * t.plan.mcu_x
    prog = _progressive_flag(progressive, mcus)
    L = lib()
    L.mjh_write_jpg_libjpeg_to_memory.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                                  C.c_int, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    out, n = C.c_void_p(), C.c_size_t()
    if not L.mjh_write_jpg_libjpeg_to_memory(a.ctypes.data_as(C.c_void_p), w, h, comp, int(quality), o.ncomp, o.lh, o.lv, o.luma, o.chroma,
                                             int(bool(flip)), MJW_OPTIMIZE_HUFFMAN if optimize else 0, mcus, int(prog), C.byref(out), C.byref(n)):
        return None
    return _take_malloced(out, n.value)


class Plane(C.Structure):
    """mij_plane (include/mij.h): sample (y, x) is the byte at src + y * row_pitch + x * x_pitch."""
    _fields_ = [("src", C.c_void_p), ("row_pitch", C.c_int64), ("x_pitch", C.c_int64)]


class InPlanes(C.Structure):
    """mij_in_planes (include/mij.h)."""
    _fields_ = [("planes", Plane * 3), ("width", C.c_int32), ("height", C.c_int32), ("opts", EncOpts), ("convert", C.c_void_p),
                ("flip_vertically", C.c_int32)]


def plane_shapes(width, height, sampling):
    """the (rows, columns) of the Y, Cb and Cr planes of a width x height picture (include/mij_host.h, PLANE ENCODING); grey: Y only"""
    ncomp, lh, lv = plane_sampling(sampling)
    chroma = ((height + lv - 1) // lv, (width + lh - 1) // lh)
    return [(height, width)] + [chroma] * (ncomp - 1)


def plane_sampling(sampling):
    """sampling_factors for plane encoding, where the sampling is required: ValueError for None too"""
    if sampling is None:
        raise ValueError("plane encoding needs its sampling: one of %s" % ", ".join(repr(k) for k in SAMPLINGS))
    return sampling_factors(sampling)


def video_range_convert():
    """mjw_video_range: the InConvert that takes studio-range samples (Y 16..235, chroma 16..240) to JFIF's full range"""
    L = lib()
    L.mjw_video_range.argtypes = [C.POINTER(InConvert)]
    L.mjw_video_range.restype = None
    cv = InConvert(MIJ_DT_U8)
    L.mjw_video_range(C.byref(cv))
    return cv


def _plane_convert(video_range, convert):
    """-> an InConvert or None: video_range=True is mjw_video_range's, convert a ((scale_y, scale_cb, scale_cr), (bias ...)) pair or an
    InConvert of the caller's.  ValueError for both given and for values that are not finite."""
    if video_range and convert is not None:
        raise ValueError("video_range and convert both say how samples are converted: give one")
    if video_range:
        return video_range_convert()
    if convert is None:
        return None
    if not isinstance(convert, InConvert):
        scale, bias = convert
        convert = InConvert(MIJ_DT_U8, [float(v) for v in scale], [float(v) for v in bias])
    if not all(np.isfinite(convert.scale[k]) and np.isfinite(convert.bias[k]) for k in range(3)):
        raise ValueError("the conversion's scale and bias must be finite")
    return convert


def split_planes(picture, sampling):
    """a picture of planes -- (Y, Cb, Cr), (Y, CbCr) with CbCr of shape [ch, cw, 2] (NV12), or Y alone for "grey" (bare, or in a sequence
    of one) -- as the list of its 2-D planes, views of the caller's arrays; ValueError for anything else.  Works on numpy arrays and on
    tensors alike (only .ndim / .shape and indexing are used)."""
    ncomp, _, _ = plane_sampling(sampling)
    parts = [picture] if hasattr(picture, "shape") else list(picture)
    if len(parts) == 2 and ncomp == 3 and len(parts[1].shape) == 3 and parts[1].shape[2] == 2:
        parts = [parts[0], parts[1][:, :, 0], parts[1][:, :, 1]]
    if ncomp == 1 and len(parts) != 1:
        raise ValueError("a grey picture is its Y plane alone: chroma planes were given")
    if len(parts) != ncomp:
        raise ValueError("sampling %r takes (Y, Cb, Cr) or (Y, CbCr[ch, cw, 2]); got %d planes" % (sampling, len(parts)))
    for k, a in enumerate(parts):
        if len(a.shape) != 2:
            raise ValueError("plane %d is %d-D; planes are 2-D" % (k, len(a.shape)))
    h, w = parts[0].shape
    for k, (a, want) in enumerate(zip(parts, plane_shapes(w, h, sampling))):
        if tuple(a.shape) != want:
            raise ValueError("plane %d is %dx%d (rows x columns); a %dx%d picture at sampling %r needs %dx%d" %
                             (k, a.shape[0], a.shape[1], h, w, sampling, want[0], want[1]))
    return parts


def _numpy_planes(picture, sampling, positive=False):
    """-> ([(address, row_pitch, x_pitch)], width, height, keep): the planes of numpy arrays, arbitrary 2-D uint8 views, pitches from
    their strides.  positive: views with a negative stride are copied first (the GPU encoder's slots take pitches > 0)."""
    parts = split_planes(picture, sampling)
    keep, out = [], []
    for k, a in enumerate(parts):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
            raise ValueError("plane %d must be a uint8 numpy array" % k)
        if 0 in a.shape:
            raise ValueError("plane %d is empty" % k)
        if positive and any(st < 0 for st in a.strides):
            a = np.ascontiguousarray(a)
        keep.append(a)
        # a stride of an axis of one element addresses nothing: 0 rows down, 1 sample across
        out.append((a.ctypes.data, a.strides[0] if a.shape[0] > 1 else 0, (a.strides[1] or 1) if a.shape[1] > 1 else 1))
    return out, parts[0].shape[1], parts[0].shape[0], keep


def in_planes(triples, width, height, sampling, qtables=None, convert=None, flip=False):
    """-> (InPlanes, keep): the mij_in_planes of (address, row_pitch, x_pitch) triples; keep holds what the struct points into"""
    ncomp, lh, lv = plane_sampling(sampling)
    luma, chroma = (None, None) if qtables is None else _qtable_pair(qtables)
    p = InPlanes()
    for k, (addr, rp, xp) in enumerate(triples):
        p.planes[k] = Plane(addr, rp, xp)
    p.width, p.height = int(width), int(height)
    p.opts = EncOpts(ncomp, lh, lv, luma, chroma)
    p.convert = C.cast(C.pointer(convert), C.c_void_p) if convert is not None else None
    p.flip_vertically = int(bool(flip))
    return p, (luma, chroma, convert)


def planes_plan(width, height, sampling, quality=90, qtables=None):
    """mjw_pplan_init -> TranscodePlan; None where the writer refuses the size"""
    ncomp, lh, lv = plane_sampling(sampling)
    luma, chroma = (None, None) if qtables is None else _qtable_pair(qtables)
    L = lib()
    L.mjw_pplan_init.argtypes = [C.POINTER(TranscodePlan), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p]
    t = TranscodePlan()
    if not L.mjw_pplan_init(C.byref(t), int(width), int(height), int(quality), ncomp, lh, lv, luma, chroma):
        return None
    return t


def host_transform_planes(picture, sampling, quality=90, qtables=None, video_range=False, flip=False, convert=None):
    """mjw_pplan_init + mjw_ptransform_host: the units of a plane slot computed on the HOST -> (TranscodePlan, int16 [n_du, 64]); the CPU
    twin of Encoder.add_planes.  picture: see split_planes; numpy arrays may be arbitrary 2-D views."""
    triples, w, h, keep = _numpy_planes(picture, sampling)
    cv = _plane_convert(video_range, convert)
    t = planes_plan(w, h, sampling, quality, qtables)
    if t is None:
        return None, None
    L = lib()
    L.mjw_ptransform_host.argtypes = [C.POINTER(TranscodePlan), C.POINTER(Plane), C.c_void_p, C.c_int, C.c_void_p]
    pl = (Plane * 3)(*[Plane(*tr) for tr in triples])
    du = np.empty(t.du_elems(), dtype=np.int16)
    if not L.mjw_ptransform_host(C.byref(t), pl, C.byref(cv) if cv is not None else None, int(bool(flip)), du.ctypes.data_as(C.c_void_p)):
        return None, None
    return t, du.reshape(-1, 64)


def host_transform_libjpeg_planes(picture, sampling, quality=90, qtables=None, video_range=False, flip=False, convert=None):
    """mjw_pplan_init + mjw_lj_ptransform_host: host_transform_planes with libjpeg's forward DCT, quantiser and dummy blocks (include/mij_host.h,
    LIBJPEG ENCODING); (None, None) for what is refused ("440")"""
    triples, w, h, keep = _numpy_planes(picture, sampling)
    cv = _plane_convert(video_range, convert)
    t = planes_plan(w, h, sampling, quality, qtables)
    if t is None:
        return None, None
    L = lib()
    L.mjw_lj_ptransform_host.argtypes = [C.POINTER(TranscodePlan), C.POINTER(Plane), C.c_void_p, C.c_int, C.c_void_p]
    pl = (Plane * 3)(*[Plane(*tr) for tr in triples])
    du = np.empty(t.du_elems(), dtype=np.int16)
    if not L.mjw_lj_ptransform_host(C.byref(t), pl, C.byref(cv) if cv is not None else None, int(bool(flip)), du.ctypes.data_as(C.c_void_p)):
        return None, None
    return t, du.reshape(-1, 64)


def write_jpg_planes_to_memory(picture, sampling, quality=90, qtables=None, video_range=False, flip=False, optimize=False, restart_rows=None,
                               restart_mcus=None, progressive=False, convert=None):
    """mjh_write_jpg_planes_to_memory: the host writer fed with Y, Cb and Cr planes (include/mij_host.h, PLANE ENCODING) -> bytes, None
    where it refuses.  restart_rows counts MCU rows of the sampling's own MCU size."""
    triples, w, h, keep = _numpy_planes(picture, sampling)
    cv = _plane_convert(video_range, convert)
    ncomp, lh, lv = plane_sampling(sampling)
    luma, chroma = (None, None) if qtables is None else _qtable_pair(qtables)
    rows, mcus = _restart_mcus(restart_rows), _restart_mcus(restart_mcus)
    if rows and mcus:
        raise ValueError("restart_rows and restart_mcus are two ways to say the same thing: give one")
    if rows:
        mcus = rows * ((w + 8 * lh - 1) // (8 * lh))
    prog = _progressive_flag(progressive, mcus)
    L = lib()
    L.mjh_write_jpg_planes_to_memory.argtypes = [C.POINTER(Plane), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                                 C.c_void_p, C.c_int, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    pl = (Plane * 3)(*[Plane(*tr) for tr in triples])
    out, n = C.c_void_p(), C.c_size_t()
    if not L.mjh_write_jpg_planes_to_memory(pl, w, h, int(quality), ncomp, lh, lv, luma, chroma, C.byref(cv) if cv is not None else None,
                                            int(bool(flip)), MJW_OPTIMIZE_HUFFMAN if optimize else 0, mcus, int(prog), C.byref(out), C.byref(n)):
        return None
    return _take_malloced(out, n.value)


def requant_magic(b):
    """mjw_requant_magic -> (m, inc): n // b == ((n + inc) * m) >> 32 for every n < 2^24, the division of the conversion kernel"""
    L = lib()
    L.mjw_requant_magic.argtypes = [C.c_int, C.POINTER(C.c_uint32)]
    L.mjw_requant_magic.restype = C.c_uint32
    inc = C.c_uint32()
    m = L.mjw_requant_magic(int(b), C.byref(inc))
    return int(m), int(inc.value)


def transcode_plan_requant(tplan, tables, coarsen_only=True):
    """mjw_tplan_requant: the plan with its tables replaced -> (TranscodePlan, changed), or (None, reason) where it is refused.  tables
    are passed as they are (uint8 [64] each), so that a zero entry reaches the library."""
    L = lib()
    L.mjw_tplan_requant.argtypes = [C.POINTER(TranscodePlan), C.POINTER(TranscodePlan), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_char_p)]
    luma, chroma = (np.ascontiguousarray(t, np.uint8) for t in tables)
    assert luma.shape == (64,) and chroma.shape == (64,)
    t, why = TranscodePlan(), C.c_char_p()
    r = L.mjw_tplan_requant(C.byref(t), C.byref(tplan), luma.ctypes.data_as(C.c_void_p), chroma.ctypes.data_as(C.c_void_p), int(bool(coarsen_only)),
                            C.byref(why))
    if not r:
        return None, (why.value.decode() if why.value else "refused")
    return t, r == 2


def units_requant(src, dst, du):
    """mjw_units_requant: the units of plan src (tables s) requantised for plan dst (tables d) -> int16 [n_du, 64]; None on bad arguments"""
    L = lib()
    L.mjw_units_requant.argtypes = [C.POINTER(TranscodePlan), C.POINTER(TranscodePlan), C.c_void_p, C.c_void_p]
    d = np.ascontiguousarray(du, np.int16)
    if d.size != src.du_elems():
        raise ValueError("%d data-unit elements for a picture that has %d" % (d.size, src.du_elems()))
    out = np.empty(dst.du_elems(), np.int16)
    if not L.mjw_units_requant(C.byref(src), C.byref(dst), d.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)):
        return None
    return out.reshape(-1, 64)


def transcode_memory(data, optimize=False, copy_markers=False, orientation=None, trim=False, tables=None, coarsen_only=True, crop=None,
                     grey=False, restart_rows=None, restart_mcus=None, progressive=False):
    """mjh_transcode_memory, the lossless transcode on the host alone -> (bytes, None) or (None, reason).  With an orientation
    (1..8, or "exif" for the file's own tag) it is mjh_transcode_memory_oriented; trim chooses its edge mode.  With tables = (luma,
    chroma) it is mjh_transcode_memory_requant: the coefficients requantised after the orientation.  With crop = (x0, y0, w, h) in the
    displayed frame and / or grey=True it is mjh_transcode_memory_window: grey -> orient -> crop -> requantise.  With restart_rows or
    restart_mcus (an interval in MCU rows or MCUs of the destination; both given, negative or above 65535 MCUs: refused with a reason) it
    is mjh_transcode_memory_restart_by.  With progressive=True it is mjh_transcode_memory_progressive: the same chain, written as a
    progressive stream; a restart interval with it is a ValueError."""
    L = lib()
    data = bytes(data)
    out, n, why = C.c_void_p(), C.c_size_t(), C.c_char_p()
    flags = (MJW_OPTIMIZE_HUFFMAN if optimize else 0) | (MJW_COPY_MARKERS if copy_markers else 0)
    rows, mcus = (min(max(_restart_mcus(v), -1), 1 << 30) for v in (restart_rows, restart_mcus))
    if _progressive_flag(progressive, rows or mcus):
        luma, chroma = (None, None) if tables is None else _qtable_pair(tables)
        win = None if crop is None else (C.c_int * 4)(*[int(v) for v in crop])
        L.mjh_transcode_memory_progressive.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_char_p,
                                                       C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                       C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
        o = 1 if orientation is None else 0 if orientation == "exif" else int(orientation)
        ok = L.mjh_transcode_memory_progressive(data, len(data), flags, o, int(bool(trim)), win, int(bool(grey)), luma, chroma,
                                                int(bool(coarsen_only)), 1, C.byref(out), C.byref(n), None, C.byref(why))
    elif rows or mcus:
        luma, chroma = (None, None) if tables is None else _qtable_pair(tables)
        win = None if crop is None else (C.c_int * 4)(*[int(v) for v in crop])
        L.mjh_transcode_memory_restart_by.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_char_p,
                                                      C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
        o = 1 if orientation is None else 0 if orientation == "exif" else int(orientation)
        ok = L.mjh_transcode_memory_restart_by(data, len(data), flags, o, int(bool(trim)), win, int(bool(grey)), luma, chroma,
                                               int(bool(coarsen_only)), rows, mcus, C.byref(out), C.byref(n), None, None, C.byref(why))
    elif crop is not None or grey:
        luma, chroma = (None, None) if tables is None else _qtable_pair(tables)
        win = None if crop is None else (C.c_int * 4)(*[int(v) for v in crop])
        L.mjh_transcode_memory_window.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_char_p,
                                                  C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                                  C.POINTER(C.c_char_p)]
        o = 1 if orientation is None else 0 if orientation == "exif" else int(orientation)
        ok = L.mjh_transcode_memory_window(data, len(data), flags, o, int(bool(trim)), win, int(bool(grey)), luma, chroma,
                                           int(bool(coarsen_only)), C.byref(out), C.byref(n), None, C.byref(why))
    elif tables is not None:
        luma, chroma = _qtable_pair(tables)
        L.mjh_transcode_memory_requant.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int,
                                                   C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)]
        o = 1 if orientation is None else 0 if orientation == "exif" else int(orientation)
        ok = L.mjh_transcode_memory_requant(data, len(data), flags, o, int(bool(trim)), luma, chroma, int(bool(coarsen_only)), C.byref(out),
                                            C.byref(n), C.byref(why))
    elif orientation is None:
        L.mjh_transcode_memory.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)]
        ok = L.mjh_transcode_memory(data, len(data), flags, C.byref(out), C.byref(n), C.byref(why))
    else:
        L.mjh_transcode_memory_oriented.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                    C.POINTER(C.c_char_p)]
        ok = L.mjh_transcode_memory_oriented(data, len(data), flags, 0 if orientation == "exif" else int(orientation), int(bool(trim)), C.byref(out),
                                             C.byref(n), C.byref(why))
    if not ok:
        return None, (why.value.decode() if why.value else "decode failed")
    return _take_malloced(out, n.value), None


def transcode_plan_oriented(tplan, orientation, trim=False):
    """mjw_tplan_oriented: the destination's plan of a source's -> (TranscodePlan, None), or (None, reason) where it is refused"""
    L = lib()
    L.mjw_tplan_oriented.argtypes = [C.POINTER(TranscodePlan), C.POINTER(TranscodePlan), C.c_int, C.c_int, C.POINTER(C.c_char_p)]
    t, why = TranscodePlan(), C.c_char_p()
    if not L.mjw_tplan_oriented(C.byref(t), C.byref(tplan), int(orientation), int(bool(trim)), C.byref(why)):
        return None, (why.value.decode() if why.value else "refused")
    return t, None


def transcode_plan_grey(tplan):
    """mjw_tplan_grey: the one-component plan of a plan (a grey plan is copied) -> TranscodePlan, None for a bad plan"""
    L = lib()
    L.mjw_tplan_grey.argtypes = [C.POINTER(TranscodePlan), C.POINTER(TranscodePlan)]
    t = TranscodePlan()
    return t if L.mjw_tplan_grey(C.byref(t), C.byref(tplan)) else None


def units_grey(tplan, du):
    """mjw_units_grey: a source's units -> the grey plan's (the luma blocks inside ceil(W / 8) x ceil(H / 8)), int16 [n_du, 64]"""
    dst = transcode_plan_grey(tplan)
    if dst is None:
        return None
    L = lib()
    L.mjw_units_grey.argtypes = [C.POINTER(TranscodePlan), C.c_void_p, C.c_void_p]
    d = np.ascontiguousarray(du, np.int16)
    if d.size != tplan.du_elems():
        raise ValueError("%d data-unit elements for a picture that has %d" % (d.size, tplan.du_elems()))
    out = np.empty(dst.du_elems(), np.int16)
    if not L.mjw_units_grey(C.byref(tplan), d.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)):
        return None
    return out.reshape(-1, 64)


def transcode_plan_cropped(tplan, crop):
    """mjw_tplan_cropped: the plan of the window crop = (x0, y0, w, h) of a plan's picture -> (TranscodePlan, (x0', y0', W', H')), the kept
    rectangle with its origin on the MCU grid, or (None, reason) for a window that does not lie inside the picture"""
    L = lib()
    L.mjw_tplan_cropped.argtypes = [C.POINTER(TranscodePlan), C.POINTER(TranscodePlan), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                    C.POINTER(C.c_char_p)]
    t, why, rect = TranscodePlan(), C.c_char_p(), (C.c_int * 4)()
    x0, y0, w, h = (int(v) for v in crop)
    if not L.mjw_tplan_cropped(C.byref(t), C.byref(tplan), x0, y0, w, h, rect, C.byref(why)):
        return None, (why.value.decode() if why.value else "refused")
    return t, tuple(rect)


def units_crop(tplan, du, rect):
    """mjw_units_crop: the units of the kept rectangle `rect` (as transcode_plan_cropped returned it) from the plan's, int16 [n_du, 64];
    None for a rectangle that is none"""
    dst, kept = transcode_plan_cropped(tplan, rect)
    if dst is None or kept != tuple(int(v) for v in rect):
        return None
    L = lib()
    L.mjw_units_crop.argtypes = [C.POINTER(TranscodePlan), C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    d = np.ascontiguousarray(du, np.int16)
    if d.size != tplan.du_elems():
        raise ValueError("%d data-unit elements for a picture that has %d" % (d.size, tplan.du_elems()))
    out = np.empty(dst.du_elems(), np.int16)
    if not L.mjw_units_crop(C.byref(tplan), d.ctypes.data_as(C.c_void_p), (C.c_int * 4)(*kept), out.ctypes.data_as(C.c_void_p)):
        return None
    return out.reshape(-1, 64)


def units_orient(tplan, du, orientation, trim=False):
    """mjw_units_orient: a source's units (in its plan's order) -> the destination's, int16 [n_du, 64]; None where the picture is refused"""
    dst, _ = transcode_plan_oriented(tplan, orientation, trim)
    if dst is None:
        return None
    L = lib()
    L.mjw_units_orient.argtypes = [C.POINTER(TranscodePlan), C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    d = np.ascontiguousarray(du, np.int16)
    if d.size != tplan.du_elems():
        raise ValueError("%d data-unit elements for a picture that has %d" % (d.size, tplan.du_elems()))
    out = np.empty(dst.du_elems(), np.int16)
    if not L.mjw_units_orient(C.byref(tplan), d.ctypes.data_as(C.c_void_p), int(orientation), int(bool(trim)), out.ctypes.data_as(C.c_void_p)):
        return None
    return out.reshape(-1, 64)


def write_histogram(plan, du):
    """mjw_histogram: the symbols mjw_emit emits for these units, counted -> uint32 [4, 256] (luma DC, chroma DC, luma AC, chroma AC),
    None when it is refused."""
    L = lib()
    L.mjw_histogram.argtypes = [C.POINTER(WritePlan), C.c_void_p, C.c_void_p]
    d = np.ascontiguousarray(du, dtype=np.int16)
    freq = np.zeros((4, 256), np.uint32)
    return freq if L.mjw_histogram(C.byref(plan), d.ctypes.data_as(C.c_void_p), freq.ctypes.data_as(C.c_void_p)) else None


def optimal_huffman_table(freq):
    """mjw_optimal_table: 256 counts -> (BITS[16], HUFFVAL) as lists, None when a code would exceed 32 bits before shortening."""
    L = lib()
    L.mjw_optimal_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    if f.shape != (256,):
        raise ValueError("freq must hold 256 counts")
    bits, vals, n = np.zeros(16, np.uint8), np.zeros(256, np.uint8), C.c_int()
    if not L.mjw_optimal_table(f.ctypes.data_as(C.c_void_p), bits.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), C.byref(n)):
        return None
    return bits.tolist(), vals[:n.value].tolist()


def mij_write_jpg_to_memory(pixels, quality=90, optimize=False):
    """mij_write_jpg_to_func: the writer with its transform stage on the GPU -> bytes (None on failure).  optimize:
    mij_write_jpg_to_func_ex with MJW_OPTIMIZE_HUFFMAN."""
    a = np.ascontiguousarray(pixels, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, comp = a.shape
    L = lib()
    L.mij_write_jpg_to_func_ex.argtypes = [_WRITE_CB, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_uint]
    L.mij_write_jpg_to_func.argtypes = [_WRITE_CB, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    chunks = []
    cb = _WRITE_CB(lambda _c, data, size: chunks.append(C.string_at(data, size)))
    if optimize:
        ok = L.mij_write_jpg_to_func_ex(cb, None, w, h, comp, a.ctypes.data_as(C.c_void_p), int(quality), MJW_OPTIMIZE_HUFFMAN)
    else:
        ok = L.mij_write_jpg_to_func(cb, None, w, h, comp, a.ctypes.data_as(C.c_void_p), int(quality))
    return b"".join(chunks) if ok else None


def mij_write_jpg_batch(images, quality=90, threads=16, optimize=False):
    """mij_write_jpg_batch: a list of uint8 pictures [h, w, comp] (or [h, w]; None = a NULL pixel pointer) -> list of byte streams
    (None where the picture was refused).  A negative return raises; the C side has released every stream by then.  optimize:
    mij_write_jpg_batch_ex with MJW_OPTIMIZE_HUFFMAN."""
    L = lib()
    arrs = []
    for im in images:
        if im is None:
            arrs.append(None)
            continue
        a = np.ascontiguousarray(im, dtype=np.uint8)
        arrs.append(a[:, :, None] if a.ndim == 2 else a)
    n = len(arrs)
    L.mij_write_jpg_batch.restype = C.c_int
    L.mij_write_jpg_batch.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    px = (C.c_void_p * n)(*[(a.ctypes.data if a is not None else None) for a in arrs])
    xs = (C.c_int * n)(*[(a.shape[1] if a is not None else 16) for a in arrs])
    ys = (C.c_int * n)(*[(a.shape[0] if a is not None else 16) for a in arrs])
    cs = (C.c_int * n)(*[(a.shape[2] if a is not None else 3) for a in arrs])
    out = (C.c_void_p * n)()
    lens = (C.c_size_t * n)()
    if optimize:
        L.mij_write_jpg_batch_ex.restype = C.c_int
        L.mij_write_jpg_batch_ex.argtypes = L.mij_write_jpg_batch.argtypes + [C.c_uint]
        rc = L.mij_write_jpg_batch_ex(px, xs, ys, cs, n, int(quality), int(threads), out, lens, MJW_OPTIMIZE_HUFFMAN)
    else:
        rc = L.mij_write_jpg_batch(px, xs, ys, cs, n, int(quality), int(threads), out, lens)
    if rc < 0:
        assert not any(out[i] for i in range(n)), "mij_write_jpg_batch returned an error and left streams allocated"
        raise MijError("mij_write_jpg_batch: error %d" % rc)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    res = []
    for i in range(n):
        if out[i]:
            res.append(C.string_at(out[i], lens[i]))
            libc.free(out[i])
        else:
            res.append(None)
    assert rc == sum(r is not None for r in res), "mij_write_jpg_batch: return value and streams disagree"
    return res


class InTensor(C.Structure):
    """mij_in_tensor (include/mij.h)."""
    _fields_ = [("src", C.c_void_p), ("layout", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("comp", C.c_int32),
                ("row_pitch", C.c_int64), ("plane_pitch", C.c_int64)]


class InConvert(C.Structure):
    """mij_in_convert (include/mij.h): the element type of a float device-pixel slot and its per-channel float32 scale and bias."""
    _fields_ = [("dtype", C.c_int32), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]

    def __init__(self, dtype=MIJ_DT_F32, scale=(), bias=()):
        """dtype: MIJ_DT_* or "f16" / "bf16" / "f32"; scale, bias: up to 4 values, the rest stay 0"""
        super().__init__()
        self.dtype = _DTYPES.get(dtype, dtype)
        for k, v in enumerate(scale):
            self.scale[k] = v
        for k, v in enumerate(bias):
            self.bias[k] = v


class Encoder:
    """mij_encoder: batch colour + subsample + fDCT + quantiser on the GPU; with an emission arena (stream_reserve) also the Huffman
    stage, so that finished streams come back."""

    def __init__(self, ctx, max_images, pixel_bytes, du_bytes, stage_bytes=None):
        """stage_bytes: pinned staging for host pictures (add); None = pixel_bytes (mij_enc_create), 0 for an encoder fed only by
        add_device / add_units (mij_enc_create_ex)."""
        L = lib()
        L.mij_enc_create.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p)]
        L.mij_enc_create_ex.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p)]
        L.mij_enc_destroy.argtypes = [C.c_void_p]
        L.mij_enc_add.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.mij_enc_add_clone.argtypes = [C.c_void_p, C.c_int]
        for name in ("mij_enc_reset", "mij_enc_upload", "mij_enc_launch", "mij_enc_wait", "mij_enc_timer_begin", "mij_enc_timer_end"):
            getattr(L, name).argtypes = [C.c_void_p]
        L.mij_enc_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.mij_enc_plan.argtypes = [C.c_void_p, C.c_int, C.POINTER(WritePlan)]
        L.mij_enc_timer_elapsed_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._h = C.c_void_p()
        if stage_bytes is None:
            _check(L.mij_enc_create(ctx._h, int(max_images), C.c_size_t(pixel_bytes), C.c_size_t(du_bytes), C.byref(self._h)), "mij_enc_create")
        else:
            _check(L.mij_enc_create_ex(ctx._h, int(max_images), C.c_size_t(stage_bytes), C.c_size_t(pixel_bytes), C.c_size_t(du_bytes),
                                       C.byref(self._h)), "mij_enc_create_ex")

    def reset(self):
        _check(lib().mij_enc_reset(self._h), "mij_enc_reset")

    def add(self, pixels, quality=90, flip=False, sampling=None, qtables=None):
        """mij_enc_add; with sampling ("444", "422", "440", "420", "grey") and / or qtables ((luma, chroma), 64 ints 1..255 each in zigzag
        order) mij_enc_add_ex: a slot with a sampling or tables of its own (include/mij_host.h, SAMPLED ENCODING)."""
        a = np.ascontiguousarray(pixels, dtype=np.uint8)
        if a.ndim == 2:
            a = a[:, :, None]
        h, w, comp = a.shape
        o = enc_opts(sampling, qtables)
        if o is None:
            return _check(lib().mij_enc_add(self._h, a.ctypes.data_as(C.c_void_p), w, h, comp, int(quality), int(bool(flip))), "mij_enc_add")
        L = lib()
        L.mij_enc_add_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EncOpts)]
        return _check(L.mij_enc_add_ex(self._h, a.ctypes.data_as(C.c_void_p), w, h, comp, int(quality), int(bool(flip)), C.byref(o)), "mij_enc_add_ex")

    def add_clone(self, src):
        return _check(lib().mij_enc_add_clone(self._h, int(src)), "mij_enc_add_clone")

    def upload(self):
        _check(lib().mij_enc_upload(self._h), "mij_enc_upload")

    def launch(self):
        _check(lib().mij_enc_launch(self._h), "mij_enc_launch")

    def wait(self):
        _check(lib().mij_enc_wait(self._h), "mij_enc_wait")

    def force_generic(self, on=True):
        """Per-unit kernels even where the fused 4:2:0 strip kernel applies (tests); call before upload."""
        L = lib()
        L.mij_enc_force_generic.argtypes = [C.c_void_p, C.c_int]
        _check(L.mij_enc_force_generic(self._h, int(bool(on))), "mij_enc_force_generic")

    def plan(self, slot):
        p = WritePlan()
        _check(lib().mij_enc_plan(self._h, int(slot), C.byref(p)), "mij_enc_plan")
        return p

    def fetch(self, slot):
        p = self.plan(slot)
        du = np.empty(p.du_elems(), dtype=np.int16)
        _check(lib().mij_enc_fetch(self._h, int(slot), du.ctypes.data_as(C.c_void_p), C.c_size_t(du.size)), "mij_enc_fetch")
        return du.reshape(-1, 64)

    def add_device(self, t, quality=90, flip=False, sampling=None, qtables=None):
        """mij_enc_add_device: a slot whose uint8 pixels lie in device memory, described by an InTensor.  sampling, qtables: as for add
        (mij_enc_add_device_ex)."""
        L = lib()
        o = enc_opts(sampling, qtables)
        if o is not None:
            L.mij_enc_add_device_ex.argtypes = [C.c_void_p, C.POINTER(InTensor), C.c_int, C.c_int, C.POINTER(EncOpts)]
            return _check(L.mij_enc_add_device_ex(self._h, C.byref(t), int(quality), int(bool(flip)), C.byref(o)), "mij_enc_add_device_ex")
        L.mij_enc_add_device.argtypes = [C.c_void_p, C.POINTER(InTensor), C.c_int, C.c_int]
        return _check(L.mij_enc_add_device(self._h, C.byref(t), int(quality), int(bool(flip))), "mij_enc_add_device")

    def add_device_float(self, t, convert, quality=90, flip=False, sampling=None, qtables=None):
        """mij_enc_add_device_float: a slot whose float16 / bfloat16 / float32 elements lie in device memory, described by an InTensor
        (pitches in elements), de-normalised on the GPU by the contract of include/mij.h with the InConvert's scale and bias.  sampling,
        qtables: as for add (mij_enc_add_device_float_ex)."""
        L = lib()
        o = enc_opts(sampling, qtables)
        if o is not None:
            L.mij_enc_add_device_float_ex.argtypes = [C.c_void_p, C.POINTER(InTensor), C.POINTER(InConvert), C.c_int, C.c_int, C.POINTER(EncOpts)]
            return _check(L.mij_enc_add_device_float_ex(self._h, C.byref(t), C.byref(convert), int(quality), int(bool(flip)), C.byref(o)),
                          "mij_enc_add_device_float_ex")
        L.mij_enc_add_device_float.argtypes = [C.c_void_p, C.POINTER(InTensor), C.POINTER(InConvert), C.c_int, C.c_int]
        return _check(L.mij_enc_add_device_float(self._h, C.byref(t), C.byref(convert), int(quality), int(bool(flip))), "mij_enc_add_device_float")

    def add_planes(self, picture, sampling, quality=90, qtables=None, video_range=False, flip=False, convert=None):
        """mij_enc_add_planes: a slot fed with Y, Cb and Cr planes in host memory (include/mij_host.h, PLANE ENCODING).  picture: (Y, Cb,
        Cr), (Y, CbCr[ch, cw, 2]) or Y alone for "grey"; numpy arrays may be arbitrary 2-D uint8 views, pitches come from their strides."""
        triples, w, h, keep = _numpy_planes(picture, sampling, positive=True)
        p, keep2 = in_planes(triples, w, h, sampling, qtables, _plane_convert(video_range, convert), flip)
        L = lib()
        L.mij_enc_add_planes.argtypes = [C.c_void_p, C.POINTER(InPlanes), C.c_int]
        return _check(L.mij_enc_add_planes(self._h, C.byref(p), int(quality)), "mij_enc_add_planes")

    def add_device_planes(self, triples, width, height, sampling, quality=90, qtables=None, video_range=False, flip=False, convert=None):
        """mij_enc_add_device_planes: the same slot with its planes in caller-owned device memory; triples: one (device address, row_pitch,
        x_pitch) in bytes per plane -- Y, Cb, Cr, or Y alone for "grey"."""
        ncomp = plane_sampling(sampling)[0]
        triples = list(triples)
        if len(triples) != ncomp:
            raise ValueError("sampling %r takes %d plane%s, got %d" % (sampling, ncomp, "" if ncomp == 1 else "s", len(triples)))
        p, keep = in_planes(triples, width, height, sampling, qtables, _plane_convert(video_range, convert), flip)
        L = lib()
        L.mij_enc_add_device_planes.argtypes = [C.c_void_p, C.POINTER(InPlanes), C.c_int]
        return _check(L.mij_enc_add_device_planes(self._h, C.byref(p), int(quality)), "mij_enc_add_device_planes")

    @staticmethod
    def plane_bytes(width, height, sampling):
        """mij_enc_plane_bytes: what a plane slot takes in the pixel arenas"""
        ncomp, lh, lv = plane_sampling(sampling)
        L = lib()
        L.mij_enc_plane_bytes.argtypes = [C.c_int, C.c_int, C.POINTER(EncOpts)]
        L.mij_enc_plane_bytes.restype = C.c_size_t
        o = EncOpts(ncomp, lh, lv, None, None)
        return L.mij_enc_plane_bytes(int(width), int(height), C.byref(o))

    def add_units(self, width, height, comp, quality, du):
        """mij_enc_add_units: a slot whose quantised data units (int16 [n_du, 64], zigzag order) are given."""
        L = lib()
        L.mij_enc_add_units.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        d = np.ascontiguousarray(du, dtype=np.int16)
        plan = WritePlan()
        L.mjw_plan_init.argtypes = [C.POINTER(WritePlan), C.c_int, C.c_int, C.c_int, C.c_int]
        if L.mjw_plan_init(C.byref(plan), int(width), int(height), int(comp), int(quality)) and d.size != plan.du_elems():
            raise ValueError("%d data-unit elements for a picture that has %d" % (d.size, plan.du_elems()))
        return _check(L.mij_enc_add_units(self._h, int(width), int(height), int(comp), int(quality), d.ctypes.data_as(C.c_void_p)), "mij_enc_add_units")

    def add_coef(self, batch, slot, orientation=1, trim=False, tables=None, coarsen_only=True, crop=None, grey=False):
        """mij_enc_add_coef: a slot whose units are the quantised coefficients of an uploaded Batch's slot (lossless transcode).
        MijError with the reason for a picture that is not transcodable.  The batch must stay as it is until wait() or a fetch.
        orientation 1..8 and trim: mij_enc_add_coef_oriented, the coefficients reoriented on the way (the slot's plan, units and stream
        are the destination's); MijError with the reason for a picture the edge mode refuses.
        tables = (luma, chroma), 64 entries 1..255 each in zigzag order: mij_enc_add_coef_requant, the coefficients requantised to those
        tables (their entry-wise maximum with the source's when coarsen_only) after the orientation.
        crop = (x0, y0, w, h) in the displayed frame and / or grey=True: mij_enc_add_coef_window, in the order grey -> orient -> crop ->
        requantise; slot_rect(slot) is the kept rectangle.  MijError with the reason for a window outside the picture."""
        L = lib()
        if crop is not None or grey:
            luma, chroma = (None, None) if tables is None else _qtable_pair(tables)
            win = None if crop is None else (C.c_int * 4)(*[int(v) for v in crop])
            L.mij_enc_add_coef_window.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_char_p,
                                                  C.c_char_p, C.c_int, C.POINTER(C.c_int)]
            return _check(L.mij_enc_add_coef_window(self._h, batch._h, int(slot), int(orientation), int(bool(trim)), win, int(bool(grey)), luma,
                                                    chroma, int(bool(coarsen_only)), None), "mij_enc_add_coef_window")
        if tables is not None:
            luma, chroma = _qtable_pair(tables)
            L.mij_enc_add_coef_requant.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
            return _check(L.mij_enc_add_coef_requant(self._h, batch._h, int(slot), int(orientation), int(bool(trim)), luma, chroma,
                                                     int(bool(coarsen_only))), "mij_enc_add_coef_requant")
        if orientation == 1 and not trim:
            L.mij_enc_add_coef.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            return _check(L.mij_enc_add_coef(self._h, batch._h, int(slot)), "mij_enc_add_coef")
        L.mij_enc_add_coef_oriented.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        return _check(L.mij_enc_add_coef_oriented(self._h, batch._h, int(slot), int(orientation), int(bool(trim))), "mij_enc_add_coef_oriented")

    def slot_rect(self, slot):
        """mij_enc_slot_rect: the rectangle (x0', y0', W', H') of the displayed picture a coefficient slot keeps: the crop with its origin
        moved down to the MCU grid, the whole picture where none was asked"""
        L = lib()
        L.mij_enc_slot_rect.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        r = (C.c_int * 4)()
        _check(L.mij_enc_slot_rect(self._h, int(slot), r), "mij_enc_slot_rect")
        return tuple(r)

    def slot_greyed(self, slot):
        """mij_enc_slot_greyed: whether add_coef's grey dropped the chroma of a colour source"""
        L = lib()
        L.mij_enc_slot_greyed.argtypes = [C.c_void_p, C.c_int]
        return bool(_check(L.mij_enc_slot_greyed(self._h, int(slot)), "mij_enc_slot_greyed"))

    def slot_windowed(self, slot):
        """mij_enc_slot_windowed: whether add_coef's crop or grey changed the picture (false: the slot is converted as it was without them)"""
        L = lib()
        L.mij_enc_slot_windowed.argtypes = [C.c_void_p, C.c_int]
        return bool(_check(L.mij_enc_slot_windowed(self._h, int(slot)), "mij_enc_slot_windowed"))

    def coef_tiles(self):
        """mij_enc_coef_tiles: the 64-block plane tiles the last upload queued for conversion, over all its coefficient slots"""
        L = lib()
        L.mij_enc_coef_tiles.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        n = C.c_uint32()
        _check(L.mij_enc_coef_tiles(self._h, C.byref(n)), "mij_enc_coef_tiles")
        return int(n.value)

    def slot_requantized(self, slot):
        """mij_enc_slot_requantized: whether add_coef's tables changed an entry of the slot's plan (false: a plain lossless slot)"""
        L = lib()
        L.mij_enc_slot_requantized.argtypes = [C.c_void_p, C.c_int]
        return bool(_check(L.mij_enc_slot_requantized(self._h, int(slot)), "mij_enc_slot_requantized"))

    def tplan(self, slot):
        """mij_enc_tplan: the TranscodePlan of a slot made by add_coef, or by add / add_device / add_device_float with a sampling or tables"""
        L = lib()
        L.mij_enc_tplan.argtypes = [C.c_void_p, C.c_int, C.POINTER(TranscodePlan)]
        t = TranscodePlan()
        _check(L.mij_enc_tplan(self._h, int(slot), C.byref(t)), "mij_enc_tplan")
        return t

    def slot_status(self, slot):
        """mij_enc_slot_status, after fetch_streams -> "ok", "no room" (finish it on the host from its units), "uncodable" or "host flush"
        (a progressive slot with a forced EOB-run flush or a table that cannot be built: the host finishes it too)"""
        L = lib()
        L.mij_enc_slot_status.argtypes = [C.c_void_p, C.c_int]
        return ("ok", "no room", "uncodable", "host flush")[_check(L.mij_enc_slot_status(self._h, int(slot)), "mij_enc_slot_status")]

    def coef_ms(self):
        """ms the conversion kernels (planes -> units) of the last upload took, None when there were none"""
        L = lib()
        L.mij_enc_coef_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        ms = C.c_float()
        _check(L.mij_enc_coef_ms(self._h, C.byref(ms)), "mij_enc_coef_ms")
        return None if ms.value < 0 else ms.value

    def set_optimize(self, slot, on=True):
        """mij_enc_set_optimize: the slot's stream gets Huffman tables built from its own symbol statistics; before upload."""
        L = lib()
        L.mij_enc_set_optimize.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _check(L.mij_enc_set_optimize(self._h, int(slot), int(bool(on))), "mij_enc_set_optimize")

    def set_restart(self, slot, restart_mcus):
        """mij_enc_set_restart: the slot's stream gets a restart interval of that many MCUs (0 or None: none); before upload."""
        L = lib()
        L.mij_enc_set_restart.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _check(L.mij_enc_set_restart(self._h, int(slot), _restart_mcus(restart_mcus)), "mij_enc_set_restart")

    def set_progressive(self, slot, on=True):
        """mij_enc_set_progressive: the slot's stream is written as a progressive stream (include/mij_host.h, PROGRESSIVE STREAMS); before
        upload.  MijError for a slot with a restart interval."""
        L = lib()
        L.mij_enc_set_progressive.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _check(L.mij_enc_set_progressive(self._h, int(slot), int(bool(on))), "mij_enc_set_progressive")

    def set_arith(self, slot, arith=MIJ_ARITH_LIBJPEG):
        """mij_enc_set_arith: MIJ_ARITH_LIBJPEG (or "libjpeg") gives the slot libjpeg's arithmetic and header (include/mij_host.h, LIBJPEG
        ENCODING: Pillow's file byte for byte), MIJ_ARITH_STB (or "stb", the default) the reference's; before upload.  MijError for slots of
        units or coefficients, "440" and pictures of 2 or 4 channels."""
        L = lib()
        L.mij_enc_set_arith.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _check(L.mij_enc_set_arith(self._h, int(slot), int(ARITHMETICS.get(arith, arith))), "mij_enc_set_arith")

    def slot_arith(self, slot):
        """mij_enc_slot_arith: MIJ_ARITH_STB or MIJ_ARITH_LIBJPEG"""
        L = lib()
        L.mij_enc_slot_arith.argtypes = [C.c_void_p, C.c_int]
        return _check(L.mij_enc_slot_arith(self._h, int(slot)), "mij_enc_slot_arith")

    def group_work(self):
        """mij_enc_group_work of every group: the work items the last upload queued per transform kernel of the kernel table"""
        L = lib()
        L.mij_enc_group_work.argtypes = [C.c_void_p, C.c_int]
        return [_check(L.mij_enc_group_work(self._h, g), "mij_enc_group_work") for g in range(ENC_GROUPS)]

    def slot_progressive(self, slot):
        """mij_enc_slot_progressive: whether progressive output was asked for the slot"""
        L = lib()
        L.mij_enc_slot_progressive.argtypes = [C.c_void_p, C.c_int]
        return bool(_check(L.mij_enc_slot_progressive(self._h, int(slot)), "mij_enc_slot_progressive"))

    def slot_restart(self, slot):
        """mij_enc_slot_restart: the slot's restart interval in MCUs, 0 when it has none"""
        L = lib()
        L.mij_enc_slot_restart.argtypes = [C.c_void_p, C.c_int]
        return _check(L.mij_enc_slot_restart(self._h, int(slot)), "mij_enc_slot_restart")

    def slot_optimized(self, slot):
        """mij_enc_slot_optimized, after fetch_streams: True when the slot's stream carries its own tables, False when optimisation
        was not asked for it or it fell back to the plain tables."""
        L = lib()
        L.mij_enc_slot_optimized.argtypes = [C.c_void_p, C.c_int]
        return bool(_check(L.mij_enc_slot_optimized(self._h, int(slot)), "mij_enc_slot_optimized"))

    def stream_reserve(self, nbytes):
        """mij_enc_stream_reserve: the GPU emission arena (0 releases it); before upload."""
        L = lib()
        L.mij_enc_stream_reserve.argtypes = [C.c_void_p, C.c_size_t]
        _check(L.mij_enc_stream_reserve(self._h, C.c_size_t(nbytes)), "mij_enc_stream_reserve")

    def fetch_streams(self):
        """mij_enc_fetch_streams: waits, brings the streams back; -> the number of slots that fit."""
        L = lib()
        L.mij_enc_fetch_streams.argtypes = [C.c_void_p]
        return _check(L.mij_enc_fetch_streams(self._h), "mij_enc_fetch_streams")

    def stream(self, slot):
        """mij_enc_stream -> (bytes, length), or (None, the length it needs) for a slot that did not fit."""
        L = lib()
        L.mij_enc_stream.restype = C.c_void_p
        L.mij_enc_stream.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
        n = C.c_size_t()
        p = L.mij_enc_stream(self._h, int(slot), C.byref(n))
        return (C.string_at(p, n.value) if p else None), n.value

    def timer_begin(self):
        _check(lib().mij_enc_timer_begin(self._h), "mij_enc_timer_begin")

    def timer_end(self):
        _check(lib().mij_enc_timer_end(self._h), "mij_enc_timer_end")

    def timer_ms(self):
        ms = C.c_float()
        _check(lib().mij_enc_timer_elapsed_ms(self._h, C.byref(ms)), "mij_enc_timer_elapsed_ms")
        return ms.value

    def close(self):
        if self._h:
            lib().mij_enc_destroy(self._h)
            self._h = C.c_void_p()
