"""image-codecs_amd -- Python view of the MI355X-native JPEG path (ctypes over the C-ABI).

The product is the shared library ``lib/libimagecodecs_mi355x.so`` built from ``csrc/``:
  * ``stbi_*``  the reference's public surface (include/image_api.h; reference definitions in
                convert.c:188-266,286-336,402-411, image_api.c:74-145, codec/jpeg_write.c:368-388),
  * ``mij_*``   the GPU back end's C-ABI (include/mij.h; replaces the kernel seam
                codec/jpeg.c:83-85),
  * ``mjh_*``   the host entropy decoder (csrc/jpeg_entropy.h; codec/jpeg.c:88-558,1119-1756).
This module only binds those entry points so that tests and bench.py read like calls into the
reference: same names, same argument meaning, same error behaviour.  It never computes pixels
itself and it has no CPU fallback: without the library (or, for decode, without a gfx950 GPU)
calls fail loudly.

Because the directory name contains a hyphen the package is imported through the
``image_codecs_amd`` shim at the repository root (``import image_codecs_amd as ica``).
"""
from .binding import (  # noqa: F401
    LIB_PATH,
    MijError,
    ImageDesc,
    Batch,
    OutTensor,
    OutResize,
    OutPlane,
    OutPlanes,
    FILTERS,
    MIJ_FILTER_BOX,
    MIJ_FILTER_BILINEAR,
    MIJ_FILTER_HAMMING,
    MIJ_FILTER_BICUBIC,
    MIJ_FILTER_LANCZOS,
    resize_coeffs,
    exif_orientation,
    exif_set_orientation,
    MIJ_DT_U8,
    MIJ_DT_F16,
    MIJ_DT_BF16,
    MIJ_DT_F32,
    MIJ_LAYOUT_HWC,
    MIJ_LAYOUT_CHW,
    MIJ_ARITH_STB,
    MIJ_ARITH_LIBJPEG,
    Context,
    Encoder,
    InTensor,
    InConvert,
    PinnedBuffer,
    host_transform,
    emit_jpeg,
    TranscodePlan,
    MJW_COPY_MARKERS,
    transcode_plan,
    transcode_header,
    units_from_region,
    units_codable,
    emit_transcoded,
    copy_markers,
    transcode_memory,
    transcode_plan_oriented,
    units_orient,
    transcode_plan_grey,
    units_grey,
    transcode_plan_cropped,
    units_crop,
    quality_tables,
    SAMPLINGS,
    sampling_factors,
    sampling_name,
    sampled_plan,
    host_transform_sampled,
    write_jpg_sampled_to_memory,
    ARITHMETICS,
    ENC_GROUPS,
    libjpeg_plan,
    host_transform_libjpeg,
    host_transform_libjpeg_planes,
    libjpeg_quantise_all,
    libjpeg_reframe,
    write_jpg_libjpeg_to_memory,
    plane_shapes,
    split_planes,
    planes_plan,
    video_range_convert,
    host_transform_planes,
    write_jpg_planes_to_memory,
    requant_magic,
    transcode_plan_requant,
    units_requant,
    write_histogram,
    optimal_huffman_table,
    MJW_OPTIMIZE_HUFFMAN,
    mij_write_jpg_to_memory,
    mij_write_jpg_batch,
    HostDecoder,
    lib,
    build_library,
    stbi_failure_reason,
    stbi_info_from_memory,
    stbi_load,
    stbi_load_from_memory,
    stbi_load_from_callbacks,
    stbi_load_from_file,
    stbi_info,
    stbi_info_from_file,
    stbi_info_from_callbacks,
    stbi_write_jpg,
    stbi_load_16_from_memory,
    stbi_loadf,
    stbi_loadf_from_memory,
    stbi_loadf_from_file,
    stbi_loadf_from_callbacks,
    stbi_ldr_to_hdr_gamma,
    stbi_ldr_to_hdr_scale,
    stbi_hdr_to_ldr_gamma,
    stbi_hdr_to_ldr_scale,
    ldr_to_hdr_lut,
    stbi_set_flip_vertically_on_load,
    stbi_write_jpg_to_memory,
    detile_coefficients,
    host_decode_staged,
    host_decode_rows,
    compact_offsets,
    expand_compact_region,
    decode_jpegs_multi,
    gpu_available,
)
from .synth import synth_rgb, synth_jpeg, synth_rgb_edges  # noqa: F401

_TENSOR_OUT = ("TensorDecoder", "tensor_tables", "ycbcr_subsampling")
_TENSOR_ENCODE = ("TensorEncoder",)
_TRANSCODE = ("Transcoder",)


def __getattr__(name):
    """TensorDecoder and tensor_tables live in tensor_out, TensorEncoder in tensor_encode; both import torch and are loaded on first
    use, so that importing the package does not import torch."""
    if name in _TENSOR_OUT:
        from . import tensor_out
        return getattr(tensor_out, name)
    if name in _TENSOR_ENCODE:
        from . import tensor_encode
        return getattr(tensor_encode, name)
    if name in _TRANSCODE:  # no torch behind this one; loaded on first use like the other front ends
        from . import transcode
        return getattr(transcode, name)
    raise AttributeError("module 'image_codecs_amd' has no attribute %r" % name)
