"""Sources for the lossless-transcode tests (host and GPU): (name, bytes) lists made with the helpers that exist."""
import functools

import numpy as np

import helpers
import header_cases as hc

FIXED_SIZES = ((1, 1), (8, 8), (16, 16), (17, 9), (33, 31), (80, 80))


def _ica():
    import image_codecs_amd as ica
    return ica


@functools.lru_cache(maxsize=None)
def writer_sources():
    """[(name, source bytes, picture, quality)]: the project's writer at q = 90 (4:2:0) and q = 95 (4:4:4)"""
    ica = _ica()
    out = []
    for q in (90, 95):
        for (w, h) in FIXED_SIZES:
            img = ica.synth_rgb(w, h, seed=w + h)
            out.append(("writer q%d %dx%d" % (q, w, h), ica.stbi_write_jpg_to_memory(img, q), img, q))
    return out


def _plan444(w, h, seed=5):
    ica = _ica()
    return ica.host_transform(ica.synth_rgb(w, h, seed=seed), 95)


@functools.lru_cache(maxsize=None)
def layout_sources():
    """[(name, bytes)]: every transcodable layout, baseline with and without restart intervals, progressive, grey; odd sizes, sizes
    that are no MCU multiple, and the seams the device path has (128-unit emission tiles, 64-block plane tiles)"""
    ica = _ica()
    out = []
    for hv, sizes in (((2, 1), ((40, 24), (33, 31))), ((1, 2), ((24, 40), (33, 31))), ((2, 2), ((80, 80), (17, 9))), ((1, 1), ((56, 56), (9, 7)))):
        for (w, h) in sizes:
            plan, du = _plan444(w, h)
            for rst in (0, 3):
                out.append(("baseline %dx%d luma %dx%d rst %d" % (w, h, hv[0], hv[1], rst),
                            helpers.baseline_layout_from_444(plan, du, [hv, (1, 1), (1, 1)], restart_mcus=rst)))
    for (w, h) in ((64, 64), (72, 64), (33, 20)):
        plan, du = _plan444(w, h)
        out.append(("baseline grey %dx%d" % (w, h), helpers.baseline_from_du(plan, du, layout="grey")))
    plan, du = ica.host_transform(ica.synth_rgb(50, 38, seed=2), 90)
    out.append(("progressive 4:2:0 50x38", helpers.progressive_from_du(plan, du)))
    plan, du = _plan444(41, 23)
    out.append(("progressive 4:4:4 41x23", helpers.progressive_from_du(plan, du)))
    out.append(("progressive 4:2:2 41x23", helpers.progressive_422_from_444(plan, du)))
    out.append(("progressive grey 41x23", helpers.progressive_grey_from_444(plan, du)))
    return out


def golden_sources(golden):
    """the transcodable files among the goldens"""
    ica = _ica()
    out = []
    for name in golden.names:
        data = golden.jpg(name)
        try:
            desc, _ = ica.HostDecoder.decode(data, 0)
        except ica.MijError:
            continue
        if ica.transcode_plan(desc)[0] is not None:
            out.append(("golden " + name, data))
    return out


@functools.lru_cache(maxsize=None)
def escaped_source():
    """a q = 100 high-contrast picture: blocks with coefficients beyond a byte"""
    ica = _ica()
    return ica.stbi_write_jpg_to_memory(ica.synth_rgb_edges(72, 56, seed=1), 100)


def planes_source(w, h, hv, edit, seed=3):
    """a baseline stream of layout hv through the test-side writer (optimal tables, so any magnitude can be coded) from tame planes that
    `edit` changes in place"""
    planes = hc.tame(w, h, hv, seed)
    edit(planes)
    return hc.plain(w, h, hv, planes).bytes()


def different_chroma_tables(w=24, h=16):
    """4:4:4 with a third quantisation table for Cr whose contents differ from Cb's"""
    q2 = tuple(2 if k == 5 else 1 for k in range(64))
    return hc.plain(w, h, [(1, 1)] * 3, tq=[0, 1, 2], qt={2: q2}, seed=4).bytes()


def wide_table_entry(w=24, h=16):
    """4:4:4 whose luma quantisation table is written with 16-bit entries, one of them 300"""
    data = hc.plain(w, h, [(1, 1)] * 3, seed=6).bytes()
    i = data.index(b"\xff\xdb\x00\x43\x00")
    vals = [300 if k == 7 else v for k, v in enumerate(data[i + 5:i + 69])]
    seg = b"\xff\xdb\x00\x83\x10" + b"".join(bytes([v >> 8, v & 255]) for v in vals)
    return data[:i] + seg + data[i + 69:]
