"""Shared by the plane-output tests (include/mij.h, PLANE OUTPUT): the pictures, their planes by the model (computed once, shared, never
changed) and the sizes the kernel's paths turn on."""
import coef_cases as CC
import planes_out_model as PM
from roi_cases import dense

# 1 x 1; 8 x 8 (4:2:0: the second luma block column and row hold no sample); 17 x 9 (the last chroma block of 4:2:0 holds one column);
# 33 x 17; 267 x 69 (4:2:0: 34 x 9 = 306 luma blocks that hold samples of 340 in the plane -- more than one work item of 256 lanes --
# and 17 x 5 = 85 chroma blocks: more than one wavefront)
SIZES = ((1, 1), (8, 8), (17, 9), (33, 17), (267, 69))
BIG = (267, 69)
LAYOUTS = ("420", "422", "440", "444", "grey", "411", "cmyk")

_cache = {}


def hv_of(layout):
    return CC.LAYOUTS[layout][0]


def planes_of(oracle, case):
    """the model's planes of a coef_cases.Case, read-only"""
    k = ("planes", case.name)
    if k not in _cache:
        if "idct" not in _cache:
            _cache["idct"] = PM.Idct(oracle)
        pl = PM.planes_of_case(_cache["idct"], case, hv_of(case.layout))
        for p in pl:
            p.setflags(write=False)
        _cache[k] = pl
    return _cache[k]


def stream_planes(oracle, data):
    """the model's planes of a real file, read-only -> (planes, (W, H, hv, progressive))"""
    k = ("stream", hash(bytes(data)), len(data))
    if k not in _cache:
        if "idct" not in _cache:
            _cache["idct"] = PM.Idct(oracle)
        pl, geo = PM.planes_of_stream(_cache["idct"], data)
        for p in pl:
            p.setflags(write=False)
        _cache[k] = (pl, geo)
    return _cache[k]


def picture(layout, size, seed=0):
    """roi_cases.dense: every position in use, every seventh block escaped"""
    return dense(layout, tuple(size), seed)
