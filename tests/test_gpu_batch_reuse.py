"""One decode batch over several uploads (mij_batch_reset, mij_batch_upload, mij_batch_launch): the work list, the five output plans, the
scratch planes and the per-slot tables are kept from upload to upload and reallocated when an upload outgrows them, which no test of a
single feature sees.  A first batch with one slot of every kind the upload code distinguishes, a second one large enough to reallocate
every list (the growth rule is need + need / 2 + 64; the scratch planes take exactly what is needed), the first one again in lists larger
than it needs, and two more slots added to it without a reset.  After each launch every slot's pixels are the CPU decoder's byte for byte,
every float and tensor output is the model's of the test of its feature, and batches 1 and 3 report the same kernels and rectangles.

What the test restates from the runtime to prove that batch 2 reallocates (mij_runtime.hip: lay_out_work, l1_prepack, plan_put and the
*_plan functions; mij_kernels.h):
    work list    pack list + every family list.  A slot's own list: mij_batch_slot_work_items; the pack list: one item per 256 blocks of
                 whole 64-block tiles per component of each host-staged slot that is packed on the device; pass 1 of a two-pass slot: one item
                 per 256 blocks per component.  l1_prepack puts the tiles of the progressive slots into the same list first.
    float plan   256-aligned 32-byte descriptors + 4096 table bytes per request + 8 bytes per 32768 output bytes
    tensor plans each of the four holds a descriptor (at most 256 bytes) and 4096 table bytes for every tensor request of the batch, the
                 coefficients of its resized requests (out * (2 + taps) * 4 bytes an axis) and at most one 16-byte work item per output pixel
"""
import numpy as np
import pytest
import torch

import loadf_expect as fx
import orient_model as om
import resize_model as rm
import scaled_model as SM
import tensor_model as tm
from roi_cases import dense

pytestmark = pytest.mark.gpu

MB = 1 << 20
MAX_SLOTS = 64
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SENTINEL = -3.0
# the four forms of a tensor request: (resized, orientation)
FORMS = {"plain": (False, 1), "resized": (True, 1), "plain_t": (False, 6), "resized_t": (True, 7)}


def grow(n):
    return n + n // 2 + 64


def progressive(ica, helpers, w, h, seed):
    """a progressive file whose L1 bound the host walk leaves to the device (as test_gpu_compact.py builds them)"""
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)
    plan, du = ica.host_transform(img, 92)
    return helpers.progressive_from_du(plan, du.copy(), 1)


def first_batch(ica, helpers):
    """one slot of every kind: (kind, picture, argument).  Pictures: a JPEG's bytes, or a coef_cases.Case"""
    j = ica.synth_jpeg
    return [
        ("walk", j(64, 48, 1, 90), None),
        ("host", j(48, 32, 2, 90), None),
        ("compact", j(33, 17, 3, 90), None),
        ("prog", progressive(ica, helpers, 40, 24, 4), None),
        ("clone", None, 1),
        ("two_pass", dense("411", (16, 16)), None),
        ("roi", dense("444", (64, 48)), (17, 9, 20, 14)),
        ("scale", dense("420", (48, 32)), 2),
        ("f32", j(40, 24, 5, 90), None),
        ("plain", j(48, 32, 6, 90), (3, 2, 24, 16)),
        ("resized", j(48, 32, 7, 90), ((3, 2, 24, 16), (8, 6), "bilinear")),
        ("plain_t", j(48, 32, 8, 90), (2, 3, 16, 24)),
        ("resized_t", j(48, 32, 9, 90), ((2, 3, 16, 24), (6, 8), "lanczos")),
    ]


def second_batch(ica, helpers):
    """outgrows every list of the first: 256 x 256 pictures, packed on the device; a 256 x 256 two-pass picture; three float requests; five
    tensor requests of each form"""
    j = ica.synth_jpeg
    big = [j(256, 256, 20 + k, 90) for k in range(3)]
    specs = [("walk", j(256, 256, 11, 90), None), ("two_pass", dense("411", (256, 256)), None), ("prog", progressive(ica, helpers, 120, 88, 12), None),
             ("roi", dense("444", (256, 256)), (100, 50, 60, 90)), ("scale", dense("420", (256, 256)), 4)]
    specs += [("host", big[k % 3], None) for k in range(24)]
    specs += [("clone", None, 5)]
    specs += [("f32", big[k], None) for k in range(3)]
    for k in range(5):
        specs += [("plain", big[k % 3], (5 + k, 7, 200, 100)), ("resized", big[k % 3], ((5, 7 + k, 200, 100), (50, 30), rm.FILTERS[k % len(rm.FILTERS)])),
                  ("plain_t", big[k % 3], (7, 5 + k, 100, 200)), ("resized_t", big[k % 3], ((7 + k, 5, 100, 200), (30, 50), rm.FILTERS[(k + 2) % len(rm.FILTERS)]))]
    assert len(specs) <= MAX_SLOTS
    return specs


class Filled:
    """a batch's slots after add: per spec its slot, what its outputs must equal, and the device tensors its requests write"""

    def __init__(self):
        self.slots, self.kinds, self.want_px, self.checks, self.packed, self.prog = [], [], [], [], [], []


_px = {}


def pixels(oracle, pic):
    """the CPU decoder's picture: computed once per picture, shared, never changed"""
    data = pic if isinstance(pic, bytes) else pic.stream()
    if data not in _px:
        kind, px, _ = oracle.load(data, 3)
        assert kind == "ok"
        px.setflags(write=False)
        _px[data] = px
    return _px[data]


def add_slots(ica, oracle, b, specs, f, first=0):
    """adds specs[first:] to the batch: the slot walked on the GPU first (the walk runs before the host-staged slots are added)"""
    for kind, pic, arg in specs[first:]:
        if kind == "walk":
            st, slot = b.add_jpeg_stream(pic, 3)
            assert st == 1
            assert b.entropy_run() == []
        elif kind == "clone":
            slot = b.add_clone(f.slots[arg])
            pic = specs[arg][1]
        elif kind in ("host", "two_pass"):
            slot = b.add_jpeg(pic if isinstance(pic, bytes) else pic.stream(), 3, stage="int16")
            f.packed.append(slot)
        else:
            slot = b.add_jpeg(pic if isinstance(pic, bytes) else pic.stream(), 3)
        px = pixels(oracle, pic)
        H, W = px.shape[:2]
        check = None
        if kind == "prog":
            assert b.slot_flags(slot) & 16, "the walk did not leave the L1 bound to the device"
            f.prog.append(slot)
        elif kind == "roi":
            b.set_roi(slot, *arg)
        elif kind == "scale":
            b.set_scale(slot, arg)
            px = SM.scaled_picture(pic.dequantised(), pic.layout, (pic.w, pic.h), arg, 3)
        elif kind == "f32":
            b.set_out_f32(slot)
            check = ("f32", fx.apply(fx.lut(3), px))
        elif kind in FORMS:
            resized, o = FORMS[kind]
            win, size, name = arg if resized else (arg, None, None)
            t = tm.tables(3, torch.float32, MEAN, STD)
            d = om.orient(px, o)
            if resized:
                want = rm.window(d, win, size[::-1], name, False, True, "CHW", t, torch.float32)
                dst = torch.full((3, size[1], size[0]), SENTINEL, dtype=torch.float32, device="cuda:0")
                b.set_out_tensor_resized(slot, dst.data_ptr(), "f32", "CHW", *win, size[0], size[1], size[0], size[0] * size[1], False, True, t.numpy(), name,
                                         orientation=o)
            else:
                want = tm.window(d, win, False, True, "CHW", t, torch.float32)
                dst = torch.full((3, win[3], win[2]), SENTINEL, dtype=torch.float32, device="cuda:0")
                b.set_out_tensor(slot, dst.data_ptr(), "f32", "CHW", *win, win[2], win[2] * win[3], False, True, t.numpy(), orientation=o)
            check = ("tensor", want, dst)
        f.slots.append(slot)
        f.kinds.append((kind, arg))
        f.want_px.append(px)
        f.checks.append(check)
    torch.cuda.synchronize()


def check_outputs(b, f, tag):
    for i, slot in enumerate(f.slots):
        kind, arg = f.kinds[i]
        t = (tag, i, kind)
        got, want = b.fetch(slot), f.want_px[i]
        if kind == "roi":  # a window: the pixels inside it, and the rectangle the upload decodes holds it without being the picture
            x0, y0, w, h = arg
            rx, ry, rw, rh = b.roi_rect(slot)
            assert rx <= x0 and ry <= y0 and rx + rw >= x0 + w and ry + rh >= y0 + h and (rw, rh) != want.shape[1::-1], t
            got, want = got[y0:y0 + h, x0:x0 + w], want[y0:y0 + h, x0:x0 + w]
        assert got.shape == want.shape and np.array_equal(got, want), t
        if f.checks[i] is None:
            continue
        if f.checks[i][0] == "f32":
            assert fx.same_bits(b.fetch_f32(slot), f.checks[i][1]), t
        else:
            assert tm.same_bits(f.checks[i][2], f.checks[i][1]), t


def blocks_per_component(d):
    return [d.comp[c].bw * d.comp[c].bh for c in range(d.ncomp)]


def work_total(b, f):
    """the work list of the last upload, counted as this module's docstring says"""
    n = sum(b.work_items(s) for s in f.slots)
    for s in f.packed:
        n += sum(-(-(-(-nb // 64) * 64) // 256) for nb in blocks_per_component(b._desc(s)))
    for s in f.slots:
        if b.slot_path(s) == 2:
            n += sum(-(-nb // 256) for nb in blocks_per_component(b._desc(s)))
    return n


def prepack_total(b, f):
    return sum(-(-(-(-nb // 64) * 64) // 256) for s in f.prog for nb in blocks_per_component(b._desc(s)))


def choices(b, f):
    return [(b.slot_kernel(s), b.slot_path(s), b.roi_rect(s)) for s in f.slots]


def f32_plan_bytes(f):
    n = sum(1 for k, _ in f.kinds if k == "f32")
    return -(-32 * n // 256) * 256 + 4096 * n + 8 * sum(-(-f.want_px[i].size // 32768) for i, (k, _) in enumerate(f.kinds) if k == "f32")


def tensor_plan_bounds(f):
    """(at most, at least) the bytes of any one of the four tensor plans of this batch"""
    reqs = [arg for k, arg in f.kinds if k in FORMS]
    most = (256 + 4096) * len(reqs)
    for k, arg in f.kinds:
        if k in FORMS and FORMS[k][0]:
            (_, _, w, h), (ow, oh), _ = arg
            most += 4 * (ow * (2 + 2 * w + 8) + oh * (2 + 2 * h + 8)) + 16 * ow * oh  # taps of an axis: fewer than 2 * in + 8
        elif k in FORMS:
            most += 16 * arg[2] * arg[3]
    return most, 4096 * len(reqs)


def test_one_batch_four_uploads(ica, oracle, gpu_ctx):
    import helpers
    specs1, specs2 = first_batch(ica, helpers), second_batch(ica, helpers)
    b = ica.Batch(gpu_ctx, MAX_SLOTS, 32 * MB, 32 * MB, 32 * MB)
    try:
        b.entropy_reserve(2 * MB)
        b.reserve_out_f32(64 << 10)

        f1 = Filled()
        add_slots(ica, oracle, b, specs1, f1)
        b.upload()
        b.launch()
        b.wait()
        check_outputs(b, f1, "batch 1")
        n1, pre1, chosen1 = work_total(b, f1), prepack_total(b, f1), choices(b, f1)
        kinds1 = {c[0][0] for c in chosen1}
        assert any(c[1] == 2 for c in chosen1) and any(c[1] == 8 for c in chosen1), chosen1
        assert any(k and k.endswith("R") for k in kinds1), ("no windowed kernel", kinds1)

        b.reset()
        b.reserve_out_f32(4 * MB)  # the float arena grows between the batches
        f2 = Filled()
        add_slots(ica, oracle, b, specs2, f2)
        b.upload()
        n2 = work_total(b, f2)
        # batch 2 cannot fit what batch 1 left: the work list, the float plan, every tensor plan; the scratch planes take exactly the need
        assert n2 > grow(max(n1, pre1)), (n1, pre1, n2)
        assert f32_plan_bytes(f2) > grow(f32_plan_bytes(f1)), (f32_plan_bytes(f1), f32_plan_bytes(f2))
        assert tensor_plan_bounds(f2)[1] > grow(tensor_plan_bounds(f1)[0]), (tensor_plan_bounds(f1), tensor_plan_bounds(f2))
        assert all(sum(1 for k, _ in f.kinds if k == form) >= 1 for f in (f1, f2) for form in FORMS)
        b.launch()
        b.wait()
        check_outputs(b, f2, "batch 2")

        b.reset()
        f3 = Filled()
        add_slots(ica, oracle, b, specs1, f3)
        b.upload()
        b.launch()
        b.wait()
        check_outputs(b, f3, "batch 3")
        assert choices(b, f3) == chosen1
        assert work_total(b, f3) == n1

        # two more slots without a reset: another host-staged picture and a clone of it
        more = specs1 + [("host", ica.synth_jpeg(80, 56, 30, 90), None), ("clone", None, len(specs1))]
        add_slots(ica, oracle, b, more, f3, first=len(specs1))
        b.upload()
        b.launch()
        b.wait()
        check_outputs(b, f3, "batch 4")
        assert choices(b, f3)[:len(specs1)] == chosen1
    finally:
        b.close()
