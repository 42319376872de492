"""Reduced-size decode on the GPU (mij_batch_set_scale, k_scaled of mij_scaled_kernels.h, TensorDecoder.decode(reduce=...)): every
picture bit for bit against tests/scaled_model.py applied to the planes the picture was written from (coef_cases), for every layout
the feature serves, scales 2, 4 and 8, both plane formats and both producers of coefficient planes (host walk, GPU walk)."""
import ctypes as C

import numpy as np
import pytest
import torch

import coef_cases as CC
import idct_model as M
import orient_model as om
import resize_model as rm
import scaled_model as SM
import tensor_model as tm

pytestmark = pytest.mark.gpu

MB = 1 << 20
MIJ_E_ARG, MIJ_E_STATE = -2, -5
SCALES = (2, 4, 8)
PRODUCERS = (("host", "compact"), ("host", "int16"), ("walk", "compact"), ("walk", "int16"))
SIZES = {"420": ((1, 1), (15, 17), (33, 16), (1043, 37), (2064, 16)), "422": ((15, 9), (1043, 21)), "444": ((7, 9), (523, 19)), "grey": ((7, 9), (523, 19))}
LAYOUTS = ("420", "422", "444", "grey")

_model = {}


def _want(case, s, req):
    """the model's picture of a case: computed once, shared, never changed"""
    k = (case.name, s, req)
    if k not in _model:
        n_out = req if req else (1 if case.layout == "grey" else 3)
        px = SM.scaled_picture(case.dequantised(), case.layout, (case.w, case.h), s, n_out)
        px.setflags(write=False)
        _model[k] = px
    return _model[k]


def dense(layout, size, seed=0, restart=0):
    """every position of every block in use: small values, a DC ramp, and every seventh block with values beyond a byte (escaped)"""
    w, h = size
    r = np.random.default_rng(1000 * seed + w * 7 + h)
    planes = CC.blank(layout, w, h)
    for pl in planes:
        bh, bw, _ = pl.shape
        pl[:] = r.integers(-9, 10, pl.shape)
        pl[:, :, 0] = r.integers(-300, 301, (bh, bw))
        i = np.arange(bh * bw).reshape(bh, bw)
        pl[:, :, 1:6] += np.where((i % 7 == 3)[:, :, None], r.integers(-700, 701, (bh, bw, 5)), 0).astype(np.int16)
    return CC.Case("dense_%s_%dx%d_%d_r%d" % (layout, w, h, seed, restart), "dense", layout, w, h, planes, restart=restart)


def _fill(ica, ctx, cases, req, producer, fmt):
    """-> (batch, slot per case); the GPU walk takes what it serves, the host walk the rest (and what the walk hands back)"""
    b = ica.Batch(ctx, len(cases), 64 * MB, 64 * MB, 64 * MB)
    b.set_coef_format(fmt)
    if producer == "host":
        return b, [b.add_jpeg(c.stream(), req) for c in cases]
    b.entropy_reserve(16 * MB)
    slots, later = [None] * len(cases), []
    for i, c in enumerate(cases):
        st, slot = b.add_jpeg_stream(c.stream(), req)
        assert st in (1, 2), (c.name, st)
        if st == 1:
            slots[i] = slot
        else:
            assert c.progressive is not None, c.name
            later.append(i)
    for s in b.entropy_run():
        c = cases[slots.index(s)]
        b.fallback_prepare(s)
        d2, _ = ica.HostDecoder.decode(c.stream(), req, out=b.staging(s))
        if d2.flags:
            b.set_flags(s, d2.flags)
    for i in later:
        slots[i] = b.add_jpeg(cases[i].stream(), req)
    return b, slots


def _check(ica, ctx, cases, reqs=(3,), producers=PRODUCERS, scales=SCALES):
    for req in reqs:
        for producer, fmt in producers:
            for s in scales:
                b, slots = _fill(ica, ctx, cases, req, producer, fmt)
                try:
                    for sl in slots:
                        b.set_scale(sl, s)
                    b.submit()
                    b.wait()
                    for case, sl in zip(cases, slots):
                        tag = (case.name, "s %d" % s, "req %d" % req, producer, fmt)
                        assert b.slot_path(sl) == 8, tag
                        assert b.slot_coef_bytes(sl) == (1 if fmt == "compact" else 0), tag
                        want = _want(case, s, req)
                        assert b.out_size(sl) == (want.shape[1], want.shape[0]), tag
                        got = b.fetch(sl)
                        assert got.shape == want.shape and np.array_equal(got, want), tag + (int((got != want).sum()),)
                finally:
                    b.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_sizes_channels_formats_producers(ica, gpu_ctx, layout):
    """every size of the layout (one MCU, odd sizes, wavefronts that span MCU rows with a partial last one, more than two wavefronts in a
    row, OW * 3 not a multiple of four) at every scale, channel count, plane format and producer"""
    cases = [dense(layout, size) for size in SIZES[layout]] + [CC.edge_pairs(layout, SIZES[layout][-1])]
    _check(ica, gpu_ctx, cases, reqs=(1, 2, 3, 4))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_position(ica, gpu_ctx, layout):
    """a DC and one other position per block, all 63 positions, inside a byte and escaped; a position outside every component's kept
    rectangle gives the DC-only picture"""
    cases = [CC.one_position(layout, p, esc) for p in range(1, 64) for esc in (False, True)]
    _check(ica, gpu_ctx, cases, producers=(("host", "compact"), ("host", "int16"), ("walk", "compact")))
    hv = SM.LAYOUTS[layout]
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    n_outside = 0
    for s in SCALES:
        n = 8 // s
        nh, nv = max(n * hmax // h for h, _ in hv), max(n * vmax // v for _, v in hv)
        for case in cases:
            p = int(case.name.split("_p")[1].split("_")[0])
            r, c = divmod(int(M.NAT_OF_ZZ[p]), 8)
            if r >= nv or c >= nh:
                dc_only = [d.copy() for d in case.dequantised()]
                for d in dc_only:
                    d.reshape(d.shape[:2] + (64,))[..., 1:] = 0
                assert np.array_equal(_want(case, s, 3), SM.scaled_picture(dc_only, layout, (case.w, case.h), s, 3)), (case.name, s)
                n_outside += 1
    assert n_outside >= (0 if layout == "420" else 1) + 2 * 48


@pytest.mark.parametrize("layout", LAYOUTS)
def test_coefficient_content(ica, gpu_ctx, layout):
    """class edges, the DC sweep across both clamps, the colour grid, the members of the L1 family that need the 32-bit second pass (5904 /
    5905 forms, wrapping products, -32768), a progressive twin and a restart-interval stream"""
    forms = {f[0]: f for f in CC.strong_forms()}
    cases = [CC.edge_pairs(layout), CC.dc_sweep(layout, 0), CC.dc_sweep(layout, 2)]
    if layout in ("444", "420"):
        cases.append(CC.colour_grid(layout))
    wide = [c for c in CC.l1_family(layout) if c.needs_wide()]
    assert len(wide) >= 40 and any("m32768" in c.name for c in wide) and any("wrap" in c.name for c in wide)
    cases += wide
    cases.append(CC.l1_case(layout, forms["spread63_5905"], progressive=1))
    cases.append(CC.l1_case(layout, forms["dc-900_ac+_5904"], restart=2))
    cases.append(dense(layout, (136, 40), seed=5, restart=3))
    _check(ica, gpu_ctx, cases, reqs=(3,) if layout != "grey" else (1, 3))
    _check(ica, gpu_ctx, cases[:4], reqs=(4, 1) if layout != "grey" else (2, 4), producers=PRODUCERS[:2])


def test_mixed_batch_and_reset(ica, gpu_ctx):
    """scales 1, 2, 4, 8 and a layout without a reduced decode at scale 1 in one batch; the scale-1 slots equal, byte for byte, the same
    pictures in a batch that never heard of scaling; reset forgets the requests"""
    cases = [dense("420", (203, 77)), dense("444", (75, 41)), dense("420", (203, 77), seed=1), dense("422", (90, 30)), dense("grey", (65, 33)),
             CC.edge_pairs("411", (72, 24)), dense("420", (64, 48), seed=2)]
    scales = [1, 2, 4, 8, 2, 1, 1]
    plain = ica.Batch(gpu_ctx, len(cases), 16 * MB, 16 * MB, 16 * MB)
    b = ica.Batch(gpu_ctx, len(cases), 16 * MB, 16 * MB, 16 * MB)
    try:
        ps = [plain.add_jpeg(c.stream(), 3) for c in cases]
        plain.submit()
        plain.wait()
        for round_ in range(2):
            slots = [b.add_jpeg(c.stream(), 3) for c in cases]
            for sl, s in zip(slots, scales):
                if round_ == 0:
                    b.set_scale(sl, s)
            b.submit()
            b.wait()
            for case, sl, psl, s in zip(cases, slots, ps, scales):
                if s == 1 or round_ == 1:  # after the reset nothing is scaled any more
                    assert b.slot_path(sl) == plain.slot_path(psl) != 8, case.name
                    assert b.out_size(sl) == (case.w, case.h)
                    assert b.hash_out(sl) == plain.hash_out(psl), case.name
                else:
                    assert b.slot_path(sl) == 8
                    assert np.array_equal(b.fetch(sl), _want(case, s, 3)), (case.name, s)
            if round_ == 0:
                # a clone starts at scale 1; two reduced slots of one picture compare equal on the device, two different ones do not
                assert b.diff_slots([(slots[2], slots[2])]) == 0
                b.reset()
    finally:
        b.close()
        plain.close()


def test_diff_slots_of_reduced_pictures(ica, gpu_ctx):
    a, c = dense("420", (203, 77)), dense("420", (203, 77), seed=1)
    b = ica.Batch(gpu_ctx, 4, 16 * MB, 16 * MB, 16 * MB)
    try:
        s0, s1, s2 = b.add_jpeg(a.stream(), 3), b.add_jpeg(a.stream(), 3), b.add_jpeg(c.stream(), 3)
        s3 = b.add_clone(s0)
        for sl in (s0, s1, s2):
            b.set_scale(sl, 4)
        b.submit()
        b.wait()
        assert b.slot_path(s3) != 8 and b.out_size(s3) == (203, 77)  # clones start at 1
        assert b.diff_slots([(s0, s1)]) == 0 and b.diff_slots([(s0, s2)]) > 0
        assert b.hash_out(s0) == b.hash_out(s1) != b.hash_out(s2)
        with pytest.raises(ica.MijError):
            b.diff_slots([(s0, s3)])
    finally:
        b.close()


@pytest.fixture(scope="module")
def dec(ica, gpu_ctx):
    d = ica.TensorDecoder("cuda:0")
    yield d
    d.close()


def test_downstream_tensor_requests(ica, dec):
    """plain crop, bilinear resize and orientation 6 from a reduced slot: the models applied to the model's reduced picture; the padding of
    the destination stays untouched"""
    case = dense("420", (203, 77), seed=3)
    data = case.stream()
    for s in SCALES:
        px = _want(case, s, 3)
        H, W = px.shape[:2]
        for o in (1, 6):
            d = om.orient(px, o)
            dh, dw = d.shape[:2]
            win = (1, 2, dw - 3, dh - 3)
            for size in (None, (5, 7)):
                for layout, dtype in (("CHW", torch.float16), ("HWC", torch.uint8)):
                    t = None if dtype == torch.uint8 else tm.tables(3, dtype)
                    oh, ow = size or (win[3], win[2])
                    big = torch.full((1, 3, oh + 2, ow + 3) if layout == "CHW" else (1, oh + 2, ow + 3, 3), 0.5 if dtype != torch.uint8 else 0xA5, dtype=dtype, device="cuda:0")
                    out = big[:, :, 1:oh + 1, 2:ow + 2] if layout == "CHW" else big[:, 1:oh + 1, 2:ow + 2, :]
                    before = big.clone()
                    got, reasons = dec.decode([data], crops=[win], size=size, layout=layout, dtype=dtype, orientation=o, reduce=s, out=out)
                    assert reasons == [None]
                    want = tm.window(d, win, False, False, layout, t, dtype) if size is None else rm.window(d, win, size, "bilinear", False, False, layout, t, dtype)
                    assert tm.same_bits(got[0], want), (s, o, size, layout)
                    mask = torch.ones_like(big, dtype=torch.bool)
                    (mask[:, :, 1:oh + 1, 2:ow + 2] if layout == "CHW" else mask[:, 1:oh + 1, 2:ow + 2, :]).fill_(False)
                    assert torch.equal(big[mask].view(tm.BITS[dtype]), before[mask].view(tm.BITS[dtype])), (s, o, size, layout)
        # a window that fits the full-size picture but not the reduced one is refused
        with pytest.raises(ValueError):
            dec.decode([data], crops=[(0, 0, W + 1, H)], reduce=s)


def test_decoder_reduce(ica, dec):
    """reduce= as one int, per picture, and "auto" over pictures of different sizes and layouts, one 4:1:1 among them"""
    cases = [dense("420", (203, 77), seed=4), dense("444", (120, 90)), dense("422", (64, 300)), dense("grey", (33, 40)), CC.edge_pairs("411", (200, 64))]
    # one int: pictures of one size
    same = [cases[0], dense("420", (203, 77), seed=6)]
    got, reasons = dec.decode([c.stream() for c in same], reduce=4, dtype=torch.uint8, layout="HWC")
    assert reasons == [None, None] and tuple(got.shape) == (2, 20, 51, 3)
    for i, c in enumerate(same):
        assert np.array_equal(got[i].cpu().numpy(), _want(c, 4, 3))
    # per picture, resized to one size; the 4:1:1 file is rejected at s = 2 and decoded at 1
    per = [2, 8, 4, 1, 2]
    got, reasons = dec.decode([c.stream() for c in cases], reduce=per, size=(9, 11), dtype=torch.uint8, layout="HWC", req_comp=3)
    assert reasons[:4] == [None] * 4 and reasons[4] and "reduced" in reasons[4]
    assert not got[4].any()
    full_grey = None
    for i, (c, s) in enumerate(zip(cases[:4], per)):
        if s == 1:
            one, _ = dec.decode([c.stream()], size=(9, 11), dtype=torch.uint8, layout="HWC", req_comp=3)
            full_grey = one[0]
            assert torch.equal(got[i], full_grey)
        else:
            assert np.array_equal(got[i].cpu().numpy(), rm.resize(_want(c, s, 3), 11, 9, "bilinear")), (c.name, s)
    assert full_grey is not None
    # auto: the largest s whose reduced picture is still at least 11 x 9 in the displayed frame
    orients = [1, 6, 1, 1, 1]
    got, reasons = dec.decode([c.stream() for c in cases], reduce="auto", size=(9, 11), dtype=torch.uint8, layout="HWC", req_comp=3, orientation=orients)
    assert reasons == [None] * 5
    chosen = []
    for i, (c, o) in enumerate(zip(cases, orients)):
        dw, dh = om.displayed_size(c.w, c.h, o)
        s = 1 if c.layout == "411" else max([1] + [k for k in SCALES if -(-dw // k) >= 11 and -(-dh // k) >= 9])
        chosen.append(s)
        if s == 1:
            one, _ = dec.decode([c.stream()], size=(9, 11), dtype=torch.uint8, layout="HWC", req_comp=3, orientation=o)
            assert torch.equal(got[i], one[0]), c.name
        else:
            assert np.array_equal(got[i].cpu().numpy(), rm.resize(om.orient(_want(c, s, 3), o), 11, 9, "bilinear")), (c.name, s)
    assert chosen == [8, 8, 4, 2, 1]


def _rc(ica, b, slot, denom):
    L = ica.lib()
    L.mij_batch_set_scale.argtypes = [C.c_void_p, C.c_int, C.c_int]
    return L.mij_batch_set_scale(b._h, int(slot), int(denom))


def test_refusals(ica, gpu_ctx):
    b = ica.Batch(gpu_ctx, 16, 16 * MB, 16 * MB, 16 * MB)
    try:
        ok = b.add_jpeg(dense("420", (40, 24)).stream(), 3)
        for denom in (3, 0, -1, 16, 5):
            assert _rc(ica, b, ok, denom) == MIJ_E_ARG and b"denominator" in ica.lib().mij_last_error()
        assert _rc(ica, b, 99, 2) == MIJ_E_ARG
        for layout in ("440", "411", "cmyk", "ycck", "rgb"):
            sl = b.add_jpeg(CC.edge_pairs(layout, (40, 24)).stream(), 3)
            for denom in SCALES:
                assert _rc(ica, b, sl, denom) == MIJ_E_ARG, layout
                assert b"reduced size" in ica.lib().mij_last_error()
            assert _rc(ica, b, sl, 1) == 0
        # float output and reduced decode exclude each other, in either order
        b.reserve_out_f32(4 * MB)
        f = b.add_jpeg(dense("444", (40, 24)).stream(), 3)
        b.set_out_f32(f)
        assert _rc(ica, b, f, 2) == MIJ_E_ARG and b"float" in ica.lib().mij_last_error()
        g = b.add_jpeg(dense("444", (40, 24)).stream(), 3)
        assert _rc(ica, b, g, 2) == 0
        with pytest.raises(ica.MijError, match="float"):
            b.set_out_f32(g)
        assert _rc(ica, b, g, 4) == 0 and b.out_size(g) == (10, 6)  # asked again: replaced
        assert _rc(ica, b, ok, 2) == 0
        b.upload()
        assert _rc(ica, b, ok, 4) == MIJ_E_STATE
        b.launch()
        b.wait()
        assert b.slot_path(ok) == 8 and b.slot_path(g) == 8 and b.slot_path(f) == 3
    finally:
        b.close()
