"""Every decode kernel family, and the output stages that read decoded pixels, with their slots at and behind byte 2^32 of the batch's
arenas (far_slots.FarBatch): a slot that straddles the line of the output arena and slots wholly behind it, their coefficient planes
behind the line of the coefficient arena, in front of them some 4 GiB of decoded spacers in which a store with a wrapped offset lands.
The encoder's kernels -- strip and per-unit transform, the gathers of device pixels, the emission, the conversion of coefficient
planes into units -- likewise behind byte 2^32 of its pixel and unit arenas (far_slots.FarEncoder).

Each test asserts its premise (the offsets, from the public size functions) and the kernel every slot took before it compares a pixel;
expected pixels are the CPU models' (upsample_model, tensor_model, resize_model, orient_model, loadf_expect), never another GPU decode;
expected units and streams are the host writer's and the host transcoder's (host_transform, emit_jpeg, transcode_memory) and the numpy
models of test_gpu_transcode_requant.py."""
import numpy as np
import pytest
import torch

import far_slots as F
import orient_model as om
import resize_model as rm
import sample_cases as S
import tensor_model as tm
import upsample_model as U

pytestmark = pytest.mark.gpu

LINE = F.LINE
SENTINEL = 0xA5
_model = {}


def _want(case, n_out):
    """upsample_model's picture of a case: once per colour branch, shared, never changed"""
    k = (case.name, n_out >= 3)
    if k not in _model:
        px = U.picture(case, 4 if n_out >= 3 else 2)
        px.setflags(write=False)
        _model[k] = px
    px = _model[k]
    return px if n_out in (2, 4) else px[..., :-1]


def _noise_jpeg(ica, w, h, seed):
    """an encoder-made 4:2:0 picture of full-amplitude noise that stays below the wide-IDCT limit (test_gpu_band_march's): MK_420's
    pipelined and marching twins take only such"""
    px = np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)
    data = ica.stbi_write_jpg_to_memory(px, 90)
    d, _ = ica.HostDecoder.decode(data, 3)
    assert not (d.flags & 1)
    return data


def _decoder_cases():
    """one width per band form of every band layout at height 17, one 4:2:0 picture of three column segments (367 MCU columns), the
    1 x 1 families (4:4:4, RGB-tagged, CMYK, grey), 4:1:1 for the two-pass path's k_resample_color, and one WIDE picture per family"""
    cases = []
    for layout in ("420", "422", "440"):
        for form, lo, hi in S.form_ranges(layout):
            cases.append(S.make("noise", layout, S.BAND_MCU_W[layout] * hi - 5, 17))
    cases.append(S.make("noise", "420", 16 * 367 - 3, 17))
    for layout in ("444", "rgb", "cmyk", "grey", "411"):
        cases.append(S.make("poison", layout, 37, 19))
    for layout in ("420", "422", "440", "444", "grey", "rgb"):
        mw, mh = S.mcu_px(layout)
        cases.append(S.make("noise", layout, 2 * mw + 3, mh + 1, wide=True))
    return cases


def _check_cases(fb, cases, slots, req, fmt, fg, tag):
    """kernel of every slot first, then its pixels against the model and the bytes behind it against the paint"""
    b = fb.b
    kinds = []
    for case, sl in zip(cases, slots):
        kind, var, nseg = b.slot_kernel(sl)
        t = tag + (case.name, kind, var, nseg)
        assert (kind, nseg) == S.expected_kernel(case.layout, case.w, req, fg), t
        assert b.slot_coef_bytes(sl) == (1 if fmt == "compact" else 0), t
        assert bool(var & 2) == case.needs_wide() or "RS" in kind or kind == "MK_RESAMPLE", t
        kinds.append(kind)
    for case, sl in zip(cases, slots):
        want = _want(case, req)
        px = fb.picture(sl, want.shape)
        if not np.array_equal(px, want):
            bad = np.argwhere((px != want).any(axis=2))
            raise AssertionError(tag + (case.name, b.slot_kernel(sl), "offset %d" % b.out_offset(sl), "%d pixels differ" % len(bad), "rows",
                                        sorted(set(bad[:, 0].tolist()))[:8], "columns", sorted(set(bad[:, 1].tolist()))[:16]))
    return kinds


@pytest.mark.parametrize("fmt", ("compact", "int16"))
@pytest.mark.parametrize("req", (3, 4, 1))
def test_decode_kernels_behind_the_line(ica, gpu_ctx, oracle, monkeypatch, req, fmt):
    """DevImage.out_off, DevComp.coef_off / dc_off / hi_off at and past 2^32 for every fused family: the band kernels in every form, column
    segments, k_fused444, k_fused1x1c (RGB-tagged and CMYK), k_fused_grey, their WIDE variants, and MK_420's pipelined (three channels,
    a width that is no multiple of four) and marching (four channels) twins on an encoder-made 1919 x 17 picture"""
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    cases = _decoder_cases()
    twin = _noise_jpeg(ica, 1919, 17, 77)
    items = [(c.stream(), req) for c in cases] + [(twin, req)]
    fb = F.FarBatch(ica, gpu_ctx, oracle, req, fmt, items)
    try:
        fb.run()
        slots = fb.slots
        kinds = _check_cases(fb, cases, slots[:-1], req, fmt, 0, (req, fmt))
        if req >= 3:
            assert {"MK_420T", "MK_420S", "MK_420", "MK_420W", "MK_420X", "MK_420C", "MK_422", "MK_440", "MK_444", "MK_1X1C", "MK_GREY"} <= set(kinds), kinds
        if fmt == "compact":
            assert sum(fb.b.slot_escapes(sl) for sl in slots) > 0
        # the twins of MK_420: compact planes only
        tw = slots[-1]
        assert fb.b.slot_kernel(tw)[0] == ("MK_420" if req >= 3 else "MK_GREY")
        if req >= 3:
            assert fb.b.slot_pipelined(tw) == (fmt == "compact") and fb.b.slot_marched(tw) == (fmt == "compact" and req == 4), (req, fmt)
        kind, want, _ = oracle.load(twin, req)
        assert kind == "ok" and np.array_equal(fb.picture(tw, want.shape), want), ("1919 x 17", req, fmt)
        fb.check_tail()
        fb.check_spacers()
    finally:
        fb.close()


@pytest.mark.parametrize("fg", (1, 2))
def test_two_pass_behind_the_line(ica, gpu_ctx, oracle, monkeypatch, fg):
    """force_generic on the whole batch: the spacers go two-pass too, so DevComp.plane_off (rebased at launch into the scratch arena)
    passes 2^32 along with out_off and coef_off: k_planes writes and k_resample_fast (fg 1: every RS_* kind the cases reach) /
    k_resample_color (fg 2, and 4:1:1 and the widths that are no multiple of four under fg 1) read there.  The spacer is 4:4:4 here: its
    scratch planes are as large as its pixels, so the first slot under test straddles the line of the scratch arena as well."""
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    cases = [S.make("noise", "420", 380, 17)]  # the straddling slot: large enough to begin a whole block row of the trimming picture early
    cases += [S.make("noise", layout, w, 17) for layout in ("420", "422", "440", "444", "411") for w in (36, 37)]
    cases += [S.make("poison", "cmyk", 36, 19), S.make("noise", "grey", 37, 19), S.make("noise", "420", 35, 17, wide=True)]
    for req, fmt in ((3, "compact"), (4, "int16")) if fg == 1 else ((3, "int16"),):
        fb = F.FarBatch(ica, gpu_ctx, oracle, 3, fmt, [(c.stream(), req) for c in cases], force_generic=fg, spacer_layout="444")
        try:
            first = fb.first
            d = fb.descs[first]
            pb = sum(F.align(d.comp[c].bw * 8 * d.comp[c].bh * 8) for c in range(d.ncomp))
            assert fb.plane_offset(first) < LINE < fb.plane_offset(first) + pb, ("scratch planes of the first slot", fb.plane_offset(first), pb)
            assert all(fb.plane_offset(sl) >= LINE for sl in fb.slots[1:])
            fb.run()
            assert fb.b.slot_path(0) == 2 and fb.b.slot_kernel(0)[0] == S.expected_kernel("444", F.SPACER_SIZE[0], 3, fg)[0]
            kinds = _check_cases(fb, cases, fb.slots, req, fmt, fg, (fg, req, fmt))
            if fg == 1:
                assert {"MK_RESAMPLE", "MK_RS_FAST+RS_HV2", "MK_RS_FAST+RS_H2", "MK_RS_FAST+RS_V2", "MK_RS_FAST+RS_ROW1"} <= set(kinds), kinds
            else:
                assert set(kinds) == {"MK_RESAMPLE"}
            fb.check_tail()
            fb.check_spacers()
        finally:
            fb.close()


def _host_planes(ica, data, req):
    """the host walk's planes, block by block per component"""
    d, planes = ica.HostDecoder.decode(data, req)
    return d, ica.detile_coefficients(d, planes)


@pytest.mark.parametrize("fmt", ("compact", "int16"))
def test_gpu_walk_and_pack_write_far_planes(ica, gpu_ctx, oracle, monkeypatch, fmt):
    """the producers of far coefficient planes other than the host's staging copy: the GPU Huffman walk (mij_batch_add_stream slots behind
    the spacers, a restart-interval stream among them) in its record form (the default) and, with MIJ_ES_RECORDS=0 set while the arena is
    reserved, in its zigzag-image form; and, for compact planes, k_pack_c8 packing int16 staging on the device.  Planes against the host
    walk's through fetch_coef, pixels against the model; req_comp 3, 4 and 1 once each."""
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    import coef_cases as CC
    cases = [S.make("noise", layout, w, 17) for layout, w in (("420", 379), ("422", 37), ("440", 37), ("444", 37), ("grey", 37), ("411", 37), ("rgb", 37))]
    base = S.make("noise", "420", 100, 40)
    cases.append(CC.Case(base.name + "_rst2", "noise", "420", 100, 40, base.planes, restart=2))
    for producer, req in (("walk", 3), ("walk_zz", 4)) + ((("int16", 1),) if fmt == "compact" else ()):
        if producer == "walk_zz":
            monkeypatch.setenv("MIJ_ES_RECORDS", "0")
        else:
            monkeypatch.delenv("MIJ_ES_RECORDS", raising=False)
        fb = F.FarBatch(ica, gpu_ctx, oracle, req, fmt, [(c.stream(), req) for c in cases], producer="walk" if producer == "walk_zz" else producer)
        monkeypatch.delenv("MIJ_ES_RECORDS", raising=False)
        try:
            fb.run()
            if producer == "int16":
                assert fb.b.pack_ms() is not None, "nothing was packed on the device"
            if fmt == "compact":  # the hi_off plane is written far by this producer too
                assert sum(fb.b.slot_escapes(sl) for sl in fb.slots) > 0, producer
            _check_cases(fb, cases, fb.slots, req, fmt, 0, (producer, fmt))
            for case, sl in zip(cases, fb.slots):
                desc, want = _host_planes(ica, case.stream(), req)
                for ci, (pg, pw) in enumerate(zip(ica.detile_coefficients(desc, fb.b.fetch_coef(sl)), want)):
                    assert np.array_equal(pg, pw), (producer, fmt, case.name, ci, "planes differ from the host walk's", int((pg != pw).sum()))
            fb.check_tail()
            fb.check_spacers()
        finally:
            fb.close()


def test_pack_takes_the_l1_bound_behind_the_line(ica, gpu_ctx, oracle, monkeypatch):
    """k_pack_c8 with MIJ_FLAG_L1_ON_DEVICE: host-staged progressive pictures in a compact batch behind the spacers.  The host walk
    leaves their per-block L1 bound to the device, so the pack reads int16 staging at src16_off and writes coef_off / dc_off / hi_off
    behind the line, and decides MIJ_FLAG_WIDE_IDCT there: of every strong form of coef_cases, one picture whose strongest block is exactly
    at MIJ_BLOCK_L1_LIMIT (5903: stays off the WIDE kernels) and one just past it (5904: takes them)."""
    import coef_cases as CC
    import idct_model as M
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    family = CC.l1_family("420", progressive=1)
    cases = [c for c in family if c.max_l1() in (M.L1_LIMIT, M.L1_LIMIT + 1)]
    assert {c.max_l1() for c in cases} == {M.L1_LIMIT, M.L1_LIMIT + 1} and len(cases) >= 4
    fb = F.FarBatch(ica, gpu_ctx, oracle, 3, "compact", [(c.stream(), 3) for c in cases])
    try:
        b = fb.b
        assert all(b.slot_flags(sl) & 16 for sl in fb.slots), "the host walk did not leave the L1 bound to the device"
        fb.run()
        # (this pack runs ahead of the decode plan, outside the events of pack_ms: that MIJ_FLAG_L1_ON_DEVICE is cleared below says it ran)
        assert sum(b.slot_escapes(sl) for sl in fb.slots) > 0, "no escaped block among the packed slots"
        for case, sl in zip(cases, fb.slots):
            flags = b.slot_flags(sl)
            assert not flags & 16 and bool(flags & 1) == case.needs_wide() == (case.max_l1() > M.L1_LIMIT), (case.name, flags, case.max_l1())
            kind, var, nseg = b.slot_kernel(sl)
            assert (kind, nseg) == S.expected_kernel("420", case.w, 3, 0) and bool(var & 2) == case.needs_wide(), (case.name, kind, var)
            assert b.slot_coef_bytes(sl) == 1
            desc, planes = _host_planes(ica, case.stream(), 3)
            for ci, (pg, pw) in enumerate(zip(ica.detile_coefficients(desc, b.fetch_coef(sl)), planes)):
                assert np.array_equal(pg, pw), (case.name, ci, "planes differ from the host walk's", int((pg != pw).sum()))
            ok, want, _ = oracle.load(case.stream(), 3)
            assert ok == "ok" and np.array_equal(fb.picture(sl, want.shape), want), (case.name, case.max_l1())
        fb.check_tail()
        fb.check_spacers()
    finally:
        fb.close()


# ------------------------------------------------------------------ output stages that read a far src_off

def _norm(dtype, n):
    return (None, None) if dtype == torch.uint8 else ((0.485, 0.456, 0.406, 0.5)[:n], (0.229, 0.224, 0.225, 0.25)[:n])


def _tensor_requests():
    """(dtype, layout, flip_x, flip_y, orientation, size or None, filter): every dtype in both layouts with flips at orientation 1, the
    transposing kernels through orientations 6 and 5, and resized requests one down and one up with two filters, plain and transposed"""
    dts = (torch.uint8, torch.float16, torch.bfloat16, torch.float32)
    out = []
    for k, dt in enumerate(dts):
        for layout in ("HWC", "CHW"):
            out.append((dt, layout, bool(k & 1), layout == "CHW", 1, None, None))
    for k, o in enumerate((6, 5)):
        for layout in ("HWC", "CHW"):
            out.append((dts[(2 * k + (layout == "CHW")) % 4], layout, layout == "HWC", bool(k), o, None, None))
    for o in (1, 6, 5):
        out.append((torch.float16, "CHW", False, True, o, (13, 17), "bilinear"))   # down
        out.append((torch.uint8, "HWC", True, False, o, (71, 90), "bicubic"))      # up
    return out


def test_tensor_output_reads_far_slots(ica, gpu_ctx, oracle, monkeypatch):
    """DevTensor.src_off / DevResize.t.src_off at and past 2^32: k_out_tensor, k_out_tensor_t, k_out_resize and k_out_resize_t read a
    straddling and far slots of one 61 x 43 4:2:0 picture into small sentinel-painted tensors, every byte of which is compared"""
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    case = S.make("noise", "420", 61, 43)
    px = _want(case, 3)
    reqs = _tensor_requests()
    fb = F.FarBatch(ica, gpu_ctx, oracle, 3, "compact", [(case.stream(), 3)] * len(reqs))
    try:
        bufs = []
        for sl, (dt, layout, fx, fy, o, size, name) in zip(fb.slots, reqs):
            dw, dh = om.displayed_size(61, 43, o)
            win = (3, 2, dw - 7, dh - 5)
            oh, ow = size if size is not None else (win[3], win[2])
            es, n = tm.ESIZE[dt], 3
            rp = (ow * n if layout == "HWC" else ow) + 3
            pp = (oh - 1) * rp + ow + 5 if layout == "CHW" else 0
            off = 16 // es + 1
            last = (oh - 1) * rp + ((n - 1) * pp + ow - 1 if layout == "CHW" else ow * n - 1)
            buf = torch.full(((off + last + 1) * es + 64,), SENTINEL, dtype=torch.uint8, device="cuda:0")
            t = tm.tables(n, dt, *_norm(dt, n)) if dt != torch.uint8 else None
            tb = None if t is None else t.view(tm.BITS[dt]).numpy()
            if size is None:
                fb.b.set_out_tensor(sl, buf.data_ptr() + off * es, tm.CODE[dt], layout, *win, rp, pp, fx, fy, tb, orientation=o)
            else:
                fb.b.set_out_tensor_resized(sl, buf.data_ptr() + off * es, tm.CODE[dt], layout, *win, ow, oh, rp, pp, fx, fy, tb, name, orientation=o)
            bufs.append((buf, win, oh, ow, rp, pp, off, t))
        torch.cuda.synchronize()
        fb.run()
        torch.cuda.synchronize()
        for sl in fb.slots:
            assert fb.b.slot_kernel(sl)[0] == "MK_420T" and np.array_equal(fb.picture(sl, px.shape), px), sl
        for (dt, layout, fx, fy, o, size, name), (buf, win, oh, ow, rp, pp, off, t) in zip(reqs, bufs):
            es, n = tm.ESIZE[dt], 3
            d = om.orient(px, o)
            vals = tm.window(d, win, fx, fy, layout, t, dt) if size is None else rm.window(d, win, size, name, fx, fy, layout, t, dt)
            vals = vals.view(tm.BITS[dt]).contiguous().view(torch.uint8).view(-1, es)
            want = torch.full((buf.numel(),), SENTINEL, dtype=torch.uint8)
            if layout == "CHW":
                c, y, x = torch.meshgrid(torch.arange(n), torch.arange(oh), torch.arange(ow), indexing="ij")
                el = off + c * pp + y * rp + x
            else:
                y, x, c = torch.meshgrid(torch.arange(oh), torch.arange(ow), torch.arange(n), indexing="ij")
                el = off + y * rp + x * n + c
            want[(el.reshape(-1, 1) * es + torch.arange(es)).reshape(-1)] = vals.reshape(-1)
            bad = (buf.cpu() != want).nonzero()
            assert bad.numel() == 0, ((dt, layout, fx, fy, o, size, name), bad[:8].tolist())
        fb.check_tail()
        fb.check_spacers()
    finally:
        fb.close()


def test_float_output_behind_the_line(ica, gpu_ctx, oracle, monkeypatch):
    """DevF32.src_off and dst_off past 2^32: the first 86 spacers ask for floats as well (50 MB each: fewer, larger requests than one
    per spacer would be), which carries the float arena past the line before the slots under test ask; their floats against
    loadf_expect applied to the model's pixels, spacer 0's against the CPU decode's"""
    import loadf_expect as fx
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    cases = [S.make("noise", "420", 61, 43), S.make("noise", "444", 37, 19), S.make("poison", "grey", 37, 19)]
    fb = F.FarBatch(ica, gpu_ctx, oracle, 3, "compact", [(c.stream(), 3) for c in cases])
    try:
        b = fb.b
        per = ica.Batch.out_f32_bytes(fb.descs[0])
        n_f = -(-LINE // per)
        assert n_f < fb.n_spacers
        b.reserve_out_f32(n_f * per + sum(ica.Batch.out_f32_bytes(fb.descs[sl]) for sl in fb.slots) + (1 << 20))
        table = fx.lut(3)
        for sl in list(range(n_f)) + fb.slots:
            b.set_out_f32(sl, table)
        fb.run()
        run = n_f * per  # the float arena is laid out in the order of the requests
        for case, sl in zip(cases, fb.slots):
            assert run >= LINE and b.device_out_f32(sl) - b.device_out_f32(0) == run, (case.name, run)
            run += ica.Batch.out_f32_bytes(fb.descs[sl])
            want = _want(case, 3)
            assert np.array_equal(fb.picture(sl, want.shape), want), case.name
            assert fx.same_bits(b.fetch_f32(sl), fx.apply(table, want)), case.name
        from roi_cases import want as cpu_decode
        assert fx.same_bits(b.fetch_f32(0), fx.apply(table, cpu_decode(oracle, fb.sp, 3)))
        fb.check_tail()
        fb.check_spacers()
    finally:
        fb.close()


def test_reduced_size_behind_the_line(ica, gpu_ctx, oracle, monkeypatch):
    """k_scaled in the four layouts it serves (luma only, 4:4:4, 4:2:0, 4:2:2) at 1/2, 1/4 and 1/8, reading far coefficient planes and
    writing a straddling and far slots; against scaled_model"""
    import scaled_model as SM
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    combos = [(layout, s) for layout in ("420", "grey", "444", "422") for s in (2, 4, 8)]
    cases = [S.make("noise", layout, 77, 45) for layout, _ in combos]
    fb = F.FarBatch(ica, gpu_ctx, oracle, 3, "compact", [(c.stream(), 3) for c in cases])
    try:
        for sl, (_, s) in zip(fb.slots, combos):
            fb.b.set_scale(sl, s)
        fb.run()
        for case, sl, (layout, s) in zip(cases, fb.slots, combos):
            kind = fb.b.slot_kernel(sl)[0]
            assert kind == "MK_SCALED+SC_" + {"420": "420", "grey": "Y", "444": "444", "422": "422"}[layout] and fb.b.slot_path(sl) == 8, (layout, s, kind)
            want = SM.scaled_picture(case.dequantised(), layout, (case.w, case.h), s, 3)
            assert fb.b.out_size(sl) == (want.shape[1], want.shape[0])
            assert np.array_equal(fb.picture(sl, want.shape), want), (layout, s)
        fb.check_tail()
        fb.check_spacers()
    finally:
        fb.close()


def test_regions_behind_the_line(ica, gpu_ctx, oracle, monkeypatch):
    """set_roi on a band-kernel slot and on a k_fused444 slot behind the line, and set_roi_auto on one of each with a tensor request:
    inside the window the model's pixels, outside the decoded rectangle the paint"""
    import roi_cases as RC
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    c420, c444 = S.make("noise", "420", 100, 70), S.make("noise", "444", 61, 43)
    cases = [c420, c444, c420, c444]
    wins = [(35, 18, 30, 33), (17, 9, 20, 17), (35, 18, 30, 33), (17, 9, 20, 17)]
    fb = F.FarBatch(ica, gpu_ctx, oracle, 3, "compact", [(c.stream(), 3) for c in cases])
    try:
        b = fb.b
        bufs = []
        for k, (sl, win) in enumerate(zip(fb.slots, wins)):
            if k < 2:
                b.set_roi(sl, *win)
                continue
            buf = torch.full((win[3], win[2], 3), SENTINEL, dtype=torch.uint8, device="cuda:0")
            b.set_out_tensor(sl, buf.data_ptr(), "u8", "HWC", *win, win[2] * 3)
            b.set_roi_auto(sl)
            bufs.append(buf)
        torch.cuda.synchronize()
        fb.run()
        torch.cuda.synchronize()
        for k, (case, sl, win) in enumerate(zip(cases, fb.slots, wins)):
            want = _want(case, 3)
            assert b.slot_path(sl) == RC.expected_path(case.layout, 3, 1), (k, b.slot_path(sl))
            rx, ry, rw, rh = b.roi_rect(sl)
            x0, y0, w, h = win
            assert rx <= x0 and ry <= y0 and rx + rw >= x0 + w and ry + rh >= y0 + h and (rw, rh) != (case.w, case.h), (k, (rx, ry, rw, rh))
            got = fb.picture(sl, want.shape)
            off = b.out_offset(sl) - fb.base
            pat = fb.pat[off:off + want.size].reshape(want.shape)
            assert np.array_equal(got[y0:y0 + h, x0:x0 + w], want[y0:y0 + h, x0:x0 + w]), (k, "inside")
            outside = np.ones(want.shape[:2], bool)
            outside[ry:ry + rh, rx:rx + rw] = False
            assert np.array_equal(got[outside], pat[outside]), (k, "outside the decoded rectangle")
            if k >= 2:
                assert tm.same_bits(bufs[k - 2], tm.window(want, win, layout="HWC")), (k, "tensor")
        fb.check_tail()
        fb.check_spacers()
    finally:
        fb.close()


def test_destination_tensor_behind_the_line(ica, gpu_ctx, oracle):
    """the destination itself behind the line: the CHW view of picture 64 of one [3, 65, 8192, 8192] uint8 allocation begins at byte 2^32
    of it, and its plane_pitch, 65 * 2^26 elements, takes channel 1 past 2^32 elements from the view's start and channel 2 past 2^33.
    The memory is never touched outside three small windows, which are sentinel-painted and compared byte for byte."""
    case = S.make("noise", "420", 61, 43)
    px = _want(case, 3)
    N, H, W = 65, 8192, 8192
    try:
        big = torch.empty((3, N, H, W), dtype=torch.uint8, device="cuda:0")
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip("out of memory creating the destination allocation itself: %s" % e)
    try:
        view = big[:, N - 1]  # [3, H, W]
        pp = view.stride(0)
        assert view.data_ptr() - big.data_ptr() >= LINE and pp > LINE and view.stride(1) == W
        corner = view[:, H - 64:, W - 128:]  # the last rows and columns of every plane
        corner.fill_(SENTINEL)
        b = ica.Batch(gpu_ctx, 1, 8 << 20, 8 << 20, 8 << 20)
        try:
            sl = b.add_jpeg(case.stream(), 3)
            win = (0, 0, 61, 43)
            b.set_out_tensor(sl, corner.data_ptr(), "u8", "CHW", *win, corner.stride(1), pp, True, False, None)
            torch.cuda.synchronize()
            b.submit()
            b.wait()
        finally:
            b.close()
        got = corner.cpu()
        want = torch.full(got.shape, SENTINEL, dtype=torch.uint8)
        want[:, :43, :61] = tm.window(px, win, True, False, "CHW", None, torch.uint8)
        assert torch.equal(got, want), (got != want).nonzero()[:8].tolist()
    finally:
        del big
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ the encoder: pixel and unit arenas past 2^32

ENC_WIDTHS = (250, 1, 17, 33, 528)  # 250 first: the straddling slot has to hold more than 4096 bytes of pixels and of units; 528 = 512 + 16
ENC_H = 19


def _first_difference(got, want):
    if got.shape != want.shape:
        return "%s units, want %s" % (got.shape, want.shape)
    d = np.argwhere(got != want)
    return "unit %d k %d: got %d want %d (%d values differ)" % (d[0][0], d[0][1], got[tuple(d[0])], want[tuple(d[0])], len(d))


@pytest.mark.parametrize("generic", (False, True))
def test_encoder_inputs_behind_the_line(ica, gpu_ctx, generic):
    """EncImage.pix_off / du_off, EncGather.pix_off and the emission kernels' du_base at and past 2^32: behind some 4 GiB of flat spacers,
    at quality 90 (4:2:0) and 95 (4:4:4) and widths 1, 17, 33, 250 and 528, host pixels, uint8 device pixels as strided HWC and CHW
    views (k_enc_gather), float16 / bfloat16 / float32 device pixels (k_enc_gather_float) and given adversarial units; every other slot
    with optimised tables (k_emit_hist / k_emit_build next to k_emit_len / count / write), the other half in the generic run.
    generic: mij_enc_force_generic, the per-unit kernels k_encode_y / k_encode_c in place of the strip kernels (the encoder has no
    per-slot kernel query: the switch is the whole batch's).  Units and streams are the host writer's for the model's picture."""
    import denorm_model as dm
    import emit_model as em
    import test_gpu_tensor_encode_float as TF
    rng = np.random.default_rng(20 + generic)
    fe = F.FarEncoder(ica, gpu_ctx, 7 * 2 * len(ENC_WIDTHS), force_generic=generic)
    keep, want = [], []  # want: (slot, what, plan, units)
    try:
        def expect(slot, what, pic, q):
            plan, du = ica.host_transform(pic, q)
            want.append((slot, what, plan, du))

        for q in (90, 95):
            for w in ENC_WIDTHS:
                img = rng.integers(0, 256, (ENC_H, w, 3), dtype=np.uint8)
                expect(fe.add(img, q), ("host", w, q), img, q)
                big = torch.zeros((ENC_H, w + 5, 3), dtype=torch.uint8, device="cuda:0")
                v = big[:, 2:2 + w]
                v.copy_(torch.from_numpy(img))
                keep.append(big)
                expect(fe.add_device(TF.in_tensor(ica, v, "HWC"), w, ENC_H, 3, q), ("u8 HWC view", w, q), img, q)
                big = torch.zeros((3, ENC_H + 2, w + 3), dtype=torch.uint8, device="cuda:0")
                v = big[:, 1:1 + ENC_H, 3:3 + w]
                v.copy_(torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))))
                keep.append(big)
                assert not v.is_contiguous()
                expect(fe.add_device(TF.in_tensor(ica, v, "CHW"), w, ENC_H, 3, q), ("u8 CHW view", w, q), img, q)
                for k, dtype in enumerate(TF.DTYPES):
                    x = TF.normalised(rng, (ENC_H, w, 3), 3, dtype)
                    cv, scale, bias = TF.convert(ica, dtype, 3)
                    pic = dm.picture(dm.widen(x), scale, bias)
                    layout = "CHW" if (k + (q == 95)) & 1 else "HWC"
                    t = (x.permute(2, 0, 1).contiguous() if layout == "CHW" else x).cuda()
                    keep.append(t)
                    expect(fe.add_device_float(TF.in_tensor(ica, t, layout), cv, w, ENC_H, 3, q), (str(dtype), layout, w, q), pic, q)
                plan, _ = ica.host_transform(np.zeros((ENC_H, w, 3), np.uint8), q)
                du = em.adversarial_units(rng, plan.mcu_x * plan.mcu_y, plan.du_per_mcu)
                want.append((fe.add_units(w, ENC_H, 3, q, du), ("units", w, q), plan, du))
        assert [s for s, _, _, _ in want] == fe.slots and len(want) == 70
        fe.premise()
        assert sum(1 for s in fe.slots if fe.pix_bytes_of[s] and fe.pix_off[s] >= LINE) >= 50
        optimized = {s for k, s in enumerate(fe.slots) if (k & 1) != generic}
        for s in optimized:
            fe.enc.set_optimize(s)
        torch.cuda.synchronize()
        fe.enc.upload()
        fe.enc.launch()
        n = fe.enc.fetch_streams()
        assert n == fe.n_spacers + 1 + len(want), "a stream did not fit the emission arena"
        for slot, what, plan, du in want:
            got = fe.enc.fetch(slot)
            assert np.array_equal(got, du), (what, generic, fe.du_off[slot], _first_difference(got, du))
        for slot, what, plan, du in want:
            assert fe.enc.slot_status(slot) == "ok", what
            assert fe.enc.stream(slot)[0] == ica.emit_jpeg(plan, du, slot in optimized), (what, generic, slot in optimized, fe.du_off[slot])
        fe.check_spacers()
    finally:
        fe.close()


@pytest.mark.parametrize("fmt", ("compact", "int16"))
def test_transcode_from_far_planes_into_far_units(ica, gpu_ctx, oracle, fmt):
    """CoefSlot.coef_off / dc_off / hi_off and du_off all at and past 2^32: mij_enc_add_coef on batch slots whose planes lie behind the
    line of the coefficient arena, into encoder slots behind the line of the unit arena (the first straddles it).  Orientations 1, 6
    (transposing) and 3 (both axes mirrored) with the partial MCUs trimmed, requantising slots among them (quality 50, and explicit
    tables on the pictures of test_gpu_transcode_requant.special: ties, values that vanish, the clamp).  Plans, tables and units are
    orient_coef_model's / requant_model's, streams transcode_memory's; where the host contract finds a slot not codable -- one picture
    holds a single AC value of 1500 -- that slot's status is "uncodable" and every other slot's "ok"."""
    import test_gpu_transcode_requant as R
    pics = [R.pictures("420")[0], R.pictures("420")[1], R.pictures("444")[1], R.pictures("422")[0], R.pictures("440")[3], R.pictures("grey")[1],
            R.special("420"), R.special("444")]
    bad = R._one_value(5, 1500, 1)
    datas = [p.data for p in pics[:4]] + [bad] + [p.data for p in pics[4:]]
    index = [0, 1, 2, 3, 5, 6, 7, 8]  # pics[i] is item index[i]; item 4, in the middle, is the uncodable picture
    fb = F.FarBatch(ica, gpu_ctx, oracle, 3, fmt, [(d, 0) for d in datas])  # req_comp 0, as Transcoder decodes
    fe = None
    try:
        b = fb.b
        b.upload()  # the planes into device memory (k_pack_c8 where needed); no pixel kernel has to run
        b.wait()
        if fmt == "compact":
            assert sum(b.slot_escapes(sl) for sl in fb.slots) > 0
        explicit, q50 = (R.EXPLICIT, False), R._tables_of(ica, {"quality": 50})
        combos = [(i, o, None) for i in range(len(pics)) for o in (1, 6, 3)]
        combos += [(0, 6, q50), (2, 3, q50), (3, 1, q50), (6, 1, explicit), (6, 6, explicit), (7, 3, explicit)]
        fe = F.FarEncoder(ica, gpu_ctx, len(combos) + 2)
        slots = {}
        for k, c in enumerate(combos):
            i, o, tgt = c
            src = fb.slots[index[i]]
            slots[c] = fe.add_coef(b, src, o, True) if tgt is None else fe.add_coef(b, src, o, True, tgt[0], tgt[1])
            if k == len(combos) // 2:
                bad_slot = fe.add_coef(b, fb.slots[4])
        fe.premise()
        optimized = {s for k, s in enumerate(fe.slots) if k & 1}
        for s in optimized:
            fe.enc.set_optimize(s)
        fe.enc.upload()
        fe.enc.launch()
        fe.enc.fetch_streams()
        assert ica.transcode_memory(bad)[0] is None and "AC coefficient outside" in ica.transcode_memory(bad)[1]
        assert fe.enc.slot_status(bad_slot) == "uncodable" and fe.enc.stream(bad_slot)[0] is None
        codable = 0
        for c, slot in slots.items():
            i, o, tgt = c
            pic = pics[i]
            w, d, units = R._model(ica, pic, o, True, tgt)
            plan = fe.enc.tplan(slot)
            assert (plan.plan.width, plan.plan.height, plan.plan.mcu_x, plan.plan.mcu_y, plan.lh, plan.lv) == \
                (w.w, w.h, w.geom.mcu_x, w.geom.mcu_y, w.hv[0][0], w.hv[0][1]), (pic.name, o)
            assert list(plan.plan.ytab) == list(d[0]) and list(plan.plan.ctab) == list(d[1]), (pic.name, o)
            assert fe.enc.slot_requantized(slot) == (tgt is not None), (pic.name, o)
            R._assert_units(fe.enc.fetch(slot), units, "%s o %d target %s (%s) unit offset %d" % (pic.name, o, tgt is not None, fmt, fe.du_off[slot]))
            host, why = ica.transcode_memory(pic.data, optimize=slot in optimized, orientation=o, trim=True, tables=None if tgt is None else tgt[0],
                                             coarsen_only=True if tgt is None else tgt[1])
            if host is None:
                assert "outside" in why and fe.enc.slot_status(slot) == "uncodable" and fe.enc.stream(slot)[0] is None, (pic.name, o, why)
            else:
                assert fe.enc.slot_status(slot) == "ok" and fe.enc.stream(slot)[0] == host, (pic.name, o, tgt is not None, slot in optimized)
                codable += 1
        assert codable >= 18 and sum(1 for c, s in slots.items() if c[2] is not None and fe.enc.slot_status(s) == "ok") >= 3
        fe.check_spacers()
    finally:
        if fe is not None:
            fe.close()
        fb.close()
