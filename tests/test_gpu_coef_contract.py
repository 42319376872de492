"""The stream families of coef_cases.py -- single coefficients ON the L1 limit of the int16 IDCT contract (include/mij.h) and ON the
edges of the sparse classes (mij_kernels.h, "sparse blocks") -- through every decode kernel family, both plane formats and every
producer of coefficient planes; pixels against the oracle bit for bit, MIJ_FLAG_WIDE_IDCT against the model's verdict (idct_model.py),
and the class counters against counts derived from the picture's planes and the kernels' wavefront geometry (coef_cases.wave_members).

Which kernels classify (read off mij_kernels.h: the callers of load_idct_block with the count flag): the band kernels (4:2:0, 4:4:0,
4:2:2), k_fused_grey, k_fused1x1c and k_idct_planes of the two-pass family.  k_fused444 keeps the full transform and counts nothing:
pixels only there.  Column-segmented band kernels (pictures beyond 5840 / 4300 pixels) transform a halo column per segment: pixels only.

Producers: "host" -- the host walk staging the batch's own format (compact planes, or int16 planes for an int16 batch); "pack" -- the
host walk staging int16, packed on the device by k_pack_c8; "walk" / "walk_zz" -- the GPU Huffman walk with the record stream / with
MIJ_ES_RECORDS=0; progressive files (MIJ_FLAG_L1_ON_DEVICE in compact batches); stbi_load_from_memory.

The GPU walk serves baseline files of one or three components in one interleaved scan, 16-bit tables included (mjh_extract_scan;
test_gpu_walk_declines_what_it_does_not_serve pins it): every such family stream must be taken (status 1); status 2 is allowed only for
four-component and progressive files, which take the host walk and are listed by name in `declined`.  One deviation from "nothing comes
back in entropy_run()'s fallback list": the walk keeps DC differences in twelve bits and, by its own anomaly list
(mij_entropy_kernels.h), hands a stream with a DC difference beyond category 11 -- which no conforming stream has -- back to the host.
The L1 forms that put the whole sum on a lone DC term (difference of category 13) are such streams; they stay in the family, and the
fallback list must hold exactly them (Case.dc_category).  Their "dcramp" twins carry the same strong block behind DC terms that rise in
conforming steps, so that the DC part of the sum at 5903 / 5904 / 5905 is still taken by the walk itself; every other family stream
keeps to eleven bits (pinned on the CPU in test_coef_contract_host.py).

MIJ_FLAG_WIDE_IDCT is asserted against the model for every picture of every family, not only the L1 one."""
import numpy as np
import pytest

import coef_cases as CC

pytestmark = pytest.mark.gpu

PRODUCERS = (("host", "compact"), ("host", "int16"), ("pack", "compact"), ("walk", "compact"), ("walk", "int16"), ("walk_zz", "compact"))
CLASSIFYING = (1, 2, 4, 5, 6, 7)
MB = 1 << 20

_want = {}


def _pixels(oracle, case, req):
    k = (case.name, req)
    if k not in _want:
        kind, px, _ = oracle.load(case.stream(), req)
        assert kind == "ok", (case.name, px)
        _want[k] = px
    return _want[k]


def _fill(ica, gpu_ctx, monkeypatch, cases, req, producer, fmt, bits=None, band_rows=None):
    """-> (batch, slot per case, names the GPU walk declined)"""
    for var, val in (("MIJ_BAND_ROWS", band_rows), ("MIJ_ES_BITS_OVERRIDE", bits), ("MIJ_ES_RECORDS", 0 if producer == "walk_zz" else None)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(val))
    b = ica.Batch(gpu_ctx, len(cases), 128 * MB, 128 * MB, 128 * MB)
    b.set_coef_format(fmt)
    declined = []
    if producer in ("host", "pack"):
        slots = [b.add_jpeg(c.stream(), req, stage="int16" if producer == "pack" else None) for c in cases]
    else:
        b.entropy_reserve(32 * MB)
        slots, later = [None] * len(cases), []
        for i, c in enumerate(cases):
            st, slot = b.add_jpeg_stream(c.stream(), req)
            assert st in (1, 2), (c.name, st, b.last_reason)
            if st == 1:
                slots[i] = slot
            else:
                assert c.progressive is not None or c.layout not in CC.GPU_WALK_LAYOUTS, ("the GPU walk declined a baseline stream of a layout it serves", c.name, b.last_reason)
                later.append(i)
                declined.append(c.name)
        fallback = b.entropy_run()
        # kept: everything but the streams with a DC difference beyond category 11, which no conforming stream has and which the walk, by
        # its own anomaly list (mij_entropy_kernels.h), hands back for the host walk -- exactly those, at every subsequence length used here
        handed = sorted(c.name for c, s in zip(cases, slots) if s in fallback)
        assert handed == sorted(c.name for c, s in zip(cases, slots) if s is not None and c.dc_category() > 11), ("the GPU walk's fallback list", handed, bits)
        for c, s in zip(cases, slots):
            if s in fallback:
                b.fallback_prepare(s)
                d2, _ = ica.HostDecoder.decode(c.stream(), req, out=b.staging(s))
                if d2.flags:
                    b.set_flags(s, d2.flags)
        for i in later:  # what the walk does not serve takes the host walk
            slots[i] = b.add_jpeg(cases[i].stream(), req)
    for var in ("MIJ_BAND_ROWS", "MIJ_ES_BITS_OVERRIDE", "MIJ_ES_RECORDS"):
        monkeypatch.delenv(var, raising=False)
    return b, slots, declined


_counts = {}


def _class_counts(case, path, compact, wide):
    k = (case.name, path, compact, wide)
    if k not in _counts:
        _counts[k] = CC.expected_class_counts(case, path, compact, wide)
    return _counts[k]


def _expected_path(case, req, generic):
    if generic:
        return 2
    return 5 if req < 3 else CC.PATH_OF[case.layout]


def _segmented(case):
    return case.w > CC.SEG_WIDTH.get(case.layout, 1 << 30)


def _run(ica, oracle, gpu_ctx, monkeypatch, cases, reqs=(3, 4), producers=PRODUCERS, generics=(0,), classes=True, band_rows=(None,), bits=None, progressive_l1=False):
    """decode `cases` through every (producer, format) x band height x kernel family asked for and check everything the module's
    docstring lists; -> names the GPU walk declined"""
    declined_all = set()
    for req in reqs:
        for producer, fmt in producers:
            for rows in band_rows:
                b, slots, declined = _fill(ica, gpu_ctx, monkeypatch, cases, req, producer, fmt, bits, rows)
                declined_all |= set(declined)
                tag = (producer, fmt, "req %d" % req, "band rows %s" % rows, "bits %s" % bits)
                if progressive_l1 and fmt == "compact" and producer == "host":
                    assert all(b.slot_flags(s) & 16 for s in slots), ("the walk did not leave the L1 bound to the device", tag)
                for generic in generics:
                    b.force_generic(generic)
                    b.upload()
                    b.count_idct_classes(True)
                    b.launch()
                    b.wait()
                    counts = b.idct_class_counts()
                    b.count_idct_classes(False)
                    expect = [0, 0, 0, 0]
                    countable = classes
                    for case, s in zip(cases, slots):
                        path = b.slot_path(s)
                        assert path == _expected_path(case, req, generic), (case.name, path, generic, tag)
                        assert b.slot_coef_bytes(s) == (1 if fmt == "compact" else 0), (case.name, tag)
                        f = b.slot_flags(s)
                        assert not (f & 16), (case.name, f, tag)
                        assert bool(f & 1) == case.needs_wide(), ("MIJ_FLAG_WIDE_IDCT", case.name, "L1 %d" % case.max_l1(), "flags %d" % f, tag)
                        got, want = b.fetch(s), _pixels(oracle, case, req)
                        assert np.array_equal(got, want), (case.name, generic, tag, "L1 %d" % case.max_l1(), "flags %d" % f, int((got != want).sum()),
                                                           np.argwhere((got != want).any(axis=2))[:4].tolist())
                        if path in CLASSIFYING and _segmented(case) and not generic:
                            assert all(_segmented(c) for c in cases), "a column-segmented picture switches the counter check off: such pictures go in batches of their own"
                            countable = False  # column segments transform a halo column each: pixels only
                        elif path in CLASSIFYING:
                            expect = [a + c for a, c in zip(expect, _class_counts(case, path, fmt == "compact", case.needs_wide()))]
                    if countable:
                        assert counts == expect, ("class counters", counts, expect, generic, tag, [c.name for c in cases][:3])
                b.force_generic(0)
                b.close()
    return declined_all


# ---------------------------------------------------------------- one position

BAND = ("420", "440", "422")


def _producers_for(layout):
    return PRODUCERS if layout in CC.GPU_WALK_LAYOUTS else tuple(p for p in PRODUCERS if not p[0].startswith("walk"))


@pytest.mark.parametrize("layout", ["420", "440", "422", "444", "grey", "cmyk"])
def test_one_position_all_63(ica, oracle, gpu_ctx, monkeypatch, layout):
    """All 63 AC positions, alone in every block of every component, inside a byte and beyond it: every kernel family at one width, the
    two-pass family with force_generic 1 and 2, both formats, every producer.  A picture at position p runs only class block_class(p)
    (compact planes: class 3 wherever a wavefront holds an escaped block)."""
    cases = [CC.one_position(layout, p, esc) for p in range(1, 64) for esc in (False, True)]
    reqs = (3, 4, 1) if layout == "grey" else (3, 4)
    declined = _run(ica, oracle, gpu_ctx, monkeypatch, cases, reqs, _producers_for(layout), generics=(0, 1, 2))
    assert declined == set()
    if layout in BAND:
        _run(ica, oracle, gpu_ctx, monkeypatch, cases, (3,), (("host", "compact"), ("host", "int16")), band_rows=(1,))


def test_one_position_runs_one_class_only(ica, oracle, gpu_ctx, monkeypatch):
    """the sharper form of the class check, one picture per batch so that the counters are that picture's own: the three classes the
    position does not belong to count zero -- in the band kernel and in k_idct_planes, both formats"""
    for layout in ("420", "grey"):
        for p in CC.EDGE_POSITIONS + [1, 2, 3, 63]:
            case = CC.one_position(layout, p, False)
            cls = int(CC.M.block_class(CC.M.zz_to_nat(np.eye(64, dtype=np.int64)[p])))
            for fmt in ("compact", "int16"):
                b = ica.Batch(gpu_ctx, 1, 16 * MB, 16 * MB, 16 * MB)
                b.set_coef_format(fmt)
                s = b.add_jpeg(case.stream(), 3)
                for generic in (0, 1):
                    b.force_generic(generic)
                    b.upload()
                    b.count_idct_classes(True)
                    b.launch()
                    b.wait()
                    counts = b.idct_class_counts()
                    b.count_idct_classes(False)
                    assert counts[cls] > 0 and sum(counts) == counts[cls], (layout, p, cls, fmt, generic, counts)
                    assert np.array_equal(b.fetch(s), _pixels(oracle, case, 3)), (layout, p, fmt, generic)
                b.close()


# ---------------------------------------------------------------- class edges

@pytest.mark.parametrize("layout", ["420", "440", "422"])
def test_class_edges_at_every_band_form(ica, oracle, gpu_ctx, monkeypatch, layout):
    """positions on either side of each class edge -- natural (1,1) | (0,2) (2,0); (3,3) | (0,4) (4,0); (7,7) -- and pictures that are
    DC-only except for ONE block of a higher class at lane 0, 31, 32, 63 of a wavefront and in the partial last one, at a width for every
    form of the band kernel (coef_cases.BAND_WIDTHS; the form follows from the width, the binding does not show it).  One batch per
    width, so that the class counters are checked for every form with one, two, four, eight and sixteen waves: the higher class runs in
    exactly the wavefronts that hold the odd block.  Pixels only for the column-segmented widths (4:2:0: 5856, 4:4:0: 4312), whose
    workgroups transform a halo column per segment; through k_idct_planes (force_generic 1) those are counted too."""
    producers = (("host", "compact"), ("host", "int16"), ("walk", "compact"))
    counted = 0
    for w in CC.BAND_WIDTHS[layout]:
        cases = CC.edge_cases(layout, (w, CC.BAND_HEIGHT[layout]))
        assert len({_segmented(c) for c in cases}) == 1
        counted += not _segmented(cases[0])
        assert _run(ica, oracle, gpu_ctx, monkeypatch, cases, (3, 4), producers, generics=(0, 1), band_rows=(None, 1)) == set()
    assert counted == {"420": 5, "440": 2, "422": 5}[layout]


@pytest.mark.parametrize("layout", ["444", "grey", "411", "rgb", "cmyk", "ycck"])
def test_class_edges_in_the_block_per_lane_kernels(ica, oracle, gpu_ctx, monkeypatch, layout):
    """the same through k_fused444 (pixels only), k_fused_grey, k_fused1x1c in its three colour modes, and k_idct_planes (4:1:1 takes the
    two-pass family by itself; the others with force_generic 1 and 2)"""
    cases = CC.edge_cases(layout)
    reqs = (3, 4, 1) if layout == "grey" else (3, 4)
    assert _run(ica, oracle, gpu_ctx, monkeypatch, cases, reqs, _producers_for(layout), generics=(0, 1, 2)) == set()


def test_one_odd_block_raises_exactly_its_wavefront(ica, oracle, gpu_ctx, monkeypatch):
    """one picture per batch: a DC-only picture with one block of class c runs class c in exactly ONE wavefront and class 0 in all the
    others, in the band kernel and in k_idct_planes, in both formats"""
    for layout in ("420", "422", "grey", "cmyk"):
        for cls in (1, 2, 3):
            for place in range(5):
                case = CC.odd_lane(layout, cls, place)
                for fmt in ("compact", "int16"):
                    b = ica.Batch(gpu_ctx, 1, 16 * MB, 16 * MB, 16 * MB)
                    b.set_coef_format(fmt)
                    s = b.add_jpeg(case.stream(), 3)
                    for generic in (0, 1):
                        b.force_generic(generic)
                        b.upload()
                        b.count_idct_classes(True)
                        b.launch()
                        b.wait()
                        counts = b.idct_class_counts()
                        b.count_idct_classes(False)
                        path = b.slot_path(s)
                        total = sum(len(CC.wave_members(path, c, p.shape[0], p.shape[1], *CC.LAYOUTS[layout][0][0])) for c, p in enumerate(case.planes))
                        want = [total - 1, 0, 0, 0]
                        want[cls] = 1
                        assert counts == want, (case.name, fmt, generic, counts, want)
                        assert np.array_equal(b.fetch(s), _pixels(oracle, case, 3)), (case.name, fmt, generic)
                    b.close()


# ---------------------------------------------------------------- the L1 limit

@pytest.mark.parametrize("layout", ["420", "444", "422", "grey", "440", "411", "rgb", "cmyk", "ycck"])
def test_l1_limit_flag_and_pixels(ica, oracle, gpu_ctx, monkeypatch, layout):
    """tame pictures with one block whose L1 is exactly 5903, 5904 or 5905 in every form of coef_cases.strong_forms, at every place of
    coef_cases.l1_family: after upload slot_flags & 1 == the model's needs_wide for every producer, and the pixels are the oracle's (at
    5905 the int16 second pass is wrong for some of these blocks -- test_coef_contract_host.py -- so an under-reported sum shows)"""
    cases = CC.l1_family(layout)
    assert {c.max_l1() for c in cases} >= {5903, 5904, 5905, 32768}
    reqs = (3, 4, 1) if layout == "grey" else (3, 4)
    declined = _run(ica, oracle, gpu_ctx, monkeypatch, cases, reqs, _producers_for(layout), generics=(0, 1), band_rows=(None, 1) if layout in BAND else (None,))
    assert declined == set() and any(c.sixteen_bit for c in cases)


@pytest.mark.parametrize("script", [0, 1])
@pytest.mark.parametrize("layout", ["420", "444", "422", "grey"])
def test_l1_limit_progressive(ica, oracle, gpu_ctx, monkeypatch, layout, script):
    """the progressive twins: in a compact batch the walk leaves the bound to k_pack_c8 (MIJ_FLAG_L1_ON_DEVICE), in an int16 batch it is
    progressive_l1's; either way the flag is the model's verdict"""
    cases = CC.l1_family(layout, progressive=script)
    reqs = (3, 1) if layout == "grey" else (3,)
    _run(ica, oracle, gpu_ctx, monkeypatch, cases, reqs, (("host", "compact"), ("host", "int16"), ("pack", "compact")), generics=(0, 1), progressive_l1=True)


def test_l1_strong_block_straddling_a_subsequence(ica, oracle, gpu_ctx, monkeypatch):
    """GPU walk with MIJ_ES_BITS_OVERRIDE chosen so that the strong block begins in one subsequence and ends in a later one (checked
    on the CPU with the plain walk of coef_cases): the part of its L1 that another lane finishes is added by k_es_tails (zigzag-image
    form) / lies in the record stream another lane wrote (record form)"""
    groups = {}
    for case, bits in CC.straddle_cases():
        assert bits >= 1024 and CC.straddling_bits(case, (bits,)) == bits
        groups.setdefault(bits, []).append(case)
    for bits, cases in sorted(groups.items()):
        assert _run(ica, oracle, gpu_ctx, monkeypatch, cases, (3,), (("walk", "compact"), ("walk", "int16"), ("walk_zz", "compact")), bits=bits) == set()


# ---------------------------------------------------------------- DC sweep, colour grid, the public entry

@pytest.mark.parametrize("layout", ["420", "444", "422", "grey", "440", "411", "cmyk"])
def test_dc_sweep(ica, oracle, gpu_ctx, monkeypatch, layout):
    """DC-only blocks from below the clamp at 0 to above the clamp at 255 in steps of one: alone (idct_block_dc) and with a class-1 / 2 / 3
    lane in every wavefront (the DC term through idct_block_low and the full transform)"""
    cases = [CC.dc_sweep(layout, n) for n in range(4)]
    reqs = (3, 4, 1) if layout == "grey" else (3, 4)
    assert _run(ica, oracle, gpu_ctx, monkeypatch, cases, reqs, _producers_for(layout), generics=(0, 1, 2)) == set()


def test_colour_grid(ica, oracle, gpu_ctx, monkeypatch):
    """flat blocks whose (Y, Cb, Cr) run over all of 0, 1, 127, 128, 129, 254, 255 and a coarse grid between: every clamp of the colour row
    at both ends, in the 4:4:4 and 4:2:0 kernels, and as RGB / CMYK / YCCK through k_fused1x1c; the two-pass family too"""
    for layout in ("444", "420", "rgb", "cmyk", "ycck"):
        assert _run(ica, oracle, gpu_ctx, monkeypatch, [CC.colour_grid(layout)], (3, 4), _producers_for(layout), generics=(0, 1, 2)) == set()


def test_families_through_stbi_load_from_memory(ica, oracle, gpu_ctx, monkeypatch):
    """the public entry (one-picture batches; with MIJ_GPU_WALK_MIN_PIXELS=0 the GPU walk at 1024-bit subsequences where it applies)"""
    cases = []
    for layout in ("420", "444", "422", "grey", "440", "cmyk"):
        cases += CC.l1_family(layout)
        cases += [CC.one_position(layout, p, True) for p in CC.EDGE_POSITIONS] + [CC.edge_pairs(layout), CC.odd_lane(layout, 2, 3), CC.dc_sweep(layout, 1)]
    for layout in ("420", "grey"):
        cases += CC.l1_family(layout, progressive=1)
    cases += [CC.colour_grid(l) for l in ("444", "420", "ycck")]
    for walk in (False, True):
        if walk:
            monkeypatch.setenv("MIJ_GPU_WALK_MIN_PIXELS", "0")
        for case in cases:
            for req in ((3, 1) if case.layout == "grey" else (3,)):
                got = ica.stbi_load_from_memory(case.stream(), req)
                assert got is not None, (case.name, ica.stbi_failure_reason())
                assert np.array_equal(got[0], _pixels(oracle, case, req)), (case.name, req, walk, case.max_l1())


def test_gpu_walk_declines_what_it_does_not_serve(ica, gpu_ctx):
    """status 2 (nothing added) for the layouts outside the walk's scope and for progressive files: what `declined` above may hold"""
    b = ica.Batch(gpu_ctx, 16, 16 * MB, 16 * MB, 16 * MB)
    b.entropy_reserve(4 * MB)
    for layout in CC.LAYOUTS:
        assert b.add_jpeg_stream(CC.edge_pairs(layout).stream(), 3)[0] == (1 if layout in CC.GPU_WALK_LAYOUTS else 2), layout
    assert b.add_jpeg_stream(CC.l1_family("420", progressive=1)[0].stream(), 3)[0] == 2
    # a real Pq = 1 table does not put a stream outside the walk's scope: the per-position L1 branch of k_es_pack / k_es_pack2 is walked
    sixteen = [c for c in CC.l1_family("420") if c.sixteen_bit and c.max_l1() == 5904][0]
    assert b"\xff\xdb\x00\x83\x10" in sixteen.stream() and b.add_jpeg_stream(sixteen.stream(), 3)[0] == 1
    b.close()
