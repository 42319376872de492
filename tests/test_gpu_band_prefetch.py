"""Phase A of the 4:2:0 band kernel as a software pipeline (mij_kernels.h, fused_band PF / k_fused420p): a wave holds
the loaded coefficients of its next task while it transforms the current one, and the first task of the next MCU row while phase B runs.
The launch takes the pipelined twin for compact planes that are not WIDE where the row's LDS leaves a CU three workgroups at most:
92 to 121 MCU columns (1457 to 1936 pixels).  Everything here is compared with the CPU checker byte for byte, with bands of one MCU row (nothing
to hand over), of two (one hand-over) and as many as the planner likes; the kind, variant and path of every slot are asserted, since the twin
must not show in them."""
import numpy as np
import pytest

import helpers
import sample_cases as sc

pytestmark = pytest.mark.gpu

WIDTHS = (1472, 1920, 1936, 1921, 1919)  # 92 columns: 10 wave tasks on 4 waves (3 3 2 2), last chroma wave 28 lanes; 120: 12 tasks, last luma wave half full; 121: the form's last width; unaligned rows
HEIGHTS = (16, 17, 40, 70)               # one and two MCU rows; three; five with the last mostly padding
BAND_ROWS = (None, "1", "2")
ARENA = 96 << 20

_cache = {}


def _shared(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _want(oracle, key, datas, req):
    def make():
        out = []
        for d in datas:
            kind, px, _ = oracle.load(d, req)
            assert kind == "ok", px
            out.append(px)
        return out
    return _shared((key, req), make)


def _set_band_rows(monkeypatch, band_rows):
    if band_rows is None:
        monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    else:
        monkeypatch.setenv("MIJ_BAND_ROWS", band_rows)  # read when the batch is created


def _decode(ica, gpu_ctx, datas, req, gpu_walk, fmt="compact"):
    b = ica.Batch(gpu_ctx, len(datas), ARENA, ARENA, ARENA)
    b.set_coef_format(fmt)
    if gpu_walk:
        b.entropy_reserve(32 << 20)
    ok, slots, reasons = b.decode_jpegs(datas, req, threads=2, gpu_entropy=gpu_walk)
    assert ok == len(datas), reasons
    return b, slots


def _check(b, slots, wants, families, what, compact=True, wide=False, twin=True):
    """twin: whether the slots' launch must be the pipelined kernel (one flag, or one per slot).  The twin shows in no kind, variant or segment
    count, so it is asked for by name (Batch.slot_pipelined): with the twin compiled out or its LDS threshold moved, these tests fail."""
    for i, (s, want) in enumerate(zip(slots, wants)):
        assert b.slot_path(s) == 1, (what, i, b.slot_path(s))
        kind, var, nseg = b.slot_kernel(s)
        assert (kind, nseg) == (families[i], 1) and (var & 1) == int(compact) and bool(var & 2) == wide, (what, i, kind, var, nseg)
        assert b.slot_pipelined(s) == (twin if isinstance(twin, bool) else twin[i]), (what, i, kind, var)
        got = b.fetch(s)
        assert np.array_equal(got, want), (what, i, want.shape, int((got != want).sum()), np.argwhere((got != want).any(axis=2))[:4].tolist())


def _size_streams(ica):
    return _shared("sizes", lambda: [ica.synth_jpeg(w, h, (w + h) & 7, 90) for w in WIDTHS for h in HEIGHTS])


@pytest.mark.parametrize("gpu_walk", [False, True])
@pytest.mark.parametrize("band_rows", BAND_ROWS)
def test_pipelined_widths_and_heights(ica, oracle, gpu_ctx, monkeypatch, band_rows, gpu_walk):
    datas = _size_streams(ica)
    families = [sc.band_form("420", -(-w // 16))[0] for w in WIDTHS for h in HEIGHTS]
    assert set(families) == {"MK_420"}
    _set_band_rows(monkeypatch, band_rows)
    for req in (3, 4):
        b, slots = _decode(ica, gpu_ctx, datas, req, gpu_walk)
        b.submit()
        b.wait()
        _check(b, slots, _want(oracle, "sizes", datas, req), families, (band_rows, gpu_walk, req))
        b.close()


def _escaped_stream(ica):
    """The recipe of tests/test_gpu_compact.py::_streams at 1920 x 48 -- host_transform, 30 % of the blocks given 1-5 coefficients of magnitude
    128-399, baseline_from_du -- on a picture and at positions that keep every block under the wide-IDCT limit (sum |coefficient x quantiser|
    <= 5903), since a WIDE stream takes the plain kernel: faint noise round mid-grey (DC and AC near zero), luma blocks hit at zigzag
    positions 1, 2, 4, 5 (quantiser 2 at quality 90: at most 4 x 399 x 2), chroma blocks at 1 and 2 (quantiser 4: at most 2 x 399 x 4).
    Escaped and plain blocks share tiles and wavefronts, and the escape bytes are fetched inside a task that has its successor's loads in
    flight."""
    def make():
        rng = np.random.default_rng(77)
        img = rng.integers(120, 137, (48, 1920, 3)).astype(np.uint8)
        plan, du = ica.host_transform(img, 90)
        assert plan.du_per_mcu == 6  # 4:2:0: four luma units, Cb, Cr
        du = du.copy()
        for blk in np.nonzero(rng.random(du.shape[0]) < 0.3)[0]:
            pos = (1, 2, 4, 5) if blk % 6 < 4 else (1, 2)
            for _ in range(int(rng.integers(1, 6))):
                du[blk, pos[int(rng.integers(0, len(pos)))]] = int(rng.integers(128, 400)) * (1 if rng.random() < 0.5 else -1)
        du[:, 0] = np.clip(du[:, 0], -900, 900)
        data = helpers.baseline_from_du(plan, du, restart_mcus=0, layout="native")
        d, _ = ica.HostDecoder.decode(data, 3)
        assert not (d.flags & 1), "the stream is flagged for the wide IDCT: it would not take the pipelined kernel"
        return [data]
    return _shared("escaped", make)


@pytest.mark.parametrize("gpu_walk", [False, True])
@pytest.mark.parametrize("band_rows", BAND_ROWS)
def test_escaped_blocks_inside_a_pipelined_task(ica, oracle, gpu_ctx, monkeypatch, band_rows, gpu_walk):
    datas = _escaped_stream(ica)
    _set_band_rows(monkeypatch, band_rows)
    for req in (3, 4):
        b, slots = _decode(ica, gpu_ctx, datas, req, gpu_walk)
        b.submit()
        b.wait()
        assert b.slot_escapes(slots[0]) > 0
        _check(b, slots, _want(oracle, "escaped", datas, req), ["MK_420"], (band_rows, gpu_walk, req))
        b.close()


def _wide_stream(ica):
    """the recipe of test_gpu_parity.py::test_wide_idct_path_is_exact at 1920 x 32: quantisers of 100-255 make the first IDCT pass overflow
    int16, the host flags the stream MIJ_FLAG_WIDE_IDCT and the kernel takes the 32-bit second pass (variant bit 1): not pipelined"""
    def make():
        data = bytearray(ica.synth_jpeg(1920, 32, 5, 90))
        i = bytes(data).index(b"\xff\xdb")
        rng = np.random.default_rng(1920)
        for k in range(64):
            data[i + 5 + k] = int(rng.integers(100, 256))
        data = bytes(data)
        d, _ = ica.HostDecoder.decode(data, 3)
        assert d.flags & 1, "the stream was not flagged for the wide IDCT"
        return [data]
    return _shared("wide", make)


@pytest.mark.parametrize("band_rows", BAND_ROWS)
def test_forms_that_are_not_pipelined_stay_exact(ica, oracle, gpu_ctx, monkeypatch, band_rows):
    wide = _wide_stream(ica)
    plain = _shared("plain32", lambda: [ica.synth_jpeg(1920, 32, 6, 90)])
    _set_band_rows(monkeypatch, band_rows)
    for req in (3, 4):
        for gpu_walk in (False, True):
            b, slots = _decode(ica, gpu_ctx, wide, req, gpu_walk)
            b.submit()
            b.wait()
            _check(b, slots, _want(oracle, "wide", wide, req), ["MK_420"], ("wide", band_rows, gpu_walk, req), wide=True, twin=False)
            b.close()
            b, slots = _decode(ica, gpu_ctx, plain, req, gpu_walk, fmt="int16")
            b.submit()
            b.wait()
            _check(b, slots, _want(oracle, "plain32", plain, req), ["MK_420"], ("int16", band_rows, gpu_walk, req), compact=False, twin=False)
            b.close()


@pytest.mark.parametrize("band_rows", BAND_ROWS)
@pytest.mark.parametrize("width", [1920, 1472])
def test_class_counters_count_every_wave_task_once(ica, oracle, gpu_ctx, monkeypatch, width, band_rows):
    """One count per wave task of phase A, whatever the bands: an MCU row is nYw + 2 nCw tasks (luma: two block rows of 2 mcu_x blocks in
    wavefronts of 64; Cb and Cr: mcu_x blocks each), a launch mcu_y rows.  The halo tasks at band edges (2 nCw per inner edge and side) pass no
    counter and add nothing, so the sum does not depend on the bands.  The lanes the pipeline fills with copies of a row's last block must not
    change a class: the four counts are those of a second launch, and the pixels are the checker's."""
    datas = _shared(("counted", width), lambda: [ica.synth_jpeg(width, 48, 3, 90)])
    mcu_x, mcu_y = -(-width // 16), 3
    tasks = mcu_y * ((2 * 2 * mcu_x + 63) // 64 + 2 * ((mcu_x + 63) // 64))
    assert tasks == {1920: 36, 1472: 30}[width]
    _set_band_rows(monkeypatch, band_rows)
    b, slots = _decode(ica, gpu_ctx, datas, 3, False)
    b.upload()
    seen = []
    for _ in range(2):
        b.count_idct_classes(True)
        b.launch()
        b.wait()
        seen.append(b.idct_class_counts())
    b.count_idct_classes(False)
    assert sum(seen[0]) == tasks, (seen, tasks)
    assert seen[0] == seen[1], seen
    _check(b, slots, _want(oracle, ("counted", width), datas, 3), ["MK_420"], (width, band_rows))
    b.close()


@pytest.mark.parametrize("gpu_walk", [False, True])
@pytest.mark.parametrize("band_rows", BAND_ROWS)
def test_mixed_batch_with_the_pipelined_picture_last(ica, oracle, gpu_ctx, monkeypatch, band_rows, gpu_walk):
    """Two waves (896), the base form below the twin's range (1280: in one list with 1920, whose LDS decides for both), eight waves (2304), and
    1920 as the last slot of the arena: its last task's unused load stays inside its own planes"""
    widths = (896, 1280, 2304, 1920)
    datas = _shared("mixed", lambda: [ica.synth_jpeg(w, 40, w & 7, 90) for w in widths])
    families = [sc.band_form("420", -(-w // 16))[0] for w in widths]
    assert families == ["MK_420S", "MK_420", "MK_420W", "MK_420"]
    _set_band_rows(monkeypatch, band_rows)
    for req in (3, 4):
        b, slots = _decode(ica, gpu_ctx, datas, req, gpu_walk)
        b.submit()
        b.wait()
        _check(b, slots, _want(oracle, "mixed", datas, req), families, (band_rows, gpu_walk, req), twin=[False, True, False, True])
        b.close()


def test_the_twin_is_taken_from_92_to_121_mcu_columns(ica, oracle, gpu_ctx, monkeypatch):
    """The launch takes the pipelined kernel where the row's LDS (448 B per MCU column against 160 KiB) leaves a CU three workgroups at most:
    91 columns (1456 pixels) leave four, 92 (1457) three; 121 (1936) is the last width of the four-wave form, 122 (1937) goes to k_fused420w.
    One picture per batch, since a list's widest row decides for the list."""
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    for w, family, twin in ((1456, "MK_420", False), (1457, "MK_420", True), (1936, "MK_420", True), (1937, "MK_420W", False)):
        assert sc.band_form("420", -(-w // 16))[0] == family
        datas = _shared(("edge", w), lambda: [ica.synth_jpeg(w, 33, w & 7, 90)])
        b, slots = _decode(ica, gpu_ctx, datas, 3, False)
        b.submit()
        b.wait()
        _check(b, slots, _want(oracle, ("edge", w), datas, 3), [family], ("edge", w), twin=twin)
        b.close()
