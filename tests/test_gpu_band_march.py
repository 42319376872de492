"""Phase B of the 4:2:0 band kernel marching down its lanes' own strips (mij_kernels.h, fused_band MARCH / k_fused420m; DESIGN.md section 3.1,
round 5): a lane owns strips tid and tid + 256 of every row pair of its band, keeps the upper chroma row of a pair (aligned, edges fixed) and
the luma row above an MCU row in registers, and loads the lower chroma row only.  A pipelined launch of MK_420 takes this twin when every picture
of its list has rows of whole dwords (RGBA, or a width that is a multiple of four) of at most 2048 pixels; otherwise k_fused420p as before.

Everything is compared with the CPU checker byte for byte.  The pictures are independent uniform noise per channel: neighbouring chroma rows
of the synthetic gradient are nearly equal, so a lane that carried row C-2 instead of C-1, or kept a stale luma row, could pass on it.  Bands
of one MCU row (carry initialised from the halo row and the epilogue run with nothing in between), of two, and as many as the planner likes."""
import numpy as np
import pytest

import helpers
import sample_cases as sc

pytestmark = pytest.mark.gpu

# 92 columns: a second strip for lanes 0-111 only; 120; 121, the form's last; 1924 and 1460: W % 4 == 0 but W % 16 != 0, the right edge's
# selector in a strip that is not the MCU row's last possible one (wc = 962 / 730) and the last MCU column padded
WIDTHS = (1472, 1920, 1936, 1924, 1460)
HEIGHTS = (16, 17, 40, 70)  # one and two MCU rows; three; five with the last mostly padding
BAND_ROWS = (None, "1", "2")
ARENA = 96 << 20
_cache = {}


def _shared(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _noise_jpeg(ica, w, h, seed):
    px = np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)  # full amplitude stays below the wide-IDCT limit at quality 90
    data = ica.stbi_write_jpg_to_memory(px, 90)
    d, _ = ica.HostDecoder.decode(data, 3)
    assert not (d.flags & 1), "the stream is flagged for the wide IDCT: it would not take the twin"
    return data


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


def _decode(ica, gpu_ctx, datas, req, gpu_walk=False, fmt="compact"):
    b = ica.Batch(gpu_ctx, len(datas), ARENA, ARENA, ARENA)
    b.set_coef_format(fmt)
    if gpu_walk:
        b.entropy_reserve(32 << 20)
    ok, slots, reasons = b.decode_jpegs(datas, req, threads=2, gpu_entropy=gpu_walk)
    assert ok == len(datas), reasons
    b.submit()
    b.wait()
    return b, slots


def _check(b, slots, wants, what, marched=True, pipelined=True, compact=True, wide=False):
    """Which phase B ran shows in no kind or variant: it is asked for by name (Batch.slot_marched), one flag or one per slot"""
    for i, (s, want) in enumerate(zip(slots, wants)):
        kind, var, nseg = b.slot_kernel(s)
        assert (kind, nseg) == ("MK_420", 1) and (var & 1) == int(compact) and bool(var & 2) == wide, (what, i, kind, var, nseg)
        assert b.slot_pipelined(s) == pipelined, (what, i)
        assert b.slot_marched(s) == (marched if isinstance(marched, bool) else marched[i]), (what, i)
        got = b.fetch(s)
        assert np.array_equal(got, want), (what, i, want.shape, int((got != want).sum()), np.argwhere((got != want).any(axis=2))[:4].tolist())


def _size_streams(ica):
    return _shared("sizes", lambda: [_noise_jpeg(ica, w, h, 1000 * w + h) for w in WIDTHS for h in HEIGHTS])


@pytest.mark.parametrize("gpu_walk", [False, True])
@pytest.mark.parametrize("band_rows", BAND_ROWS)
def test_marched_widths_and_heights(ica, oracle, gpu_ctx, monkeypatch, band_rows, gpu_walk):
    datas = _size_streams(ica)
    assert {sc.band_form("420", -(-w // 16))[0] for w in WIDTHS} == {"MK_420"}
    _set_band_rows(monkeypatch, band_rows)
    for req in (3, 4):
        b, slots = _decode(ica, gpu_ctx, datas, req, gpu_walk)
        _check(b, slots, _want(oracle, "sizes", datas, req), (band_rows, gpu_walk, req))
        b.close()


@pytest.mark.parametrize("band_rows", BAND_ROWS)
def test_rows_that_are_not_whole_dwords(ica, oracle, gpu_ctx, monkeypatch, band_rows):
    """RGB rows of 1919 and 1921 pixels are not dword-aligned: the pipelined twin with the strip loop, as before.  RGBA rows are: the twin
    takes them and its one partial strip (W % 4 pixels behind the whole strips, the chroma columns beyond the picture clamped).  One RGB
    picture of 1921 keeps the whole list, 1920 included, with the strip loop."""
    odd = _shared("odd", lambda: [_noise_jpeg(ica, w, h, 1000 * w + h) for w in (1919, 1921, 1922) for h in (17, 40)])
    mixed = _shared("mixed1921", lambda: [_noise_jpeg(ica, 1920, 40, 5), _noise_jpeg(ica, 1921, 40, 6)])
    _set_band_rows(monkeypatch, band_rows)
    for req in (3, 4):
        b, slots = _decode(ica, gpu_ctx, odd, req)
        _check(b, slots, _want(oracle, "odd", odd, req), ("odd", band_rows, req), marched=req == 4)
        b.close()
        b, slots = _decode(ica, gpu_ctx, mixed, req)
        _check(b, slots, _want(oracle, "mixed1921", mixed, req), ("mixed", band_rows, req), marched=req == 4)
        b.close()


@pytest.mark.parametrize("band_rows", BAND_ROWS)
def test_a_narrower_picture_in_the_same_list(ica, oracle, gpu_ctx, monkeypatch, band_rows):
    """1280 x 32 is MK_420 below the twins' range; in one list with 1920 the list's LDS decides for both.  80 MCU columns: lanes 64-255 have
    no second strip and read the (unused) samples of one from the rows behind."""
    datas = _shared("narrow", lambda: [_noise_jpeg(ica, 1920, 33, 7), _noise_jpeg(ica, 1280, 32, 8)])
    assert [sc.band_form("420", -(-w // 16))[0] for w in (1920, 1280)] == ["MK_420", "MK_420"]
    _set_band_rows(monkeypatch, band_rows)
    for req in (3, 4):
        b, slots = _decode(ica, gpu_ctx, datas, req)
        _check(b, slots, _want(oracle, "narrow", datas, req), ("narrow", band_rows, req))
        b.close()


def _wide_stream(ica):
    """the recipe of test_gpu_parity.py::test_wide_idct_path_is_exact at 1920 x 32: quantisers of 100-255, the host flags the stream
    MIJ_FLAG_WIDE_IDCT and the launch takes the plain kernel"""
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


def test_plain_kernel_forms_are_not_marched(ica, oracle, gpu_ctx, monkeypatch):
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    wide = _wide_stream(ica)
    plain = _shared("plain32", lambda: [_noise_jpeg(ica, 1920, 32, 9)])
    for req in (3, 4):
        b, slots = _decode(ica, gpu_ctx, wide, req)
        _check(b, slots, _want(oracle, "wide", wide, req), ("wide", req), marched=False, pipelined=False, wide=True)
        b.close()
        b, slots = _decode(ica, gpu_ctx, plain, req, fmt="int16")
        _check(b, slots, _want(oracle, "plain32", plain, req), ("int16", req), marched=False, pipelined=False, compact=False)
        b.close()


def _escaped_stream(ica):
    """The recipe of tests/test_gpu_band_prefetch.py::_escaped_stream at 1920 x 48: host_transform, 30 % of the blocks given 1-5 coefficients
    of magnitude 128-399 at positions that keep every block under the wide-IDCT limit, baseline_from_du.  Escaped and plain blocks share
    tiles and wavefronts in phase A; phase B carries their rows like any other."""
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
        assert not (d.flags & 1), "the stream is flagged for the wide IDCT: it would not take the twin"
        return [data]
    return _shared("escaped", make)


def test_escaped_blocks_through_the_marched_twin(ica, oracle, gpu_ctx, monkeypatch):
    datas = _escaped_stream(ica)
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    for req in (3, 4):
        b, slots = _decode(ica, gpu_ctx, datas, req)
        assert b.slot_escapes(slots[0]) > 0
        _check(b, slots, _want(oracle, "escaped", datas, req), ("escaped", req))
        b.close()
