"""The band kernels fetch only the coefficient chunks a block row's extent class allows (mij_kernels.h, fused_band "Row classes";
include/mij.h, "row-extent table").  Pictures from row_class_cases.py -- every block row of another class than its neighbours, the one
coefficient in the row's first block, its last or next to a tile seam, one row escaping the byte range -- decoded through every form of
the 4:2:0 / 4:4:0 band kernel and compared with the CPU checker byte for byte: RGB and RGBA, compact and int16 planes, one band, bands of
one MCU row (every band edge and both halo rows lie next to a row of another class) and of two, a clone of every slot, and every slot
staged once more from outside the library, whose table must read 3 throughout and whose pixels must not change.  The table a slot got
from the host walk must be the one numpy computes from the coefficients fetched back from the device."""
import numpy as np
import pytest

import row_class_cases as RC
import sample_cases as sc

pytestmark = pytest.mark.gpu

# (layout, width, height, shift, what): the marched twin, the pipelined twin without the march (RGB rows that are not whole dwords), the
# two-wave and one-wave forms of the plain loop (512 and 256 pixels), the four-wave plain kernel below the twin's range (1040), the
# eight-wave form, column segments, 4:4:0
SIZES = [("420", 1472, 48, 0, "marched"), ("420", 1936, 80, 13, "marched"), ("420", 1474, 48, 26, "pipelined"), ("420", 512, 48, 39, "two-wave"),
         ("420", 2560, 32, 5, "w"), ("420", 256, 48, 18, "one-wave"), ("420", 6000, 32, 31, "segments"), ("440", 512, 48, 8, "440"),
         ("420", 1040, 48, 21, "plain")]
BAND_ROWS = ("8", "1", "2")  # one band; as many as MCU rows (three at 48 rows); three at 80 rows
ARENA = 48 << 20
SMALL = 8 << 20
_cache = {}


def _shared(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _cases():
    return _shared("cases", lambda: [RC.make(layout, w, h, shift) for layout, w, h, shift, _ in SIZES])


def _wants(oracle, req):
    def make():
        out = []
        for case, _ in _cases():
            kind, px, _ = oracle.load(case.stream(), req)
            assert kind == "ok", px
            out.append(px)
        return out
    return _shared(("want", req), make)


def _same(got, want, what):
    assert np.array_equal(got, want), (what, want.shape, int((got != want).sum()), np.argwhere((got != want).any(axis=2))[:4].tolist())


def _packed(d, rows):
    """the kernels' form of a table: per MCU row the largest class of each component's block rows, two bits a component, ones above"""
    out = np.full(d.mcu_y, 0xff, np.uint8)
    off = 0
    for c in range(d.ncomp):
        v = d.comp[c].bh // d.mcu_y
        cls = rows[off:off + d.comp[c].bh].reshape(d.mcu_y, v).max(axis=1)
        out = (out & ~np.uint8(3 << (2 * c))) | (cls << (2 * c)).astype(np.uint8)
        off += d.comp[c].bh
    return out


# a launch takes one kernel for its whole list (mij_runtime.hip, band_prefetch and band_march): the widest row decides between the plain
# kernel and the pipelined twin, one row that is not whole dwords keeps the list from marching.  So the twin without the march and the
# plain kernel get batches of their own; the other forms are lists of their own anyway.
GROUPS = (("marched", "w", "two-wave", "one-wave", "segments", "440"), ("pipelined",), ("plain",))


def _stage_from_outside(ica, b, data, req, fmt):
    """a slot whose staging the caller writes: mij_batch_add, the planes of a walk of the caller's own copied into mij_batch_stage_region,
    mij_batch_set_flags -- the library has seen no block of it, its table stays 3"""
    d, region = ica.host_decode_staged(data, req, want_compact=fmt == "compact")
    s = b.add(ica.HostDecoder.probe(data, req))
    b.stage_region(s)[:region.size] = region
    b.set_flags(s, d.flags)
    return s


@pytest.mark.parametrize("fmt", ["compact", "int16"])
@pytest.mark.parametrize("band_rows", BAND_ROWS)
def test_every_band_form_with_clones_and_restaged_slots(ica, oracle, gpu_ctx, monkeypatch, band_rows, fmt):
    monkeypatch.setenv("MIJ_BAND_ROWS", band_rows)  # read when the batch is created
    for group in GROUPS:
        idx = [i for i, size in enumerate(SIZES) if size[4] in group]
        datas = [_cases()[i][0].stream() for i in idx]
        n = len(datas)
        for req in (3, 4):
            wants = _wants(oracle, req)
            b = ica.Batch(gpu_ctx, 3 * n, ARENA, ARENA, ARENA)
            b.set_coef_format(fmt)
            ok, slots, reasons = b.decode_jpegs(datas, req, threads=2, gpu_entropy=False)
            assert ok == n, reasons
            clones = [b.add_clone(s) for s in slots]
            outside = [_stage_from_outside(ica, b, d, req, fmt) for d in datas]
            b.submit()
            b.wait()
            for k, i in enumerate(idx):
                layout, w, h, shift, what = SIZES[i]
                case, table = _cases()[i]
                family, nseg = sc.band_form(layout, -(-w // (16 if layout == "420" else 8)))
                kind, var, segs = b.slot_kernel(slots[k])
                assert (kind, segs) == (family, nseg) and (var & 1) == int(fmt == "compact") and not var & 2, (what, kind, var, segs)
                if fmt == "compact":
                    assert b.slot_marched(slots[k]) == (what == "marched" or (what == "pipelined" and req == 4)), (what, req)
                    assert b.slot_pipelined(slots[k]) == (what in ("marched", "pipelined")), what
                    assert family == {"plain": "MK_420", "two-wave": "MK_420S", "one-wave": "MK_420T", "w": "MK_420W", "segments": "MK_420C", "440": "MK_440"}.get(what, family), (what, family)
                rows = b.slot_row_classes(slots[k])
                if fmt == "compact":
                    d = b._desc(slots[k])
                    assert np.array_equal(rows, RC.table_of(ica.detile_coefficients(d, b.fetch_coef(slots[k])))), (what, rows.tolist())
                    assert np.array_equal(rows, table), (what, rows.tolist(), table.tolist())
                else:
                    assert (rows == 3).all(), (what, rows.tolist())  # the walk into int16 planes folds nothing
                assert np.array_equal(b.slot_row_classes(clones[k]), rows), what
                assert (b.slot_row_classes(outside[k]) == 3).all(), what
                # ... and what the kernels read is that table packed per MCU row, on the device: the slot's, the clone's, threes outside
                packed = _packed(b._desc(slots[k]), rows)
                assert (packed != 0xff).any() == (fmt == "compact"), what
                assert np.array_equal(b.slot_row_classes_device(slots[k]), packed), (what, packed.tolist())
                assert np.array_equal(b.slot_row_classes_device(clones[k]), packed), what
                assert (b.slot_row_classes_device(outside[k]) == 0xff).all(), what
                for s, who in ((slots[k], "slot"), (clones[k], "clone"), (outside[k], "outside")):
                    _same(b.fetch(s), wants[i], (what, who, band_rows, fmt, req))
            b.close()


def test_restaging_a_slot_from_outside_resets_its_table(ica, oracle, gpu_ctx, monkeypatch):
    """a slot the host walk staged, decoded, then written once more through stage_region by the caller: 3 throughout, the same pixels"""
    monkeypatch.delenv("MIJ_BAND_ROWS", raising=False)
    case, table = _cases()[0]
    want = _wants(oracle, 3)[0]
    b = ica.Batch(gpu_ctx, 2, SMALL, SMALL, SMALL)
    slots = [b.add_jpeg(case.stream(), 3)]  # the binding's own host stage hands the walk's table in, like the batch front ends
    b.submit()
    b.wait()
    assert np.array_equal(b.slot_row_classes(slots[0]), table) and (table < 3).any()
    _same(b.fetch(slots[0]), want, "first")
    d, region = ica.host_decode_staged(case.stream(), 3)
    stage = b.stage_region(slots[0])
    assert (b.slot_row_classes(slots[0]) == 3).all()  # handing the staging out is what resets it
    stage[:region.size] = region
    b.set_flags(slots[0], d.flags)
    b.submit()
    b.wait()
    assert (b.slot_row_classes(slots[0]) == 3).all()
    _same(b.fetch(slots[0]), want, "restaged")
    b.close()


@pytest.mark.parametrize("band_rows", BAND_ROWS)
def test_class_counts_are_those_of_a_table_of_threes(ica, gpu_ctx, monkeypatch, band_rows):
    """MIJ_DEV_COUNT_CLASSES counts what it counted: the wavefronts per class of the slots the host walk staged equal those of the same
    pictures staged from outside, whose tables read 3 -- the class test on the chunks a row's class lets through finds the class the full
    test finds.  One picture per batch pair, so that the counts are that picture's."""
    monkeypatch.setenv("MIJ_BAND_ROWS", band_rows)
    for i, (layout, w, h, shift, what) in enumerate(SIZES):
        data = _cases()[i][0].stream()
        seen = []
        for inside in (True, False):
            b = ica.Batch(gpu_ctx, 1, SMALL, SMALL, SMALL)
            if inside:
                ok, slots, reasons = b.decode_jpegs([data], 3, threads=1, gpu_entropy=False)
                assert ok == 1, reasons
            else:
                slots = [_stage_from_outside(ica, b, data, 3, "compact")]
            b.upload()
            assert ((b.slot_row_classes(slots[0]) < 3).any()) == inside, what
            b.count_idct_classes(True)
            b.launch()
            b.wait()
            seen.append(b.idct_class_counts())
            b.count_idct_classes(False)
            b.close()
        assert seen[0] == seen[1] and sum(seen[0]) > 0 and seen[0][0] > 0 and seen[0][3] > 0, (what, seen)
