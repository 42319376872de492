"""The row-extent table the host Huffman walk makes (include/mij.h, "row-extent table"; jpeg_entropy.c, decode_block_c8 and
mjh_row_classes): one byte per block row and component, the largest extent class of the row's blocks -- folded into the baseline walk's
block loop from the positions it writes.  Pictures from row_class_cases.py: every block row holds one coefficient at (0,1), (1,0), (1,1),
(0,2), (2,0), (3,3), (0,4), (4,0) or (7,7), or none, or one beyond a byte, in the row's first block, its last, or either side of a tile
seam.  The table must equal the one numpy computes from the coefficients the same walk staged (expanded from the compact planes; the
device's copy of them, Batch.fetch_coef, is compared in tests/test_gpu_row_classes.py, as is a slot staged through stage_region, which
needs a batch).  No GPU."""
import numpy as np
import pytest

import coef_cases as CC
import helpers
import row_class_cases as RC

# 1040 x 704: 65 chroma blocks a row (every chroma row has a tile seam inside it, every other luma row of 130), 44 chroma and 88 luma rows:
# every pattern at every place in every component; the band kernels' smaller sizes, shifted so that their few rows differ
SIZES = [("420", 1040, 704, 0), ("440", 520, 704, 3), ("420", 1472, 48, 12), ("420", 256, 48, 27), ("440", 512, 48, 40)]


def _decoded(ica, data, compact=True):
    d, region, rows = ica.host_decode_rows(data, 3, want_compact=compact)
    arena = ica.expand_compact_region(d, region) if d.flags & 4 else region.view(np.int16)
    return d, ica.detile_coefficients(d, arena), rows


@pytest.mark.parametrize("layout,w,h,shift", SIZES)
def test_table_equals_the_classes_of_the_staged_coefficients(ica, layout, w, h, shift):
    case, want = RC.make(layout, w, h, shift)
    d, nat, rows = _decoded(ica, case.stream())
    assert d.flags & 4 and not d.flags & 1, d.flags  # staged compact, not WIDE
    assert rows.size == sum(d.comp[c].bh for c in range(d.ncomp))
    from_coef = RC.table_of(nat)
    assert np.array_equal(rows, from_coef), np.argwhere(rows != from_coef)[:8].tolist()
    assert np.array_equal(rows, want), np.argwhere(rows != want)[:8].tolist()  # ... which are the classes the picture was made with
    if h >= 704:
        bh = [d.comp[c].bh for c in range(d.ncomp)]
        for c, off in enumerate(np.cumsum([0] + bh[:-1])):
            assert sorted(set(rows[off:off + bh[c]].tolist())) == [0, 1, 2, 3], c
    assert bool(d.flags & 8) == bool((want == 3).any() and any(p == "escape" for p in RC.PATTERNS))


def test_every_pattern_and_place_occurs_in_every_component():
    """the generator's own promise at the large size: 11 patterns x 4 places per component, the seam places on blocks 63 | 64 of a tile"""
    case, _ = RC.make("420", 1040, 704, 0)
    for c, p in enumerate(case.planes):
        bh, bw, _ = p.shape
        seen = set()
        for r in range(bh):
            k = (r + 4 * c) % len(RC.PATTERNS)
            place = (r // len(RC.PATTERNS) + c) % RC.PLACES
            seen.add((k, place))
            bx = RC._block_of(place, r, bw)
            if place >= 2 and any((r * bw + x) % 64 == 0 for x in range(1, bw)):
                assert (r * bw + bx) % 64 == (63 if place == 2 else 0), (c, r, bx)
        assert len(seen) == len(RC.PATTERNS) * RC.PLACES, (c, len(seen))


def test_a_natural_picture_agrees_too(ica):
    data = ica.synth_jpeg(328, 200, 4, 90)
    d, nat, rows = _decoded(ica, data)
    assert np.array_equal(rows, RC.table_of(nat, wide=bool(d.flags & 1)))


def test_progressive_int16_staging_and_wide_streams_read_3(ica):
    case, want = RC.make("420", 256, 48, 2)
    assert (want < 3).any()
    # the same coefficients as a progressive file: its scans read-modify-write int16 planes, nobody folds an extent
    prog = CC.Case(case.name + "-prog", case.family, case.layout, case.w, case.h, [p.copy() for p in case.planes], progressive=1)
    d, nat, rows = _decoded(ica, prog.stream())
    assert not d.flags & 4 and (rows == 3).all(), rows.tolist()
    # the baseline file walked into int16 planes
    d, nat, rows = _decoded(ica, case.stream(), compact=False)
    assert not d.flags & 4 and (rows == 3).all(), rows.tolist()
    # a stream that needs the wide IDCT (tests/test_gpu_band_prefetch.py, _wide_stream): compact planes, 3 throughout
    data = bytearray(ica.synth_jpeg(256, 32, 5, 90))
    i = bytes(data).index(b"\xff\xdb")
    rng = np.random.default_rng(256)
    for k in range(64):
        data[i + 5 + k] = int(rng.integers(100, 256))
    d, nat, rows = _decoded(ica, bytes(data))
    assert d.flags & 1 and d.flags & 4 and (rows == 3).all(), (d.flags, rows.tolist())


def test_the_plain_entry_point_is_unchanged(ica):
    """mjh_decode_memory_fmt is mjh_decode_memory_rows without a table: same descriptor, same region"""
    case, _ = RC.make("420", 256, 48, 4)
    d1, r1 = ica.host_decode_staged(case.stream(), 3)
    d2, r2, _ = ica.host_decode_rows(case.stream(), 3)
    assert bytes(d1) == bytes(d2)
    main = ica.compact_offsets(d1)[1]
    assert np.array_equal(r1[:main], r2[:main])
