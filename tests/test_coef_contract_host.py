"""The int16 IDCT contract (include/mij.h, MIJ_BLOCK_L1_LIMIT) and the stream families of coef_cases.py on the CPU: the plain model of
idct_model.py equals the oracle's transform, the narrow second pass is exact up to the limit and NOT beyond it (which is what makes a
producer that under-reports a block's L1 visible in pixels), and every host producer of MIJ_FLAG_WIDE_IDCT -- the baseline walk into
int16 staging, its twin into compact staging, and progressive_l1 -- reaches the model's verdict exactly on both sides of the limit."""
import numpy as np
import pytest

import coef_cases as CC
import idct_model as M

L1_LAYOUTS = ("420", "444", "422", "grey", "440", "411", "rgb", "cmyk", "ycck")
PROG_LAYOUTS = ("420", "444", "422", "grey")


def _block_cases():
    """the cases whose every block goes through the model block by block: all L1 families, and a sample of the other families (their blocks
    repeat from layout to layout and from width to width)"""
    cases = []
    for layout in L1_LAYOUTS:
        cases += CC.l1_family(layout)
    for layout in PROG_LAYOUTS:
        for script in (0, 1):
            cases += CC.l1_family(layout, progressive=script)
    for layout in ("420", "444", "grey"):
        cases += [CC.one_position(layout, p, esc) for p in (1, 2, 5, 35, 63) for esc in (False, True)]
        cases += [CC.odd_lane(layout, cls, place) for cls in (1, 2, 3) for place in range(5)]
        cases += [CC.edge_pairs(layout), CC.dc_sweep(layout, 0), CC.dc_sweep(layout, 2)]
    cases += [CC.colour_grid(l) for l in ("444", "420", "rgb", "cmyk", "ycck")]
    return cases


def _blocks(cases):
    return np.concatenate([d.reshape(-1, 8, 8) for c in cases for d in c.dequantised()])


def test_model_idct_equals_the_oracle(oracle):
    """idct_exact == orc_idct_block on every distinct block of the families and on seeded random blocks, tame and wild"""
    fam = np.unique(_blocks(_block_cases()), axis=0)
    rng = np.random.default_rng(11)
    tame = rng.integers(-40, 41, (300, 8, 8)) * (rng.random((300, 8, 8)) < 0.3)
    wild = rng.integers(-32768, 32768, (300, 8, 8))
    spiky = np.zeros((200, 8, 8), np.int64)
    for k in range(200):
        spiky[k, rng.integers(0, 8), rng.integers(0, 8)] = rng.integers(-32768, 32768)
        spiky[k, 0, 0] = rng.integers(-2000, 2000)
    blocks = np.concatenate([fam, tame, wild, spiky])
    got = M.idct_exact(blocks)
    for k in range(blocks.shape[0]):
        want = oracle.idct(blocks[k].reshape(64)).reshape(8, 8)
        assert np.array_equal(got[k], want), (k, blocks[k].tolist())


def test_narrow_second_pass_is_exact_up_to_the_limit_and_not_beyond():
    """Every family block with L1 <= 5903 comes out of the int16 second pass as out of the exact one; at 5905 at least one does not
    (5683 * 5905 + 512 >= 2^25: the first-pass value leaves int16), so a producer that reported 5903 for it would be caught by pixels."""
    blocks = np.unique(_blocks(_block_cases()), axis=0)
    l1 = M.block_l1(blocks, 1)
    within = blocks[l1 <= M.L1_LIMIT]
    assert within.shape[0] > 1000
    assert np.array_equal(M.idct_narrow(within), M.idct_exact(within))
    # random blocks scaled onto the limit as well
    rng = np.random.default_rng(3)
    r = rng.integers(-200, 201, (500, 8, 8)) * (rng.random((500, 8, 8)) < 0.4)
    r = r[(M.block_l1(r, 1) <= M.L1_LIMIT)]
    assert np.array_equal(M.idct_narrow(r), M.idct_exact(r))
    beyond = blocks[l1 == 5905]
    assert beyond.shape[0] >= 16
    differs = [(M.idct_narrow(b) != M.idct_exact(b)).any() for b in beyond]
    assert any(differs)
    # and the form the contract's arithmetic is about: everything on the weight-5683 input of a column
    b = np.zeros((8, 8), np.int64)
    b[1, 0] = 5905
    assert int(M.first_pass(b).max()) > 32767 and (M.idct_narrow(b) != M.idct_exact(b)).any()
    b[1, 0] = 5903
    assert int(np.abs(M.first_pass(b)).max()) <= 32767
    assert int(np.abs(M.first_pass_weights()).max()) == 5683


def test_block_class_model():
    b = np.zeros((8, 8), np.int64)
    assert M.block_class(b) == 0
    b[0, 0] = 7
    assert M.block_class(b) == 0
    for (r, c), want in (((0, 1), 1), ((1, 0), 1), ((1, 1), 1), ((0, 2), 2), ((2, 0), 2), ((3, 3), 2), ((3, 0), 2), ((0, 4), 3), ((4, 0), 3), ((5, 2), 3), ((7, 7), 3)):
        b = np.zeros((8, 8), np.int64)
        b[r, c] = -1
        assert M.block_class(b) == want, (r, c)
    assert [int(M.block_class(M.zz_to_nat(np.eye(64, dtype=np.int64)[p]))) for p in CC.EDGE_POSITIONS] == [1, 2, 2, 2, 3, 3, 3]


@pytest.mark.parametrize("layout", L1_LAYOUTS)
def test_host_walks_raise_wide_exactly_at_the_limit(ica, oracle, layout):
    """flags & 1 of the int16-staging walk (mjh_decode_memory) and of the compact-staging walk (mjh_decode_memory_fmt) == needs_wide of the
    model, for every stream of the L1 family; the family has streams at 5903 (0), 5904 and 5905 (1) in every form"""
    cases = CC.l1_family(layout)
    verdicts = set()
    for case in cases:
        data = case.stream()
        assert oracle.load(data, 3)[0] == "ok", case.name
        want = case.needs_wide()
        verdicts.add((case.max_l1(), want))
        d, _ = ica.HostDecoder.decode(data, 3)
        assert bool(d.flags & 1) == want, ("int16 staging", case.name, case.max_l1(), d.flags)
        d2, _ = ica.host_decode_staged(data, 3, want_compact=True)
        assert bool(d2.flags & 4), case.name
        assert bool(d2.flags & 1) == want, ("compact staging", case.name, case.max_l1(), d2.flags)
        d3, _ = ica.host_decode_staged(data, 3, want_compact=False)
        assert bool(d3.flags & 1) == want, ("fmt walk, int16 staging", case.name, case.max_l1(), d3.flags)
    assert {(5903, False), (5904, True), (5905, True), (32768, True)} <= verdicts


@pytest.mark.parametrize("script", [0, 1])
@pytest.mark.parametrize("layout", PROG_LAYOUTS)
def test_progressive_l1_raises_wide_exactly_at_the_limit(ica, oracle, layout, script):
    """the progressive twins: mjh_decode_memory computes the bound over the finished planes (progressive_l1)"""
    for case in CC.l1_family(layout, progressive=script):
        data = case.stream()
        assert oracle.load(data, 3)[0] == "ok", case.name
        d, planes = ica.HostDecoder.decode(data, 3)
        assert bool(d.flags & 1) == case.needs_wide(), (case.name, case.max_l1(), d.flags)
        # the planes the scans built are the planes the case was written from
        for got, want in zip(ica.detile_coefficients(d, planes), case.quantised()):
            assert np.array_equal(got, want), case.name


def test_host_planes_are_the_cases_planes(ica):
    """the walk stages exactly the coefficients the generator wrote (so the model's view of a case is the decoder's), 16-bit tables included"""
    for case in CC.l1_family("420")[::7] + CC.l1_family("cmyk")[::11] + [CC.one_position("422", 17, True), CC.odd_lane("440", 2, 3)]:
        d, planes = ica.HostDecoder.decode(case.stream(), 3)
        for got, want in zip(ica.detile_coefficients(d, planes), case.quantised()):
            assert np.array_equal(got, want), case.name


def test_every_family_stream_decodes_in_the_oracle_and_is_deterministic(oracle):
    cases, again = CC.everything(), CC.everything()
    assert len(cases) == len(again) and len({c.name for c in cases}) == len(cases)
    for a, b in zip(cases, again):
        assert a.stream() == b.stream(), a.name
        kind, px, _ = oracle.load(a.stream(), 3)
        assert kind == "ok", (a.name, px)
        assert px.shape[:2] == (a.h, a.w)
        # conforming DC differences (eleven bits at most) everywhere but in the forms that put a whole L1 on a lone DC term: those the GPU
        # walk hands back by design, and test_gpu_coef_contract.py expects exactly them in its fallback list
        lone_dc = a.family == "l1" and ("_dc+_" in a.name or "_dc-_" in a.name)
        assert (a.dc_category() > 11) == lone_dc, (a.name, a.dc_category())


def test_flat_blocks_reach_every_clamp_of_the_colour_row(oracle):
    """the colour grid does what it is for: the decoded 4:4:4 picture holds a block of every (Y, Cb, Cr) of the grid, among them channels
    clamped at 0 and at 255"""
    case = CC.colour_grid("444")
    px = oracle.load(case.stream(), 3)[1]
    centre = px[4::8, 4::8].reshape(-1, 3)
    assert centre.shape[0] == len(CC.GRID) ** 3
    for ch in range(3):
        assert centre[:, ch].min() == 0 and centre[:, ch].max() == 255
    y = M.idct_exact(case.dequantised()[0].reshape(-1, 8, 8))
    assert sorted(set(y[:, 0, 0].tolist())) == CC.GRID and (y == y[:, :1, :1]).all()


def test_straddling_subsequence_length_exists_for_the_spread_block():
    """the GPU test needs a subsequence length of 1024 bits or more at which the strong block straddles a boundary: the plain walk of
    coef_cases finds every block in the stream (it ends on the segment's last byte), and straddle_case finds a place that a boundary cuts"""
    pairs = CC.straddle_cases()
    assert {c.layout for c, _ in pairs} == set(CC.GPU_WALK_LAYOUTS) and {c.max_l1() for c, _ in pairs} == {5903, 5904, 5905}
    for case, bits in pairs:
        ranges, nbits = CC.block_bit_ranges(case.stream())
        assert ranges[-1][1] <= nbits and nbits - ranges[-1][1] < 8
        assert bits >= 1024 and CC.straddling_bits(case, (bits,)) == bits, case.name
