"""Hand-made data units for the progressive writer (tests/test_progressive_host.py, tests/test_gpu_progressive.py): each case is a grey or
4:2:0 transcode plan and units chosen for one property of libjpeg's progressive coding (include/mij_host.h, PROGRESSIVE STREAMS) -- end-of-band
runs against the tile seams of the GPU emission (MIJ_EMIT_TILE = 128 blocks), the two forced flushes, single magnitudes, ZRLs in first and
refinement scans."""
import numpy as np

TILE = 128


def plan(ica, w, h, layout="grey"):
    """the transcode plan of a w x h grey or 4:2:0 picture with the writer's quality-90 tables"""
    t = ica.binding.TranscodePlan()
    grey = layout == "grey"
    mw = 8 if grey else 16
    t.ncomp, t.lh, t.lv = (1, 1, 1) if grey else (3, 2, 2)
    p = t.plan
    p.width, p.height, p.comp, p.subsample = w, h, t.ncomp, 0 if grey else 1
    p.mcu_x, p.mcu_y, p.du_per_mcu = -(-w // mw), -(-h // mw), 1 if grey else 6
    luma, chroma = ica.binding.quality_tables(90)
    for k in range(64):
        p.ytab[k], p.ctab[k] = int(luma[k]), int(luma[k] if grey else chroma[k])
    return t


def _units(t):
    return np.zeros((t.plan.mcu_x * t.plan.mcu_y * t.plan.du_per_mcu, 64), np.int16)


def cases(ica, huge=False):
    """-> [(name, plan, units, forced)]: forced names the flush libjpeg makes early in it ("bits", "run") or None.  huge adds the 33124-block
    flat picture whose run reaches 0x7FFF."""
    out = []
    t = plan(ica, 192, 128)  # 24 x 16 blocks
    du = _units(t)
    du[:, 0] = 40
    du[0, 1:6], du[300, 1:9] = [9, -3, 1, 0, 2], [-17, 5, 0, 0, 1, -1, 2, 3]
    out.append(("run_across_two_seams", t, du, None))
    du = _units(t)
    du[5, 1:4], du[TILE, 1:4], du[TILE, 63] = [3, 1, -2], [4, -1, 6], 1
    out.append(("run_ends_at_unit_128", t, du, None))
    du = _units(t)
    du[np.arange(len(du)), 0] = (np.arange(len(du)) % 7) * 30 - 90
    du[10, 1:5], du[10, 40] = [1, -1, 5, -9], -2
    out.append(("run_reaches_the_scan_end", t, du, None))
    t16 = plan(ica, 128, 8)  # 16 blocks
    du = _units(t16)
    du[:, 1:] = np.where((np.arange(63) + np.arange(16)[:, None]) & 1, -5, 6)
    out.append(("pending_bits_945", t16, du, "bits"))
    t10 = plan(ica, 80, 8)
    du = _units(t10)
    for b, (m, sgn) in enumerate([(m, s) for m in (1, 2, 3, 4, 1023) for s in (1, -1)]):
        du[b, 1 + 6 * b] = m * sgn
    out.append(("single_magnitudes", t10, du, None))
    t4 = plan(ica, 32, 8)
    du = _units(t4)
    du[0, 1], du[0, 40] = 8, -8          # first scans: 34 zeros in the band 6..63
    du[1, 1], du[1, 30], du[1, 50] = 8, 1, 2  # refinement: a correction bit waits behind the ZRL of 28 zeros in front of a new coefficient
    du[2, 2], du[2, 20], du[2, 21], du[2, 63] = -12, 7, -1, 1  # an already non-zero lane takes the sixteen zeros of its run before a new one follows
    du[3, 63] = -3
    out.append(("zrl_first_and_refinement", t4, du, None))
    rng = np.random.default_rng(11)
    for layout, w, h in (("grey", 200, 120), ("420", 150, 90)):
        tr = plan(ica, w, h, layout)
        du = _units(tr)
        n = len(du)
        du[:, 0] = np.cumsum(rng.integers(-20, 21, n))
        for b in rng.choice(n, n // 3, replace=False):  # a third of the units sparse, some dense, the rest empty
            k = rng.choice(np.arange(1, 64), rng.integers(1, 12), replace=False)
            du[b, k] = rng.choice([-9, -4, -3, -2, -1, 1, 1, 1, 2, 3, 5, 17], len(k))
        for b in rng.choice(n, 6, replace=False):
            du[b, 1:] = rng.integers(-6, 7, 63)
        if layout == "420":  # luma's MCU padding blocks are in no AC scan: they keep their DC only, so that the units come back as they went
            m = np.arange(n) // 6
            p = np.arange(n) % 6
            bx, by = (m % tr.plan.mcu_x) * 2 + (p & 1), (m // tr.plan.mcu_x) * 2 + (p >> 1)
            du[(p < 4) & ((bx >= -(-w // 8)) | (by >= -(-h // 8))), 1:] = 0
        out.append(("random_sparse_" + layout, tr, du, None))
    if huge:
        th = plan(ica, 1456, 1456)
        du = _units(th)
        du[:, 0] = 11
        out.append(("flat_33124_blocks", th, du, "run"))
    return out


def units_of(ica, stream):
    """the units a stream decodes to (host walk)"""
    desc, region = ica.binding.host_decode_staged(stream, 0, False)[:2]
    return ica.binding.units_from_region(desc, region, False)
