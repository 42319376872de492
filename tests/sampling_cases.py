"""Shared by the sampled-encoding tests (include/mij_host.h, SAMPLED ENCODING): pictures, the host walk of a stream into blocks by
coordinates, and the tables the tests ask for."""
import numpy as np

SAMPLINGS = ("444", "422", "440", "420", "grey")
FACTORS = {"444": (3, 1, 1), "422": (3, 2, 1), "440": (3, 1, 2), "420": (3, 2, 2), "grey": (1, 1, 1)}
# MCU columns two more than the strip length of the sampling's kernel, over three MCU rows: strips run over the ends of MCU rows and
# the last strip is partial (k_encode422: 32 MCUs of 16 x 8; k_encode440: 64 of 8 x 16; k_encode_grey: 256 of 8 x 8; 4:2:0: 32 of
# 16 x 16; 4:4:4: 64 of 8 x 8)
SEAM_SIZE = {"422": (544, 24), "440": (528, 48), "grey": (2064, 24), "420": (544, 48), "444": (528, 24)}
SMALL_SIZES = ((1, 1), (7, 5), (17, 9), (9, 17))


def picture(w, h, comp, seed):
    """smooth gradients plus noise, so that every quality leaves AC coefficients and the channels differ"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 5 + y * 3 + 40 * k) % 256 for k in range(comp)], axis=-1).astype(np.int32)
    return np.clip(base + rng.integers(-24, 25, size=(h, w, comp)), 0, 255).astype(np.uint8)


def own_sampling(quality):
    """what the writer itself picks"""
    return "420" if (quality or 90) <= 90 else "444"


def walk(ica, data):
    """host walk of a stream -> (TranscodePlan, units int16 [n, 64]) in the plan's unit order"""
    desc, region = ica.host_decode_staged(data, 0, True)
    compact = bool(desc.flags & 4)
    tplan, why = ica.transcode_plan(desc)
    assert tplan is not None, why
    du = ica.units_from_region(desc, region, compact)
    assert du is not None
    return tplan, du


def blocks(tplan, du):
    """units -> [luma [bh, bw, 64], Cb, Cr] (one entry for grey), by block coordinates"""
    mx, my = tplan.plan.mcu_x, tplan.plan.mcu_y
    lh, lv = (1, 1) if tplan.ncomp == 1 else (tplan.lh, tplan.lv)
    ny = lh * lv
    dpm = tplan.plan.du_per_mcu
    u = np.asarray(du).reshape(my, mx, dpm, 64)
    luma = u[:, :, :ny].reshape(my, mx, lv, lh, 64).transpose(0, 2, 1, 3, 4).reshape(my * lv, mx * lh, 64)
    out = [luma]
    for c in range(tplan.ncomp - 1):
        out.append(u[:, :, ny + c])
    return out


def stream_tables(data):
    """the DQT tables of a stream by identifier, zigzag order as written"""
    data = bytes(data)
    out, i = {}, 2
    while i + 4 <= len(data) and data[i] == 0xFF and data[i + 1] != 0xDA:
        n = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xDB:
            seg = data[i + 4:i + 2 + n]
            while seg:
                assert seg[0] >> 4 == 0
                out[seg[0] & 15] = list(seg[1:65])
                seg = seg[65:]
        i += 2 + n
    return out


def random_tables(seed):
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.integers(1, 256, 64)], [int(v) for v in rng.integers(1, 256, 64)]
