"""Writes tests/golden/restart_libjpeg.npz: pairs of tiny JPEG files made by Pillow (libjpeg), one without and one with restart markers,
for tests/test_restart_host.py and tests/test_gpu_restart.py.  libjpeg is an independent judge of the writer's restart contract
(include/mij_host.h, RESTART INTERVALS): the lossless transcode of the plain file at the same interval must give the restart file's
bytes from its DRI segment on.

Every picture is uniform noise coded at quality 90 with optimize=False.  Run from the repository root:  python tests/golden/make_golden_restart.py
"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
# (name, sampling or None for grey, width, height, MCU width, MCU height)
SHAPES = [("444", "444", 40, 24, 8, 8), ("422", "422", 50, 33, 16, 8), ("420", "420", 83, 61, 16, 16), ("grey", None, 33, 17, 8, 8)]


def picture(name, w, h, grey):
    rng = np.random.default_rng([ord(c) for c in name] + [w, h])
    a = rng.integers(0, 256, (h, w) if grey else (h, w, 3), dtype=np.uint8)
    return Image.fromarray(a, "L" if grey else "RGB")


def encode(img, sampling, **kw):
    buf = io.BytesIO()
    if sampling is not None:
        kw["subsampling"] = SUBSAMPLING[sampling]
    img.save(buf, "JPEG", quality=90, optimize=False, **kw)
    return buf.getvalue()


def cases():
    """-> [(name, plain bytes, restart bytes, Ri, MCU count)]"""
    out = []
    for name, sampling, w, h, mw, mh in SHAPES:
        img = picture(name, w, h, sampling is None)
        plain = encode(img, sampling)
        mcu_x, mcu_y = (w + mw - 1) // mw, (h + mh - 1) // mh
        if sampling is not None:
            out.append((name + "_rows1", plain, encode(img, sampling, restart_marker_rows=1), mcu_x, mcu_x * mcu_y))
        for blocks in (1, 2):
            out.append(("%s_blocks%d" % (name, blocks), plain, encode(img, sampling, restart_marker_blocks=blocks), blocks, mcu_x * mcu_y))
    return out


def dri_of(data):
    """the interval a file's DRI segment declares (0 without one) and the offset of that segment"""
    i = 2
    while i + 4 <= len(data) and data[i] == 0xFF:
        m, n = data[i + 1], data[i + 2] << 8 | data[i + 3]
        if m == 0xDD:
            return data[i + 4] << 8 | data[i + 5], i
        if m == 0xDA:
            break
        i += 2 + n
    return 0, -1


def entropy(data):
    """the bytes behind the SOS segment up to EOI"""
    i = data.index(b"\xff\xda")
    return data[i + 2 + (data[i + 2] << 8 | data[i + 3]):-2]


def properties(cs):
    """what the set must contain (asserted here and by the tests)"""
    ends_ff = sum(len([1 for k in range(8) if b"\xff\x00\xff" + bytes([0xD0 + k]) in entropy(r)]) > 0 for _, _, r, _, _ in cs)
    intervals = [(-(-n // ri)) for _, _, _, ri, n in cs]
    assert ends_ff >= 1, "no interval whose padded last byte is 0xFF"
    assert max(intervals) >= 9, "no file with 9 intervals or more (marker wrap)"
    assert any(n % ri == 0 for _, _, _, ri, n in cs) and any(n % ri for _, _, _, ri, n in cs), "MCU count a multiple of Ri, and not"
    for name, _, r, ri, _ in cs:
        assert dri_of(r)[0] == ri, (name, dri_of(r), ri)


def main():
    cs = cases()
    properties(cs)
    arrays = {"names": np.array([c[0] for c in cs]), "ri": np.array([c[3] for c in cs], np.int32)}
    for name, plain, rst, _, _ in cs:  # the plain file once per shape: plain_<shape>, restart_<shape>_<interval>
        arrays["plain_" + name.split("_")[0]] = np.frombuffer(plain, np.uint8)
        arrays["restart_" + name] = np.frombuffer(rst, np.uint8)
    path = os.path.join(HERE, "restart_libjpeg.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 100 * 1024, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes,", len(cs), "pairs")


if __name__ == "__main__":
    main()
