"""Writes tests/golden/libjpeg_pillow.npz: small JPEG files made by Pillow (libjpeg-turbo) and the pixels Pillow decodes them to --
convert("RGB"), or "L" for grey files -- for tests/test_libjpeg_model_host.py and tests/test_gpu_libjpeg.py.  Pillow is the judge of the
LIBJPEG ARITHMETIC contract (include/mij.h): tests/libjpeg_model.py and the kernels must give these bytes.  Nothing here reads the
reference.

Files: samplings 4:4:4, 4:2:2, 4:2:0 and grey, each at the sizes of SIZES (1 x 1 up to 97 x 61: the unfiltered small-width rule, odd
chroma sizes, the edge clamps, whole and partial MCUs), one baseline and one progressive file per sampling and size, with quality
(30, 75, 95, 100, and 2 for the clamps) and content (noise, ramp) cycling so that every sampling meets every quality and both contents;
one 160 x 120 4:2:0 file, large enough for the GPU Huffman walk; and 4:4:0 files.  Pillow cannot write 4:4:0, but a square 4:2:2 file
has as many MCUs as a 4:4:0 file of its size, each with the same blocks: with luma's sampling byte in SOF changed from 0x21 to 0x12 it
is a valid 4:4:0 file, which Pillow decodes.  Run from the repository root:
python tests/golden/make_golden_libjpeg.py
"""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
SIZES = [(1, 1), (2, 2), (3, 5), (4, 4), (5, 3), (7, 9), (8, 8), (15, 17), (16, 16), (17, 15), (31, 33), (33, 31), (97, 61)]
QUALITIES = [30, 75, 95, 100, 2]
SIZES_440 = [1, 7, 9, 16, 17, 33]
WALK = ("420", 160, 120, 90, "ramp")  # the GPU Huffman walk's file


def picture(seed, w, h, grey, content):
    from PIL import Image
    rng = np.random.default_rng(seed)
    shape = (h, w) if grey else (h, w, 3)
    if content == "noise":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
    else:
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        ramp = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), (x + y) * 255.0 / max(w + h - 2, 1)], -1)
        a = np.clip((ramp[..., 0] if grey else ramp) + rng.normal(0, 4.0, shape), 0, 255).astype(np.uint8)
    return Image.fromarray(a, "L" if grey else "RGB")


def encode(img, sampling, quality, progressive):
    buf = io.BytesIO()
    kw = {} if sampling == "grey" else {"subsampling": SUBSAMPLING[sampling]}
    img.save(buf, "JPEG", quality=quality, progressive=progressive, **kw)
    return buf.getvalue()


def pillow_pixels(data, grey):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.mode == ("L" if grey else "RGB"), im.mode
    return np.asarray(im if grey else im.convert("RGB")).copy()


def as_440(data):
    """a 4:2:2 file -> the same bytes with luma's sampling byte 0x21 -> 0x12"""
    i = 2
    while data[i + 1] != 0xC0:
        assert data[i] == 0xFF and data[i + 1] != 0xDA, i
        i += 2 + (data[i + 2] << 8 | data[i + 3])
    at = i + 4 + 6 + 1
    assert data[at] == 0x21 and data[at + 3] == 0x11 and data[at + 6] == 0x11
    return data[:at] + b"\x12" + data[at + 1:]


def cases():
    """-> [(name, file bytes, Pillow's pixels)]"""
    out = []
    for si, sampling in enumerate(("444", "422", "420", "grey")):
        for zi, (w, h) in enumerate(SIZES):
            for progressive in (False, True):
                k = zi + si + (2 if progressive else 0)
                quality, content = QUALITIES[k % 5], ("noise", "ramp")[(zi + progressive) % 2]
                name = "%s_%dx%d_q%d_%s_%s" % (sampling, w, h, quality, content, "p" if progressive else "b")
                data = encode(picture([si, w, h, quality, progressive], w, h, sampling == "grey", content), sampling, quality, progressive)
                out.append((name, data, pillow_pixels(data, sampling == "grey")))
    for zi, n in enumerate(SIZES_440):
        quality, content = QUALITIES[zi % 5], ("noise", "ramp")[zi % 2]
        data = as_440(encode(picture([440, n, quality], n, n, False, content), "422", quality, False))
        out.append(("440_%dx%d_q%d_%s_b" % (n, n, quality, content), data, pillow_pixels(data, False)))
    sampling, w, h, quality, content = WALK
    data = encode(picture([9, w, h], w, h, False, content), sampling, quality, False)
    out.append(("%s_%dx%d_q%d_%s_b" % (sampling, w, h, quality, content), data, pillow_pixels(data, False)))
    return out


def properties(cs):
    """what the set must contain (asserted here and by the tests)"""
    names = [c[0] for c in cs]
    assert len(set(names)) == len(names)
    for sampling in ("444", "422", "420", "grey"):
        mine = [n.split("_") for n in names if n.startswith(sampling + "_")]
        assert {m[2] for m in mine} >= {"q%d" % q for q in QUALITIES}, sampling
        assert {m[3] for m in mine} == {"noise", "ramp"} and {m[4] for m in mine} == {"b", "p"}, sampling
    for name, data, pix in cs:
        assert (b"\xff\xc2" in data) == name.endswith("_p"), name
        w, h = (int(v) for v in name.split("_")[1].split("x"))
        assert pix.shape[:2] == (h, w) and pix.dtype == np.uint8, name


def main():
    cs = cases()
    properties(cs)
    arrays = {"names": np.array([c[0] for c in cs])}
    for name, data, pix in cs:
        arrays["jpg_" + name] = np.frombuffer(data, np.uint8)
        arrays["pix_" + name] = pix
    path = os.path.join(HERE, "libjpeg_pillow.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 700 * 1024, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes,", len(cs), "files")


if __name__ == "__main__":
    main()
