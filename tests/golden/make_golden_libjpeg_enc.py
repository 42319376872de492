"""Writes tests/golden/libjpeg_pillow_enc.npz: small pictures and the JPEG files Pillow (libjpeg-turbo) writes for them, for
tests/test_encode_libjpeg_host.py and tests/test_gpu_encode_libjpeg.py.  Pillow is the judge of the LIBJPEG ENCODING contract
(include/mij_host.h): tests/libjpeg_enc_model.py, the host twin and the kernels must give these files.  Nothing here reads the reference.

Files: samplings 4:4:4, 4:2:2, 4:2:0 and grey, each at the sizes of SIZES -- between them every right and bottom dummy-block case, the
corner where a dummy block feeds the dummy row under it, and the repeated chroma sample row -- with the qualities of QUALITIES and the
contents of CONTENTS cycling so that every sampling meets every quality and every content.  Per sampling one file each with
optimize=True, progressive=True and restart_marker_rows=1; one "YCbCr"-mode 4:4:4 file, whose source pixels are Y, Cb, Cr as they lie.
Grey files are written from "L" pictures: their sources are [H, W].  Run from the repository root:
python tests/golden/make_golden_libjpeg_enc.py
"""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
SAMPLINGS = ("444", "422", "420", "grey")
SIZES = [(1, 1), (7, 9), (8, 8), (9, 8), (8, 9), (16, 16), (17, 15), (24, 24), (33, 31), (40, 24), (97, 61), (160, 120)]
QUALITIES = [2, 50, 75, 90, 95, 100]
CONTENTS = ("natural", "noise", "saturated")
VARIANTS = {"o": {"optimize": True}, "p": {"progressive": True}, "r": {"restart_marker_rows": 1}}
VARIANT_SIZE, VARIANT_QUALITY = (97, 61), 75
YCC = ("ycc444", 24, 24, 90)


def picture(seed, w, h, grey, content):
    """uint8 [h, w] or [h, w, 3]"""
    rng = np.random.default_rng(seed)
    shape = (h, w) if grey else (h, w, 3)
    if content == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if content == "saturated":
        return (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    ramp = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), 128 + 100 * np.sin(x / 5.0) * np.cos(y / 7.0)], -1)
    return np.clip((ramp[..., 0] if grey else ramp) + rng.normal(0, 3.0, shape), 0, 255).astype(np.uint8)


def encode(pixels, sampling, quality, mode=None, **kw):
    from PIL import Image
    img = Image.fromarray(pixels, mode or ("L" if pixels.ndim == 2 else "RGB"))
    buf = io.BytesIO()
    if sampling != "grey":
        kw["subsampling"] = SUBSAMPLING[sampling]
    img.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def cases():
    """-> [(name, source pixels, Pillow's file)]; name: sampling _ WxH _ qQ _ content _ kind (b plain, o, p, r: VARIANTS)"""
    out = []
    for si, sampling in enumerate(SAMPLINGS):
        grey = sampling == "grey"
        for zi, (w, h) in enumerate(SIZES):
            quality, content = QUALITIES[(zi + si) % 6], CONTENTS[(zi + zi // 3 + si) % 3]
            if (w, h) == (160, 120):
                content = "natural"  # the large one compresses
            pix = picture([si, w, h, quality], w, h, grey, content)
            out.append(("%s_%dx%d_q%d_%s_b" % (sampling, w, h, quality, content), pix, encode(pix, sampling, quality)))
        w, h = VARIANT_SIZE
        for kind, kw in VARIANTS.items():
            pix = picture([si, w, h, ord(kind)], w, h, grey, "natural")
            out.append(("%s_%dx%d_q%d_natural_%s" % (sampling, w, h, VARIANT_QUALITY, kind), pix, encode(pix, sampling, VARIANT_QUALITY, **kw)))
    name, w, h, quality = YCC
    pix = picture([7, w, h], w, h, False, "noise")
    out.append(("%s_%dx%d_q%d_noise_b" % (name, w, h, quality), pix, encode(pix, "444", quality, mode="YCbCr")))
    return out


def properties(cs):
    """what the set must contain (asserted here and by the tests)"""
    names = [c[0] for c in cs]
    assert len(set(names)) == len(names)
    for sampling in SAMPLINGS:
        mine = [n.split("_") for n in names if n.startswith(sampling + "_")]
        assert {m[1] for m in mine} == {"%dx%d" % s for s in SIZES}, sampling
        assert {m[2] for m in mine} == {"q%d" % q for q in QUALITIES}, sampling
        assert {m[3] for m in mine} == set(CONTENTS) and {m[4] for m in mine} == {"b", "o", "p", "r"}, sampling
    assert sum(n.startswith("ycc444_") for n in names) == 1
    for name, pix, data in cs:
        data = bytes(data)
        kind = name.split("_")[4]
        w, h = (int(v) for v in name.split("_")[1].split("x"))
        assert pix.shape[:2] == (h, w) and pix.dtype == np.uint8 and (pix.ndim == 2) == name.startswith("grey_"), name
        assert (b"\xff\xc2" in data) == (kind == "p") and (b"\xff\xdd\x00\x04" in data) == (kind == "r"), name


def main():
    cs = cases()
    properties(cs)
    arrays = {"names": np.array([c[0] for c in cs])}
    for name, pix, data in cs:
        arrays["src_" + name] = pix
        arrays["jpg_" + name] = np.frombuffer(data, np.uint8)
    path = os.path.join(HERE, "libjpeg_pillow_enc.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 700 * 1024, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes,", len(cs), "files")


if __name__ == "__main__":
    main()
