"""Writes tests/golden/progressive_libjpeg.npz: pairs of tiny JPEG files made by Pillow (libjpeg) from the same picture at quality 90, one
baseline with optimize=True and one with progressive=True, for tests/test_progressive_host.py and tests/test_gpu_progressive.py.  libjpeg
is an independent judge of the writer's progressive contract (include/mij_host.h, PROGRESSIVE STREAMS): the lossless transcode of the
plain file with the progressive request must give the progressive file's bytes from its SOF2 segment on.

Four pictures are uniform noise; the fifth is a blurred ramp with mild noise, so that end-of-band runs longer than one block and
refinement correction bits occur (noise alone gives almost no runs).  Run from the repository root:
python tests/golden/make_golden_progressive.py
"""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
# (name, sampling or None for grey, width, height, smooth)
SHAPES = [("444", "444", 40, 24, False), ("422", "422", 50, 33, False), ("420", "420", 83, 61, False), ("grey", None, 33, 17, False),
          ("smooth", "420", 200, 133, True)]
# components: Ss, Se, Ah, Al -- jpeg_simple_progression as libjpeg-turbo writes it
SCRIPT_COLOUR = [((1, 2, 3), 0, 0, 0, 1), ((1,), 1, 5, 0, 2), ((3,), 1, 63, 0, 1), ((2,), 1, 63, 0, 1), ((1,), 6, 63, 0, 2), ((1,), 1, 63, 2, 1),
                 ((1, 2, 3), 0, 0, 1, 0), ((3,), 1, 63, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0)]
SCRIPT_GREY = [((1,), 0, 0, 0, 1), ((1,), 1, 5, 0, 2), ((1,), 6, 63, 0, 2), ((1,), 1, 63, 2, 1), ((1,), 0, 0, 1, 0), ((1,), 1, 63, 1, 0)]


def picture(name, w, h, grey, smooth):
    from PIL import Image, ImageFilter
    rng = np.random.default_rng([ord(c) for c in name] + [w, h])
    if not smooth:
        return Image.fromarray(rng.integers(0, 256, (h, w) if grey else (h, w, 3), dtype=np.uint8), "L" if grey else "RGB")
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    ramp = np.stack([x * 255.0 / w, y * 255.0 / h, (x + y) * 255.0 / (w + h)], -1)
    a = np.clip(ramp + rng.normal(0, 6.0, (h, w, 3)), 0, 255).astype(np.uint8)
    return Image.fromarray(a, "RGB").filter(ImageFilter.GaussianBlur(1.5))


def encode(img, sampling, **kw):
    buf = io.BytesIO()
    if sampling is not None:
        kw["subsampling"] = SUBSAMPLING[sampling]
    img.save(buf, "JPEG", quality=90, **kw)
    return buf.getvalue()


def segments(data):
    """[(marker, payload, offset)] of every marker segment; an SOS payload is its header only, the entropy-coded bytes are skipped"""
    out, i = [], 2
    while i + 4 <= len(data):
        assert data[i] == 0xFF, i
        m, n = data[i + 1], data[i + 2] << 8 | data[i + 3]
        if m == 0xD9:
            break
        out.append((m, data[i + 4:i + 2 + n], i))
        i += 2 + n
        if m == 0xDA:
            while not (data[i] == 0xFF and data[i + 1] != 0 and not 0xD0 <= data[i + 1] <= 0xD7):
                i += 1
    return out


def scan_script(data):
    """the scans of a file as the SCRIPT lists above write them"""
    out = []
    for m, p, _ in segments(data):
        if m == 0xDA:
            n = p[0]
            out.append((tuple(p[1 + 2 * k] for k in range(n)), p[1 + 2 * n], p[2 + 2 * n], p[3 + 2 * n] >> 4, p[3 + 2 * n] & 15))
    return out


def ac_symbols(data):
    """every HUFFVAL of the file's AC tables"""
    vals = []
    for m, p, _ in segments(data):
        if m == 0xC4 and p[0] >> 4 == 1:
            vals += list(p[17:17 + sum(p[1:17])])
    return vals


def cases():
    """-> [(name, plain bytes, progressive bytes)]"""
    out = []
    from PIL import Image
    for name, sampling, w, h, smooth in SHAPES:
        img = picture(name, w, h, sampling is None, smooth)
        plain, prog = encode(img, sampling, optimize=True), encode(img, sampling, progressive=True)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(plain))), np.asarray(Image.open(io.BytesIO(prog)))), name
        out.append((name, plain, prog))
    return out


def properties(cs):
    """what the set must contain (asserted here and by the tests)"""
    for name, plain, prog in cs:
        assert scan_script(prog) == (SCRIPT_GREY if name == "grey" else SCRIPT_COLOUR), (name, scan_script(prog))
        assert len(scan_script(plain)) == 1 and b"\xff\xc2" in prog[:700] and b"\xff\xc0" in plain[:700]
    runs = [v for _, _, prog in cs for v in ac_symbols(prog) if v & 15 == 0 and 1 <= v >> 4 <= 14]
    assert runs, "no EOBn symbol with n >= 1 in any AC table"


def main():
    cs = cases()
    properties(cs)
    arrays = {"names": np.array([c[0] for c in cs])}
    for name, plain, prog in cs:
        arrays["plain_" + name] = np.frombuffer(plain, np.uint8)
        arrays["progressive_" + name] = np.frombuffer(prog, np.uint8)
    path = os.path.join(HERE, "progressive_libjpeg.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 100 * 1024, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes,", len(cs), "pairs")


if __name__ == "__main__":
    main()
