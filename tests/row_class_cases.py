"""Pictures whose block rows have chosen extent classes, for the row-extent table (include/mij.h, "row-extent table"; mij_kernels.h, "Row
classes"): every block row of every component holds small DC terms and ONE non-zero AC coefficient -- or none, or one beyond a byte -- at
a chosen position of a chosen block, so a row's class is that coefficient's and neighbouring rows differ (a band edge always lies between
two classes, and the halo rows of a band are of another class than its own).  Written through coef_cases.Case (all-ones tables), so the
planes are the generator's and the expected table follows from them alone."""
import numpy as np

import coef_cases as CC
import idct_model as M

# (row, col) of a row's one AC coefficient -> the class it gives its row; None: a DC-only row; "escape": 300 at (0, 1), class 1 by its
# position and 3 because the block escapes the byte range
PATTERNS = [None, (0, 1), (1, 0), (1, 1), (0, 2), (2, 0), (3, 3), (0, 4), (4, 0), (7, 7), "escape"]
CLASS_OF = [0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3]
PLACES = 4  # the row's first block, its last, and the blocks either side of a 64-block tile seam inside the row (where it has one)


def _block_of(place, by, bw):
    if place == 0:
        return 0
    if place == 1:
        return bw - 1
    seams = [bx for bx in range(1, bw) if (by * bw + bx) % 64 == 0]  # block bx opens a tile, bx - 1 closes one
    if not seams:
        return (bw // 2) if place == 2 else max(bw // 2 - 1, 0)
    return seams[0] - 1 if place == 2 else seams[0]


def make(layout, w, h, shift=0):
    """-> (coef_cases.Case, expected table): row r of component c takes pattern (r + shift + 4 c) mod 11 at place ((r + shift) // 11 + c) mod 4:
    44 rows see every pattern at every place, a few rows see several classes, and `shift` moves both from picture to picture"""
    planes = CC.blank(layout, w, h)
    want = []
    for c, p in enumerate(planes):
        bh, bw, _ = p.shape
        i = np.arange(bh * bw).reshape(bh, bw) + 17 * c + shift
        p[:, :, 0] = (i * 7) % 41 - 20
        for r in range(bh):
            k = (r + shift + 4 * c) % len(PATTERNS)
            pat = PATTERNS[k]
            bx = _block_of(((r + shift) // len(PATTERNS) + c) % PLACES, r, bw)
            if pat == "escape":
                p[r, bx, int(M.ZZ_OF_NAT[1])] = 300
            elif pat is not None:
                p[r, bx, int(M.ZZ_OF_NAT[8 * pat[0] + pat[1]])] = 3 if (r + c) % 2 else -3
            want.append(CLASS_OF[k])
    case = CC.Case("rows-%s-%dx%d-%d" % (layout, w, h, shift), "row_classes", layout, w, h, planes)
    assert not case.needs_wide()
    return case, np.array(want, np.uint8)


def table_of(nat_planes, wide=False):
    """the row-extent table of decoded coefficients ([bh, bw, 8, 8] natural per component): per block row the largest class of its blocks,
    an escaped block counting as 3; 3 throughout for a stream that needs the wide IDCT"""
    out = []
    for nat in nat_planes:
        cls = np.where(M.escaped(nat), 3, M.block_class(nat))
        out.append(cls.max(axis=1))
    t = np.concatenate(out).astype(np.uint8)
    return np.full_like(t, 3) if wide else t
