"""Region-of-interest decode measurements.  Writes profiles/roi.json.

Decode launch time of a resident batch of COUNT x 1080p 4:2:0 q=90 pictures (the distinct ones host-walked once, the rest clones), four
batches alternated in one process, device events, median of STEPS after a warm-up of 25 ms or more:
  none   no region: what the parent commit launches (same work lists, same kernels)
  a      section 4d's case 3: a random 224 x 224 window per picture
  b      section 4e's case B: a random-resized-crop window per picture (area 0.08 .. 1 of the picture, aspect 3/4 .. 4/3)
  c      a region equal to the whole picture, which the planner drops: expected equal to `none`
Each variant is reported with the share of the picture's MCUs its windows touch.  Inside every region the pixels of a few slots are checked
against the oracle before anything is timed."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library: one HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_codecs_amd as ica  # noqa: E402

W, H, S = 1920, 1080, 224


def rrc_window(r):
    """torchvision's RandomResizedCrop.get_params for scale (0.08, 1), ratio (3/4, 4/3)"""
    for _ in range(10):
        area = W * H * r.uniform(0.08, 1.0)
        ratio = math.exp(r.uniform(math.log(3 / 4), math.log(4 / 3)))
        w, h = int(round(math.sqrt(area * ratio))), int(round(math.sqrt(area / ratio)))
        if 0 < w <= W and 0 < h <= H:
            return int(r.integers(0, W - w + 1)), int(r.integers(0, H - h + 1)), w, h
    return (W - H) // 2, 0, H, H


def windows_of(kind, count, seed=1):
    r = np.random.default_rng(seed)
    if kind == "none":
        return [None] * count
    if kind == "a":
        return [(int(r.integers(0, W - S + 1)), int(r.integers(0, H - S + 1)), S, S) for _ in range(count)]
    if kind == "b":
        return [rrc_window(r) for _ in range(count)]
    return [(0, 0, W, H)] * count


def resident(ctx, datas, count, wins):
    d0 = ica.HostDecoder.probe(datas[0], 3)
    cb, ob = ica.Batch.coef_bytes(d0), ica.Batch.out_bytes(d0)
    b = ica.Batch(ctx, count, cb * len(datas), cb * count, ob * count)
    src = [b.add_jpeg(d, 3) for d in datas]
    slots = list(src)
    while len(slots) < count:
        slots.append(b.add_clone(src[len(slots) % len(src)]))
    for s, w in zip(slots, wins):
        if w is not None:
            b.set_roi(s, *w)
    return b, slots


def timed(batches, steps):
    """alternate the batches; -> median launch ms per name"""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.05:  # warm-up: well over 25 ms of launches
        for b in batches.values():
            b.launch()
        for b in batches.values():
            b.wait()
    ms = {k: [] for k in batches}
    for _ in range(steps):
        for k, b in batches.items():
            b.launch()
            b.timer_begin()
            b.launch()
            b.timer_end()
            b.wait()
            ms[k].append(b.timer_ms())
    return {k: float(np.median(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi.json"))
    args = ap.parse_args()
    ica.build_library()
    ctx = ica.Context(0)
    oracle = __import__("helpers").Oracle()
    datas = [ica.synth_jpeg(W, H, s, 90) for s in range(args.distinct)]
    want = [oracle.load(d, 3)[1] for d in datas[:2]]
    result = {"count": args.count, "distinct": args.distinct, "steps": args.steps, "picture": [W, H], "variants": {}}
    batches, share = {}, {}
    for kind in ("none", "a", "b", "c"):
        wins = windows_of(kind, args.count)
        b, slots = resident(ctx, datas, args.count, wins)
        b.submit()
        b.wait()
        mcus = 0
        for i, (sl, w) in enumerate(zip(slots, wins)):
            rx, ry, rw, rh = b.roi_rect(sl)
            mcus += (-(-(rx + rw) // 16) - rx // 16) * (-(-(ry + rh) // 16) - ry // 16)
            if i % args.distinct < 2 and (i < 2 * args.distinct or i >= args.count - args.distinct):  # pixels first
                x0, y0, ww, hh = w or (0, 0, W, H)
                assert np.array_equal(b.fetch(sl)[y0:y0 + hh, x0:x0 + ww], want[i % args.distinct][y0:y0 + hh, x0:x0 + ww]), (kind, i, w)
        batches[kind], share[kind] = b, mcus / (args.count * 120.0 * 68.0)
    ms = timed(batches, args.steps)
    for kind, b in batches.items():
        result["variants"][kind] = {"launch_ms": ms[kind], "mcu_share": share[kind], "vs_none": ms[kind] / ms["none"]}
        print(json.dumps({kind: result["variants"][kind]}), flush=True)
        b.close()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
