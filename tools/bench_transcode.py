#!/usr/bin/env python3
"""Measures the lossless transcode (image_codecs_amd.Transcoder) on 256 1080p 4:2:0 q = 90 sources -- 16 distinct synth_rgb pictures
written by the project's writer, the rest repeated -- and, in the same run for comparison, TensorEncoder.encode of the decoded pictures
(decode to pixels, forward DCT and quantiser again: the lossy way to the same end).

Event-timed: the conversion kernel alone (planes -> units; its achieved TB/s over bytes read + written) and the emission launches.
Wall: Transcoder.transcode and TensorEncoder.encode, best of --steps after --warmup.  Not bench.py: nothing here is a yardstick.

    python tools/bench_transcode.py [--n 256] [--distinct 16] [--steps 5] [--warmup 2] [--out profiles/transcode.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # before the library is first loaded: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import image_codecs_amd as ica  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcode.json"))
    a = ap.parse_args()
    ica.build_library()
    pictures = [ica.synth_rgb(a.width, a.height, seed=100 + k) for k in range(a.distinct)]
    distinct = [ica.stbi_write_jpg_to_memory(p, 90) for p in pictures]
    srcs = [distinct[i % a.distinct] for i in range(a.n)]
    print("sources ready", file=sys.stderr, flush=True)
    # bytes the conversion kernel moves: the compact planes' main part (low bytes + DC array; escape bytes only for flagged blocks, which
    # a q = 90 picture has next to none of) read, the units written
    desc = ica.HostDecoder.probe(distinct[0], 0)
    tiles = sum((desc.comp[c].bw * desc.comp[c].bh + 63) // 64 for c in range(desc.ncomp))
    units = sum(desc.comp[c].bw * desc.comp[c].bh for c in range(desc.ncomp))
    conv_bytes = a.n * (tiles * (4096 + 128) + units * 128)

    res = {"n": a.n, "distinct": a.distinct, "width": a.width, "height": a.height, "quality": 90, "steps": a.steps, "warmup": a.warmup,
           "bytes_in": sum(len(s) for s in srcs), "conversion_bytes_moved": conv_bytes}
    t = ica.Transcoder()
    for optimize in (True, False):
        rows = []
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            out = t.transcode(srcs, optimize=optimize, copy_markers="none")
            wall = (time.perf_counter() - t0) * 1e3
            assert all(o is not None for o in out), t.last_reasons
            print("transcode optimize=%s step %d: %.1f ms" % (optimize, step, wall), file=sys.stderr, flush=True)
            if step >= a.warmup:
                rows.append((wall, t.last_timing["convert_ms"], t.last_timing["emit_ms"], t.last_host_emitted))
        best = min(rows)
        conv = min(r[1] for r in rows)
        emit = min(r[2] for r in rows)
        key = "optimized" if optimize else "plain"
        res[key] = {"wall_ms": round(best[0], 3), "convert_ms": round(conv, 4), "emit_ms": round(emit, 3),
                    "convert_share_of_emit": round(conv / emit, 4), "convert_TBps": round(conv_bytes / (conv * 1e-3) / 1e12, 3),
                    "host_emitted": best[3], "bytes_out": sum(len(o) for o in out),
                    "pictures_per_s_wall": round(a.n / (best[0] * 1e-3), 1)}
    assert out[0] == distinct[0], "the writer's own file is a fixed point of the plain transcode"
    t.close()

    # the lossy way: decode to pixels, encode again from device tensors (quality 90, optimised tables)
    tens = [torch.from_numpy(np.ascontiguousarray(ica.stbi_load_from_memory(d, 3)[0].transpose(2, 0, 1))).cuda() for d in distinct]
    batch = [tens[i % a.distinct] for i in range(a.n)]
    enc = ica.TensorEncoder()
    rows = []
    for step in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = enc.encode(batch, quality=90, optimize=True)
        wall = (time.perf_counter() - t0) * 1e3
        if step >= a.warmup:
            rows.append(wall)
    res["tensor_encode_optimized"] = {"wall_ms": round(min(rows), 3), "bytes_out": sum(len(o) for o in out),
                                      "pictures_per_s_wall": round(a.n / (min(rows) * 1e-3), 1)}
    enc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
