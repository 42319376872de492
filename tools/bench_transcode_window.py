#!/usr/bin/env python3
"""Measures crop and greyscale in the GPU transcode (Transcoder.transcode(crop=, grey=)) on 256 1080p 4:2:0 q = 90 sources -- 16 distinct
synth_rgb pictures written by the project's writer, the rest repeated: the plain lossless transcode, the centred quarter, grey, and both
of those with orientation=6, taken in turns inside every step of one process so that all five see the same machine.

Event-timed: the conversion kernels alone (convert_ms: planes -> units, where the window is cut and the work list culled) and the
emission launches.  Wall: the whole Transcoder.transcode call, front end included -- the stream is sequential, so the front end walks the
whole picture whatever the window.  Per mode the best of --steps after --warmup in each of --rounds rounds, and the spread of the rounds'
bests; the plane tiles the last chunk queued; output bytes against source bytes.

One condition needs no baseline: the centred quarter reads and writes at most a quarter of the blocks plus partial tiles, so its
convert_ms must be below the plain conversion's of the same run ("crop_convert_below_plain"); if it is not, the culling is not working.
Not bench.py: nothing here is a yardstick.

    python tools/bench_transcode_window.py [--n 256] [--steps 5] [--warmup 2] [--rounds 3] [--out profiles/transcode_window.json]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def modes(w, h):
    """edge="trim": 1080 rows are no multiple of 16, and orientation 6 mirrors them; its displayed frame is (h trimmed) x w"""
    ht = h // 16 * 16
    return (("plain", {}), ("crop_quarter", {"crop": (w // 4, h // 4, w // 2, h // 2)}), ("grey", {"grey": True}),
            ("crop_quarter_orientation6", {"crop": (ht // 4, w // 4, ht // 2, w // 2), "orientation": 6, "edge": "trim"}),
            ("grey_orientation6", {"grey": True, "orientation": 6, "edge": "trim"}))


def measure(ica, srcs, todo, steps, warmup):
    """-> {mode: {wall_ms, convert_ms, emit_ms: best of the timed steps; tiles, bytes_out, host_emitted}}"""
    t = ica.Transcoder()
    rows = {name: [] for name, _ in todo}
    last = {}
    try:
        for step in range(warmup + steps):
            for name, kw in todo:
                t0 = time.perf_counter()
                out = t.transcode(srcs, optimize=True, copy_markers="none", **kw)  # synchronous: the streams are in host memory
                wall = (time.perf_counter() - t0) * 1e3
                assert all(o is not None for o in out), t.last_reasons
                if step >= warmup:
                    rows[name].append((wall, t.last_timing["convert_ms"], t.last_timing["emit_ms"]))
                last[name] = (sum(len(o) for o in out), t.last_host_emitted, t._enc.coef_tiles())
                print("%s step %d: %.1f ms, convert %.3f ms" % (name, step, wall, t.last_timing["convert_ms"]), file=sys.stderr, flush=True)
    finally:
        t.close()
    return {name: {"wall_ms": round(min(r[0] for r in rows[name]), 3), "convert_ms": round(min(r[1] for r in rows[name]), 4),
                   "emit_ms": round(min(r[2] for r in rows[name]), 3), "bytes_out": last[name][0], "host_emitted": last[name][1],
                   "tiles_last_chunk": last[name][2]} for name, _ in todo}


def summary(rounds, name):
    """the rounds' figures of one mode: the best, and the spread (largest minus smallest of the rounds' bests)"""
    out = {"rounds": [r[name] for r in rounds]}
    for key in ("wall_ms", "convert_ms", "emit_ms"):
        vals = [r[name][key] for r in rounds]
        out[key] = min(vals)
        out[key + "_spread"] = round(max(vals) - min(vals), 4)
    out["bytes_out"] = rounds[-1][name]["bytes_out"]
    out["tiles_last_chunk"] = rounds[-1][name]["tiles_last_chunk"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "transcode_window.json"))
    a = ap.parse_args()

    import torch  # noqa: F401  before the library is first loaded: one HIP runtime for both
    sys.path.insert(0, HERE)
    import image_codecs_amd as ica
    ica.build_library()
    if not ica.gpu_available():
        raise SystemExit("no HIP device: nothing here can be measured without one")
    distinct = [ica.stbi_write_jpg_to_memory(ica.synth_rgb(a.width, a.height, seed=100 + k), 90) for k in range(a.distinct)]
    srcs = [distinct[i % a.distinct] for i in range(a.n)]
    print("sources ready", file=sys.stderr, flush=True)
    todo = modes(a.width, a.height)
    rounds = [measure(ica, srcs, todo, a.steps, a.warmup) for _ in range(a.rounds)]
    res = {"n": a.n, "distinct": a.distinct, "width": a.width, "height": a.height, "source_quality": 90, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "bytes_in": sum(len(s) for s in srcs), "modes": {name: {k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()} for name, kw in todo}}
    for name, _ in todo:
        res[name] = summary(rounds, name)
        res[name]["bytes_out_over_bytes_in"] = round(res[name]["bytes_out"] / res["bytes_in"], 4)
        res[name]["convert_ms_over_plain"] = round(res[name]["convert_ms"] / res["plain"]["convert_ms"], 3)
    # in every round, not only at the best: the quarter's conversion is cheaper than the whole picture's
    res["crop_convert_below_plain"] = all(r["crop_quarter"]["convert_ms"] < r["plain"]["convert_ms"] for r in rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    if not res["crop_convert_below_plain"]:
        raise SystemExit("the centred quarter's conversion is not cheaper than the whole picture's: the work list is not culled")


if __name__ == "__main__":
    main()
