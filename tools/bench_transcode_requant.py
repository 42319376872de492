#!/usr/bin/env python3
"""Measures requantisation in the GPU transcode (Transcoder.transcode(quality=)) on 256 1080p 4:2:0 q = 90 sources -- 16 distinct
synth_rgb pictures written by the project's writer, the rest repeated: the plain lossless transcode, quality=75, and quality=75 with
orientation=6, taken in turns inside every step so that all three see the same machine.

Event-timed: the conversion kernels alone (convert_ms: planes -> units, where the requantisation happens) and the emission launches.
Wall: the whole Transcoder.transcode call.  Per mode the best of --steps after --warmup in each of --rounds rounds, and the spread of the
rounds' bests; output bytes against source bytes.

--parent DIR: a checkout of the parent commit with its library built.  Each round then starts a fresh child process that runs this file
against that tree (--plain-only: only arguments the parent knows) and one that runs it the same way against this tree ("plain_alone"),
before the three modes' own turn, so that the two libraries alternate on the same device in the same session and are compared like for
like: the "plain" row shares its process and its arena with the two requantising modes, "plain_alone" and "parent_plain" do not.
Not bench.py: nothing here is a yardstick.

    python tools/bench_transcode_requant.py [--parent DIR] [--n 256] [--steps 5] [--warmup 2] [--rounds 3] [--out profiles/transcode_requant.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# edge="trim": 1080 rows are no multiple of 16, and orientation 6 mirrors them
MODES = (("plain", {}), ("quality75", {"quality": 75}), ("quality75_orientation6", {"quality": 75, "orientation": 6, "edge": "trim"}))


def measure(ica, srcs, modes, steps, warmup):
    """-> {mode: {wall_ms, convert_ms, emit_ms: best of the timed steps; bytes_out, host_emitted, requantized}}"""
    t = ica.Transcoder()
    rows = {name: [] for name, _ in modes}
    last = {}
    try:
        for step in range(warmup + steps):
            for name, kw in modes:
                t0 = time.perf_counter()
                out = t.transcode(srcs, optimize=True, copy_markers="none", **kw)  # synchronous: the streams are in host memory
                wall = (time.perf_counter() - t0) * 1e3
                assert all(o is not None for o in out), t.last_reasons
                if step >= warmup:
                    rows[name].append((wall, t.last_timing["convert_ms"], t.last_timing["emit_ms"]))
                last[name] = (sum(len(o) for o in out), t.last_host_emitted, sum(getattr(t, "last_requantized", [])))
                print("%s step %d: %.1f ms, convert %.3f ms" % (name, step, wall, t.last_timing["convert_ms"]), file=sys.stderr, flush=True)
    finally:
        t.close()
    return {name: {"wall_ms": round(min(r[0] for r in rows[name]), 3), "convert_ms": round(min(r[1] for r in rows[name]), 4),
                   "emit_ms": round(min(r[2] for r in rows[name]), 3), "bytes_out": last[name][0], "host_emitted": last[name][1],
                   "requantized": last[name][2]} for name, _ in modes}


def summary(rounds, name):
    """the rounds' figures of one mode: the best, and the spread (largest minus smallest of the rounds' bests)"""
    out = {"rounds": [r[name] for r in rounds]}
    for key in ("wall_ms", "convert_ms", "emit_ms"):
        vals = [r[name][key] for r in rounds]
        out[key] = min(vals)
        out[key + "_spread"] = round(max(vals) - min(vals), 4)
    out["bytes_out"] = rounds[-1][name]["bytes_out"]
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
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, library built")
    ap.add_argument("--root", default=HERE, help="the tree whose package is measured (the child process of --parent uses it)")
    ap.add_argument("--plain-only", action="store_true", help="one round of the plain mode alone, its figures as one JSON line on stdout")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "transcode_requant.json"))
    a = ap.parse_args()

    import torch  # noqa: F401  before the library is first loaded: one HIP runtime for both
    sys.path.insert(0, os.path.abspath(a.root))
    import image_codecs_amd as ica
    ica.build_library()
    if not ica.gpu_available():
        raise SystemExit("no HIP device: nothing here can be measured without one")
    distinct = [ica.stbi_write_jpg_to_memory(ica.synth_rgb(a.width, a.height, seed=100 + k), 90) for k in range(a.distinct)]
    srcs = [distinct[i % a.distinct] for i in range(a.n)]
    print("sources ready (%s)" % a.root, file=sys.stderr, flush=True)
    if a.plain_only:
        print(json.dumps(measure(ica, srcs, MODES[:1], a.steps, a.warmup), sort_keys=True))
        return

    def child(root):
        cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", "--root", root, "--n", str(a.n), "--distinct", str(a.distinct),
               "--width", str(a.width), "--height", str(a.height), "--steps", str(a.steps), "--warmup", str(a.warmup)]
        # MIJ_LIB: that tree's library as it was built, never rebuilt behind its back (binding.build_library)
        env = dict(os.environ, MIJ_LIB=os.path.join(root, "image-codecs_amd", "lib", "libimagecodecs_mi355x.so"))
        done = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=600, env=env)
        return json.loads(done.stdout.decode().strip().splitlines()[-1])

    mine, alone, parent = [], [], []
    for r in range(a.rounds):
        if a.parent:
            parent.append(child(os.path.abspath(a.parent)))
            alone.append(child(HERE))
        mine.append(measure(ica, srcs, MODES, a.steps, a.warmup))
    res = {"n": a.n, "distinct": a.distinct, "width": a.width, "height": a.height, "source_quality": 90, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "bytes_in": sum(len(s) for s in srcs)}
    for name, _ in MODES:
        res[name] = summary(mine, name)
        res[name]["bytes_out_over_bytes_in"] = round(res[name]["bytes_out"] / res["bytes_in"], 4)
    res["parent_plain"] = summary(parent, "plain") if parent else None
    res["plain_alone"] = summary(alone, "plain") if alone else None
    for name in ("quality75", "quality75_orientation6"):
        res[name]["convert_ms_over_plain"] = round(res[name]["convert_ms"] / res["plain"]["convert_ms"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
