#!/usr/bin/env python3
"""Measures progressive output in the GPU transcode (Transcoder.transcode(progressive=True)) on the 256 1080p 4:2:0 q = 90 sources of the other
transcode benches -- 16 distinct synth_rgb pictures written by the project's writer, the rest repeated: optimised baseline and progressive,
taken in turns inside every step of one run.

Per mode: the whole call's wall time, the emission launches' event time (for progressive that includes its four launches in front of the
six), the stream bytes, and how many slots the host finished (forced EOB-run flushes, or no room).  Best of --steps after --warmup in each of
--rounds rounds, and the spread of the rounds' bests.

Non-progressive emission against the parent commit: with --parent DIR (a built checkout of the parent) the baseline mode is also measured in
child processes, one per round and tree, the two trees in turns (parent, this, parent, this, ...), and the difference of their bests is
reported next to the spread between the parent's own rounds.  No threshold is fixed here: none of these numbers existed before.
Not bench.py: nothing here is a yardstick.

    python tools/bench_transcode_progressive.py [--n 256] [--steps 5] [--warmup 2] [--rounds 3] [--parent DIR] [--out profiles/transcode_progressive.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("baseline", {}), ("progressive", {"progressive": True}))


def sources(ica, a):
    distinct = [ica.stbi_write_jpg_to_memory(ica.synth_rgb(a.width, a.height, seed=100 + k), 90) for k in range(a.distinct)]
    return [distinct[i % a.distinct] for i in range(a.n)]


def measure(ica, srcs, todo, steps, warmup):
    """-> {mode: {wall_ms, emit_ms: best of the timed steps; bytes_out, host_emitted}}"""
    t = ica.Transcoder()
    rows, last = {name: [] for name, _ in todo}, {}
    try:
        for step in range(warmup + steps):
            for name, kw in todo:
                t0 = time.perf_counter()
                out = t.transcode(srcs, optimize=True, copy_markers="none", **kw)
                wall = (time.perf_counter() - t0) * 1e3
                assert all(o is not None for o in out), t.last_reasons
                if step >= warmup:
                    rows[name].append((wall, t.last_timing["emit_ms"]))
                last[name] = out, t.last_host_emitted
                print("%s step %d: %.1f ms, emit %.3f ms, host %d" % (name, step, wall, t.last_timing["emit_ms"], t.last_host_emitted), file=sys.stderr, flush=True)
        return {name: {"wall_ms": round(min(r[0] for r in rows[name]), 3), "emit_ms": round(min(r[1] for r in rows[name]), 3),
                       "bytes_out": sum(len(o) for o in last[name][0]), "host_emitted": last[name][1]} for name, _ in todo}
    finally:
        t.close()


def worker(a):
    """one round of the baseline mode with the library of the tree at --tree, as a process of its own; prints one JSON line"""
    import torch  # noqa: F401  before the library is first loaded: one HIP runtime for both
    sys.path.insert(0, a.tree)
    import image_codecs_amd as ica
    ica.build_library()
    assert os.path.realpath(os.path.dirname(ica.__file__)).startswith(os.path.realpath(a.tree)), ica.__file__
    print(json.dumps(measure(ica, sources(ica, a), MODES[:1], a.steps, a.warmup)["baseline"]))


def against_parent(a):
    rows = {"parent": [], "this": []}
    for _ in range(a.rounds):
        for name, tree in (("parent", a.parent), ("this", HERE)):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--n", str(a.n), "--distinct", str(a.distinct), "--width", str(a.width),
                   "--height", str(a.height), "--steps", str(a.steps), "--warmup", str(a.warmup)]
            # each tree's own built library, never rebuilt behind the measurement's back
            env = dict(os.environ, MIJ_LIB=os.path.join(tree, "image-codecs_amd", "lib", "libimagecodecs_mi355x.so"))
            rows[name].append(json.loads(subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=600, env=env).stdout.decode().strip().splitlines()[-1]))
    out = {"rounds": rows}
    for key in ("wall_ms", "emit_ms"):
        p, t = [r[key] for r in rows["parent"]], [r[key] for r in rows["this"]]
        out[key] = {"parent": min(p), "this": min(t), "this_minus_parent": round(min(t) - min(p), 4), "parent_spread": round(max(p) - min(p), 4),
                    "this_spread": round(max(t) - min(t), 4)}
    out["same_bytes"] = len({r["bytes_out"] for r in rows["parent"] + rows["this"]}) == 1
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
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: baseline emission is measured against it")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "transcode_progressive.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    res = {"n": a.n, "distinct": a.distinct, "width": a.width, "height": a.height, "source_quality": 90, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "modes": {name: kw for name, kw in MODES}}
    if a.parent:  # first, and in processes of their own: this process has not touched the GPU yet
        res["baseline_against_parent"] = against_parent(a)
    import torch  # noqa: F401
    sys.path.insert(0, HERE)
    import image_codecs_amd as ica
    ica.build_library()
    if not ica.gpu_available():
        raise SystemExit("no HIP device: nothing here can be measured without one")
    srcs = sources(ica, a)
    res["bytes_in"] = sum(len(s) for s in srcs)
    print("sources ready", file=sys.stderr, flush=True)
    rounds = [measure(ica, srcs, MODES, a.steps, a.warmup) for _ in range(a.rounds)]
    for name, _ in MODES:
        out = {"rounds": [r[name] for r in rounds], "bytes_out": rounds[-1][name]["bytes_out"], "host_emitted": rounds[-1][name]["host_emitted"]}
        for key in ("wall_ms", "emit_ms"):
            vals = [r[name][key] for r in rounds]
            out[key] = min(vals)
            out[key + "_spread"] = round(max(vals) - min(vals), 4)
        res[name] = out
    res["progressive"]["bytes_out_over_baseline"] = round(res["progressive"]["bytes_out"] / res["baseline"]["bytes_out"], 5)
    for key in ("wall_ms", "emit_ms"):
        res["progressive"][key + "_over_baseline"] = round(res["progressive"][key] / res["baseline"][key], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
