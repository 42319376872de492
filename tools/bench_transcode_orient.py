#!/usr/bin/env python3
"""Measures the reorienting transcode (Transcoder.transcode(orientation=o, edge="trim")) on the batch tools/bench_transcode.py uses -- 256
1080p 4:2:0 q = 90 sources, 16 distinct -- for o = 1..8: the conversion kernel (planes -> units, where the whole transform happens) and
the emission launches, event-timed.  edge="trim" because 1080 is no multiple of 16: the orientations that mirror y drop the last MCU row.

With --parent-lib (a library built from the parent commit) the parent's conversion kernel is measured on the same batch in the same
session: every round starts one child process per library, parent first, so the two alternate; a round's figure is the best of --steps
after --warmup, and the spread of a figure is (max - min) / min over the rounds.  o = 1 through the new entry point
(mij_enc_add_coef_oriented) should lie within that spread of the parent's kernel.  Not bench.py: nothing here is a yardstick.

    python tools/bench_transcode_orient.py [--parent-lib PATH] [--rounds 3] [--steps 5] [--warmup 2] [--out profiles/transcode_orient.json]
"""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    """one process, one library: the batch through the plain entry point ("plain") and, with the new library, through every orientation"""
    import image_codecs_amd as ica
    with open(a.sources, "rb") as f:
        srcs = pickle.load(f)
    t = ica.Transcoder()
    res = {}
    for key in (["plain"] if a.child == "parent" else ["plain"] + list(range(1, 9))):
        conv, emit, out_bytes = [], [], 0
        for step in range(a.warmup + a.steps):
            if key == "plain":
                out = t.transcode(srcs, copy_markers="none")
            else:
                out = t.transcode(srcs, copy_markers="none", orientation=key, edge="trim")
            assert all(o is not None for o in out), t.last_reasons
            if step >= a.warmup:
                assert t.last_host_emitted == 0
                conv.append(t.last_timing["convert_ms"])
                emit.append(t.last_timing["emit_ms"])
            out_bytes = sum(len(o) for o in out)
        res[str(key)] = {"convert_ms": min(conv), "emit_ms": min(emit), "bytes_out": out_bytes}
    t.close()
    print(json.dumps(res))


def spread(v):
    return round((max(v) - min(v)) / min(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcode_orient.json"))
    ap.add_argument("--child", choices=["parent", "new"], default=None)
    ap.add_argument("--sources", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import image_codecs_amd as ica
    ica.build_library()
    distinct = [ica.stbi_write_jpg_to_memory(ica.synth_rgb(a.width, a.height, seed=100 + k), 90) for k in range(a.distinct)]
    srcs = [distinct[i % a.distinct] for i in range(a.n)]
    print("sources ready", file=sys.stderr, flush=True)
    runs = {"parent": [], "new": []}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "sources.pickle")
        with open(path, "wb") as f:
            pickle.dump(srcs, f)
        for rnd in range(a.rounds):
            for which in (["parent"] if a.parent_lib else []) + ["new"]:
                env = dict(os.environ)
                if which == "parent":
                    env["MIJ_LIB"] = os.path.abspath(a.parent_lib)
                else:
                    env.pop("MIJ_LIB", None)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--sources", path, "--steps", str(a.steps), "--warmup", str(a.warmup)]
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    sys.exit("round %d, %s library: exit status %d\n%s" % (rnd, which, p.returncode, p.stderr[-2000:]))
                runs[which].append(json.loads(p.stdout.strip().splitlines()[-1]))
                print("round %d %s: %s" % (rnd, which, {k: round(v["convert_ms"], 4) for k, v in runs[which][-1].items()}), file=sys.stderr, flush=True)
    res = {"n": a.n, "distinct": a.distinct, "width": a.width, "height": a.height, "quality": 90, "edge": "trim", "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "bytes_in": sum(len(s) for s in srcs), "orientation": {}}
    base = min(r["1"]["convert_ms"] for r in runs["new"])
    for key in ["plain"] + [str(o) for o in range(1, 9)]:
        conv = [r[key]["convert_ms"] for r in runs["new"]]
        emit = [r[key]["emit_ms"] for r in runs["new"]]
        res["orientation"][key] = {"convert_ms": round(min(conv), 4), "convert_ms_rounds": [round(v, 4) for v in conv], "convert_spread": spread(conv),
                                   "convert_ratio_to_o1": round(min(conv) / base, 3), "emit_ms": round(min(emit), 3),
                                   "bytes_out": runs["new"][0][key]["bytes_out"]}
    if runs["parent"]:
        conv = [r["plain"]["convert_ms"] for r in runs["parent"]]
        res["parent"] = {"convert_ms": round(min(conv), 4), "convert_ms_rounds": [round(v, 4) for v in conv], "convert_spread": spread(conv),
                         "emit_ms": round(min(r["plain"]["emit_ms"] for r in runs["parent"]), 3),
                         "o1_over_parent": round(base / min(conv), 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
