#!/usr/bin/env python3
"""Measures the pixel encoder per sampling ("444", "422", "440", "420", "grey"; include/mij_host.h, SAMPLED ENCODING) on 256 1080p CHW
uint8 pictures at quality 90 -- 16 distinct synth_rgb pictures, the rest repeated:

  transform   the strip kernel alone, pictures resident in HBM -> data units in HBM (event time of a launch without an emission arena),
              and the algorithmic bytes it reads and writes per second.  "420" and "444" run k_encode420 and k_encode444, the kernels a
              default slot runs, in the same run: they are the yardsticks for the three new kernels.
  encode      the whole TensorEncoder.encode(subsampling=...) call, wall time, and the bytes of the streams.

Best of --steps after --warmup in each of --rounds rounds, the samplings taken in turns inside every step, and the spread of the
rounds' bests.

The default call against the parent commit: with --parent DIR (a built checkout of the parent) encode() without the new arguments is
measured at quality 90 and 95 in child processes, one per round and tree, the two trees in turns, and the difference of their bests is
reported next to the spread between the parent's own rounds.  No threshold is fixed here: none of the sampling numbers existed before.
Not bench.py: nothing here is a yardstick.

    python tools/bench_encode_sampling.py [--n 256] [--steps 5] [--warmup 2] [--rounds 3] [--parent DIR] [--out profiles/encode_sampling.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("420", "444", "422", "440", "grey")
FACTORS = {"444": (3, 1, 1), "422": (3, 2, 1), "440": (3, 1, 2), "420": (3, 2, 2), "grey": (1, 1, 1)}


def algo_bytes(name, w, h):
    """bytes one picture's transform reads (staged packed RGB, whole MCU columns) and writes (its data units)"""
    ncomp, lh, lv = FACTORS[name]
    mx, my = -(-w // (8 * lh)), -(-h // (8 * lv))
    return mx * 8 * lh * h * 3, mx * my * (1 if ncomp == 1 else lh * lv + 2) * 128


def transform_ms(ica, ctx, a, launches=5):
    """-> {name: ms per launch over a.n pictures}, one round"""
    import numpy as np
    img = ica.synth_rgb(a.width, a.height, 0)
    out = {}
    for name in NAMES:
        rd, wr = algo_bytes(name, a.width, a.height)
        enc = ica.Encoder(ctx, a.n, (rd + 256) * a.n, (wr + 256) * a.n, stage_bytes=rd + 256)
        try:
            s0 = enc.add(img, 90, sampling=name)
            for _ in range(a.n - 1):
                enc.add_clone(s0)
            enc.upload()
            enc.launch()
            enc.wait()
            want = ica.host_transform_sampled(img, 90, name)[1]
            assert np.array_equal(enc.fetch(0), want) and np.array_equal(enc.fetch(a.n - 1), want), name
            for _ in range(3):
                enc.launch()
            enc.wait()
            enc.timer_begin()
            for _ in range(launches):
                enc.launch()
            enc.timer_end()
            out[name] = enc.timer_ms() / launches
        finally:
            enc.close()
    return out


def pictures(ica, a):
    import numpy as np
    import torch
    distinct = np.stack([ica.synth_rgb(a.width, a.height, seed=100 + k) for k in range(a.distinct)])
    t = torch.from_numpy(distinct).cuda().permute(0, 3, 1, 2).contiguous()  # [distinct, 3, H, W]
    return t[torch.arange(a.n, device=t.device) % a.distinct].contiguous()


def encode_ms(ica, batch, todo, steps, warmup):
    """-> {key: (best wall ms, stream bytes, host emitted)} for todo = [(key, kwargs of encode)], taken in turns inside every step"""
    t = ica.TensorEncoder()
    rows, last = {k: [] for k, _ in todo}, {}
    try:
        for step in range(warmup + steps):
            for key, kw in todo:
                t0 = time.perf_counter()
                out = t.encode(batch, **kw)
                ms = (time.perf_counter() - t0) * 1e3
                if step >= warmup:
                    rows[key].append(ms)
                last[key] = sum(len(o) for o in out), t.last_host_emitted
                print("%s step %d: %.1f ms" % (key, step, ms), file=sys.stderr, flush=True)
    finally:
        t.close()
    return {k: (min(rows[k]), last[k][0], last[k][1]) for k, _ in todo}


def worker(a):
    """one round of the default call at quality 90 and 95 with the library of the tree at --tree, as a process of its own"""
    import torch  # noqa: F401  before the library is first loaded: one HIP runtime for both
    sys.path.insert(0, a.tree)
    import image_codecs_amd as ica
    ica.build_library()
    assert os.path.realpath(os.path.dirname(ica.__file__)).startswith(os.path.realpath(a.tree)), ica.__file__
    res = encode_ms(ica, pictures(ica, a), [("q90", {"quality": 90}), ("q95", {"quality": 95})], a.steps, a.warmup)
    print(json.dumps({k: {"wall_ms": round(v[0], 3), "bytes_out": v[1]} for k, v in res.items()}))


def against_parent(a):
    rows = {"parent": [], "this": []}
    for _ in range(a.rounds):
        for name, tree in (("parent", a.parent), ("this", HERE)):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--n", str(a.n), "--distinct", str(a.distinct), "--width",
                   str(a.width), "--height", str(a.height), "--steps", str(a.steps), "--warmup", str(a.warmup)]
            # each tree's own built library, never rebuilt behind the measurement's back
            env = dict(os.environ, MIJ_LIB=os.path.join(tree, "image-codecs_amd", "lib", "libimagecodecs_mi355x.so"))
            rows[name].append(json.loads(subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=600, env=env).stdout.decode().strip().splitlines()[-1]))
    out = {"rounds": rows}
    for q in ("q90", "q95"):
        p, t = [r[q]["wall_ms"] for r in rows["parent"]], [r[q]["wall_ms"] for r in rows["this"]]
        out[q] = {"parent": min(p), "this": min(t), "this_minus_parent": round(min(t) - min(p), 4), "parent_spread": round(max(p) - min(p), 4),
                  "this_spread": round(max(t) - min(t), 4),
                  "same_bytes": len({r[q]["bytes_out"] for r in rows["parent"] + rows["this"]}) == 1}
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
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: the default call is measured against it")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "encode_sampling.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    res = {"n": a.n, "distinct": a.distinct, "width": a.width, "height": a.height, "quality": 90, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds}
    if a.parent:  # first, and in processes of their own: this process has not touched the GPU yet
        res["default_against_parent"] = against_parent(a)
    import torch  # noqa: F401
    sys.path.insert(0, HERE)
    import image_codecs_amd as ica
    ica.build_library()
    if not ica.gpu_available():
        raise SystemExit("no HIP device: nothing here can be measured without one")
    ctx = ica.Context()
    tr = [transform_ms(ica, ctx, a) for _ in range(a.rounds)]
    ctx.close()
    batch = pictures(ica, a)
    print("pictures ready", file=sys.stderr, flush=True)
    todo = [(name, {"quality": 90, "subsampling": name}) for name in NAMES]
    en = [encode_ms(ica, batch, todo, a.steps, a.warmup) for _ in range(a.rounds)]
    npx = a.n * a.width * a.height
    for name in NAMES:
        rd, wr = algo_bytes(name, a.width, a.height)
        t, e = [r[name] for r in tr], [r[name][0] for r in en]
        res[name] = {"transform_ms": round(min(t), 4), "transform_ms_spread": round(max(t) - min(t), 4),
                     "transform_bytes_read": rd * a.n, "transform_bytes_written": wr * a.n,
                     "transform_gb_s": round((rd + wr) * a.n / min(t) / 1e6, 1), "transform_mpix_s": round(npx / min(t) / 1e3, 1),
                     "encode_ms": round(min(e), 3), "encode_ms_spread": round(max(e) - min(e), 3), "encode_mpix_s": round(npx / min(e) / 1e3, 1),
                     "stream_bytes": en[-1][name][1], "host_emitted": en[-1][name][2]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
