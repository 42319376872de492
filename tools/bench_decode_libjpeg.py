#!/usr/bin/env python3
"""Measures the decode with libjpeg's arithmetic (include/mij.h, LIBJPEG ARITHMETIC; k_lj_idct, k_lj_color) on 256 1080p 4:2:0 pictures
at quality 90 -- 16 distinct synth_jpeg files, the rest clones of their coefficient planes -- all in one session:

  kernel   the two new kernels (mij_batch_set_arith on every slot); beside them the yardstick, the forced two-pass path
           (mij_batch_force_generic(1): k_idct_planes + k_resample_fast) on the same batch, on --parent-lib where given, so that the
           spread of ITS rounds is the spread the new path is judged against; and the default fused decode (k_fused420*), for scale.
           Kernel times are those of `rocprofv3 --kernel-trace`, each variant in a child process of its own that uploads once and
           launches --launches times; the variants are taken in turns, --rounds rounds.
  default  TensorDecoder.decode of the same files on this library and on --parent-lib, in child processes, in turns: the difference
           of the bests next to the spread of the parent's own rounds.

    python tools/bench_decode_libjpeg.py [--n 256] [--steps 5] [--warmup 2] [--rounds 3] [--launches 20] [--parent-lib PATH]
                                         [--out profiles/decode_libjpeg.json]
Not bench.py: nothing here is a yardstick, and there is no bar to clear."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
THIS_LIB = os.path.join(HERE, "image-codecs_amd", "lib", "libimagecodecs_mi355x.so")
STEMS = ("k_lj_idct", "k_lj_color", "k_idct_planes", "k_resample", "k_fused420")


def files(ica, a):
    return [ica.synth_jpeg(a.width, a.height, seed=100 + k, quality=90) for k in range(a.distinct)]


def kernel_child(a):
    """one variant: upload once, launch a.launches times; prints one JSON line with the event time per launch"""
    import image_codecs_amd as ica
    datas = files(ica, a)
    d = ica.HostDecoder.probe(datas[0], 3)
    ctx = ica.Context()
    cb, ob = ica.Batch.coef_bytes(d), ica.Batch.out_bytes(d)
    b = ica.Batch(ctx, a.n, (cb + 256) * a.distinct, (cb + 256) * a.n, (ob + 256) * a.n)
    roots = [b.add_jpeg(x, 3) for x in datas]
    slots = roots + [b.add_clone(roots[k % a.distinct]) for k in range(a.distinct, a.n)]
    if a.kernel_child == "two_pass":
        b.force_generic(1)
    elif a.kernel_child == "libjpeg":
        for sl in slots:
            b.set_arith(sl, ica.MIJ_ARITH_LIBJPEG)
    b.upload()
    b.launch()
    b.wait()
    paths = sorted({b.slot_path(sl) for sl in slots})
    b.timer_begin()
    for _ in range(a.launches):
        b.launch()
    b.timer_end()
    ms = b.timer_ms() / a.launches
    same = b.diff_slots([(slots[-1], slots[(a.n - 1) % a.distinct])]) == 0  # a clone's picture equals its source's
    b.close()
    ctx.close()
    print(json.dumps({"variant": a.kernel_child, "event_ms_per_launch": ms, "paths": paths, "clone_equals_source": bool(same)}))


def trace_ms(outdir):
    """{kernel name stem: [durations in ms, in start order]} of a rocprofv3 kernel trace"""
    rows = []
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    out = {}
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        for stem in STEMS:
            if stem in r["Kernel_Name"]:
                out.setdefault(stem, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    return out


def kernel_round(a, variant, lib):
    """one child under rocprofv3 -> its JSON line plus "kernel_ms": {stem: ms per launch} (the warm-up launch, the first, left out)"""
    outdir = tempfile.mkdtemp(prefix="libjpeg_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", outdir, "--", sys.executable, os.path.abspath(__file__), "--kernel-child", variant,
               "--n", str(a.n), "--distinct", str(a.distinct), "--width", str(a.width), "--height", str(a.height), "--launches", str(a.launches)]
        p = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=600, env=dict(os.environ, MIJ_LIB=lib))
        child = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])
        tr = trace_ms(outdir)
    finally:
        shutil.rmtree(outdir, ignore_errors=True)
    child["kernel_ms"] = {}
    for stem, v in tr.items():
        per_launch = len(v) // (a.launches + 1)
        child["kernel_ms"][stem] = sum(v[per_launch:]) / a.launches
    return child


def default_child(a):
    import torch
    import image_codecs_amd as ica
    datas = files(ica, a)
    datas = [datas[k % a.distinct] for k in range(a.n)]
    dec = ica.TensorDecoder("cuda:0")
    best, digest = None, None
    for step in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, why = dec.decode(datas, dtype=torch.uint8, layout="HWC")
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if step >= a.warmup:
            best = ms if best is None else min(best, ms)
        digest = int(out[-1].to(torch.int64).sum().item())
    dec.close()
    print(json.dumps({"wall_ms": best, "digest": digest}))


def against_parent(a):
    rows = {"parent": [], "this": []}
    for _ in range(a.rounds):
        for name, lib in (("parent", a.parent_lib), ("this", THIS_LIB)):
            cmd = [sys.executable, os.path.abspath(__file__), "--default-child", "--n", str(a.n), "--distinct", str(a.distinct), "--width", str(a.width), "--height",
                   str(a.height), "--steps", str(a.steps), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=600, env=dict(os.environ, MIJ_LIB=lib))
            rows[name].append(json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1]))
            print("default %s: %.1f ms" % (name, rows[name][-1]["wall_ms"]), file=sys.stderr, flush=True)
    p, t = [r["wall_ms"] for r in rows["parent"]], [r["wall_ms"] for r in rows["this"]]
    return {"rounds": rows, "parent_ms": round(min(p), 3), "this_ms": round(min(t), 3), "this_minus_parent_ms": round(min(t) - min(p), 3),
            "parent_spread_ms": round(max(p) - min(p), 3), "this_spread_ms": round(max(t) - min(t), 3),
            "same_pixels": len({r["digest"] for r in rows["parent"] + rows["this"]}) == 1}


def write(a, res):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the library built from the parent commit: the yardstick kernels and the default call run on it")
    ap.add_argument("--kernel-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--default-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "decode_libjpeg.json"))
    a = ap.parse_args()
    if a.kernel_child:
        return kernel_child(a)
    if a.default_child:
        return default_child(a)
    if a.parent_lib:
        a.parent_lib = os.path.abspath(a.parent_lib)
    res = {"n": a.n, "distinct": a.distinct, "width": a.width, "height": a.height, "quality": 90, "sampling": "420", "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "launches": a.launches, "parent_lib": bool(a.parent_lib)}
    yard = "two_pass_parent" if a.parent_lib else "two_pass"
    variants = [(yard, "two_pass", a.parent_lib or THIS_LIB), ("libjpeg", "libjpeg", THIS_LIB), ("fused", "fused", THIS_LIB)]
    runs = {name: [] for name, _, _ in variants}
    for r in range(a.rounds):
        for name, variant, lib in variants:
            runs[name].append(kernel_round(a, variant, lib))
            print("round %d %s: %s (events %.3f ms per launch)" % (r, name, runs[name][-1]["kernel_ms"], runs[name][-1]["event_ms_per_launch"]), file=sys.stderr, flush=True)
        res["kernel_rounds"] = runs
        write(a, res)  # what is measured so far

    def row(name, stems):
        out = {}
        for stem in stems:
            if any(stem not in r["kernel_ms"] for r in runs[name]):
                raise SystemExit("no %s in the kernel trace of %s: not measured (the partial results are in %s)" % (stem, name, a.out))
            v = [r["kernel_ms"][stem] for r in runs[name]]
            out[stem + "_ms"], out[stem + "_ms_spread"] = round(min(v), 4), round(max(v) - min(v), 4)
        tot = [sum(r["kernel_ms"][s] for s in stems) for r in runs[name]]
        ev = [r["event_ms_per_launch"] for r in runs[name]]
        out["total_ms"], out["total_ms_spread"], out["launch_event_ms"] = round(min(tot), 4), round(max(tot) - min(tot), 4), round(min(ev), 4)
        return out
    res["kernel"] = {yard: row(yard, ("k_idct_planes", "k_resample")), "libjpeg": row("libjpeg", ("k_lj_idct", "k_lj_color")), "fused": row("fused", ("k_fused420",))}
    res["kernel"]["libjpeg_minus_two_pass_ms"] = round(res["kernel"]["libjpeg"]["total_ms"] - res["kernel"][yard]["total_ms"], 4)
    res["kernel"]["two_pass_spread_ms"] = res["kernel"][yard]["total_ms_spread"]
    write(a, res)
    if a.parent_lib:
        res["default_against_parent"] = against_parent(a)
        write(a, res)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
