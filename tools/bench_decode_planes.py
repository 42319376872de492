#!/usr/bin/env python3
"""Measures plane output (include/mij.h, PLANE OUTPUT; k_planes_out, TensorDecoder.decode_ycbcr) on 256 1080p 4:2:0 pictures at quality
90 -- 16 distinct synth_jpeg files, the rest repeated (clones of their coefficient planes for the kernel runs) -- all in one session:

  kernel   k_planes_out with planar and with NV12 destinations, and beside them the yardstick: k_idct_planes (pass 1 of the two-pass
           path, mij_batch_force_generic) on the same coefficient planes, which runs the same transform and stores the same samples to
           padded scratch planes.  Kernel times are those of `rocprofv3 --kernel-trace`, each variant in a child process of its own that
           only uploads once and launches --launches times; the variants are taken in turns, --rounds rounds.  With --parent-lib (the
           library built from the parent commit) the yardstick runs on that library, so the spread of ITS rounds is the spread the new
           kernel is judged against.  Bytes read are the compact planes' low bytes and DC terms of the components touched (escape
           bytes, which only escaped blocks read, are not counted); bytes written are the samples stored.
  call     decode_ycbcr (planar, nv12, luma only) against what a caller pays without it: decode(dtype=uint8, layout="HWC"), then
           RGB -> YCbCr and 2 x 2 mean pooling in torch.  Wall time around a device synchronise, the variants in turns inside every
           step, best of --steps after --warmup in each round.  No threshold.
  default  TensorDecoder.decode of the same files on this library and on --parent-lib, in child processes, in turns: the difference of
           the bests next to the spread of the parent's own rounds.

    python tools/bench_decode_planes.py [--n 256] [--steps 5] [--warmup 2] [--rounds 3] [--launches 20] [--parent-lib PATH]
                                        [--out profiles/decode_planes.json]
Not bench.py: nothing here is a yardstick."""
import argparse
import csv
import ctypes as C
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


def files(ica, a):
    return [ica.synth_jpeg(a.width, a.height, seed=100 + k, quality=90) for k in range(a.distinct)]


def geometry(ica, data):
    """-> (bytes of compact planes a full decode reads, samples stored to planes, samples stored to padded scratch planes, luma share of each)"""
    d = ica.HostDecoder.probe(data)
    tiles = [(d.comp[c].bw * d.comp[c].bh + 63) // 64 for c in range(d.ncomp)]
    rd = [t * (4096 + 128) for t in tiles]
    wr = [d.comp[c].x * d.comp[c].y for c in range(d.ncomp)]
    pad = [d.comp[c].bw * 8 * d.comp[c].bh * 8 for c in range(d.ncomp)]
    return rd, wr, pad


# ------------------------------------------------------------------ kernel runs (children under rocprofv3)

def hip_of_process():
    paths = {ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}
    h = C.CDLL(sorted(paths)[0])
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipFree.argtypes = [C.c_void_p]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return h


def kernel_child(a):
    """one variant: upload once, launch a.launches times; prints one JSON line with the event time per launch"""
    import numpy as np
    import image_codecs_amd as ica
    datas = files(ica, a)
    d = ica.HostDecoder.probe(datas[0])
    ctx = ica.Context()
    cb, ob = ica.Batch.coef_bytes(d), ica.Batch.out_bytes(d)
    b = ica.Batch(ctx, a.n, (cb + 256) * a.distinct, (cb + 256) * a.n, (ob + 256) * a.n)
    roots = [b.add_jpeg(x, 0) for x in datas]
    slots = roots + [b.add_clone(roots[k % a.distinct]) for k in range(a.distinct, a.n)]
    hip, dst, per = None, C.c_void_p(), 0
    if a.kernel_child == "idct_planes":
        b.force_generic(1)
    else:
        yw, yh, cw, ch = d.comp[0].x, d.comp[0].y, d.comp[1].x, d.comp[1].y
        ypitch, cpitch = -(-yw // 16) * 16, -(-cw // 16) * 16
        per = -(-(ypitch * yh + 2 * cpitch * ch) // 256) * 256
        hip = hip_of_process()
        assert hip.hipMalloc(C.byref(dst), per * a.n) == 0
        for k, sl in enumerate(slots):
            p = dst.value + k * per
            if a.kernel_child == "planar":
                req = [(p, ypitch, 1), (p + ypitch * yh, cpitch, 1), (p + ypitch * yh + cpitch * ch, cpitch, 1)]
            elif a.kernel_child == "nv12":
                req = [(p, ypitch, 1), (p + ypitch * yh, 2 * cpitch, 2), (p + ypitch * yh + 1, 2 * cpitch, 2)]
            else:
                req = [(p, ypitch, 1)]
            b.set_out_planes(sl, req)
    b.upload()
    b.launch()
    b.wait()
    kinds = sorted({b.slot_kernel(sl)[0] for sl in slots})
    b.timer_begin()
    for _ in range(a.launches):
        b.launch()
    b.timer_end()
    ms = b.timer_ms() / a.launches
    check = None
    if hip is not None:  # the last slot's luma against the host's own idea of the file: the first picture row of a clone equals its source's
        row = np.empty(d.comp[0].x, np.uint8)
        other = np.empty(d.comp[0].x, np.uint8)
        assert hip.hipMemcpy(row.ctypes.data_as(C.c_void_p), C.c_void_p(dst.value + (a.n - 1) * per), row.size, 2) == 0
        assert hip.hipMemcpy(other.ctypes.data_as(C.c_void_p), C.c_void_p(dst.value + ((a.n - 1) % a.distinct) * per), row.size, 2) == 0
        check = bool(np.array_equal(row, other))
    b.close()
    if hip is not None:
        hip.hipFree(dst)
    ctx.close()
    print(json.dumps({"variant": a.kernel_child, "event_ms_per_launch": ms, "kinds": kinds, "clone_equals_source": check}))


def trace_ms(outdir, a):
    """{kernel name stem: [durations in ms]} of a rocprofv3 kernel trace, the launches of the timed loop only (the last a.launches of each)"""
    rows = []
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    out = {}
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"]
        for stem in ("k_planes_out", "k_idct_planes", "k_resample", "k_fused420"):
            if stem in name:
                out.setdefault(stem, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    return out


def kernel_round(a, variant, lib):
    """-> {"kernel_ms": {stem: ms per launch}, "event_ms": ...}: one child under rocprofv3.  A launch of plane slots of both IDCT variants is two
    kernels; their times are added per launch"""
    outdir = tempfile.mkdtemp(prefix="planes_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", outdir, "--", sys.executable, os.path.abspath(__file__), "--kernel-child", variant,
               "--n", str(a.n), "--distinct", str(a.distinct), "--width", str(a.width), "--height", str(a.height), "--launches", str(a.launches)]
        p = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=900, env=dict(os.environ, MIJ_LIB=lib))
        child = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])
        tr = trace_ms(outdir, a)
    finally:
        shutil.rmtree(outdir, ignore_errors=True)
    ms = {}
    for stem, v in tr.items():
        per_launch = len(v) // (a.launches + 1)  # kernels of this stem per launch (the warm-up launch is the first)
        timed = v[per_launch:] if per_launch else v
        ms[stem] = sum(timed) / a.launches
    child["kernel_ms"] = ms
    return child


# ------------------------------------------------------------------ the default call (children, one per library and round)

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
            p = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=900, env=dict(os.environ, MIJ_LIB=lib))
            rows[name].append(json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1]))
            print("default %s: %.1f ms" % (name, rows[name][-1]["wall_ms"]), file=sys.stderr, flush=True)
    p, t = [r["wall_ms"] for r in rows["parent"]], [r["wall_ms"] for r in rows["this"]]
    return {"rounds": rows, "parent_ms": round(min(p), 3), "this_ms": round(min(t), 3), "this_minus_parent_ms": round(min(t) - min(p), 3),
            "parent_spread_ms": round(max(p) - min(p), 3), "this_spread_ms": round(max(t) - min(t), 3),
            "same_pixels": len({r["digest"] for r in rows["parent"] + rows["this"]}) == 1}


# ------------------------------------------------------------------ the calls

def torch_ycbcr420(torch, rgb):
    """what a caller does today with decode's [N, H, W, 3] uint8: JFIF's RGB -> YCbCr in float, chroma the mean of 2 x 2 pixels (edges
    repeated), rounded -> (Y [N, H, W], Cb, Cr [N, ceil(H / 2), ceil(W / 2)])"""
    ys, cbs, crs = [], [], []
    for i in range(0, rgb.shape[0], 16):  # in slices: the floats of 256 1080p pictures need not all live at once
        f = rgb[i:i + 16].float()
        r, g, b = f[..., 0], f[..., 1], f[..., 2]
        H, W = r.shape[-2:]
        pool = lambda c: torch.nn.functional.avg_pool2d(torch.nn.functional.pad(c[:, None], (0, W % 2, 0, H % 2), mode="replicate"), 2)[:, 0]
        ys.append((0.299 * r + 0.587 * g + 0.114 * b).round().clamp(0, 255).to(torch.uint8))
        cbs.append(pool(-0.16874 * r - 0.33126 * g + 0.5 * b + 128.0).round().clamp(0, 255).to(torch.uint8))
        crs.append(pool(0.5 * r - 0.41869 * g - 0.08131 * b + 128.0).round().clamp(0, 255).to(torch.uint8))
    return torch.cat(ys), torch.cat(cbs), torch.cat(crs)


def calls_round(ica, torch, datas, a):
    dec = ica.TensorDecoder("cuda:0")
    rows = {}

    def timed(key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        rows.setdefault(key, []).append((time.perf_counter() - t0) * 1e3)
        return out

    try:
        for step in range(a.warmup + a.steps):
            for fmt in ("planar", "nv12"):
                out = timed("decode_ycbcr_" + fmt, lambda: dec.decode_ycbcr(datas, format=fmt))
                assert all(w is None for w in out[1])
                del out
            out = timed("decode_ycbcr_luma_only", lambda: dec.decode_ycbcr(datas, luma_only=True))
            del out
            rgb, why = timed("decode_rgb_u8_hwc", lambda: dec.decode(datas, dtype=torch.uint8, layout="HWC"))
            ycc = timed("torch_rgb_to_ycbcr420", lambda: torch_ycbcr420(torch, rgb))
            del rgb, ycc
            print("step %d: %s" % (step, " ".join("%s %.1f" % (k, v[-1]) for k, v in rows.items())), file=sys.stderr, flush=True)
    finally:
        dec.close()
    return {k: min(v[a.warmup:]) for k, v in rows.items()}


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
    ap.add_argument("--parent-lib", default=None, help="the library built from the parent commit: the yardstick kernel and the default call run on it")
    ap.add_argument("--kernel-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--default-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernels", action="store_true", help="skip the kernel runs (they need rocprofv3)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "decode_planes.json"))
    a = ap.parse_args()
    if a.kernel_child:
        return kernel_child(a)
    if a.default_child:
        return default_child(a)
    res = {"n": a.n, "distinct": a.distinct, "width": a.width, "height": a.height, "quality": 90, "sampling": "420", "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "launches": a.launches, "parent_lib": bool(a.parent_lib)}
    if a.parent_lib:  # children first: this process has not touched the GPU yet
        res["default_against_parent"] = against_parent(a)
    import torch
    import image_codecs_amd as ica
    ica.build_library()
    if not ica.gpu_available():
        raise SystemExit("no HIP device: nothing here can be measured without one")
    distinct = files(ica, a)
    rd, wr, pad = geometry(ica, distinct[0])
    datas = [distinct[k % a.distinct] for k in range(a.n)]
    cr = [calls_round(ica, torch, datas, a) for _ in range(a.rounds)]
    calls = {}
    for k in cr[0]:
        v = [r[k] for r in cr]
        calls[k + "_ms"] = round(min(v), 3)
        calls[k + "_ms_spread"] = round(max(v) - min(v), 3)
    calls["via_rgb_and_torch_ms"] = round(calls["decode_rgb_u8_hwc_ms"] + calls["torch_rgb_to_ycbcr420_ms"], 3)
    res["call"] = calls
    torch.cuda.empty_cache()
    write(a, res)  # what is measured so far, should the profiler runs below fail
    if not a.no_kernels:
        variants = [("k_idct_planes_parent" if a.parent_lib else "k_idct_planes", "idct_planes", a.parent_lib or THIS_LIB), ("k_planes_out_planar", "planar", THIS_LIB),
                    ("k_planes_out_nv12", "nv12", THIS_LIB), ("k_planes_out_luma_only", "luma", THIS_LIB)]
        runs = {name: [] for name, _, _ in variants}
        for r in range(a.rounds):
            for name, variant, lib in variants:
                runs[name].append(kernel_round(a, variant, lib))
                print("round %d %s: %s (events %.3f ms per launch)" % (r, name, runs[name][-1]["kernel_ms"], runs[name][-1]["event_ms_per_launch"]), file=sys.stderr, flush=True)
        res["kernel_rounds"] = runs
        write(a, res)

        def row(name, stem, read, written):
            if any(stem not in r["kernel_ms"] for r in res["kernel_rounds"][name]):
                raise SystemExit("no %s in the kernel trace of %s: not measured (the partial results are in %s)" % (stem, name, a.out))
            v = [r["kernel_ms"][stem] for r in res["kernel_rounds"][name]]
            ev = [r["event_ms_per_launch"] for r in res["kernel_rounds"][name]]
            return {"ms": round(min(v), 4), "launch_event_ms": round(min(ev), 4), "ms_spread": round(max(v) - min(v), 4), "bytes_read": read * a.n, "bytes_written": written * a.n,
                    "tb_s": round((read + written) * a.n / min(v) / 1e9, 3)}
        yard = variants[0][0]
        res["kernel"] = {yard: row(yard, "k_idct_planes", sum(rd), sum(pad)), "k_planes_out_planar": row("k_planes_out_planar", "k_planes_out", sum(rd), sum(wr)),
                         "k_planes_out_nv12": row("k_planes_out_nv12", "k_planes_out", sum(rd), sum(wr)),
                         "k_planes_out_luma_only": row("k_planes_out_luma_only", "k_planes_out", rd[0], wr[0])}
        res["kernel"]["planar_minus_yardstick_ms"] = round(res["kernel"]["k_planes_out_planar"]["ms"] - res["kernel"][yard]["ms"], 4)
        res["kernel"]["yardstick_spread_ms"] = res["kernel"][yard]["ms_spread"]
        res["kernel"]["lds_staged_store_form"] = "not tried"
    write(a, res)
    print(json.dumps(res, sort_keys=True))


def write(a, res):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
