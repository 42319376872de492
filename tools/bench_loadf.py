"""Float output measurements (DESIGN.md section "Float output").

  kernel  --content natural|noise   a resident batch of COUNT x 1080p 4:2:0 q=90 pictures, RGB, float output on every slot,
                                    launched LAUNCHES times: run it under `rocprofv3 --kernel-trace --stats` (a run of its own)
                                    for k_out_f32's time; prints the algorithmic bytes the conversion moves
  ab                                device-event time of the whole launch with and without float slots, the two batches
                                    alternated in the same process
  single                            one stbi_loadf_from_memory call against one stbi_load_from_memory call at 512^2, 1080p
                                    and 4096^2 (alternated; median of the last 3/4 of CALLS)
  threads                           THREADS threads loading 1080p pictures at once, 8-bit against float loader (wall clock)
Every mode checks a few of its outputs against stbi__ldr_to_hdr applied with libm's pow (tests/loadf_expect.py) first."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_codecs_amd as ica  # noqa: E402
import loadf_expect as fx  # noqa: E402

W, H = 1920, 1080


def picture(content, seed):
    if content == "noise":  # every byte independent: the LDS lookups of a wave spread over all banks
        rgb = np.random.default_rng(1000 + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
        return ica.stbi_write_jpg_to_memory(rgb, 90)
    return ica.synth_jpeg(W, H, seed, 90)


def resident(ctx, datas, count, f32):
    """count slots: the distinct pictures host-walked once, the rest clones (own device buffers); float output on every slot"""
    d0 = ica.HostDecoder.probe(datas[0], 3)
    cb, ob = ica.Batch.coef_bytes(d0), ica.Batch.out_bytes(d0)
    b = ica.Batch(ctx, count, cb * len(datas), cb * count, ob * count)
    src = [b.add_jpeg(d, 3) for d in datas]
    for i in range(len(datas), count):
        b.add_clone(src[i % len(datas)])
    if f32:
        b.reserve_out_f32(ica.Batch.out_f32_bytes(d0) * count)
        for s in range(count):
            b.set_out_f32(s)
    b.upload()
    b.wait()
    return b


def check(b, slots):
    t = fx.lut(3)
    for s in slots:
        assert fx.same_bits(b.fetch_f32(s), fx.apply(t, b.fetch(s))), "slot %d: floats differ from the table applied to its bytes" % s


def mode_kernel(args):
    ctx = ica.Context()
    datas = [picture(args.content, s) for s in range(4)]
    b = resident(ctx, datas, args.count, True)
    b.launch()
    b.wait()
    check(b, [0, 1, args.count - 1])
    for _ in range(args.launches):
        b.launch()
    b.wait()
    rd, wr = 3 * W * H, 4 * 3 * W * H
    print(json.dumps({"mode": "kernel", "content": args.content, "count": args.count, "launches": args.launches,
                      "algo_bytes_per_picture": rd + wr, "algo_bytes_per_launch": (rd + wr) * args.count,
                      "floor_ms_at_8TBps": round((rd + wr) * args.count / 8e12 * 1e3, 3)}))
    b.close()
    ctx.close()


def mode_ab(args):
    ctx = ica.Context()
    datas = [picture("natural", s) for s in range(4)]
    plain, flt = resident(ctx, datas, args.count, False), resident(ctx, datas, args.count, True)
    for bt in (plain, flt):
        for _ in range(3):
            bt.launch()
        bt.wait()
    check(flt, [0, args.count - 1])
    ms = {"plain": [], "f32": []}
    for _ in range(args.rounds):
        for name, bt in (("plain", plain), ("f32", flt)):
            bt.timer_begin()
            for _ in range(args.steps):
                bt.launch()
            bt.timer_end()
            bt.wait()
            ms[name].append(bt.timer_ms() / args.steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps({"mode": "ab", "count": args.count, "steps": args.steps, "rounds": args.rounds,
                      "launch_ms_median": {k: round(v, 3) for k, v in med.items()},
                      "launch_ms_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                      "f32_pass_ms": round(med["f32"] - med["plain"], 3)}))
    plain.close()
    flt.close()
    ctx.close()


def mode_single(args):
    out = {}
    for (w, h) in ((512, 512), (1920, 1080), (4096, 4096)):
        data = ica.stbi_write_jpg_to_memory(ica.synth_rgb(w, h, 1), 90)
        u8 = ica.stbi_load_from_memory(data, 3)[0]
        assert fx.same_bits(ica.stbi_loadf_from_memory(data, 3)[0], fx.apply(fx.lut(3), u8))
        ts = {"load": [], "loadf": []}
        for i in range(args.calls):
            for name, fn in (("load", ica.lib().stbi_load_from_memory), ("loadf", ica.lib().stbi_loadf_from_memory)):
                x, y, c = ica.binding.C.c_int(), ica.binding.C.c_int(), ica.binding.C.c_int()
                t0 = time.perf_counter()
                p = fn(data, len(data), x, y, c, 3)
                ts[name].append(time.perf_counter() - t0)
                assert p
                ica.lib().stbi_image_free(p)
        row = {k + "_ms": round(float(np.median(v[args.calls // 4:])) * 1e3, 3) for k, v in ts.items()}
        row["pixels"] = w * h
        out["%dx%d" % (w, h)] = row
    print(json.dumps({"mode": "single", "calls": args.calls, "median_ms": out}))


def mode_threads(args):
    """THREADS threads, each making CALLS calls on its own 1080p picture: the 8-bit loader and the float loader in turn, wall clock"""
    import threading
    datas = [ica.synth_jpeg(W, H, s, 90) for s in range(args.threads)]
    u8 = ica.stbi_load_from_memory(datas[0], 3)[0]
    assert fx.same_bits(ica.stbi_loadf_from_memory(datas[0], 3)[0], fx.apply(fx.lut(3), u8))
    L = ica.lib()
    C = ica.binding.C
    out = {}
    for rnd in range(args.rounds):
        for name, fn in (("load", L.stbi_load_from_memory), ("loadf", L.stbi_loadf_from_memory)):
            def run(i):
                x, y, c = C.c_int(), C.c_int(), C.c_int()
                for _ in range(args.calls):
                    p = fn(datas[i], len(datas[i]), x, y, c, 3)
                    assert p
                    L.stbi_image_free(p)
            ts = [threading.Thread(target=run, args=(i,)) for i in range(args.threads)]
            t0 = time.perf_counter()
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            dt = time.perf_counter() - t0
            if rnd:  # the first round warms every thread's batch
                out.setdefault(name, []).append(round(args.threads * args.calls * W * H / dt / 1e9, 3))
    print(json.dumps({"mode": "threads", "threads": args.threads, "calls_per_thread": args.calls, "picture": "%dx%d" % (W, H),
                      "gpix_per_s": out, "gpix_per_s_median": {k: float(np.median(v)) for k, v in out.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "ab", "single", "threads"])
    ap.add_argument("--content", choices=["natural", "noise"], default="natural")
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    ica.build_library()
    if not ica.gpu_available():
        raise SystemExit("bench_loadf: no HIP device (measurements need the GPU)")
    ica.lib()
    L = ica.lib()
    P = ica.binding.C.POINTER
    L.stbi_loadf_from_memory.restype = P(ica.binding.C.c_float)
    L.stbi_loadf_from_memory.argtypes = L.stbi_load_from_memory.argtypes
    {"kernel": mode_kernel, "ab": mode_ab, "single": mode_single, "threads": mode_threads}[args.mode](args)


if __name__ == "__main__":
    main()
