"""Resized tensor output measurements.  Writes profiles/tensor_resize.json.

  A-C  a resident batch of COUNT x 1080p 4:2:0 q=90 pictures (the distinct ones host-walked once, the rest clones), launched with and
       without resized requests, the two batches alternated in one process; the difference of the device-event times of the launches
       (median of STEPS) is k_out_resize's time.  A: whole picture -> 224 x 224, bilinear, CHW f16 normalised.  B: seeded
       random-resized crops (scale 0.08-1 of the area, ratio 3/4-4/3) -> 224 x 224 with random flips, CHW bf16 normalised.  C: case A
       with bicubic and with lanczos.  Reported: algorithmic bytes (3 bytes read per window pixel + 3 * element size written per output
       pixel) over that time, as a fraction of 8 TB/s.
  E2E  TensorDecoder.decode(size=(224, 224)) end to end on COUNT x 1080p (wall clock), in Gpix/s of source pixels.
  --kernel CASE  only launch case CASE's batch LAUNCHES times (run it under `rocprofv3 --kernel-trace --stats`, a run of its own).
Every case checks a few of its outputs against tests/resize_model.py applied to the oracle's pixels first."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_codecs_amd as ica  # noqa: E402  (after torch: one HIP runtime)
import resize_model as rm  # noqa: E402
import tensor_model as tm  # noqa: E402

W, H, S = 1920, 1080, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CASES = {"A_whole_bilinear_f16": (torch.float16, "bilinear", False), "B_rrc_bilinear_bf16": (torch.bfloat16, "bilinear", True),
         "C_whole_bicubic_f16": (torch.float16, "bicubic", False), "C_whole_lanczos_f16": (torch.float16, "lanczos", False)}


def resident(ctx, datas, count):
    d0 = ica.HostDecoder.probe(datas[0], 3)
    cb, ob = ica.Batch.coef_bytes(d0), ica.Batch.out_bytes(d0)
    b = ica.Batch(ctx, count, cb * len(datas), cb * count, ob * count)
    src = [b.add_jpeg(d, 3) for d in datas]
    slots = list(src)
    while len(slots) < count:
        slots.append(b.add_clone(src[len(slots) % len(src)]))
    return b, slots


def windows(case, count, rng):
    if not CASES[case][2]:
        return [(0, 0, W, H)] * count, [False] * count, [False] * count
    wins = []
    for _ in range(count):  # RandomResizedCrop's sampler
        while True:
            area = W * H * rng.uniform(0.08, 1.0)
            ratio = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
            w, h = int(round(np.sqrt(area * ratio))), int(round(np.sqrt(area / ratio)))
            if 0 < w <= W and 0 < h <= H:
                break
        wins.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return wins, [bool(v) for v in rng.integers(0, 2, count)], [bool(v) for v in rng.integers(0, 2, count)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel", choices=sorted(CASES))
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--e2e-images", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_resize.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ica.build_library()
    ctx = ica.Context(0)
    oracle = __import__("helpers").Oracle()
    datas = [ica.synth_jpeg(W, H, s, 90) for s in range(args.distinct)]
    wants = [oracle.load(d, 3)[1] for d in datas]
    rng = np.random.default_rng(3)
    plain, _ = resident(ctx, datas, args.count)
    plain.submit()
    plain.wait()
    result = {"count": args.count, "distinct": args.distinct, "steps": args.steps, "size": [S, S], "cases": {}}
    for case in ([args.kernel] if args.kernel else list(CASES)):
        dtype, filt, crop = CASES[case]
        wins, fx, fy = windows(case, args.count, rng)
        out = torch.empty((args.count, 3, S, S), dtype=dtype, device="cuda:0")
        b, slots = resident(ctx, datas, args.count)
        t = tm.tables(3, dtype, MEAN, STD)
        tb = t.view(tm.BITS[dtype]).numpy()
        st, es = out.stride(), out.element_size()
        t0 = time.perf_counter()
        for i, s in enumerate(slots):
            x0, y0, w, h = wins[i]
            b.set_out_tensor_resized(s, out.data_ptr() + i * st[0] * es, tm.CODE[dtype], "CHW", x0, y0, w, h, S, S, st[2], st[1], fx[i], fy[i], tb,
                                     filt)
        t_set = time.perf_counter() - t0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.submit()
        b.wait()
        t_first = time.perf_counter() - t0
        for i in (0, 1, args.count - 1):  # slot i is a clone of distinct picture i % distinct
            want = rm.window(wants[i % args.distinct], wins[i], (S, S), filt, fx[i], fy[i], "CHW", t, dtype)
            assert tm.same_bits(out[i], want), (case, i)
        if args.kernel:
            for _ in range(args.launches):
                b.launch()
            b.wait()
            print(json.dumps({"case": case, "launches": args.launches}))
            return
        ms = {"with": [], "without": []}
        for _ in range(args.steps):
            for name, bt in (("with", b), ("without", plain)):
                bt.launch()  # warm
                bt.timer_begin()
                bt.launch()
                bt.timer_end()
                bt.wait()
                ms[name].append(bt.timer_ms())
        mw, mo = float(np.median(ms["with"])), float(np.median(ms["without"]))
        nread = sum(w * h * 3 for (_, _, w, h) in wins)
        nwrite = args.count * S * S * 3 * es
        k = mw - mo
        result["cases"][case] = {"filter": filt, "dtype": str(dtype).replace("torch.", ""), "launch_ms_with": mw, "launch_ms_without": mo,
                                 "resize_pass_ms": k, "bytes_read": nread, "bytes_written": nwrite,
                                 "tb_per_s": (nread + nwrite) / (k * 1e-3) / 1e12 if k > 0 else None,
                                 "frac_of_8tbs": (nread + nwrite) / (k * 1e-3) / 8e12 if k > 0 else None,
                                 "host_set_requests_s": t_set, "first_submit_wait_s": t_first}
        print(json.dumps({case: result["cases"][case]}), flush=True)
        b.close()
        del out
        torch.cuda.empty_cache()
    plain.close()
    # E2E: whole 1080p pictures -> 224 x 224 CHW f16 normalised through TensorDecoder
    n = args.e2e_images
    jl = [datas[i % args.distinct] for i in range(n)]
    dec = ica.TensorDecoder("cuda:0")
    threads = min(16, os.cpu_count() or 1)
    got, _ = dec.decode(jl[:8], dtype=torch.float16, mean=MEAN, std=STD, threads=threads, size=(S, S))
    tdec = []
    for _ in range(3):
        t0 = time.perf_counter()
        got, reasons = dec.decode(jl, dtype=torch.float16, mean=MEAN, std=STD, threads=threads, size=(S, S))
        tdec.append(time.perf_counter() - t0)
        assert reasons == [None] * n
    assert tm.same_bits(got[n - 1], rm.window(wants[(n - 1) % args.distinct], (0, 0, W, H), (S, S), "bilinear", layout="CHW",
                                              table=tm.tables(3, torch.float16, MEAN, STD), dtype=torch.float16))
    dec.close()
    tt = float(np.median(tdec))
    result["e2e"] = {"images": n, "threads": threads, "size": [S, S], "tensor_decode_resized_s": tt, "source_gpix_s": n * W * H / tt / 1e9}
    print(json.dumps({"e2e": result["e2e"]}), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
