"""Tensor output measurements.  Writes profiles/tensor_out.json.

  1-3  a resident batch of COUNT x 1080p 4:2:0 q=90 pictures (the distinct ones host-walked once, the rest clones), launched with and
       without tensor requests, the two batches alternated in one process; the difference of the device-event times of the launches
       is k_out_tensor's time.  Cases: whole picture CHW f16 normalised, HWC u8, CHW f32, and COUNT random 224 x 224 crops with random
       flips (bf16 CHW).  Reported: algorithmic bytes (n_out bytes read + n_out * element size written per pixel of the window) over
       that time, as a fraction of 8 TB/s.
  4    TensorDecoder.decode end to end on COUNT x 1080p (wall clock, Gpix/s) next to Batch.decode_jpegs + fetch to host.
  --kernel CASE  only launch case CASE's batch LAUNCHES times (run it under `rocprofv3 --kernel-trace --stats`, a run of its own).
Every case checks a few of its outputs against tests/tensor_model.py applied to the oracle's pixels first."""
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
import tensor_model as tm  # noqa: E402

W, H = 1920, 1080
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CASES = {"chw_f16_norm": (torch.float16, "CHW", True, False), "hwc_u8": (torch.uint8, "HWC", False, False),
         "chw_f32_norm": (torch.float32, "CHW", True, False), "crop224_bf16_norm": (torch.bfloat16, "CHW", True, True)}


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
    if not CASES[case][3]:
        return [(0, 0, W, H)] * count, [False] * count, [False] * count
    wins = [(int(rng.integers(0, W - 223)), int(rng.integers(0, H - 223)), 224, 224) for _ in range(count)]
    return wins, [bool(v) for v in rng.integers(0, 2, count)], [bool(v) for v in rng.integers(0, 2, count)]


def request(b, slots, case, out, wins, fx, fy):
    dtype, layout, norm, _ = CASES[case]
    t = None if dtype == torch.uint8 else tm.tables(3, dtype, MEAN if norm else None, STD if norm else None)
    tb = None if t is None else t.view(tm.BITS[dtype]).numpy()
    st, es = out.stride(), out.element_size()
    for i, s in enumerate(slots):
        x0, y0, w, h = wins[i]
        b.set_out_tensor(s, out.data_ptr() + i * st[0] * es, tm.CODE[dtype], layout, x0, y0, w, h, st[2] if layout == "CHW" else st[1],
                         st[1] if layout == "CHW" else 0, fx[i], fy[i], tb)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel", choices=sorted(CASES))
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--e2e-images", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_out.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ica.build_library()
    ctx = ica.Context(0)
    oracle = __import__("helpers").Oracle()
    datas = [ica.synth_jpeg(W, H, s, 90) for s in range(args.distinct)]
    wants = [oracle.load(d, 3)[1] for d in datas]
    rng = np.random.default_rng(3)
    plain, pslots = resident(ctx, datas, args.count)
    plain.submit()
    plain.wait()
    result = {"count": args.count, "distinct": args.distinct, "steps": args.steps, "cases": {}}
    for case in ([args.kernel] if args.kernel else sorted(CASES)):
        dtype, layout, norm, crop = CASES[case]
        wins, fx, fy = windows(case, args.count, rng)
        w, h = wins[0][2], wins[0][3]
        out = torch.empty((args.count, 3, h, w) if layout == "CHW" else (args.count, h, w, 3), dtype=dtype, device="cuda:0")
        b, slots = resident(ctx, datas, args.count)
        t = request(b, slots, case, out, wins, fx, fy)
        torch.cuda.synchronize()
        b.submit()
        b.wait()
        for i in (0, 1, args.count - 1):  # slot i is a clone of distinct picture i % distinct
            want = tm.window(wants[i % args.distinct], wins[i], fx[i], fy[i], layout, t, dtype)
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
        nbytes = args.count * w * h * 3 * (1 + out.element_size())
        k = mw - mo
        result["cases"][case] = {"launch_ms_with": mw, "launch_ms_without": mo, "tensor_pass_ms": k, "algorithmic_bytes": nbytes,
                                 "tb_per_s": nbytes / (k * 1e-3) / 1e12 if k > 0 else None,
                                 "frac_of_8tbs": nbytes / (k * 1e-3) / 8e12 if k > 0 else None}
        print(json.dumps({case: result["cases"][case]}), flush=True)
        b.close()
        del out
        torch.cuda.empty_cache()
    plain.close()
    # 4: end to end, 1080p CHW f16 normalised into a device tensor against decode + fetch to host
    n = args.e2e_images
    jl = [datas[i % args.distinct] for i in range(n)]
    dec = ica.TensorDecoder("cuda:0")
    threads = min(16, os.cpu_count() or 1)
    got, _ = dec.decode(jl[:8], dtype=torch.float16, mean=MEAN, std=STD, threads=threads)
    tdec = []
    for _ in range(3):
        t0 = time.perf_counter()
        got, reasons = dec.decode(jl, dtype=torch.float16, mean=MEAN, std=STD, threads=threads)
        tdec.append(time.perf_counter() - t0)
        assert reasons == [None] * n
    assert tm.same_bits(got[n - 1], tm.window(wants[(n - 1) % args.distinct], (0, 0, W, H), layout="CHW",
                                             table=tm.tables(3, torch.float16, MEAN, STD), dtype=torch.float16))
    del got
    dec.close()
    torch.cuda.empty_cache()
    d0 = ica.HostDecoder.probe(datas[0], 3)
    cb, ob = ica.Batch.coef_bytes(d0), ica.Batch.out_bytes(d0)
    bh = ica.Batch(ctx, n, cb * n, cb * n, ob * n)
    thost = []
    for _ in range(3):
        bh.reset()
        t0 = time.perf_counter()
        ok, slots, _ = bh.decode_jpegs(jl, 3, threads=threads)
        bh.submit()
        bh.wait()
        px = [bh.fetch(s) for s in slots]
        thost.append(time.perf_counter() - t0)
    assert np.array_equal(px[0], wants[0])
    bh.close()
    tt, th = float(np.median(tdec)), float(np.median(thost))
    result["e2e"] = {"images": n, "threads": threads, "tensor_decode_s": tt, "tensor_gpix_s": n * W * H / tt / 1e9,
                     "decode_fetch_host_s": th, "decode_fetch_host_gpix_s": n * W * H / th / 1e9}
    print(json.dumps({"e2e": result["e2e"]}), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
