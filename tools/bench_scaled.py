"""Reduced-size decode measurements.  Writes profiles/scaled.json.

  A    decode launch time of a resident batch of COUNT x 1080p 4:2:0 q=90 pictures (the distinct ones host-walked once, the rest
       clones with the same scale) at s = 1, 2, 4, 8: four batches alternated in one process, device events, median of STEPS after a
       warm-up of 25 ms or more.  Reported with the bytes each needs (2 B x NV x NH per block and component read, n_out x OW x OH
       written) and their share of 8 TB/s.
  B    section 4e's case A: whole 1080p -> 224 x 224 bilinear CHW f16 normalised, with reduce=None (the unchanged full-size path) and
       with reduce="auto" (s = 4: 480 x 270): launch time of decode plus output passes, alternated the same way, and
       TensorDecoder.decode end to end (wall clock).
  --kernel S  only launch the s = S batch LAUNCHES times (run it under `rocprofv3 --kernel-trace --stats`, a run of its own).
Pixels are checked against tests/scaled_model.py (and the oracle at s = 1) before anything is timed."""
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
from image_codecs_amd.tensor_out import auto_reduce  # noqa: E402
import idct_model as M  # noqa: E402
import resize_model as rm  # noqa: E402
import scaled_model as SM  # noqa: E402
import tensor_model as tm  # noqa: E402

W, H, S = 1920, 1080, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HV = [(2, 2), (1, 1), (1, 1)]


def planes_of(data):
    desc, arena = ica.HostDecoder.decode(data, 3)
    nat = ica.detile_coefficients(desc, arena)
    return desc, [M.dequant(nat[c].astype(np.int64), np.array(desc.dequant[desc.comp[c].tq], np.int64).reshape(8, 8)) for c in range(desc.ncomp)]


def resident(ctx, datas, count, scale):
    """slot i holds distinct picture i % len(datas): every slot host-walked from the same few streams (clones start at scale 1)"""
    d0 = ica.HostDecoder.probe(datas[0], 3)
    cb, ob = ica.Batch.coef_bytes(d0), ica.Batch.out_bytes(d0)
    b = ica.Batch(ctx, count, cb * len(datas), cb * count, ob * count)
    src = [b.add_jpeg(d, 3) for d in datas]
    slots = list(src)
    while len(slots) < count:
        slots.append(b.add_clone(src[len(slots) % len(src)]))
    if scale > 1:
        for s in slots:
            b.set_scale(s, scale)
    return b, slots


def decode_bytes(desc, s):
    n = 8 // s
    rd = sum(desc.comp[c].bw * desc.comp[c].bh * 2 * (n * desc.h_max // desc.comp[c].h) * (n * desc.v_max // desc.comp[c].v) for c in range(desc.ncomp))
    return rd, 3 * -(-W // s) * -(-H // s)


def timed(batches, steps):
    """alternate the batches; -> median launch ms per name"""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.05:  # warm-up: well over 25 ms of launches
        for b in batches.values():
            b.launch()
        for b in batches.values():
            b.wait()
    ms = {k: [] for k in batches}
    for _ in range(steps):
        for k, b in batches.items():
            b.launch()
            b.timer_begin()
            b.launch()
            b.timer_end()
            b.wait()
            ms[k].append(b.timer_ms())
    return {k: float(np.median(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel", type=int, choices=(1, 2, 4, 8))
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--e2e-images", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaled.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ica.build_library()
    ctx = ica.Context(0)
    oracle = __import__("helpers").Oracle()
    datas = [ica.synth_jpeg(W, H, s, 90) for s in range(args.distinct)]
    planes = [planes_of(d) for d in datas[:2]]
    desc = planes[0][0]
    want = {s: [SM.scaled_picture(p, HV, (W, H), s, 3) for _, p in planes] for s in (2, 4, 8)}
    want[1] = [oracle.load(d, 3)[1] for d in datas[:2]]
    result = {"count": args.count, "distinct": args.distinct, "steps": args.steps, "picture": [W, H], "decode": {}, "to_224": {}}

    # A: decode launches
    batches = {}
    for s in ([args.kernel] if args.kernel else [1, 2, 4, 8]):
        b, slots = resident(ctx, datas, args.count, s)
        b.submit()
        b.wait()
        for i in (0, 1, args.distinct, args.distinct + 1):
            if i < args.count:
                assert np.array_equal(b.fetch(slots[i]), want[s][i % args.distinct]), (s, i)
        batches[s] = b
    if args.kernel:
        b = batches[args.kernel]
        for _ in range(args.launches):
            b.launch()
        b.wait()
        print(json.dumps({"scale": args.kernel, "launches": args.launches}))
        return
    ms = timed(batches, args.steps)
    for s, b in batches.items():
        rd, wr = decode_bytes(desc, s)
        total = (rd + wr) * args.count
        result["decode"]["s%d" % s] = {"launch_ms": ms[s], "bytes_read": rd * args.count, "bytes_written": wr * args.count,
                                       "tb_per_s": total / (ms[s] * 1e-3) / 1e12, "frac_of_8tbs": total / (ms[s] * 1e-3) / 8e12}
        print(json.dumps({"decode s=%d" % s: result["decode"]["s%d" % s]}), flush=True)
        b.close()

    # B: whole 1080p -> 224 x 224 bilinear CHW f16, from the full-size and from the 1/4 picture
    t = tm.tables(3, torch.float16, MEAN, STD)
    tb = t.view(tm.BITS[torch.float16]).numpy()
    batches, outs = {}, {}
    for name, s in (("reduce_none", 1), ("reduce_auto", auto_reduce(W, H, S, S))):
        out = torch.empty((args.count, 3, S, S), dtype=torch.float16, device="cuda:0")
        b, slots = resident(ctx, datas, args.count, s)
        st, es = out.stride(), out.element_size()
        ow, oh = -(-W // s), -(-H // s)
        for i, sl in enumerate(slots):
            b.set_out_tensor_resized(sl, out.data_ptr() + i * st[0] * es, tm.CODE[torch.float16], "CHW", 0, 0, ow, oh, S, S, st[2], st[1], False, False, tb,
                                     "bilinear")
        torch.cuda.synchronize()
        b.submit()
        b.wait()
        for i in (0, 1, args.count - 1):
            if i % args.distinct < 2:
                w = rm.window(want[s][i % args.distinct], (0, 0, ow, oh), (S, S), "bilinear", False, False, "CHW", t, torch.float16)
                assert tm.same_bits(out[i], w), (name, i)
        batches[name], outs[name] = b, out
        result["to_224"][name] = {"scale": s}
    ms = timed(batches, args.steps)
    for name, b in batches.items():
        result["to_224"][name]["launch_ms"] = ms[name]
        b.close()
    del outs
    torch.cuda.empty_cache()
    n = args.e2e_images
    jl = [datas[i % args.distinct] for i in range(n)]
    dec = ica.TensorDecoder("cuda:0")
    threads = min(16, os.cpu_count() or 1)
    for name, red in (("reduce_none", None), ("reduce_auto", "auto")):
        dec.decode(jl[:8], dtype=torch.float16, mean=MEAN, std=STD, threads=threads, size=(S, S), reduce=red)
        tdec = []
        for _ in range(3):
            t0 = time.perf_counter()
            got, reasons = dec.decode(jl, dtype=torch.float16, mean=MEAN, std=STD, threads=threads, size=(S, S), reduce=red)
            tdec.append(time.perf_counter() - t0)
            assert reasons == [None] * n
        tt = float(np.median(tdec))
        result["to_224"][name].update({"e2e_images": n, "e2e_threads": threads, "e2e_s": tt, "e2e_source_gpix_s": n * W * H / tt / 1e9})
        print(json.dumps({name: result["to_224"][name]}), flush=True)
    dec.close()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
