"""Oriented tensor output measurements.  Writes profiles/tensor_orient.json.

  A  a resident batch of COUNT x 1080p 4:2:0 q=90 pictures (the distinct ones host-walked once, the rest clones), whole picture to CHW
     f16 normalised, at orientations 1, 3 and 6; B  the same to 224 x 224 bilinear, at orientations 1, 2 and 6.  Each batch is launched
     with and without its requests, the two alternated in one process; the difference of the device-event times of the launches
     (median of STEPS) is the output pass's time.  Reported with algorithmic bytes (3 bytes read per source pixel + 3 * 2 written per
     output pixel) as a fraction of 8 TB/s, and as a ratio to orientation 1.
  E2E  TensorDecoder.decode(orientation="exif", size=(224, 224)) end to end on COUNT x 1080p files tagged 6 against the same files
       untagged (wall clock, median of 3), in Gpix/s of source pixels.  The tagged files are synth_jpeg output with an Exif APP1
       inserted after SOI, made here.
  --kernel CASE  only launch case CASE's batch LAUNCHES times (run it under `rocprofv3 --kernel-trace --stats`, a run of its own).
Every case checks a few of its outputs against tests/orient_model.py with tensor_model / resize_model on the oracle's pixels first."""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_codecs_amd as ica  # noqa: E402  (after torch: one HIP runtime)
import orient_model as om  # noqa: E402
import resize_model as rm  # noqa: E402
import tensor_model as tm  # noqa: E402

W, H, S = 1920, 1080, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CASES = {"A_whole_o1": (1, False), "A_whole_o3": (3, False), "A_whole_o6": (6, False),
         "B_224_o1": (1, True), "B_224_o2": (2, True), "B_224_o6": (6, True)}


def tagged(jpeg, o):
    """jpeg with an Exif APP1 (big-endian TIFF, IFD0 holding Orientation = o) right after SOI"""
    tiff = b"MM\0*" + struct.pack(">IH", 8, 1) + struct.pack(">HHIH2x", 0x0112, 3, 1, o) + struct.pack(">I", 0)
    p = b"Exif\0\0" + tiff
    return jpeg[:2] + b"\xff\xe1" + struct.pack(">H", len(p) + 2) + p + jpeg[2:]


def resident(ctx, datas, count):
    d0 = ica.HostDecoder.probe(datas[0], 3)
    cb, ob = ica.Batch.coef_bytes(d0), ica.Batch.out_bytes(d0)
    b = ica.Batch(ctx, count, cb * len(datas), cb * count, ob * count)
    src = [b.add_jpeg(d, 3) for d in datas]
    slots = list(src)
    while len(slots) < count:
        slots.append(b.add_clone(src[len(slots) % len(src)]))
    return b, slots


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel", choices=sorted(CASES))
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--e2e-images", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_orient.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ica.build_library()
    ctx = ica.Context(0)
    oracle = __import__("helpers").Oracle()
    datas = [ica.synth_jpeg(W, H, s, 90) for s in range(args.distinct)]
    wants = [oracle.load(d, 3)[1] for d in datas]
    plain, _ = resident(ctx, datas, args.count)
    plain.submit()
    plain.wait()
    dtype = torch.float16
    t = tm.tables(3, dtype, MEAN, STD)
    tb = t.view(tm.BITS[dtype]).numpy()
    result = {"count": args.count, "distinct": args.distinct, "steps": args.steps, "cases": {}}
    for case in ([args.kernel] if args.kernel else list(CASES)):
        o, rsz = CASES[case]
        dw, dh = om.displayed_size(W, H, o)
        oh, ow = (S, S) if rsz else (dh, dw)
        out = torch.empty((args.count, 3, oh, ow), dtype=dtype, device="cuda:0")
        b, slots = resident(ctx, datas, args.count)
        st, es = out.stride(), out.element_size()
        for i, s in enumerate(slots):
            if rsz:
                b.set_out_tensor_resized(s, out.data_ptr() + i * st[0] * es, tm.CODE[dtype], "CHW", 0, 0, dw, dh, S, S, st[2], st[1], False, False, tb,
                                         "bilinear", orientation=o)
            else:
                b.set_out_tensor(s, out.data_ptr() + i * st[0] * es, tm.CODE[dtype], "CHW", 0, 0, dw, dh, st[2], st[1], False, False, tb, orientation=o)
        torch.cuda.synchronize()
        b.submit()
        b.wait()
        for i in (0, 1, args.count - 1):  # slot i is a clone of distinct picture i % distinct
            d = om.orient(wants[i % args.distinct], o)
            want = rm.window(d, (0, 0, dw, dh), (S, S), "bilinear", layout="CHW", table=t, dtype=dtype) if rsz else \
                tm.window(d, (0, 0, dw, dh), layout="CHW", table=t, dtype=dtype)
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
        nread, nwrite = args.count * W * H * 3, args.count * oh * ow * 3 * es
        k = mw - mo
        result["cases"][case] = {"orientation": o, "size": [oh, ow], "launch_ms_with": mw, "launch_ms_without": mo, "pass_ms": k,
                                 "bytes_read": nread, "bytes_written": nwrite, "frac_of_8tbs": (nread + nwrite) / (k * 1e-3) / 8e12 if k > 0 else None}
        print(json.dumps({case: result["cases"][case]}), flush=True)
        b.close()
        del out
        torch.cuda.empty_cache()
    plain.close()
    for c in result["cases"].values():
        ref = result["cases"]["A_whole_o1" if c["size"] != [S, S] else "B_224_o1"]["pass_ms"]
        c["ratio_to_o1"] = c["pass_ms"] / ref if ref > 0 else None
    # E2E: the same files tagged 6 and untagged through TensorDecoder.decode(orientation="exif", size=(224, 224))
    n = args.e2e_images
    dec = ica.TensorDecoder("cuda:0")
    threads = min(16, os.cpu_count() or 1)
    e2e = {"images": n, "threads": threads, "size": [S, S]}
    for name, files in (("untagged", datas), ("tagged_6", [tagged(d, 6) for d in datas])):
        jl = [files[i % args.distinct] for i in range(n)]
        dec.decode(jl[:8], dtype=torch.float16, mean=MEAN, std=STD, threads=threads, size=(S, S), orientation="exif")
        tdec = []
        for _ in range(3):
            t0 = time.perf_counter()
            got, reasons = dec.decode(jl, dtype=torch.float16, mean=MEAN, std=STD, threads=threads, size=(S, S), orientation="exif")
            tdec.append(time.perf_counter() - t0)
            assert reasons == [None] * n
        o = ica.exif_orientation(jl[-1])
        dw, dh = om.displayed_size(W, H, o)
        assert tm.same_bits(got[n - 1], rm.window(om.orient(wants[(n - 1) % args.distinct], o), (0, 0, dw, dh), (S, S), "bilinear", layout="CHW",
                                                  table=t, dtype=torch.float16))
        tt = float(np.median(tdec))
        e2e[name] = {"orientation": o, "decode_s": tt, "source_gpix_s": n * W * H / tt / 1e9}
    e2e["tagged_over_untagged"] = e2e["tagged_6"]["decode_s"] / e2e["untagged"]["decode_s"]
    result["e2e"] = e2e
    print(json.dumps({"e2e": e2e}), flush=True)
    dec.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
