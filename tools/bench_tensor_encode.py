"""GPU Huffman emission and TensorEncoder measurements.  Writes one JSON line to profiles/tensor_encode.json.

  T/E  BASELINE config 5's shape: COUNT x 1080p (16 distinct synth_rgb seeds, the rest clones), at q=90 (4:2:0) and q=95 (4:4:4).
       Two encoders over the same slots, launched alternately STEPS times: one without an emission arena (the transform alone) and
       one with (transform + emission).  Device-event times of each launch; emission ms = median(with) - median(without).
  D2H  after a wait: the streams' fetch (mij_enc_fetch_streams: lengths + used arena) against the data units' fetch
       (mij_enc_fetch_all), bytes and wall ms.
  E2E  TensorEncoder.encode of a [N2, 3, 1080, 1920] uint8 CUDA tensor against mij_write_jpg_batch of the same pictures from host
       memory (16 host threads), alternated ROUNDS times; Gpix/s of wall clock.
  --kernel  only the q=90 encoder with emission, LAUNCHES launches (run it under `rocprofv3 --kernel-trace --stats`, a run of its own).
Streams are checked against the reference's stored lengths and SHA-256 (tests/golden/writer_golden_r3.npz) first."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import image_codecs_amd as ica  # noqa: E402  (after torch: one HIP runtime)

W, H = 1920, 1080
WG = os.path.join(ROOT, "tests", "golden", "writer_golden_r3.npz")


def encoder(ctx, imgs, count, q, arena):
    pix = ica.binding.lib().mij_enc_pixel_bytes
    pix.restype = C.c_size_t
    pix.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    pb = pix(W, H, 3, q)
    mcu = 16 if q <= 90 else 8
    dub = ((W + mcu - 1) // mcu) * ((H + mcu - 1) // mcu) * (6 if q <= 90 else 3) * 128
    enc = ica.Encoder(ctx, count, pb * count, dub * count, stage_bytes=pb * len(imgs))
    if arena:
        enc.stream_reserve(arena)
    src = [enc.add(a, q) for a in imgs]
    while len(src) < count:
        src.append(enc.add_clone(src[len(src) % len(imgs)]))
    enc.upload()
    return enc, dub * count


def launch_ms(enc):
    enc.timer_begin()
    enc.launch()
    enc.timer_end()
    return enc.timer_ms()


def leg(ctx, imgs, count, q, steps, wg):
    lens = wg["bench/q%d/len" % q]
    arena = int(max(int(v) for v in lens) * 1.1) * count
    a, du_bytes = encoder(ctx, imgs, count, q, 0)
    b, _ = encoder(ctx, imgs, count, q, arena)
    launch_ms(a), launch_ms(b)  # warm
    ta, tb = [], []
    for _ in range(steps):
        ta.append(launch_ms(a))
        tb.append(launch_ms(b))
    # correctness of the last launch: every distinct picture's stream has the reference's digest
    b.wait()
    t0 = time.perf_counter()
    nfit = b.fetch_streams()
    d2h_streams_ms = (time.perf_counter() - t0) * 1e3
    assert nfit == count, nfit
    shas = wg["bench/q%d/sha256" % q]
    used = 0
    for s in range(count):
        data, n = b.stream(s)
        used += n
        if s < len(lens):
            assert len(data) == int(lens[s]) and hashlib.sha256(data).digest() == bytes(shas[s]), (q, s)
    d2h_units_ms = None
    if q <= 90:  # the units' pinned mirror is as large as the unit arena (6.4 GB here; 12.7 GB at 4:4:4, not measured)
        L = ica.lib()
        L.mij_enc_fetch_all.argtypes = [C.c_void_p]
        a.wait()
        assert L.mij_enc_fetch_all(a._h) == 0  # allocates the mirror
        t0 = time.perf_counter()
        assert L.mij_enc_fetch_all(a._h) == 0
        d2h_units_ms = round((time.perf_counter() - t0) * 1e3, 3)
    a.close()
    b.close()
    mt, mb = float(np.median(ta)), float(np.median(tb))
    return {"quality": q, "pictures": count, "transform_ms": {"median": round(mt, 3), "min": round(min(ta), 3)},
            "transform_plus_emission_ms": {"median": round(mb, 3), "min": round(min(tb), 3)}, "emission_ms": round(mb - mt, 3),
            "emission_over_transform": round((mb - mt) / mt, 3),
            "d2h": {"stream_bytes": used, "unit_bytes": du_bytes, "ratio": round(du_bytes / used, 2), "streams_ms": round(d2h_streams_ms, 3),
                    "units_ms": d2h_units_ms}}


def e2e(imgs, n, rounds, q):
    batch = torch.from_numpy(np.stack([imgs[i % len(imgs)] for i in range(n)])).cuda().permute(0, 3, 1, 2).contiguous()
    host = [imgs[i % len(imgs)] for i in range(n)]
    te = ica.TensorEncoder()
    want = te.encode(batch, quality=q)  # warm: arena sized, encoder built
    assert want == ica.mij_write_jpg_batch(host, q, 16)
    tt, th = [], []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = te.encode(batch, quality=q)
        tt.append(time.perf_counter() - t0)
        assert te.last_host_emitted == 0 and got[0] == want[0] and got[-1] == want[-1]
        t0 = time.perf_counter()
        ica.mij_write_jpg_batch(host, q, 16)
        th.append(time.perf_counter() - t0)
    te.close()
    gpx = n * W * H / 1e9
    return {"pictures": n, "quality": q, "tensor_encode_s": {"median": round(float(np.median(tt)), 4), "min": round(min(tt), 4)},
            "tensor_encode_gpix_s": round(gpx / float(np.median(tt)), 3),
            "write_jpg_batch_s": {"median": round(float(np.median(th)), 4), "min": round(min(th), 4)},
            "write_jpg_batch_gpix_s": round(gpx / float(np.median(th)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--e2e", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_encode.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available() or not ica.gpu_available():
        raise SystemExit("bench_tensor_encode: no GPU")
    wg = np.load(WG, allow_pickle=False)
    imgs = [ica.synth_rgb(W, H, s) for s in range(16)]
    ctx = ica.Context()
    if a.kernel:
        lens = wg["bench/q90/len"]
        enc, _ = encoder(ctx, imgs, a.count, 90, int(max(int(v) for v in lens) * 1.1) * a.count)
        for _ in range(a.launches):
            enc.launch()
            enc.wait()
        assert enc.fetch_streams() == a.count
        enc.close()
        ctx.close()
        return
    arch, cus, mem = ctx.info()
    res = {"tool": "bench_tensor_encode", "device": arch, "cus": cus, "legs": [leg(ctx, imgs, a.count, 90, a.steps, wg),
                                                                               leg(ctx, imgs, a.count, 95, a.steps, wg)]}
    ctx.close()
    res["e2e"] = e2e(imgs, a.e2e, a.rounds, 90)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
