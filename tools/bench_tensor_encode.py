"""GPU Huffman emission and TensorEncoder measurements.  Writes one JSON line to profiles/tensor_encode.json.

  T/E  BASELINE config 5's shape: COUNT x 1080p (16 distinct synth_rgb seeds, the rest clones), at q=90 (4:2:0) and q=95 (4:4:4).
       Two encoders over the same slots, launched alternately STEPS times: one without an emission arena (the transform alone) and
       one with (transform + emission).  Device-event times of each launch; emission ms = median(with) - median(without).
  D2H  after a wait: the streams' fetch (mij_enc_fetch_streams: lengths + used arena) against the data units' fetch
       (mij_enc_fetch_all), bytes and wall ms.
  E2E  TensorEncoder.encode of a [N2, 3, 1080, 1920] uint8 CUDA tensor against mij_write_jpg_batch of the same pictures from host
       memory (16 host threads), alternated ROUNDS times; Gpix/s of wall clock.
  --kernel  only the q=90 encoder with emission, LAUNCHES launches (run it under `rocprofv3 --kernel-trace --stats`, a run of its own);
            with --optimize every slot asks for optimised Huffman tables.
  --opt     optimised Huffman tables: T/E's slots in three encoders -- no arena, arena with plain slots, arena
            with every slot optimised -- launched alternately STEPS times; emission ms of plain and of optimised slots, stream bytes
            of both.  One JSON line on stdout, no file.  A library without mij_enc_set_optimize gives the plain figures alone.
  --opt-ab PARENT_LIB  --opt in fresh child processes, alternating PARENT_LIB (the parent commit's library, through MIJ_LIB) and
            this tree's library AB_ROUNDS times; writes profiles/tensor_encode_opt.json.
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


def encoder(ctx, imgs, count, q, arena, optimize=False):
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
    if optimize:
        for s in src:
            enc.set_optimize(s)
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


def opt_leg(ctx, imgs, count, q, steps, wg):
    """emission ms of plain slots and of optimised slots over the same pictures; their stream bytes"""
    lens = wg["bench/q%d/len" % q]
    arena = int(max(int(v) for v in lens) * 1.1) * count
    has_opt = hasattr(ica.lib(), "mij_enc_set_optimize")
    encs = [encoder(ctx, imgs, count, q, 0)[0], encoder(ctx, imgs, count, q, arena)[0]]
    if has_opt:
        encs.append(encoder(ctx, imgs, count, q, arena, optimize=True)[0])
    for e in encs:
        launch_ms(e)  # warm
    t = [[] for _ in encs]
    for _ in range(steps):
        for k, e in enumerate(encs):
            t[k].append(launch_ms(e))
    out = {"quality": q, "pictures": count, "steps": steps}
    med = [float(np.median(x)) for x in t]
    out["transform_ms"] = round(med[0], 3)
    out["plain_emission_ms"] = {"median": round(med[1] - med[0], 3), "per_step": [round(b - a, 3) for a, b in zip(t[0], t[1])]}
    assert encs[1].fetch_streams() == count
    out["plain_bytes"] = sum(encs[1].stream(s)[1] for s in range(count))
    if has_opt:
        out["optimised_emission_ms"] = {"median": round(med[2] - med[0], 3), "per_step": [round(b - a, 3) for a, b in zip(t[0], t[2])]}
        assert encs[2].fetch_streams() == count
        out["optimised_bytes"] = sum(encs[2].stream(s)[1] for s in range(count))
        out["optimised_slots"] = sum(encs[2].slot_optimized(s) for s in range(count))
        out["bytes_ratio"] = round(out["optimised_bytes"] / out["plain_bytes"], 4)
        for s in range(min(4, len(imgs))):  # the streams themselves: the host's optimised emission of the same units
            assert encs[2].stream(s)[0] == ica.emit_jpeg(encs[2].plan(s), encs[2].fetch(s), True), (q, s)
    for e in encs:
        e.close()
    return out


def opt_ab(parent_lib, a):
    """--opt in child processes, parent library and this one in turn"""
    import subprocess
    runs = {"parent": [], "change": []}
    for r in range(a.ab_rounds):
        for name in ("parent", "change"):
            env = dict(os.environ)
            env.pop("MIJ_LIB", None)
            if name == "parent":
                env["MIJ_LIB"] = os.path.abspath(parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--opt", "--count", str(a.count), "--steps", str(a.steps)], env=env,
                               stdout=subprocess.PIPE, check=True, timeout=900)
            runs[name].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
            print(name, r, json.dumps(runs[name][-1]["legs"]), flush=True)
    res = {"tool": "bench_tensor_encode --opt-ab", "device": runs["change"][0]["device"], "pictures": a.count, "steps": a.steps, "rounds": a.ab_rounds,
           "legs": []}
    for k, q in enumerate((90, 95)):
        par = [x["legs"][k]["plain_emission_ms"]["median"] for x in runs["parent"]]
        chg = [x["legs"][k]["plain_emission_ms"]["median"] for x in runs["change"]]
        opt = [x["legs"][k]["optimised_emission_ms"]["median"] for x in runs["change"]]
        last = runs["change"][-1]["legs"][k]
        res["legs"].append({"quality": q, "plain_emission_ms_parent": par, "plain_emission_ms_change": chg, "optimised_emission_ms": opt,
                            "plain_bytes": last["plain_bytes"], "optimised_bytes": last["optimised_bytes"], "bytes_ratio": last["bytes_ratio"],
                            "optimised_slots": last["optimised_slots"]})
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, "profiles", "tensor_encode_opt.json"), "w") as f:
        f.write(line + "\n")


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
    ap.add_argument("--optimize", action="store_true")
    ap.add_argument("--opt", action="store_true")
    ap.add_argument("--opt-ab", metavar="PARENT_LIB")
    ap.add_argument("--ab-rounds", type=int, default=2)
    a = ap.parse_args()
    if a.opt_ab:  # before any GPU use in this process: the children own the device
        return opt_ab(a.opt_ab, a)
    if not torch.cuda.is_available() or not ica.gpu_available():
        raise SystemExit("bench_tensor_encode: no GPU")
    wg = np.load(WG, allow_pickle=False)
    imgs = [ica.synth_rgb(W, H, s) for s in range(16)]
    ctx = ica.Context()
    if a.kernel:
        lens = wg["bench/q90/len"]
        enc, _ = encoder(ctx, imgs, a.count, 90, int(max(int(v) for v in lens) * 1.1) * a.count, a.optimize)
        for _ in range(a.launches):
            enc.launch()
            enc.wait()
        assert enc.fetch_streams() == a.count
        enc.close()
        ctx.close()
        return
    arch, cus, mem = ctx.info()
    if a.opt:
        print(json.dumps({"tool": "bench_tensor_encode --opt", "device": arch, "legs": [opt_leg(ctx, imgs, a.count, q, a.steps, wg) for q in (90, 95)]}))
        ctx.close()
        return
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
