"""TensorEncoder.encode_normalized measurements.  Writes one JSON line to profiles/tensor_encode_float.json.

  COUNT x 1080p CHW pictures (16 distinct synth_rgb seeds, repeated), q = 90, the emission arena large enough that nothing falls back.
  E2E     wall clock of TensorEncoder.encode of the uint8 batch and of encode_normalized of the same pictures as float16 and as
          float32 (ImageNet mean / std; the float tensors are what TensorDecoder's tables make of the bytes, so all three calls must
          return the same streams, and that is checked).  Median of RUNS after WARMUP warm-ups, each run ending in the call's own wait.
  GATHER  the upload alone between the encoder's device events (mij_enc_timer_*): the gather launch and the copies of its lists, for
          uint8, float16, bfloat16 and float32 slots; bytes read + written over that time.
  TORCH   what a caller writes today in front of encode(): (x.float() * std + mean) * 255, round, clamp, cast to uint8, on the same
          float batches, wall clock with a device synchronise; and in how many bytes its result differs from the pictures.
  --u8-only          the uint8 legs alone (E2E and GATHER), one JSON line on stdout, no file: runs on a library without
                     mij_enc_add_device_float
  --ab PARENT_LIB    --u8-only in fresh child processes, alternating PARENT_LIB (the parent commit's library, through MIJ_LIB) and this
                     tree's library AB_ROUNDS times, then the full measurement in one more child; writes the file."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import image_codecs_amd as ica  # noqa: E402  (after torch: one HIP runtime)

W, H, Q = 1920, 1080, 90
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def med(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def gather_ms(ctx, batch, dt, runs, warmup):
    """device-event time of mij_enc_upload for the batch's pictures as device-pixel slots of element type dt (None: uint8)"""
    n = batch.shape[0]
    pix = (W * H * 3 + 255) // 256 * 256
    du = ((W + 15) // 16) * ((H + 15) // 16) * 6 * 128
    enc = ica.Encoder(ctx, n, pix * n, du * n, stage_bytes=0)
    scale, bias = [255.0 * s for s in STD], [255.0 * m for m in MEAN]
    t = []
    for r in range(warmup + runs):
        enc.reset()
        for i in range(n):
            it = ica.InTensor(batch[i].data_ptr(), ica.MIJ_LAYOUT_CHW, W, H, 3, batch.stride(2), batch.stride(1))
            if dt is None:
                enc.add_device(it, Q)
            else:
                enc.add_device_float(it, ica.InConvert(dt, scale, bias), Q)
        enc.timer_begin()
        enc.upload()
        enc.timer_end()
        enc.wait()
        if r >= warmup:
            t.append(enc.timer_ms())
    enc.close()
    es = batch.element_size()
    moved = n * W * H * 3 * (es + 1)  # read as elements, written as packed RGB bytes (1920 is whole MCU columns: no padding)
    m = med(t)
    m["bytes_moved"] = moved
    m["gb_per_s"] = round(moved / (m["median"] * 1e-3) / 1e9, 1)
    return m


def measure(a):
    if not torch.cuda.is_available() or not ica.gpu_available():
        raise SystemExit("bench_tensor_encode_float: no GPU")
    imgs = [ica.synth_rgb(W, H, s) for s in range(16)]
    u8 = torch.from_numpy(np.stack(imgs)).cuda().permute(0, 3, 1, 2).contiguous().repeat((a.count + 15) // 16, 1, 1, 1)[:a.count].contiguous()
    te = ica.TensorEncoder()
    want = te.encode(u8, quality=Q)
    te.reserve_arena(int(sum(len(s) for s in want) * 1.1))
    ctx = ica.Context()
    arch, cus, _ = ctx.info()
    res = {"tool": "bench_tensor_encode_float", "device": arch, "cus": cus, "pictures": a.count, "quality": Q, "runs": a.runs, "warmup": a.warmup,
           "library": os.environ.get("MIJ_LIB") or "tree", "stream_bytes": sum(len(s) for s in want)}

    def enc_u8():
        got = te.encode(u8, quality=Q)
        assert te.last_host_emitted == 0 and got[-1] == want[-1]

    res["encode_u8_ms"] = med(timed(enc_u8, a.runs, a.warmup))
    res["gather_u8_ms"] = gather_ms(ctx, u8, None, a.runs, a.warmup)
    if a.u8_only:
        te.close()
        ctx.close()
        return res
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    for name, dtype, dt in (("f16", torch.float16, ica.MIJ_DT_F16), ("bf16", torch.bfloat16, ica.MIJ_DT_BF16), ("f32", torch.float32, ica.MIJ_DT_F32)):
        tab = ica.tensor_tables(3, dtype, MEAN, STD).cuda()
        x = torch.stack([tab[c][u8[:16, c].long()] for c in range(3)], 1)  # what TensorDecoder writes for these bytes
        x = x.repeat((a.count + 15) // 16, 1, 1, 1)[:a.count].contiguous()
        res["gather_%s_ms" % name] = gather_ms(ctx, x, dt, a.runs, a.warmup)
        if name == "bf16":
            del x
            continue
        assert te.encode_normalized(x, mean=MEAN, std=STD, quality=Q) == want, name

        def enc_f():
            got = te.encode_normalized(x, mean=MEAN, std=STD, quality=Q)
            assert te.last_host_emitted == 0 and got[-1] == want[-1]

        def denorm():
            return ((x.float() * std + mean) * 255).round_().clamp_(0, 255).to(torch.uint8)

        res["torch_denorm_%s_mismatches" % name] = int((denorm() != u8).sum())
        res["encode_normalized_%s_ms" % name] = med(timed(enc_f, a.runs, a.warmup))
        res["torch_denorm_%s_ms" % name] = med(timed(denorm, a.runs, a.warmup))
        del x
        torch.cuda.empty_cache()
    te.close()
    ctx.close()
    return res


def ab(a):
    """the uint8 legs under the parent's library and this tree's in turn, then the full measurement"""
    me = [sys.executable, os.path.abspath(__file__), "--count", str(a.count), "--runs", str(a.runs), "--warmup", str(a.warmup)]
    runs = {"parent": [], "change": []}
    for r in range(a.ab_rounds):
        for name in ("parent", "change"):
            env = dict(os.environ)
            env.pop("MIJ_LIB", None)
            if name == "parent":
                env["MIJ_LIB"] = os.path.abspath(a.ab)
            p = subprocess.run(me + ["--u8-only"], env=env, stdout=subprocess.PIPE, check=True, timeout=600)
            runs[name].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
            print(name, r, json.dumps(runs[name][-1]), flush=True)
    env = dict(os.environ)
    env.pop("MIJ_LIB", None)
    p = subprocess.run(me + ["--child"], env=env, stdout=subprocess.PIPE, check=True, timeout=900)
    res = json.loads(p.stdout.decode().strip().splitlines()[-1])
    res["u8_against_parent"] = {k: {"encode_u8_ms": [x["encode_u8_ms"]["median"] for x in v], "gather_u8_ms": [x["gather_u8_ms"]["median"] for x in v]}
                                for k, v in runs.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--u8-only", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--ab", metavar="PARENT_LIB")
    ap.add_argument("--ab-rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_encode_float.json"))
    a = ap.parse_args()
    res = ab(a) if a.ab else measure(a)  # --ab: before any GPU use in this process, the children own the device
    line = json.dumps(res)
    print(line)
    if not a.u8_only and not a.child:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
