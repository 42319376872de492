#!/usr/bin/env python3
"""Measures plane encoding ("420", "444", "grey"; include/mij_host.h, PLANE ENCODING) on 256 1080p pictures at quality 90 -- 16 distinct
synth_rgb pictures, the rest repeated; their Y, Cb and Cr planes are made once on the GPU (the writer's colour expressions, rounded;
chroma the mean of its lh x lv pixels), all in one run:

  gather      k_enc_gather_planes alone: the caller's planes in HBM -> the staged planar rows in HBM (event time around an upload of
              device plane slots, which also carries the two small list copies), and the bytes it reads and writes.
  transform   k_encode_planes<LH, LV> alone: staged rows -> data units (event time of a launch without an emission arena).
  ycbcr       the whole TensorEncoder.encode_ycbcr(subsampling=...) call, wall time, and the bytes of its streams.
  rgb         beside it, TensorEncoder.encode(subsampling=...) of the RGB pictures those planes came from.
  via_torch   what a caller who holds planes pays without this: chroma repeated to full size and converted to RGB with torch, then
              encode(subsampling=...) -- the conversion alone (torch_ms) and the sum.

Best of --steps after --warmup in each of --rounds rounds, the variants taken in turns inside every step, and the spread of the rounds'
bests.  With --parent DIR (a built checkout of the parent commit) the default encode() call is measured at quality 90 and 95 against it
in child processes, one per round and tree, the two trees in turns; the difference of the bests is reported next to the spread between
the parent's own rounds.  No threshold is fixed here: none of these numbers existed before.  Not bench.py: nothing here is a yardstick.

    python tools/bench_encode_planes.py [--n 256] [--steps 5] [--warmup 2] [--rounds 3] [--parent DIR] [--out profiles/encode_planes.json]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
import bench_encode_sampling as bes  # noqa: E402  the parent comparison and the pictures are that tool's

NAMES = ("420", "444", "grey")
FACTORS = bes.FACTORS


def geometry(name, w, h):
    """-> (bytes of the caller's planes, bytes of the staged rows, bytes of the data units) of one picture"""
    ncomp, lh, lv = FACTORS[name]
    mx, my = -(-w // (8 * lh)), -(-h // (8 * lv))
    units = mx * my * (1 if ncomp == 1 else lh * lv + 2)
    src = w * h + (ncomp - 1) * (-(-w // lh)) * (-(-h // lv))
    return src, units * 64, units * 128


def planes_of(torch, batch, name):
    """[N, 3, H, W] uint8 RGB -> the planes a producer would hold: the writer's colour expressions rounded to uint8, chroma the mean of
    its lh x lv pixels (edge pixels repeated)"""
    ncomp, lh, lv = FACTORS[name]
    out = []
    for i in range(0, batch.shape[0], 16):  # in slices: the floats of 256 1080p pictures need not all live at once
        f = batch[i:i + 16].float()
        r, g, b = f[:, 0], f[:, 1], f[:, 2]
        comps = [0.299 * r + 0.587 * g + 0.114 * b]
        if ncomp == 3:
            comps += [-0.16874 * r - 0.33126 * g + 0.5 * b + 128.0, 0.5 * r - 0.41869 * g - 0.08131 * b + 128.0]
            if (lh, lv) != (1, 1):
                H, W = r.shape[-2:]
                pad = torch.nn.functional.pad
                comps[1:] = [torch.nn.functional.avg_pool2d(pad(c[:, None], (0, -W % lh, 0, -H % lv), mode="replicate"), (lv, lh))[:, 0] for c in comps[1:]]
        out.append([c.round().clamp(0, 255).to(torch.uint8) for c in comps])
    return [torch.cat([o[k] for o in out]).contiguous() for k in range(ncomp)]


def torch_rgb(torch, planes, name):
    """what a caller does today: chroma repeated to the picture's size, JFIF's YCbCr -> RGB in float, rounded -> [N, 3, H, W] uint8"""
    ncomp, lh, lv = FACTORS[name]
    y = planes[0]
    if ncomp == 1:
        return y[:, None].expand(-1, 3, -1, -1).contiguous()
    H, W = y.shape[-2:]
    yf = y.float()
    cb, cr = [(p.repeat_interleave(lv, -2).repeat_interleave(lh, -1)[:, :H, :W].float() - 128.0) for p in planes[1:]]
    rgb = torch.stack([yf + 1.402 * cr, yf - 0.344136 * cb - 0.714136 * cr, yf + 1.772 * cb], dim=1)
    return rgb.round().clamp(0, 255).to(torch.uint8)


def kernel_ms(ica, torch, ctx, a, planes, name, launches=5):
    """-> (gather ms, transform ms) per launch over a.n pictures, one round"""
    import numpy as np
    src, staged, du = geometry(name, a.width, a.height)
    enc = ica.Encoder(ctx, a.n, (staged + 256) * a.n, (du + 256) * a.n, stage_bytes=0)
    try:
        for i in range(a.n):
            enc.add_device_planes([(p[i].data_ptr(), p[i].stride(0), 1) for p in planes], a.width, a.height, name, 90)
        torch.cuda.synchronize()
        enc.upload()
        enc.launch()
        enc.wait()
        pic = [p[a.n - 1].cpu().numpy() for p in planes]
        want = ica.host_transform_planes(pic[0] if len(pic) == 1 else tuple(pic), name, 90)[1]
        assert np.array_equal(enc.fetch(a.n - 1), want), name
        g = []
        for _ in range(launches):
            enc.timer_begin()
            enc.upload()
            enc.timer_end()
            g.append(enc.timer_ms())
        enc.launch()
        enc.wait()
        enc.timer_begin()
        for _ in range(launches):
            enc.launch()
        enc.timer_end()
        return min(g), enc.timer_ms() / launches
    finally:
        enc.close()


def calls_ms(ica, torch, batch, planes, steps, warmup):
    """-> {(name, variant): (best wall ms, stream bytes, host emitted)}, the variants taken in turns inside every step"""
    t = ica.TensorEncoder()
    rows, last = {}, {}
    pics = {name: ([tuple(p[i] for p in planes[name]) for i in range(batch.shape[0])] if name != "grey" else list(planes[name][0].unbind(0)))
            for name in NAMES}

    def timed(key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        rows.setdefault(key, []).append(ms)
        return out

    try:
        for step in range(warmup + steps):
            for name in NAMES:
                out = timed((name, "ycbcr"), lambda: t.encode_ycbcr(pics[name], subsampling=name, quality=90))
                last[(name, "ycbcr")] = sum(len(o) for o in out), t.last_host_emitted
                out = timed((name, "rgb"), lambda: t.encode(batch, subsampling=name, quality=90))
                last[(name, "rgb")] = sum(len(o) for o in out), t.last_host_emitted
                rgb = timed((name, "torch"), lambda: torch_rgb(torch, planes[name], name))
                out = timed((name, "torch_encode"), lambda: t.encode(rgb, subsampling=name, quality=90))
                last[(name, "torch_encode")] = sum(len(o) for o in out), t.last_host_emitted
                del rgb
                print("%s step %d: ycbcr %.1f rgb %.1f torch %.1f + %.1f ms" % ((name, step) + tuple(rows[(name, v)][-1] for v in ("ycbcr", "rgb", "torch", "torch_encode"))),
                      file=sys.stderr, flush=True)
    finally:
        t.close()
    return {k: (min(v[warmup:]),) + last.get(k, (0, 0)) for k, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: the default call is measured against it")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "encode_planes.json"))
    a = ap.parse_args()
    res = {"n": a.n, "distinct": a.distinct, "width": a.width, "height": a.height, "quality": 90, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds}
    if a.parent:  # first, and in processes of their own: this process has not touched the GPU yet
        res["default_against_parent"] = bes.against_parent(a)
    import torch
    sys.path.insert(0, HERE)
    import image_codecs_amd as ica
    ica.build_library()
    if not ica.gpu_available():
        raise SystemExit("no HIP device: nothing here can be measured without one")
    batch = bes.pictures(ica, a)
    planes = {name: planes_of(torch, batch, name) for name in NAMES}
    print("pictures and planes ready", file=sys.stderr, flush=True)
    ctx = ica.Context()
    kr = [{name: kernel_ms(ica, torch, ctx, a, planes[name], name) for name in NAMES} for _ in range(a.rounds)]
    ctx.close()
    cr = [calls_ms(ica, torch, batch, planes, a.steps, a.warmup) for _ in range(a.rounds)]
    npx = a.n * a.width * a.height

    def best(rounds, key, what):
        v = [r[key][0] for r in rounds]
        return {what + "_ms": round(min(v), 4), what + "_ms_spread": round(max(v) - min(v), 4)}

    for name in NAMES:
        src, staged, du = geometry(name, a.width, a.height)
        g, t = [r[name][0] for r in kr], [r[name][1] for r in kr]
        row = {"gather_ms": round(min(g), 4), "gather_ms_spread": round(max(g) - min(g), 4), "gather_bytes_read": src * a.n,
               "gather_bytes_written": staged * a.n, "gather_gb_s": round((src + staged) * a.n / min(g) / 1e6, 1),
               "transform_ms": round(min(t), 4), "transform_ms_spread": round(max(t) - min(t), 4), "transform_bytes_read": staged * a.n,
               "transform_bytes_written": du * a.n, "transform_gb_s": round((staged + du) * a.n / min(t) / 1e6, 1),
               "transform_mpix_s": round(npx / min(t) / 1e3, 1)}
        for variant, what in (("ycbcr", "encode_ycbcr"), ("rgb", "encode_rgb"), ("torch", "torch_to_rgb"), ("torch_encode", "encode_of_torch_rgb")):
            row.update(best(cr, (name, variant), what))
        row["via_torch_ms"] = round(row["torch_to_rgb_ms"] + row["encode_of_torch_rgb_ms"], 4)
        row["encode_ycbcr_mpix_s"] = round(npx / row["encode_ycbcr_ms"] / 1e3, 1)
        row["stream_bytes_ycbcr"], row["host_emitted_ycbcr"] = cr[-1][(name, "ycbcr")][1:]
        row["stream_bytes_rgb"] = cr[-1][(name, "rgb")][1]
        res[name] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
