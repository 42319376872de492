#!/usr/bin/env python3
"""Measures libjpeg's arithmetic in the encoder (include/mij_host.h, LIBJPEG ENCODING; mij_enc_set_arith) on 256 1080p pictures at quality
90 for "420" and "444", all in one run:

  kernels     event time of a launch without an emission arena, per sampling: `stb` the default strip kernel (k_encode420 / k_encode444);
              `libjpeg` k_lj_enc_color + k_lj_encode_planes of pixel slots; `planes` k_lj_encode_planes alone, on plane slots with the
              request, which run pass 2 only; `color` the difference of the last two -- k_lj_enc_color is not launched on its own.  The
              units of the last slot are checked against the host twin first.
  encode      the whole TensorEncoder.encode(subsampling=..., arithmetic=...) call on a [N, 3, H, W] tensor, wall time, "stb" and
              "libjpeg" taken in turns inside every step, and the bytes of their streams.
  default_against_parent   with --parent DIR (a built checkout of the parent commit): the default encode() call at quality 90 and 95
              against it in child processes, one per round and tree, the two trees in turns; the difference of the bests next to the
              spread between the parent's own rounds.  Nothing on the default call's path changes, so it must stay within that spread.

Best of --steps after --warmup in each of --rounds rounds and the spread of the rounds' bests.  No threshold is fixed for the new
kernels: none of these numbers existed before.  Not bench.py: nothing here is a yardstick.

    python tools/bench_encode_libjpeg.py [--n 256] [--steps 5] [--warmup 2] [--rounds 3] [--parent DIR] [--out profiles/encode_libjpeg.json]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
import bench_encode_sampling as bes  # noqa: E402  the parent comparison, the pictures and the call timing are that tool's

NAMES = ("420", "444")


def kernel_ms(ica, ctx, a, name, launches=5):
    """-> {"stb", "libjpeg", "planes"}: ms per launch over a.n pictures, one round"""
    import numpy as np
    img = ica.synth_rgb(a.width, a.height, 0)
    rd, wr = bes.algo_bytes(name, a.width, a.height)
    ncomp, lh, lv = bes.FACTORS[name]
    t, want = ica.host_transform_libjpeg(img, 90, name)
    yy = np.ascontiguousarray(img[..., 0])
    planes = (yy, np.ascontiguousarray(img[::lv, ::lh, 1]), np.ascontiguousarray(img[::lv, ::lh, 2]))
    out = {}
    for what in ("stb", "libjpeg", "planes"):
        enc = ica.Encoder(ctx, a.n, (rd + 256) * a.n, (wr + 256) * a.n, stage_bytes=rd + 256)
        try:
            s0 = enc.add_planes(planes, name, 90) if what == "planes" else enc.add(img, 90, sampling=name)
            if what != "stb":
                enc.set_arith(s0, "libjpeg")
            for _ in range(a.n - 1):
                enc.add_clone(s0)
            enc.upload()
            enc.launch()
            enc.wait()
            if what == "libjpeg":
                assert np.array_equal(enc.fetch(0), want) and np.array_equal(enc.fetch(a.n - 1), want), name
            elif what == "planes":
                assert np.array_equal(enc.fetch(a.n - 1), ica.host_transform_libjpeg_planes(planes, name, 90)[1]), name
            for _ in range(3):
                enc.launch()
            enc.wait()
            enc.timer_begin()
            for _ in range(launches):
                enc.launch()
            enc.timer_end()
            out[what] = enc.timer_ms() / launches
        finally:
            enc.close()
    return out


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
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "encode_libjpeg.json"))
    a = ap.parse_args()
    res = {"n": a.n, "distinct": a.distinct, "width": a.width, "height": a.height, "quality": 90, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds}
    if a.parent:  # first, and in processes of their own: this process has not touched the GPU yet
        res["default_against_parent"] = bes.against_parent(a)
    import torch  # noqa: F401  before the library is first loaded: one HIP runtime for both
    sys.path.insert(0, HERE)
    import image_codecs_amd as ica
    ica.build_library()
    if not ica.gpu_available():
        raise SystemExit("no HIP device: nothing here can be measured without one")
    ctx = ica.Context()
    kr = [{name: kernel_ms(ica, ctx, a, name) for name in NAMES} for _ in range(a.rounds)]
    ctx.close()
    batch = bes.pictures(ica, a)
    todo = [("%s_%s" % (name, ar), {"quality": 90, "subsampling": name, "arithmetic": ar}) for name in NAMES for ar in ("stb", "libjpeg")]
    cr = [bes.encode_ms(ica, batch, todo, a.steps, a.warmup) for _ in range(a.rounds)]
    npx = a.n * a.width * a.height
    for name in NAMES:
        rd, wr = bes.algo_bytes(name, a.width, a.height)
        row = {"pixel_bytes_read": rd * a.n, "unit_bytes_written": wr * a.n, "plane_bytes": wr // 2 * a.n}
        for what in ("stb", "libjpeg", "planes"):
            v = [r[name][what] for r in kr]
            row["kernels_%s_ms" % what] = round(min(v), 4)
            row["kernels_%s_ms_spread" % what] = round(max(v) - min(v), 4)
        row["kernels_color_ms_by_difference"] = round(row["kernels_libjpeg_ms"] - row["kernels_planes_ms"], 4)
        row["kernels_libjpeg_mpix_s"] = round(npx / row["kernels_libjpeg_ms"] / 1e3, 1)
        row["kernels_stb_mpix_s"] = round(npx / row["kernels_stb_ms"] / 1e3, 1)
        for ar in ("stb", "libjpeg"):
            v = [r["%s_%s" % (name, ar)][0] for r in cr]
            row["encode_%s_ms" % ar] = round(min(v), 3)
            row["encode_%s_ms_spread" % ar] = round(max(v) - min(v), 3)
            row["stream_bytes_%s" % ar], row["host_emitted_%s" % ar] = cr[-1]["%s_%s" % (name, ar)][1:]
        res[name] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
