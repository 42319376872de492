#!/usr/bin/env python3
"""bench.py -- JPEG decode Mpixels/sec on a 4:2:0 1080p batch (BASELINE.json's metric).

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

A *step* is one pass of the GPU hot path -- de-quantise + 8x8 integer IDCT + h2v2 upsample +
YCbCr->RGB, i.e. everything the reference does between the Huffman walk and the pixel buffer
(codec/jpeg.c:325-365 dequant, :615-679, :1816-1840, :1976-2018, :2301-2432) -- over the rank's batch of
synthetic 1920x1080 4:2:0 q=90 JPEGs whose quantised coefficients are ALREADY RESIDENT IN HBM when the
timed region starts (host Huffman walk + H2D happen before it -- since round 3 nothing else: the walk writes the
planes in the format the kernel reads, legs.prepass; see DESIGN.md for the PCIe/host-inclusive rates, which are
never `value`).

Workload.  N = 1: BASELINE configs[1], 1024 images on the one GPU.  N > 1: BASELINE configs[2], ONE logical
batch of 4096 images cut into contiguous slices with image-codecs_amd/sharding.shard_range -- rank r owns
images [lo, hi) -- and no data-path collective: images are independent (decoder state is per image,
codec/jpeg.c:2445).  Every slot has its own coefficient and pixel memory (>= 6 GB per GPU >> the 256 MiB
Infinity Cache).  The planes are in the library's DEFAULT format -- compact planes with escape bytes
(include/mij.h) -- produced here by the north-star pipeline: host Huffman walk -> compact planes in pinned
staging (mjh_decode_memory_fmt) -> H2D.  No environment knob is involved.  Every owned image is verified before the timed region: the
distinct sources by hash against the int16 pipeline (and, on rank 0 at N = 1, byte for byte against the
reference itself in the cpu_baseline leg), every further image by a device-side comparison with its source.

A plain run (no --full) does only what the headline needs: set up, warm up, time exactly --steps launches, write the outputs
of the last one if --dump-outputs is given, print the line.  The verification of every image just described, the figure at
exactly --warmup launches (roofline.*_at_requested_warmup), the IDCT wavefront classes, the host stage, the legs, end to end
and the CPU baseline run with --full only; the rest of `roofline` comes from the timed steps and is in every line.

`roofline.achieved` keeps the ALGORITHMIC bytes of SURVEY.md 8(d) in the numerator (int16 coefficients,
12 487 680 B per image); `roofline.traffic` / `hbm_counter_frac` are what the HBM counters saw (fewer bytes:
compact planes), from the rocprofv3 --pmc passes committed under profiles/ (tools/profile.sh).

`roofline.idct_wavefront_classes` (and the same per decode leg): fraction of the launch's IDCT wavefronts that took the DC-only /
2x2 / 4x4 / full transform, counted by one extra untimed launch (mij_batch_count_idct_classes).

N > 1 with --full additionally: every rank runs the end-to-end GPU-walk ring on its slice at the same time with its share of the host
cores (`end_to_end.per_rank` + aggregate), rank 0 times the CPU baseline; control plane on gloo (--control-plane nccl for RCCL).

With --full the one JSON line (rank 0) also carries, all OUTSIDE the timed region and only at N = 1:
  legs.prepass          what stands between the host walk and the fused kernel over 1024 DISTINCT slots: nothing for compact
                        staging; H2D into a scratch + k_pack_c8 (timed alone) for int16 staging; frac_including_pack
  legs.int16_planes     the same kernel family on int16 tile-layout planes
  legs.harsh_batch      1024 images of a harsher declared content (noise&63 + 24 inverted rectangles per image,
                        image-codecs_amd/synth.synth_rgb_edges): escaped blocks in most wavefronts
  legs.config4          BASELINE configs[3]: 32 x 4096x4096 progressive 4:4:4 (k_fused444), 9 B/px
  legs.config5          BASELINE configs[4]: 1024 x 1080p RGB -> data units (k_encode420), bytes == reference
  legs.config5_q95_444  the same at quality 95: the writer's 4:4:4 layout, 512 images (k_encode444), 9 B/px
  legs.h2v1             512 x 1080p 4:2:2 (k_fused422), 7 B/px
  legs.wide_420         22 x 6000x4000 4:2:0: the band kernel in column segments (k_fused420c), and the two-pass kernels on the same pictures
  legs.config1          BASELINE configs[0]: one 512x512 4:2:0 JPEG per stbi_load_from_memory call (latency of the drop-in call)
  legs.two_pass         256 x 1080p through the two-pass family (sample planes in HBM, pass 2 compiled per resampler):
                        the headline images forced off the fused kernel, 4:4:0 fused and forced, Adobe CMYK through
                        k_fused1x1c and forced
  end_to_end            bitstream in host RAM -> pixels in HBM (host walk; GPU walk), never `value`
  cpu_baseline          the reference itself (oracle/_ref, compiled in place in the build container and shipped
                        as a .so; "reference") -- or, when that .so is absent (clean checkout), our CPU
                        restatement (oracle/, "port") -- on this box's host cores, same images, pixels compared.
A failing leg reports its error inside the line; it never costs the headline.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before torch / HIP initialise: one hardware queue per batch stream

W, H = 1920, 1080
ALGO_BYTES_PER_IMAGE = 2 * 64 * 48960 + 3 * W * H  # 6 266 880 + 6 220 800
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
CONFIG3_TOTAL = 4096   # BASELINE configs[2]


def usable_cores():
    """Host threads this process may really use: the affinity mask, capped by the cgroup CPU quota
    (a GPU box shows every core of the host in the mask but grants a 1-GPU job only a share)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, (q + p // 2) // p))
        except (OSError, ValueError):
            pass
    env = os.environ.get("BENCH_CPU_THREADS")
    if env:
        n = max(1, int(env))
    return n


def cpu_checker():
    """(library, kind): the reference compiled in place when its .so travelled, our CPU restatement otherwise."""
    ref_so = os.path.join(ROOT, "oracle", "_ref", "libstbref.so")
    port_so = os.path.join(ROOT, "oracle", "_build", "liboracle.so")
    if os.path.exists(ref_so):
        return C.CDLL(ref_so), "reference"
    if not os.path.exists(port_so):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "port"], check=True)
    return C.CDLL(port_so), "port"


def cpu_decode(L, kind, data, req=3):
    load = L.stbi_load_from_memory if kind == "reference" else L.orc_load_from_memory
    load.restype = C.POINTER(C.c_ubyte)
    ints = [C.POINTER(C.c_int)] * 3
    load.argtypes = [C.c_char_p, C.c_int] + ints + [C.c_int] + ([C.POINTER(C.c_char_p)] if kind == "port" else [])
    x, y, c = C.c_int(), C.c_int(), C.c_int()
    extra = [C.byref(C.c_char_p())] if kind == "port" else []
    ptr = load(data, len(data), C.byref(x), C.byref(y), C.byref(c), req, *extra)
    if not ptr:
        return None
    out = np.ctypeslib.as_array(ptr, shape=(y.value * x.value * req,)).copy()
    free = L.stbi_image_free if kind == "reference" else L.orc_free
    free.argtypes = [C.c_void_p]
    free(ptr)
    return out


def cpu_baseline(datas, want_seconds=12.0, gpu_pixels=None):
    """Times the CPU checker on a bounded sample (all host cores, one image per task); with gpu_pixels(i) it also
    acts as what it is -- the checker: its pixels for every distinct image must equal the GPU's."""
    L, kind = cpu_checker()
    f = getattr(L, "ref_decode_many" if kind == "reference" else "orc_decode_many")
    f.restype = C.c_long
    f.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    n = len(datas)
    bufs = (C.c_char_p * n)(*datas)
    lens = (C.c_int * n)(*[len(d) for d in datas])
    secs = C.c_double()
    cores = usable_cores()
    # single thread, one pass over the sample
    px1 = f(bufs, lens, n, 1, 1, 3, C.byref(secs))
    single = px1 / secs.value / 1e6
    # all usable cores: calibrate with a short run, then size the real one for ~want_seconds of wall time
    cal_reps = max(1, (2 * cores + n - 1) // n)
    f(bufs, lens, n, cal_reps, cores, 3, C.byref(secs))
    reps = max(cal_reps, min(int(want_seconds / max(secs.value, 1e-3) * cal_reps), 4096))
    px = f(bufs, lens, n, reps, cores, 3, C.byref(secs))
    parity = None
    if gpu_pixels is not None:
        parity = all(np.array_equal(cpu_decode(L, kind, d), gpu_pixels(i).reshape(-1)) for i, d in enumerate(datas))
        assert parity, "GPU pixels differ from the CPU checker's"
    model = None
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {
        "parity_with_gpu_output": parity,
        "cpu_model": model,
        "value": round(px / secs.value / 1e6, 1),
        "unit": "Mpix/s",
        "cores": cores,
        "kind": kind,
        "sample": "%d distinct 1920x1080 4:2:0 q90 images x %d passes, one image per task on %d threads (%.1f s); single thread: %.1f Mpix/s"
                  % (n, reps, cores, secs.value, single),
        "single_thread_mpix_s": round(single, 1),
    }


# ---------------------------------------------------------------------------------------------------- resident batches

def resident_batch(ica, ctx, datas, first, count, fmt, cbytes, obytes, generic=0):
    """Images first .. first+count-1 of the logical batch (image g uses source g % len(datas)) resident in HBM in the
    given plane format: the first occurrence of every source is host-walked into pinned staging, the others are clones
    with their own device buffers.  -> (batch, (source index, source slot or None) of every slot, seconds of host walk)"""
    distinct = len(datas)
    bt = ica.Batch(ctx, count, cbytes * min(distinct, count), cbytes * count, obytes * count)
    bt.set_coef_format(fmt)
    if generic:
        bt.force_generic(generic)
    src_slot, owners = {}, []
    t0 = time.time()
    for i in range(count):
        k = (first + i) % distinct
        if k not in src_slot:
            src_slot[k] = bt.add_jpeg(datas[k], 3)  # host Huffman walk straight into pinned staging
            owners.append((k, None))
        else:
            bt.add_clone(src_slot[k])  # own device buffers, filled device-to-device
            owners.append((k, src_slot[k]))
    dt = time.time() - t0
    bt.upload()
    bt.wait()
    return bt, owners, dt


def verify_batch(batch, owners, src_hash):
    """Every image of the batch: sources by hash, clones by a device-side comparison with their source."""
    pairs = []
    for slot, (k, src) in enumerate(owners):
        if src is None:
            assert batch.hash_out(slot) == src_hash[k], "source image %d differs from the reference pipeline's pixels" % k
        else:
            pairs.append((slot, src))
    for lo in range(0, len(pairs), 256):
        bad = batch.diff_slots(pairs[lo:lo + 256])
        assert bad == 0, "%d words of cloned images differ from their source" % bad
    return len(owners)


def warm(bt, launches, settle_ms):
    t_w = time.perf_counter()
    k = 0
    while k < max(1, launches) or (time.perf_counter() - t_w) * 1e3 < settle_ms:
        bt.launch()
        k += 1
        if k % 8 == 0:
            bt.wait()  # bound the queue depth while watching the wall clock
    bt.wait()
    return k


def timed_launches(bt, steps):
    """kernel ms per launch over exactly `steps` launches, HIP events on the batch's own stream"""
    bt.timer_begin()
    for _ in range(steps):
        bt.launch()
    bt.timer_end()
    bt.wait()
    return bt.timer_ms() / steps


DUMP_SAMPLE_SLOTS = 16        # images of the batch sampled for --dump-outputs (besides its last one, dumped whole)
DUMP_SAMPLE_VALUES = 1 << 18  # values per sampled image, the same positions in every one


def dump_outputs(bt, count, d):
    """--dump-outputs: the RGB8 pixels the last launch left in the batch as float32 .npy files under d -- the last image whole
    (rgb_last_image), and for a fixed seeded choice of images the same fixed seeded positions of each (rgb_sample, with the image and
    flat byte indices in rgb_sample_slots / rgb_sample_positions).  43 MB at 1080p; -> {name: shape}"""
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(20261015)
    slots = np.sort(rng.choice(count, size=min(DUMP_SAMPLE_SLOTS, count), replace=False))
    last = bt.fetch(count - 1)
    pos = np.sort(rng.choice(last.size, size=min(DUMP_SAMPLE_VALUES, last.size), replace=False))
    arrays = {
        "rgb_last_image": last.astype(np.float32),
        "rgb_sample": np.stack([bt.fetch(int(s)).reshape(-1)[pos] for s in slots]).astype(np.float32),
        "rgb_sample_slots": slots.astype(np.float64),
        "rgb_sample_positions": pos.astype(np.float64),
    }
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20, "outputs to dump exceed 64 MB"
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def frac_of(algo_bytes, ms):
    return algo_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS


def traffic_entry(key):
    """profiles/traffic.json[key] = {"hbm_bytes_per_launch": ..., "source": ...} from the committed rocprofv3 --pmc passes"""
    try:
        e = json.load(open(os.path.join(ROOT, "profiles", "traffic.json"))).get(key)
        if isinstance(e, dict) and "hbm_bytes_per_launch" in e:
            return e
    except Exception:  # noqa: BLE001
        pass
    return None


def kernel_source_hash():
    """first 16 hex digits of the SHA-256 over the kernel sources: profiles/traffic.json entries carry the hash of the build they were measured on"""
    import hashlib
    h = hashlib.sha256()
    for f in ("mij_kernels.h", "mij_entropy_kernels.h"):  # the device code; host-side runtime changes do not move the counters
        try:
            h.update(open(os.path.join(ROOT, "image-codecs_amd", "csrc", f), "rb").read())
        except OSError:
            h.update(b"missing:" + f.encode())
    return h.hexdigest()[:16]


def add_traffic(res, key):
    t = traffic_entry(key)
    res["traffic"] = t["hbm_bytes_per_launch"] if t else None
    res["traffic_source"] = ("profiles/traffic.json[%s]: %s" % (key, t.get("source", "rocprofv3 --pmc passes"))) if t else \
        "not measured for this launch shape (profiles/traffic.json has no entry %s)" % key
    res["hbm_counter_frac"] = round(t["hbm_bytes_per_launch"] / (res["kernel_ms_per_launch"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if t else None
    if t:  # the committed counters are only as fresh as the build they were taken on -- say so in the line
        res["traffic_kernel_hash"] = t.get("kernel_source_hash")
        res["traffic_stale"] = t.get("kernel_source_hash") != kernel_source_hash()


# ---------------------------------------------------------------------------------------------------- secondary legs

def idct_classes(bt):
    """one more (untimed) launch with the kernels counting wavefronts per sparse-block class (mij.h, mij_batch_count_idct_classes): the
    fraction of the launch's IDCT wavefronts that took the DC-only / 2x2 / 4x4 / full transform"""
    bt.count_idct_classes(True)
    bt.launch()
    bt.wait()
    c = bt.idct_class_counts()
    bt.count_idct_classes(False)
    tot = float(max(1, sum(c)))
    return {"dc_only": round(c[0] / tot, 4), "inside_2x2": round(c[1] / tot, 4), "inside_4x4": round(c[2] / tot, 4), "full": round(c[3] / tot, 4), "wavefronts": int(sum(c))}


def leg_decode_1080p(ica, ctx, datas, count, fmt, cbytes, obytes, args, expect_path=1, src_hash=None, checker=None, generic=0):
    """Kernel-resident timing of `count` 1080p images in the given plane format; returns (result dict, plane format seen)."""
    bt, owners, _ = resident_batch(ica, ctx, datas, 0, count, fmt, cbytes, obytes, generic)
    try:
        bt.launch()
        bt.wait()
        assert {bt.slot_path(s) for s in range(count)} == {expect_path}
        if src_hash is None:  # this leg's own sources: against the CPU checker (the reference itself when its .so travelled)
            L, kind = checker
            src_hash = []
            for k, d in enumerate(datas):
                slot = next(s for s, (kk, src) in enumerate(owners) if kk == k and src is None)
                assert np.array_equal(bt.fetch(slot).reshape(-1), cpu_decode(L, kind, d)), "source %d differs from the CPU checker" % k
                src_hash.append(bt.hash_out(slot))
        verify_batch(bt, owners, src_hash)
        n_warm = warm(bt, args.warmup, args.settle_ms)
        ms = timed_launches(bt, args.steps)
        esc = sum(bt.slot_escapes(s) for s, (k, src) in enumerate(owners) if src is None) if fmt == "compact" else 0
        return {"kernel_ms_per_launch": round(ms, 4), "images": count, "warmup_launches_issued": n_warm, "parity": True,
                "escaped_blocks_in_sources": esc, "idct_wavefront_classes": idct_classes(bt)}, bt.slot_coef_bytes(0)
    finally:
        bt.close()


def leg_config4(ica, ctx, args, checker):
    """BASELINE configs[3] at a reduced batch: 32 x 4096x4096 progressive 4:4:4, planes re-staged over ten scans on the
    host, packed on the device, k_fused444 timed resident.  Algorithmic 9 B/px."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    n, size = args.config4_images, 4096
    t0 = time.time()
    plan, du = ica.host_transform(ica.synth_rgb(size, size, 1), 95)  # quality > 90 -> 4:4:4
    data = helpers.progressive_from_du(plan, du, 1)
    d = ica.HostDecoder.probe(data, 3)
    cb, ob = ica.Batch.coef_bytes(d), ica.Batch.out_bytes(d)
    b = ica.Batch(ctx, n, cb, cb * n, ob * n)
    try:
        th = time.time()
        s0 = b.add_jpeg(data, 3)
        host_s = time.time() - th
        for _ in range(n - 1):
            b.add_clone(s0)
        b.upload()
        b.launch()
        b.wait()
        assert b.slot_path(0) == 3, b.slot_path(0)
        L, kind = checker
        assert np.array_equal(b.fetch(0).reshape(-1), cpu_decode(L, kind, data)), "config 4 pixels differ from the CPU checker"
        assert b.diff_slots([(s, 0) for s in range(1, n)]) == 0
        n_warm = warm(b, args.warmup, args.settle_ms)
        ms = timed_launches(b, args.steps)
        blocks = 3 * d.comp[0].bw * d.comp[0].bh
        algo = n * (128 * blocks + 3 * size * size)
        res = {"workload": "%d x %dx%d progressive 4:4:4 (10 scans, %d bytes each), coefficients resident" % (n, size, size, len(data)),
               "kernel": "mij::k_fused444<3,false,%s>" % ("true" if b.slot_coef_bytes(0) else "false"), "kernel_ms_per_launch": round(ms, 4),
               "algorithmic_bytes_per_launch": algo, "mpix_s": round(n * size * size / ms / 1e3, 1), "frac": round(frac_of(algo, ms), 4),
               "parity": True, "parity_against": kind, "warmup_launches_issued": n_warm,
               "host_progressive_stage_mpix_s_single_thread": round(size * size / host_s / 1e6, 1), "setup_s": round(time.time() - t0, 1)}
        add_traffic(res, "k_fused444_compact_%d" % n)
        # end to end for this layout: 16 streams in host RAM -> pixels in HBM, every scan walked on the host threads (progressive
        # scans cannot take the GPU walk: AC refinement does not re-synchronise), planes re-staged, packed, transformed
        b.close()
        b = None
        threads, ne, chunk = usable_cores(), 64, 16
        # two batches ping-pong, as in the 1080p end-to-end leg: the upload, pack and kernel of chunk k run while the host threads walk chunk k+1
        ebs = [ica.Batch(ctx, chunk, cb * chunk, cb * chunk, ob * chunk) for _ in range(2)]
        try:
            for eb in ebs:  # page in the staging, start the pool
                eb.decode_jpegs([data] * 2, 3, threads, gpu_entropy=False)
                eb.submit()
                eb.wait()
            import threading
            th = 0.0
            te = time.perf_counter()
            last, subs = {}, {}
            for k, lo in enumerate(range(0, ne, chunk)):
                eb = ebs[k & 1]
                if (k & 1) in subs:
                    subs.pop(k & 1).join()
                eb.reset()  # waits for this batch's previous chunk
                t0 = time.perf_counter()
                ok, slots, reasons = eb.decode_jpegs([data] * chunk, 3, threads, gpu_entropy=False)
                th += time.perf_counter() - t0
                assert ok == chunk, reasons
                # submit on a helper thread: upload of a progressive chunk waits once for the pack kernel's L1 maxima (1.6 GB of int16 planes
                # go up first), and the host threads should be walking the next chunk meanwhile (ctypes drops the GIL around the call)
                subs[k & 1] = threading.Thread(target=eb.submit)
                subs[k & 1].start()
                last[k & 1] = slots[-1]
            for t in subs.values():
                t.join()
            for eb in ebs:
                eb.wait()
            te = time.perf_counter() - te
            want = cpu_decode(L, kind, data)
            for side, slot in last.items():
                assert np.array_equal(ebs[side].fetch(slot).reshape(-1), want), "config 4 end to end: pixels differ from the CPU checker"
            res["end_to_end"] = {"mpix_s": round(ne * size * size / te / 1e6, 1), "images": ne, "chunk_images": chunk, "host_threads": threads,
                                 "host_stage_only_mpix_s": round(ne * size * size / th / 1e6, 1),
                                 "note": "ten scans per picture on the host threads (the reference's scan structure, codec/jpeg.c:372-558), two batches ping-pong; bound by the host stage"}
        finally:
            for eb in ebs:
                eb.close()
        return res
    finally:
        if b is not None:
            b.close()


def golden_writer_entry(quality, seed):
    """(length, sha256) the REFERENCE's writer gave for synth_rgb(1920, 1080, seed) at this quality, from the committed fixture
    tests/golden/writer_golden_r3.npz (made by tests/golden/make_golden_r3.py); None when the fixture does not cover it"""
    try:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "writer_golden_r3.npz"), allow_pickle=False)
        lens, shas = z["bench/q%d/len" % quality], z["bench/q%d/sha256" % quality]
        return (int(lens[seed]), bytes(shas[seed])) if seed < len(lens) else None
    except Exception:
        return None


def dump_evidence(tag, **arrays):
    """keeps what a failed parity check looked at: gpurun_out/evidence/<tag>_<pid>_<ns>.npz (+ .maps: /proc/self/maps, the environment's
    loader / profiler variables); never overwrites, returns the path"""
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpurun_out", "evidence")
    try:
        os.makedirs(d, exist_ok=True)
        base = os.path.join(d, "%s_%d_%d" % (tag, os.getpid(), time.time_ns()))
        np.savez_compressed(base + ".npz", **arrays)
        with open(base + ".maps", "w") as f:
            for k in sorted(os.environ):
                if k.startswith(("LD_", "ROC", "HSA", "HIP", "GPU_", "MIJ_", "AMD")):
                    f.write("%s=%s\n" % (k, os.environ[k]))
            f.write(open("/proc/self/maps").read())
        return base + ".npz"
    except Exception as ex:  # the check still fails; say why nothing was kept
        return "(not kept: %s)" % ex


def leg_config5(ica, ctx, args, checker, quality=90, count=None):
    """BASELINE configs[4]: 1024 x 1080p RGB -> quantised data units (k_encode420; quality above 90: the writer's 4:4:4 layout,
    k_encode444, 512 images); the byte streams of the distinct images equal the CPU checker's (the reference's own writer when
    its .so travelled)."""
    n, distinct = (count or args.images), 4
    sub = quality <= 90  # codec/jpeg_write.c:221
    units = 120 * 68 * 6 if sub else 240 * 135 * 3
    imgs = [ica.synth_rgb(W, H, s) for s in range(distinct)]
    pix = (W * H * 3 + 255) // 256 * 256
    dub = (units * 128 + 255) // 256 * 256
    enc = ica.Encoder(ctx, n, pix * n, dub * n)
    try:
        src = [enc.add(im, quality) for im in imgs]
        for i in range(distinct, n):
            enc.add_clone(src[i % distinct])
        enc.upload()
        enc.launch()
        enc.wait()
        L, kind = checker
        fenc = L.ref_encode if kind == "reference" else L.orc_encode
        fenc.restype = C.c_long
        fenc.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        for k, im in enumerate(imgs):
            plan_k, units_k = enc.plan(src[k]), enc.fetch(src[k])
            mine = ica.emit_jpeg(plan_k, units_k)
            if os.environ.get("MIJ_BENCH_SELFTEST_MISMATCH") == "1" and k == 0:
                mine = mine[:1000] + bytes([mine[1000] ^ 1]) + mine[1001:]  # rehearsal of the evidence branch below (tools/selftest_evidence.sh); never set otherwise
            buf = np.zeros(W * H * 3, np.uint8)
            nb = fenc(buf.ctypes.data, buf.size, W, H, 3, np.ascontiguousarray(im).ctypes.data, quality)
            if not (nb > 0 and mine == bytes(buf[:nb])):
                # Seen twice in round 2, each time in the first process of a fresh box under rocprofv3 --kernel-trace --stats, never
                # elsewhere, and the retry overwrote the record.  This branch now KEEPS the evidence: both byte
                # streams, the units the emission used (first fetch), a second fetch, the library's host transform, both plans' tables,
                # the reference-made golden length / hash of this picture, the process map and the float state go to a uniquely
                # named file under gpurun_out/evidence/ before the leg fails.
                import hashlib
                want = bytes(buf[:max(nb, 0)])
                plan_h, host_units = ica.host_transform(im, quality)
                units2 = enc.fetch(src[k])
                mine_host = ica.emit_jpeg(plan_h, host_units)
                mine_again = ica.emit_jpeg(enc.plan(src[k]), units2)
                buf2 = np.zeros(W * H * 3, np.uint8)
                nb2 = fenc(buf2.ctypes.data, buf2.size, W, H, 3, np.ascontiguousarray(im).ctypes.data, quality)
                first = next((i for i in range(min(len(mine), len(want))) if mine[i] != want[i]), min(len(mine), len(want)))
                third = np.float32(1) / np.float32(3)
                whole = ica.stbi_write_jpg_to_memory(im, quality)
                gold = golden_writer_entry(quality, k)
                where = dump_evidence(
                    "enc_q%d_img%d" % (quality, k), mine=np.frombuffer(mine, np.uint8), want=np.frombuffer(want, np.uint8), mine_host_units=np.frombuffer(mine_host, np.uint8),
                    mine_second_fetch=np.frombuffer(mine_again, np.uint8), whole=np.frombuffer(whole, np.uint8), units_first_fetch=units_k, units_second_fetch=units2,
                    units_host=host_units, ytab=np.frombuffer(bytes(plan_k.ytab), np.uint8), ctab=np.frombuffer(bytes(plan_k.ctab), np.uint8),
                    fdtbl_y=np.array(plan_k.fdtbl_y[:], np.float32), fdtbl_c=np.array(plan_k.fdtbl_c[:], np.float32),
                    host_ytab=np.frombuffer(bytes(plan_h.ytab), np.uint8), host_fdtbl_y=np.array(plan_h.fdtbl_y[:], np.float32),
                    host_fdtbl_c=np.array(plan_h.fdtbl_c[:], np.float32), checker_second=np.frombuffer(bytes(buf2[:max(nb2, 0)]), np.uint8),
                    golden_len=np.array([gold[0] if gold else -1]), golden_sha256=np.frombuffer(gold[1] if gold else b"", np.uint8))
                raise AssertionError(
                    "encoded stream %d differs from the CPU checker's (checker bytes %d, ours %d, first difference at byte %d; first fetch == second fetch: %s; "
                    "second fetch == host transform: %s; units sha1 %s; emit(host units) == checker: %s; emit(second fetch) == first emission: %s, == checker: %s; "
                    "stbi_write_jpg_to_memory == checker: %s; checker repeatable: %s; reference-made golden: checker %s, ours %s; float32 1/3 = %s; evidence kept in %s)"
                    % (k, nb, len(mine), first, bool(np.array_equal(units_k, units2)), bool(np.array_equal(units2, host_units)),
                       hashlib.sha1(np.ascontiguousarray(units_k)).hexdigest()[:12], mine_host == want, mine_again == mine, mine_again == want,
                       whole == want, nb2 == nb and bytes(buf2[:max(nb2, 0)]) == want,
                       (gold is not None and hashlib.sha256(want).digest() == gold[1]), (gold is not None and hashlib.sha256(mine).digest() == gold[1]),
                       third.view(np.uint32), where))
        assert np.array_equal(enc.fetch(n - 1), enc.fetch(src[(n - 1) % distinct]))
        n_warm = 0
        t_w = time.perf_counter()
        while n_warm < max(1, args.warmup) or (time.perf_counter() - t_w) * 1e3 < args.settle_ms:
            enc.launch()
            n_warm += 1
            if n_warm % 8 == 0:
                enc.wait()
        enc.wait()
        enc.timer_begin()
        for _ in range(args.steps):
            enc.launch()
        enc.timer_end()
        ms = enc.timer_ms() / args.steps
        algo = n * (W * H * 3 + units * 128)
        res = {"workload": "%d x 1920x1080 RGB -> %s q=%d data units, pixels resident" % (n, "4:2:0" if sub else "4:4:4", quality),
               "kernel": "mij::k_encode420" if sub else "mij::k_encode444",
               "kernel_ms_per_launch": round(ms, 4), "algorithmic_bytes_per_launch": algo, "mpix_s": round(n * W * H / ms / 1e3, 1),
               "frac": round(frac_of(algo, ms), 4), "parity": True, "parity_against": kind + " (byte streams of the %d distinct images)" % distinct,
               "warmup_launches_issued": n_warm}
        if sub:
            add_traffic(res, "k_encode420_%d" % n)
            enc.close()
            enc = None
            res["end_to_end"] = encode_end_to_end(ica, imgs, quality, kind, fenc)
        return res
    finally:
        if enc is not None:
            enc.close()


def encode_end_to_end(ica, imgs, quality, kind, fenc):
    """256 x 1080p RGB pictures in host memory -> 256 JPEG byte streams in host memory through mij_write_jpg_batch (staging copies and
    Huffman emission on the host threads around one GPU launch), timed around the C call; next to the CPU checker's writer on one thread."""
    L = ica.lib()
    n, threads = 256, usable_cores()
    arrs = [np.ascontiguousarray(imgs[i % len(imgs)]) for i in range(n)]
    L.mij_write_jpg_batch.restype = C.c_int
    L.mij_write_jpg_batch.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    px = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    xs, ys, cs = (C.c_int * n)(*[W] * n), (C.c_int * n)(*[H] * n), (C.c_int * n)(*[3] * n)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    best, first = None, None
    for rep in range(3):
        out, lens = (C.c_void_p * n)(), (C.c_size_t * n)()
        t0 = time.perf_counter()
        rc = L.mij_write_jpg_batch(px, xs, ys, cs, n, quality, threads, out, lens)
        dt = time.perf_counter() - t0
        assert rc == n, "mij_write_jpg_batch wrote %d of %d streams" % (rc, n)
        if first is None:
            first = C.string_at(out[0], lens[0])
        for i in range(n):
            libc.free(out[i])
        best = dt if best is None or dt < best else best
    buf = np.zeros(W * H * 3, np.uint8)
    t0 = time.perf_counter()
    nb = fenc(buf.ctypes.data, buf.size, W, H, 3, arrs[0].ctypes.data, quality)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    assert nb > 0 and first == bytes(buf[:nb]), "batch writer's stream 0 differs from the CPU checker's"
    return {"mpix_s": round(n * W * H / best / 1e6, 1), "images": n, "host_threads": threads, "ms_per_batch": round(best * 1e3, 2),
            "cpu_checker_ms_per_picture_one_thread": round(cpu_ms, 2), "cpu_checker": kind,
            "includes": "pixels in host RAM -> pinned staging (host threads) -> H2D -> k_encode420 -> D2H of the data units -> Huffman emission (host threads) -> byte streams in host RAM"}


def leg_prepass(ica, ctx, datas, n, cbytes, obytes, headline_ms):
    """What stands between the host walk and the fused kernel, over n DISTINCT slots (own staging, no device-side clones):
      staged_compact  round 3's pipeline: the baseline walk writes compact planes itself (mjh_decode_memory_fmt), upload is one H2D per picture of
                      its main part -- nothing runs on the device before the fused kernel
      staged_int16    the pipeline of rounds 1-2, still what progressive files take: int16 staging -> H2D into a scratch -> k_pack_c8, timed alone
                      with HIP events on the batch's stream (mij_batch_pack_ms)
    Staging of the 16 distinct pictures is copied into the other slots on the host (the walk itself is timed elsewhere); wall times include PCIe."""
    import copy
    distinct = len(datas)
    out = {"images": n, "distinct_slots": n, "note": "pack_ms = k_pack_c8 alone (HIP events); upload_wall_ms = H2D of every slot's staging + pack, host wall clock; "
           "frac_including_pack = algorithmic bytes / (fused kernel ms + pack ms) / 8 TB/s"}
    for mode in ("staged_compact", "staged_int16"):
        bt = ica.Batch(ctx, n, cbytes * n, cbytes * n, obytes * n)
        try:
            src = [bt.add_jpeg(datas[k], 3, stage=None if mode == "staged_compact" else "int16") for k in range(min(distinct, n))]
            regions = [bt.stage_region(s) for s in src]
            for i in range(len(src), n):
                k = i % distinct
                s = bt.add(copy.copy(bt.descs[src[k]]))
                bt.stage_region(s)[:] = regions[k]
                bt.set_flags(s, bt.descs[src[k]].flags)
            bt.wait()
            t0 = time.perf_counter()
            bt.upload()
            bt.wait()
            wall = (time.perf_counter() - t0) * 1e3
            pack = bt.pack_ms()
            bt.launch()
            bt.wait()
            assert {bt.slot_path(s) for s in range(n)} == {1} and bt.slot_coef_bytes(n - 1) == 1
            # parity of slots that were never cloned on the device: every 64th against its source picture
            for s in range(0, n, 64):
                assert bt.diff_slots([(s, s % distinct)]) == 0 if s >= distinct else True
            main = sum(((bt.descs[0].comp[c].bw * bt.descs[0].comp[c].bh + 63) // 64) * (4096 + 128) for c in range(3))
            out[mode] = {"pack_ms": None if pack is None else round(pack, 4), "upload_wall_ms": round(wall, 2),
                         "h2d_bytes_per_image": main if mode == "staged_compact" else int(cbytes // 8320 * 8192),
                         "frac_including_pack": round(frac_of(ALGO_BYTES_PER_IMAGE * n, headline_ms + (pack or 0.0)), 4)}
        finally:
            bt.close()
    out["pack_ms_per_1024_distinct"] = None if out["staged_int16"]["pack_ms"] is None else round(out["staged_int16"]["pack_ms"] * 1024.0 / n, 4)
    return out


def leg_h2v1(ica, ctx, args, checker):
    """512 x 1080p 4:2:2 (h2v1) through k_fused422; algorithmic 7 B/px."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    n = args.h2v1_images
    plan, du = ica.host_transform(ica.synth_rgb(W, H, 1), 95)
    data = helpers.baseline_from_du(plan, du, layout="422")
    d = ica.HostDecoder.probe(data, 3)
    cb, ob = ica.Batch.coef_bytes(d), ica.Batch.out_bytes(d)
    res, fmt = leg_decode_1080p(ica, ctx, [data], n, "compact", cb, ob, args, expect_path=4, checker=checker)
    blocks = sum(d.comp[c].bw * d.comp[c].bh for c in range(3))
    algo = n * (128 * blocks + 3 * W * H)
    ms = res["kernel_ms_per_launch"]
    res.pop("escaped_blocks_in_sources", None)
    res.update({"workload": "%d x 1920x1080 baseline 4:2:2, coefficients resident" % n, "kernel": "mij::k_fused422<3,false,%s>" % ("true" if fmt else "false"),
                "algorithmic_bytes_per_launch": algo, "mpix_s": round(n * W * H / ms / 1e3, 1), "frac": round(frac_of(algo, ms), 4), "parity_against": checker[1]})
    add_traffic(res, "k_fused422_compact_%d" % n)
    return res


def leg_wide420(ica, ctx, args, checker):
    """22 x 6000x4000 baseline 4:2:0 (a 24-megapixel camera file): a row of MCUs beyond the LDS of a CU, the band kernel in column
    segments (k_fused420c, round 3) where the two-pass kernels ran before; the same pictures through those for comparison."""
    n, w, h = 22, 6000, 4000
    data = ica.synth_jpeg(w, h, 0, 90)
    d = ica.HostDecoder.probe(data, 3)
    cb, ob = ica.Batch.coef_bytes(d), ica.Batch.out_bytes(d)
    blocks = sum(d.comp[c].bw * d.comp[c].bh for c in range(3))
    algo = n * (128 * blocks + 3 * w * h)
    out = {}
    for name, generic, path in (("segments", 0, 1), ("two_pass", 1, 2)):
        res, fmt = leg_decode_1080p(ica, ctx, [data], n, "compact", cb, ob, args, expect_path=path, checker=checker, generic=generic)
        ms = res["kernel_ms_per_launch"]
        res.pop("escaped_blocks_in_sources", None)
        res.update({"mpix_s": round(n * w * h / ms / 1e3, 1), "frac": round(frac_of(algo, ms), 4)})
        out[name] = res
    res = out["segments"]
    res.update({"workload": "%d x %dx%d baseline 4:2:0 q=90, coefficients resident" % (n, w, h), "kernel": "mij::k_fused420c<3,false,true>", "algorithmic_bytes_per_launch": algo,
                "parity_against": checker[1], "two_pass_kernels_on_the_same_pictures": {k: out["two_pass"][k] for k in ("kernel_ms_per_launch", "mpix_s", "frac", "parity")}})
    add_traffic(res, "k_fused420c_compact_%d" % n)
    return res


def leg_config1(ica, checker):
    """BASELINE configs[0]: ONE 512x512 baseline 4:2:0 q=90 JPEG through stbi_load_from_memory, the call a user of the reference
    makes -- bitstream in host memory -> malloc'ed pixels in host memory, per call: header parse, Huffman walk (on the GPU from
    this size up), kernels, D2H.  Median wall time of 200 calls from one host thread, next to the CPU checker on the same thread."""
    L = ica.lib()
    data = ica.stbi_write_jpg_to_memory(ica.synth_rgb(512, 512, 1), 90)
    x, y, c = C.c_int(), C.c_int(), C.c_int()
    L.stbi_image_free.argtypes = [C.c_void_p]

    def call():
        t0 = time.perf_counter()
        p = L.stbi_load_from_memory(data, len(data), C.byref(x), C.byref(y), C.byref(c), 3)
        dt = time.perf_counter() - t0
        assert p, "stbi_load_from_memory failed: %s" % ica.stbi_failure_reason()
        return p, dt

    p, _ = call()
    got = np.ctypeslib.as_array(p, shape=(512 * 512 * 3,)).copy()
    L.stbi_image_free(p)
    Lc, kind = checker
    want = cpu_decode(Lc, kind, data)
    assert np.array_equal(got, want), "config 1: pixels differ from the CPU checker's"
    for _ in range(20):
        L.stbi_image_free(call()[0])
    ts = []
    for _ in range(200):
        p, dt = call()
        ts.append(dt)
        L.stbi_image_free(p)
    t0 = time.perf_counter()
    for _ in range(20):
        cpu_decode(Lc, kind, data)
    cpu_ms = (time.perf_counter() - t0) / 20 * 1e3
    ms = float(np.median(ts)) * 1e3
    return {"workload": "one 512x512 baseline 4:2:0 q=90 JPEG (%d bytes) per stbi_load_from_memory call, host memory in, host memory out" % len(data),
            "ms_per_call_median": round(ms, 4), "ms_per_call_p90": round(float(np.percentile(ts, 90)) * 1e3, 4), "mpix_s": round(512 * 512 / ms / 1e3, 1),
            "cpu_checker_ms_per_call": round(cpu_ms, 4), "cpu_checker": kind, "parity": True,
            "note": "latency of the drop-in call, not a throughput figure: one image per call leaves the GPU idle (batch front ends: end_to_end)"}


def leg_two_pass(ica, ctx, datas, args, checker):
    """The two-pass family (k_idct_planes, then k_resample_fast compiled per resampler) on 256 x 1080p: the headline 4:2:0
    images forced off the fused kernel, 4:4:0 (default choice: the fused k_fused440; and forced onto the two-pass family) and
    Adobe CMYK, which only has this path.  ms = both passes of
    one launch; algorithmic bytes as for the fused kernels (2 B x coefficients + 3 x W x H)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    n = 256
    plan, du = ica.host_transform(ica.synth_rgb(W, H, 2), 92)
    d440 = helpers.baseline_layout_from_444(plan, du, [(1, 2), (1, 1), (1, 1)], -1)
    cases = (("h2v2_forced", datas[0], 1, 2), ("h1v2_440", d440, 0, 6), ("h1v2_440_forced", d440, 1, 2),
             ("cmyk_adobe", helpers.baseline_layout_from_444(plan, du, [(1, 1)] * 4, 0), 0, 7),
             ("cmyk_adobe_forced", helpers.baseline_layout_from_444(plan, du, [(1, 1)] * 4, 0), 1, 2))
    out = {"images": n, "kernels": "mij::k_idct_planes<false,true> + mij::k_resample_fast<RS_HV2 | RS_V2 | RS_ROW1, ...>; h1v2_440 (default choice): mij::k_fused440w<3,false,true> (a 1080p row leaves room for two workgroups per CU: the eight-wave form); cmyk_adobe (default choice since round 3): mij::k_fused1x1c<3,false,true>",
           "parity_against": checker[1]}
    for name, data, generic, path in cases:
        d = ica.HostDecoder.probe(data, 3)
        cb, ob = ica.Batch.coef_bytes(d), ica.Batch.out_bytes(d)
        res, _ = leg_decode_1080p(ica, ctx, [data], n, "compact", cb, ob, args, expect_path=path, checker=checker, generic=generic)
        algo = n * (128 * sum(d.comp[c].bw * d.comp[c].bh for c in range(d.ncomp)) + 3 * W * H)
        ms = res["kernel_ms_per_launch"]
        out[name] = {"ms_per_launch": round(ms, 4), "mpix_s": round(n * W * H / ms / 1e3, 1), "algorithmic_bytes_per_launch": algo,
                     "frac": round(frac_of(algo, ms), 4), "parity": res["parity"]}
    return out


def gpu_walk_ring(ica, ctx, datas, distinct, n_g, threads, src_hash, cbytes, obytes):
    """JPEG bytes in host RAM -> pixels in HBM with the Huffman walk on the GPU (mjh_decode_batch_gpu_begin / _end): a ring of `depth`
    batches of `gchunk` pictures each on its own stream, the host threads parsing headers and removing byte stuffing for the next
    chunk while the walks of the previous ones run; the same once more with every chunk's pixels copied to pinned host memory.  Runs on
    every rank at N > 1 (its own slice, its own share of the host cores): this is what north_star's scaling question is about."""
    res = {}
    ebs, gpins = [], []
    try:
        jg = [datas[i % distinct] for i in range(n_g)]  # this leg is fast: enough chunks for the pipeline to reach its steady state (the images cycle)
        depth = max(2, int(os.environ.get("MIJ_BENCH_GPU_DEPTH", "4")))  # batches in the ring = walks in flight
        # chunks of 256 pictures, four batches: measured against 128 / 512 and three / six batches (tools/bench_gpu_walk.py)
        gchunk = max(1, min(int(os.environ.get("MIJ_BENCH_GPU_CHUNK", "256")), n_g // depth))
        # no coefficient staging to speak of: it is only needed for images the GPU walk hands back
        ebs = [ica.Batch(ctx, gchunk, cbytes * 4, cbytes * gchunk, obytes * gchunk) for _ in range(depth)]
        for eb in ebs:
            eb.entropy_reserve(sum(len(x) * 9 // 8 + 4352 for x in jg[:gchunk]))
        for eb in ebs:  # warm-up
            eb.reset()
            eb.decode_jpegs(jg[:gchunk], 3, threads, gpu_entropy=True)
            eb.submit()
            eb.wait()
        last = {}
        # begin(k) runs depth-1 chunks ahead of end(k): the walk kernels are latency bound (one chunk is ~2 workgroups
        # per CU), so several walks in flight on their own streams is what fills the GPU, and the host parses the next
        # headers meanwhile
        use_pins = []  # filled for the D2H variant below: one pinned buffer per ring batch

        def finish(side, pjob, plo, plen):
            ok, slots, reasons = ebs[side].decode_jpegs_gpu_end(pjob)
            assert ok == plen, reasons
            ebs[side].submit()
            if use_pins:
                ebs[side].fetch_all_async(use_pins[side].ptr, use_pins[side].nbytes)
            last[side] = (plo + plen - 1, slots[plen - 1])

        def one_pass():
            t0 = time.perf_counter()
            pending = []  # (side, job, first image, count) in begin order
            for k, lo in enumerate(range(0, n_g, gchunk)):
                eb = ebs[k % depth]
                eb.reset()
                part = jg[lo:lo + gchunk]
                pending.append((k % depth, eb.decode_jpegs_gpu_begin(part, 3, threads), lo, len(part)))
                if len(pending) == depth:
                    finish(*pending.pop(0))
            for item in pending:
                finish(*item)
            for eb in ebs:
                eb.wait()
            return time.perf_counter() - t0

        passes = [one_pass() for _ in range(3)]  # the leg takes ~0.1 s: three passes, in order; the first follows an idle GPU
        t_gpu = sorted(passes)[1]
        for side, (img, slot) in last.items():
            assert ebs[side].hash_out(slot) == src_hash[img % distinct], "GPU-walked image differs"
        res["value_gpu_entropy"] = round(n_g * W * H / t_gpu / 1e6, 1)
        res["gpu_entropy_seconds"] = round(t_gpu, 5)
        res["gpu_entropy_images"] = n_g
        res["gpu_entropy_host_threads"] = threads
        res["gpu_entropy_sync_rounds"] = ebs[0].entropy_rounds()
        res["gpu_entropy_chunk_images"] = gchunk
        res["gpu_entropy_batches_in_flight"] = depth
        res["gpu_entropy_passes_mpix_s"] = [round(n_g * W * H / t / 1e6, 1) for t in passes]
        # the same ring with every chunk's pixels copied to pinned host memory behind its kernels (3 B/px over PCIe: the
        # link, not the GPU, sets this figure)
        gpins.extend(ica.PinnedBuffer(obytes * gchunk) for _ in range(depth))
        use_pins.extend(gpins)
        t_gd = sorted(one_pass() for _ in range(3))[1]
        for side, (img, slot) in last.items():
            off = ebs[side].out_offset(slot)
            assert np.array_equal(gpins[side].array[off:off + W * H * 3], ebs[side].fetch(slot).reshape(-1)), "D2H copy of a GPU-walked image differs"
        res["value_gpu_entropy_with_d2h"] = round(n_g * W * H / t_gd / 1e6, 1)
        res["gpu_entropy_with_d2h_seconds"] = round(t_gd, 5)
        res["d2h_gb_s"] = round(n_g * W * H * 3 / t_gd / 1e9, 1)
    except ica.MijError as exc:
        res["value_gpu_entropy"] = None
        res["gpu_entropy_error"] = str(exc)
    finally:
        for pb in gpins:
            pb.close()
        for eb in ebs:
            eb.close()
    return res


def end_to_end(ica, ctx, datas, distinct, n_img, src_hash, cbytes, obytes, args):
    """Outside the timed region (rank 0, one GPU): bitstream in host RAM -> RGB in HBM, three ways."""
    n_e = min(args.e2e_images, n_img)
    threads = usable_cores()
    chunk = max(1, min(64, n_e // 2))
    # two batches ping-pong: while the GPU uploads and transforms chunk k (async on its own stream)
    # the host threads already walk chunk k+1 -- the "H2D / kernel overlap" of SURVEY 8(e)
    ebs = [ica.Batch(ctx, chunk, cbytes * chunk, cbytes * chunk, obytes * chunk) for _ in range(2)]
    jl = [datas[i % distinct] for i in range(n_e)]
    for eb in ebs:  # warm the pool / page in staging
        eb.decode_jpegs(jl[:chunk], 3, threads, gpu_entropy=False)
        eb.submit()
        eb.wait()
    t_host = 0.0
    t0 = time.perf_counter()
    last = {}
    for k, lo in enumerate(range(0, n_e, chunk)):
        eb = ebs[k & 1]
        eb.reset()  # waits for this batch's previous chunk
        part = jl[lo:lo + chunk]
        th = time.perf_counter()
        ok, slots, reasons = eb.decode_jpegs(part, 3, threads, gpu_entropy=False)
        t_host += time.perf_counter() - th
        assert ok == len(part), reasons
        eb.submit()
        last[k & 1] = (lo + len(part) - 1, slots[len(part) - 1])
    for eb in ebs:
        eb.wait()
    t_all = time.perf_counter() - t0
    for side, (img, slot) in last.items():
        assert ebs[side].hash_out(slot) == src_hash[img % distinct]
    e2e = {
        "value": round(n_e * W * H / t_all / 1e6, 1),
        "unit": "Mpix/s",
        "images": n_e,
        "host_threads": threads,
        "chunk_images": chunk,
        "host_stage_only_mpix_s": round(n_e * W * H / t_host / 1e6, 1),
        "includes": "Huffman walk on the host threads -> pinned staging -> H2D -> pack -> fused kernel, two batches ping-pong; pixels left in HBM",
    }
    # the same pipeline with the pixels brought back to (pinned) host memory: one asynchronous D2H of the
    # chunk's output arena queued behind its kernels, completed when the batch is reused
    pins = [ica.PinnedBuffer(obytes * chunk) for _ in range(2)]
    t0 = time.perf_counter()
    for k, lo in enumerate(range(0, n_e, chunk)):
        eb = ebs[k & 1]
        eb.reset()
        part = jl[lo:lo + chunk]
        ok, slots, reasons = eb.decode_jpegs(part, 3, threads, gpu_entropy=False)
        eb.submit()
        eb.fetch_all_async(pins[k & 1].ptr, pins[k & 1].nbytes)
        last[k & 1] = (lo + len(part) - 1, slots[len(part) - 1])
    for eb in ebs:
        eb.wait()
    t_d2h = time.perf_counter() - t0
    for side, (img, slot) in last.items():
        off = ebs[side].out_offset(slot)
        got = pins[side].array[off:off + W * H * 3]
        assert np.array_equal(got, ebs[side].fetch(slot).reshape(-1)), "D2H copy differs from the device image"
    e2e["value_with_d2h"] = round(n_e * W * H / t_d2h / 1e6, 1)
    # the Huffman walk itself on the GPU (mjh_decode_batch_gpu): the host threads only parse headers and remove byte
    # stuffing, 0.45 MB of bitstream per image crosses PCIe instead of 6.3 MB of coefficients; images the GPU walk
    # refuses are walked on the host
    for eb in ebs:
        eb.close()
    ebs = []
    e2e.update(gpu_walk_ring(ica, ctx, datas, distinct, max(4096, 8 * n_e), threads, src_hash, cbytes, obytes))
    for pb in pins:
        pb.close()
    for eb in ebs:
        eb.close()
    return e2e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10,
                    help="untimed launches first: after an idle gap the first ~10 launches run 5-30 %% slower (power management ramp, profiles/r01h trace)")
    ap.add_argument("--images", type=int, default=1024, help="images on the GPU at N = 1 (BASELINE configs[1]: 1024)")
    ap.add_argument("--total-images", type=int, default=CONFIG3_TOTAL, help="N > 1: size of the ONE logical batch sliced over the ranks (BASELINE configs[2]: 4096)")
    ap.add_argument("--distinct", type=int, default=16, help="distinct synthetic images cycled to fill the batch")
    ap.add_argument("--settle-ms", type=float, default=25.0,
                    help="the settled figure's warm-up lasts at least this long (more launches than --warmup if need be; the number "
                         "issued is reported as config.warmup_launches_issued): after an idle gap launch durations take "
                         "~25 ms to settle (power management), whatever W says.  With --full the figure with exactly --warmup launches is "
                         "reported beside it (roofline.frac_at_requested_warmup)")
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline: verification of every image against the int16 pipeline, the figure at exactly "
                         "--warmup launches, IDCT wavefront classes, host stage, the secondary legs, end to end and the CPU baseline "
                         "(the --no-* / --legs options below select among them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed (rank 0's RGB8 pixels as float32: its last image whole, "
                         "a fixed seeded sample of the others) to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-e2e", action="store_true", help="with --full: skip the (untimed-region) end-to-end measurement")
    ap.add_argument("--no-legs", action="store_true", help="with --full: skip the secondary legs (int16 planes, harsh batch, configs 4 and 5, 4:2:2)")
    ap.add_argument("--legs", default="", help="with --full: comma-separated subset of the secondary legs to run (default: all)")
    ap.add_argument("--control-plane", default=os.environ.get("MIJ_CONTROL_PLANE", "gloo"), choices=["gloo", "nccl"],
                    help="N > 1: backend of the barrier / MAX / SUM / all-gather of a few scalars.  gloo by default: the data path has no collective "
                         "(independent images), so nothing is gained by taking RCCL's bring-up into the run; nccl (= RCCL) by flag")
    ap.add_argument("--e2e-images", type=int, default=512)
    ap.add_argument("--config4-images", type=int, default=32)
    ap.add_argument("--h2v1-images", type=int, default=512)
    args = ap.parse_args()

    import torch  # device sync + launcher plumbing only
    import image_codecs_amd as ica
    from image_codecs_amd.sharding import ControlPlane, shard_range

    # MIJ_BENCH_SHARE_DEVICE=1: every rank on device 0 and the control plane over gloo -- the multi-rank path rehearsed on a one-GPU box
    share = os.environ.get("MIJ_BENCH_SHARE_DEVICE") == "1"
    cp = ControlPlane(backend="gloo" if share else args.control_plane)
    if cp.world != args.gpus:
        if cp.rank == 0:
            print("warning: --gpus %d but WORLD_SIZE=%d; using WORLD_SIZE" % (args.gpus, cp.world), file=sys.stderr)
    if torch.cuda.is_available():  # the control plane may be gloo: torch's own current device still has to be this rank's (torch.cuda.synchronize below)
        torch.cuda.set_device(0 if share else cp.local_rank)
    if cp.local_rank == 0:
        ica.build_library()  # rebuilds only when a source is newer than the in-tree .so; never from several ranks at once
    cp.barrier()
    if not ica.gpu_available():
        raise SystemExit("bench.py needs a gfx950 GPU: the decode path has no CPU fallback")
    ctx = ica.Context(0 if share else cp.local_rank)
    arch, cus, mem = ctx.info()

    # ---- the logical batch and this rank's slice of it
    total = args.images if cp.world == 1 else args.total_images
    lo, hi = shard_range(total, cp.rank, cp.world)
    n_img = hi - lo
    distinct = max(1, min(args.distinct, max(1, n_img)))
    datas = [ica.synth_jpeg(W, H, seed=s, quality=90) for s in range(distinct)]
    d0 = ica.HostDecoder.probe(datas[0], 3)
    cbytes, obytes = ica.Batch.coef_bytes(d0), ica.Batch.out_bytes(d0)

    # ---- --full: reference pixels of the distinct images: host walk -> int16 planes -> fused kernel
    src_hash, host_stage_s = None, None
    if args.full:
        ref_batch, _, host_stage_s = resident_batch(ica, ctx, datas, 0, distinct, "int16", cbytes, obytes)
        ref_batch.launch()
        ref_batch.wait()
        assert {ref_batch.slot_path(s) for s in range(distinct)} == {1}, "the fused kernel did not take the batch"
        src_hash = [ref_batch.hash_out(s) for s in range(distinct)]
        ref_batch.close()

    # ---- the timed batch: this rank's slice, default plane format (with --full: every image verified)
    batch, owners, _ = resident_batch(ica, ctx, datas, lo, n_img, "compact", cbytes, obytes)
    batch.launch()
    batch.wait()
    paths = {batch.slot_path(s) for s in range(n_img)}
    assert paths == {1}, "the fused kernel did not take the batch: %r" % paths
    assert all(batch.slot_coef_bytes(s) == 1 for s in range(min(n_img, 32))), "the batch is not in the default (compact) plane format"
    n_verified = verify_batch(batch, owners, src_hash) if args.full else -1

    # ---- (a) --full: exactly --warmup untimed launches, then exactly --steps timed ones: the figure at the requested warm-up
    ms_requested = -1.0
    if args.full:
        cp.barrier()
        for _ in range(max(0, args.warmup)):
            batch.launch()
        batch.wait()
        ms_requested = timed_launches(batch, args.steps)

    # ---- (b) the settled figure: a warm-up of at least --settle-ms directly in front of the timed region;
    # timed region: exactly K steps, barrier + device sync on both sides
    n_warm = warm(batch, args.warmup, args.settle_ms)
    cp.barrier()
    torch.cuda.synchronize() if torch.cuda.is_available() else None
    batch.wait()
    t_begin = time.perf_counter()
    batch.timer_begin()
    for _ in range(args.steps):
        batch.launch()
    batch.timer_end()
    batch.wait()
    torch.cuda.synchronize() if torch.cuda.is_available() else None
    t_local = time.perf_counter() - t_begin
    kernel_ms = batch.timer_ms() / args.steps  # HIP events on the batch's own stream
    cp.barrier()
    t_max = cp.max(t_local)
    total_px = cp.sum(float(n_img) * W * H * args.steps)
    kernel_ms_max = cp.max(kernel_ms)
    ms_requested_max = cp.max(ms_requested)
    per_rank = cp.gather_floats([float(cp.rank), float(lo), float(hi), kernel_ms, ms_requested, float(n_verified)])
    dumped = dump_outputs(batch, n_img, args.dump_outputs) if (args.dump_outputs and cp.rank == 0) else None

    main_classes = idct_classes(batch) if (args.full and cp.rank == 0) else None
    solo = args.full and cp.rank == 0 and cp.world == 1
    gpu_px = [batch.fetch(next(s for s, (kk, src) in enumerate(owners) if kk == k and src is None)) for k in range(distinct)] \
        if (args.full and cp.rank == 0 and not args.no_cpu_baseline) else None
    # release the timed batch before the legs: 12.8 GB and, more to the point, its stream (a process gets 4 hardware
    # queues; a fifth stream would share one with a batch of the end-to-end ring below and serialise the two)
    batch.close()
    batch = None

    # ---- outside the timed region, one GPU only: the legs.  A failure is reported inside the line.
    legs, e2e = {}, None

    def run_leg(name, fn):
        if args.legs and name not in args.legs.split(","):
            return
        t0 = time.time()
        try:
            legs[name] = fn()
        except Exception as exc:  # noqa: BLE001
            legs[name] = {"error": "%s: %s" % (type(exc).__name__, exc)}
        legs[name]["leg_s"] = round(time.time() - t0, 1)

    if solo and not args.no_legs:
        checker = cpu_checker()

        def int16_leg():
            res, _ = leg_decode_1080p(ica, ctx, datas, n_img, "int16", cbytes, obytes, args, src_hash=src_hash)
            ms = res["kernel_ms_per_launch"]
            res.pop("escaped_blocks_in_sources", None)
            res.update({"kernel": "mij::k_fused420<3,false,false>", "frac": round(frac_of(ALGO_BYTES_PER_IMAGE * n_img, ms), 4),
                        "achieved": round(ALGO_BYTES_PER_IMAGE * n_img / (ms * 1e-3) / 1e9, 1), "unit": "GB/s",
                        "note": "the same images as int16 tile-layout planes (mij_batch_set_coef_format): 6 266 880 B of coefficients per image actually read"})
            add_traffic(res, "k_fused420_int16_%d" % n_img)
            return res

        def harsh_leg():
            hd = [ica.stbi_write_jpg_to_memory(ica.synth_rgb_edges(W, H, seed=s), 90) for s in range(distinct)]
            res, fmt = leg_decode_1080p(ica, ctx, hd, n_img, "compact", cbytes, obytes, args, checker=checker)
            ms = res["kernel_ms_per_launch"]
            res.update({"workload": "%d x 1920x1080 4:2:0 q=90 of synth_rgb_edges(seed 0..%d): noise & 63 + 24 inverted rectangles per image, %.2f bit/px"
                                    % (n_img, distinct - 1, sum(len(x) for x in hd) * 8.0 / (distinct * W * H)),
                        "kernel": "mij::k_fused420<3,false,true>", "coefficient_planes": "compact" if fmt else "int16",
                        "escaped_blocks_pct": round(100.0 * res.pop("escaped_blocks_in_sources") / (distinct * 48960), 3), "host_walk_fallbacks": 0,
                        "frac": round(frac_of(ALGO_BYTES_PER_IMAGE * n_img, ms), 4), "parity_against": checker[1]})
            add_traffic(res, "k_fused420_compact_harsh_%d" % n_img)
            return res

        run_leg("prepass", lambda: leg_prepass(ica, ctx, datas, n_img, cbytes, obytes, kernel_ms_max))
        run_leg("int16_planes", int16_leg)
        run_leg("harsh_batch", harsh_leg)
        run_leg("config4", lambda: leg_config4(ica, ctx, args, checker))
        run_leg("config5", lambda: leg_config5(ica, ctx, args, checker))
        run_leg("config5_q95_444", lambda: leg_config5(ica, ctx, args, checker, quality=95, count=512))
        run_leg("h2v1", lambda: leg_h2v1(ica, ctx, args, checker))
        run_leg("wide_420", lambda: leg_wide420(ica, ctx, args, checker))
        run_leg("two_pass", lambda: leg_two_pass(ica, ctx, datas, args, checker))
        run_leg("config1", lambda: leg_config1(ica, checker))
    if solo and not args.no_e2e:
        try:
            e2e = end_to_end(ica, ctx, datas, distinct, n_img, src_hash, cbytes, obytes, args)
        except Exception as exc:  # noqa: BLE001
            e2e = {"value": None, "error": "%s: %s" % (type(exc).__name__, exc)}

    # ---- N > 1: what north_star's scaling question is really about -- host threads and PCIe per GPU feeding N walks at once.  Every rank
    # runs the GPU-walk ring on its own slice with its share of the host cores, all ranks at the same time (barrier in front); the line
    # carries per-rank and aggregate end-to-end rates, pixels left in HBM and copied to pinned host memory.
    e2e_ranks = None
    if args.full and cp.world > 1 and not args.no_e2e:
        local_world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", str(cp.world))))
        threads = max(1, usable_cores() // local_world)
        n_ring = max(1024, 2 * n_img)
        cp.barrier()
        try:
            ring = gpu_walk_ring(ica, ctx, datas, distinct, n_ring, threads, src_hash, cbytes, obytes)
        except Exception as exc:  # noqa: BLE001
            ring = {"value_gpu_entropy": None, "gpu_entropy_error": "%s: %s" % (type(exc).__name__, exc)}
        ok = ring.get("value_gpu_entropy") is not None
        e2e_ranks = cp.gather_floats([float(cp.rank), float(n_ring if ok else 0), float(threads), ring.get("gpu_entropy_seconds", 0.0) if ok else 0.0,
                                      ring.get("gpu_entropy_with_d2h_seconds", 0.0) if ok else 0.0])
        cp.barrier()

    out = None
    if cp.rank == 0:
        algo_launch = ALGO_BYTES_PER_IMAGE * n_img  # rank 0's launch (it owns a largest slice)
        achieved = algo_launch / (kernel_ms_max * 1e-3) / 1e9
        ranks = [{"rank": int(r[0]), "images": [int(r[1]), int(r[2])], "kernel_ms_per_launch": round(r[3], 4),
                  "frac": round(frac_of(ALGO_BYTES_PER_IMAGE * (int(r[2]) - int(r[1])), r[3]), 4) if r[3] > 0 else None,
                  "kernel_mpix_s": round((int(r[2]) - int(r[1])) * W * H / r[3] / 1e3, 1) if r[3] > 0 else None,
                  "kernel_ms_at_requested_warmup": round(r[4], 4) if r[4] >= 0 else None,
                  "images_verified": int(r[5]) if r[5] >= 0 else None} for r in per_rank]
        roof = {
            "bound": "hbm",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "kernel": "mij::k_fused420<3,false,true>",
            "kernel_ms_per_launch": round(kernel_ms_max, 4),
            "algorithmic_bytes_per_launch": algo_launch,
            "frac_at_requested_warmup": round(frac_of(algo_launch, ms_requested_max), 4) if args.full else None,
            "kernel_ms_at_requested_warmup": round(ms_requested_max, 4) if args.full else None,
            "note": "frac = algorithmic bytes (int16 coefficients + RGB8, SURVEY 8d) / time / 8 TB/s; hbm_counter_frac = bytes the TCC counters saw / "
                    "time / 8 TB/s (fewer: compact planes); at this point the kernel is bound by VALU issue, not by HBM (DESIGN.md 3.1)",
        }
        add_traffic(roof, "k_fused420_compact_%d" % n_img)
        roof["idct_wavefront_classes"] = main_classes
        out = {
            "metric": "JPEG decode Mpixels/sec, 4:2:0 1080p batch, 1/2/4/8 GPU + %HBM roofline",  # BASELINE.json's string
            "value": round(total_px / t_max / 1e6, 1),
            "unit": "Mpix/s",
            "n_gpus": cp.world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(t_max / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak" if cp.world == 1 else "strong",
            "vs_baseline": None,
            "dtype": "int32 (u8/int16 in, u8 out)",
            "data": "synthetic",
            "config": {
                "workload": (("%d x 1920x1080 baseline 4:2:0 q=90 JPEGs (BASELINE configs[1]) on 1 GPU" % total) if cp.world == 1 else
                             ("ONE batch of %d x 1920x1080 baseline 4:2:0 q=90 JPEGs (BASELINE configs[2]) cut into %d contiguous slices, one per GPU" % (total, cp.world)))
                            + ", coefficients resident in HBM, fused dequant+IDCT+h2v2+YCbCr->RGB8",
                "total_images": total,
                "slices": [r["images"] for r in ranks],
                "distinct_images": distinct,
                "sharding": "independent images, contiguous slices (sharding.shard_range), one process + one HIP stream per GPU, no collective on the data path",
                "coefficient_planes": "compact (library default): low bytes + escape bytes + int16 DC array, written in that form by the host walk itself "
                                      "(mjh_decode_memory_fmt; no pack pass on the device: legs.prepass)",
                "images_verified_per_rank": [r["images_verified"] for r in ranks],
                "warmup_launches_issued": n_warm,
                "settle_ms": args.settle_ms,
                "device": arch,
                "compute_units": cus,
                "note_scaling": None if cp.world == 1 else
                                "total work is fixed at %d images for every N > 1 (strong); the N = 1 line is BASELINE configs[1], 1024 images" % total,
            },
            "roofline": roof,
            "per_rank": ranks,
        }
        out["config"]["full"] = args.full
        if dumped is not None:
            out["config"]["dumped_outputs"] = dumped
        if host_stage_s is not None:
            out["host_stage"] = {
                "huffman_walk_mpix_s_single_thread": round(distinct * W * H / host_stage_s / 1e6, 1),
                "note": "host entropy stage, 1 thread, writing pinned staging; outside the timed region",
            }
        if legs:
            out["legs"] = legs
        if e2e is not None:
            out["end_to_end"] = e2e
        if e2e_ranks is not None:
            rows = [{"rank": int(r[0]), "images": int(r[1]), "host_threads": int(r[2]),
                     "mpix_s": round(r[1] * W * H / r[3] / 1e6, 1) if r[3] > 0 else None,
                     "mpix_s_with_d2h": round(r[1] * W * H / r[4] / 1e6, 1) if r[4] > 0 else None} for r in e2e_ranks]
            good = [r for r in e2e_ranks if r[3] > 0 and r[4] > 0]
            out["end_to_end"] = {
                "unit": "Mpix/s",
                "includes": "every rank at the same time: JPEG bytes in host RAM -> header parse + byte unstuffing on the rank's host threads -> H2D of the "
                            "streams -> Huffman walk on the GPU -> fused kernel; ring of four 256-picture batches per rank; pixels left in HBM / copied to pinned host memory",
                "value_gpu_entropy": round(sum(r[1] for r in good) * W * H / max(r[3] for r in good) / 1e6, 1) if good else None,
                "value_gpu_entropy_with_d2h": round(sum(r[1] for r in good) * W * H / max(r[4] for r in good) / 1e6, 1) if good else None,
                "ranks_ok": len(good), "per_rank": rows,
            }
        if args.full and cp.rank == 0 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(datas, gpu_pixels=lambda i: gpu_px[i])
            except Exception as exc:  # noqa: BLE001
                out["cpu_baseline"] = {"value": None, "error": "%s: %s" % (type(exc).__name__, exc)}
    ctx.close()
    cp.barrier()  # rank 0 may still have been timing the CPU baseline
    cp.close()
    if out is not None:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
