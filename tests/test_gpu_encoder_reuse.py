"""One encoder over several uploads (mij_enc_reset, mij_enc_upload, mij_enc_launch): every list the upload fills is kept from batch to batch
and reallocated when a batch outgrows it, which no test of a single feature sees.  A first batch with one slot of every kind, a second one
large enough to reallocate every list (the growth rule is need + need / 2 + 64), the first one again in lists larger than it needs, and
two more slots added to it without a reset: after each launch every stream is the host writer's byte for byte, and the slots report the
options they were given."""
import functools

import numpy as np
import pytest
import torch

import denorm_model as dm
import planes_cases as pc
import sampling_cases as sc

pytestmark = pytest.mark.gpu

Q, RI = 90, 2
ARENA = 4 << 20
FLOATS = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
PLANES = ("planes_host_420", "planes_dev_420", "planes_host_grey", "planes_dev_grey")
KINDS = ("host", "dev_u8") + tuple(FLOATS) + PLANES + ("s422", "units", "coef", "coef_rq")
OPTIONS = (None, "optimize", "progressive", "restart")
SOURCES = ((48, 32, 5), (16, 16, 6), (8, 8, 7))  # the pictures of the decode batch: (w, h, seed)


def floats(kind, w, h, seed):
    """normalised floats of the slot's dtype, HWC, on the CPU"""
    v = np.random.default_rng(seed).uniform(-0.3, 1.3, size=(h, w, 3))
    return torch.from_numpy(((v - np.array(dm.IM_MEAN)) / np.array(dm.IM_STD)).astype(np.float32)).to(FLOATS[kind])


def source(ica, w, h, seed):
    """a baseline 4:2:0 file: what the decode batch holds"""
    return ica.emit_jpeg(*ica.host_transform(sc.picture(w, h, 3, seed), Q))


def coarser(ica):
    return tuple(tuple(int(v) for v in t) for t in ica.quality_tables(50))


@functools.lru_cache(maxsize=None)
def want(ica, kind, w, h, seed, option):
    """the host writer's stream for a slot of this kind, picture and option"""
    kw = {"optimize": option == "optimize", "restart_mcus": RI if option == "restart" else None, "progressive": option == "progressive"}
    if kind in ("host", "dev_u8", "units"):
        return ica.emit_jpeg(*ica.host_transform(sc.picture(w, h, 3, seed), Q), **kw)
    if kind in FLOATS:
        scale, bias = dm.scale_bias(3, dm.IM_MEAN, dm.IM_STD)
        return ica.emit_jpeg(*ica.host_transform(dm.picture(dm.widen(floats(kind, w, h, seed)), scale, bias), Q), **kw)
    if kind in PLANES:
        name = kind.rsplit("_", 1)[1]
        return ica.write_jpg_planes_to_memory(pc.arg(pc.planes(w, h, name, seed)), name, Q, **kw)
    if kind == "s422":
        return ica.write_jpg_sampled_to_memory(sc.picture(w, h, 3, seed), Q, "422", **kw)
    data, why = ica.transcode_memory(source(ica, w, h, seed), tables=coarser(ica) if kind == "coef_rq" else None, **kw)
    assert data is not None, why
    return data


def add(ica, enc, batch, keep, kind, w, h, seed):
    """one slot of `kind`; device memory it reads goes into keep"""
    if kind == "host":
        return enc.add(sc.picture(w, h, 3, seed), Q)
    if kind == "dev_u8":
        t = torch.from_numpy(sc.picture(w, h, 3, seed)).cuda()
        keep.append(t)
        return enc.add_device(ica.InTensor(t.data_ptr(), ica.MIJ_LAYOUT_HWC, w, h, 3, t.stride(0), 0), Q)
    if kind in FLOATS:
        t = floats(kind, w, h, seed).cuda()
        keep.append(t)
        scale, bias = dm.scale_bias(3, dm.IM_MEAN, dm.IM_STD)
        cv = ica.InConvert({"f16": ica.MIJ_DT_F16, "bf16": ica.MIJ_DT_BF16, "f32": ica.MIJ_DT_F32}[kind], scale, bias)
        return enc.add_device_float(ica.InTensor(t.data_ptr(), ica.MIJ_LAYOUT_HWC, w, h, 3, t.stride(0), 0), cv, Q)
    if kind in PLANES:
        name = kind.rsplit("_", 1)[1]
        pl = pc.planes(w, h, name, seed)
        if "host" in kind:
            return enc.add_planes(pc.arg(pl), name, Q)
        d = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pl]
        keep.append(d)
        return enc.add_device_planes([(t.data_ptr(), t.stride(0) if t.shape[0] > 1 else 0, t.stride(1) if t.shape[1] > 1 else 1) for t in d], w, h, name, Q)
    if kind == "s422":
        return enc.add(sc.picture(w, h, 3, seed), Q, sampling="422")
    if kind == "units":
        return enc.add_units(w, h, 3, Q, ica.host_transform(sc.picture(w, h, 3, seed), Q)[1])
    slot = enc.add_coef(batch, SOURCES.index((w, h, seed)), tables=coarser(ica) if kind == "coef_rq" else None)
    assert enc.slot_requantized(slot) == (kind == "coef_rq")
    return slot


def tiles(enc, slot, option, stream):
    """the emission tiles of a slot whose scans have at most 128 units (a tile's length): one per restart interval, one per scan"""
    if option == "progressive":
        return stream.count(b"\xff\xda")
    p = enc.plan(slot)
    return -(-p.mcu_x * p.mcu_y // RI) if option == "restart" else 1


class Counts(dict):
    def note(self, kind, option, ntiles):
        for key, n in (("slots", 1), ("tiles", ntiles), (kind, 1), (option, 1), ("%s tiles" % option, ntiles)):
            self[key] = self.get(key, 0) + n


def fill(ica, enc, batch, specs):
    """adds (kind, w, h, seed, option) slots, a clone of the first plain host slot behind them -> ([(slot, stream, option)], keep, Counts)"""
    slots, keep, counts = [], [], Counts()
    for kind, w, h, seed, option in specs:
        s = add(ica, enc, batch, keep, kind, w, h, seed)
        if option == "optimize":
            enc.set_optimize(s)
        elif option == "progressive":
            enc.set_progressive(s)
        elif option == "restart":
            enc.set_restart(s, RI)
        slots.append((s, want(ica, kind, w, h, seed, option), option))
        counts.note("coef" if kind == "coef_rq" else "float" if kind in FLOATS else "planes_dev" if kind.startswith("planes_dev") else kind, option,
                    tiles(enc, s, option, slots[-1][1]))
        if kind == "coef_rq":
            counts["requant"] = counts.get("requant", 0) + 1
    root = next(k for k, sp in enumerate(specs) if sp[0] == "host" and sp[4] is None)
    slots.append((enc.add_clone(slots[root][0]), slots[root][1], None))
    counts.note("clone", None, 1)
    return slots, keep, counts


def run(enc, slots):
    torch.cuda.synchronize()  # the device pictures are in place
    enc.upload()
    enc.launch()
    assert enc.fetch_streams() == len(slots)
    for s, stream, option in slots:
        got, n = enc.stream(s)
        assert enc.slot_status(s) == "ok" and got is not None and bytes(got) == stream, (s, option, n, len(stream))
        assert enc.slot_optimized(s) == (option == "optimize"), s
        assert enc.slot_restart(s) == (RI if option == "restart" else 0), s
        assert enc.slot_progressive(s) == (option == "progressive"), s


def batch_a():
    """one slot of every kind, pictures of mixed sizes up to 48 x 32; one slot each optimised, progressive and with a restart interval"""
    sizes = ((48, 32), (33, 17), (17, 9), (40, 24), (16, 16))
    option = {"dev_u8": "optimize", "planes_dev_420": "progressive", "s422": "restart"}
    return [(kind,) + (SOURCES[0] if kind.startswith("coef") else sizes[k % len(sizes)] + (k,)) + (option.get(kind),) for k, kind in enumerate(KINDS)]


def batch_b(n_each=70):
    """every kind n_each times at 8 x 8 and 16 x 16, the options taking turns: 3 * n_each float and 2 * n_each device plane slots, and of
    the 13 * n_each slots a quarter each optimised, progressive and with a restart interval"""
    out = []
    for r in range(n_each):
        for k, kind in enumerate(KINDS):
            i = len(out)
            size = SOURCES[1 + i % 2] if kind.startswith("coef") else ((16, 16), (8, 8))[i % 2] + (i % 5,)
            out.append((kind,) + size + (OPTIONS[(r + k) % 4],))
    return out


def test_lists_are_reused_grown_and_reused_again(ica, gpu_ctx):
    srcs = [source(ica, *s) for s in SOURCES]
    batch = ica.Batch(gpu_ctx, len(srcs), ARENA, ARENA, ARENA)
    enc = ica.Encoder(gpu_ctx, 1024, ARENA, ARENA)
    try:
        ok, sl, why = batch.decode_jpegs(srcs, 0, threads=2, gpu_entropy=False)
        assert ok == len(srcs) and list(sl) == list(range(len(srcs))), why
        batch.upload()
        enc.stream_reserve(ARENA)

        slots, keep, a = fill(ica, enc, batch, batch_a())
        assert {k: a[k] for k in ("host", "dev_u8", "float", "planes_host_420", "planes_host_grey", "planes_dev", "s422", "units", "coef", "requant",
                                  "clone", "optimize", "progressive", "restart")} == {
            "host": 1, "dev_u8": 1, "float": 3, "planes_host_420": 1, "planes_host_grey": 1, "planes_dev": 2, "s422": 1, "units": 1, "coef": 2,
            "requant": 1, "clone": 1, "optimize": 1, "progressive": 1, "restart": 1}
        run(enc, slots)

        enc.reset()
        slots, keep, b = fill(ica, enc, batch, batch_b())
        for key in ("slots", "tiles", "optimize", "optimize tiles", "progressive", "progressive tiles", "dev_u8", "float", "planes_dev", "coef", "requant"):
            assert b[key] > a[key] + a[key] // 2 + 64, (key, a[key], b[key])  # the list reallocates
        run(enc, slots)

        enc.reset()
        slots, keep, again = fill(ica, enc, batch, batch_a())
        assert again == a
        run(enc, slots)

        more = [("f32", 17, 9, 40, "optimize"), ("coef", ) + SOURCES[2] + ("progressive",)]
        for kind, w, h, seed, option in more:  # no reset: the batch is uploaded and launched again with two more slots
            s = add(ica, enc, batch, keep, kind, w, h, seed)
            (enc.set_optimize if option == "optimize" else enc.set_progressive)(s)
            slots.append((s, want(ica, kind, w, h, seed, option), option))
        run(enc, slots)
        batch.wait()
    finally:
        enc.close()
        batch.close()
    second = ica.Encoder(gpu_ctx, 4, 1 << 20, 1 << 20)  # the context outlives an encoder and takes another
    second.close()
