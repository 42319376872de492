"""Slots behind byte 2^32 of a batch's and of an encoder's device arenas (test_gpu_far_slots.py; DESIGN.md 5, "Slots past 4 GiB").

Every device descriptor carries a 64-bit arena offset next to 32-bit offsets inside the picture; one narrowing cast where the two meet
shows only in a slot that lies at or behind byte 2^32 of its arena, and no other test puts one there.  FarBatch builds a batch whose first
slots are spacers -- one 2048 x 2048 picture of the layout that suits the channel count, decoded once and cloned, so that pinned staging
stays at one picture -- then one trimming picture (grey, 256 pixels wide: 256 bytes a row) that ends a chosen number of bytes short of the
line, then the pictures under test.  The first of those straddles the line of the output arena, the others lie behind it; the coefficient
arena, whose slots are larger, is crossed inside a spacer, so every picture under test has its planes behind the line as well.

The spacers are decoded like any slot.  A store whose offset lost its upper half lands at `off mod 2^32`, which is inside a spacer: the
source spacer and the trimming picture are compared with the CPU decode after the launch under test, every clone with the source
(mij_batch_diff_slots).  The premises are asserted from the public size functions (mij_batch_out_offset; the running sum of
mij_image_coef_bytes, which is what the batch's add does), never assumed.  FarEncoder, below, does the same for the encoder."""
import numpy as np
import pytest

import roi_cases as RC

LINE = 1 << 32
MB = 1 << 20
SPACER_SIZE = (2048, 2048)
# the spacer per output channel count: its coefficient region (8320 bytes per 64 blocks, whatever the plane format) is larger than its pixels,
# so the coefficient arena crosses the line in front of the output arena
SPACER_LAYOUT = {1: "grey", 3: "420", 4: "444"}


def align(v, a=256):
    return -(-v // a) * a


def spacer(req):
    return RC.dense(SPACER_LAYOUT[req], SPACER_SIZE, seed=9)


def trim_case(rows):
    """a grey picture of 256 x rows pixels: rows * 256 output bytes asked for with one channel"""
    return RC.dense("grey", (256, rows), seed=11)


class FarBatch:
    """b: the batch; slots: the slots of the pictures under test, in the order given; first: the straddling one.
    items: [(stream, req_comp)] of the pictures under test, the first more than 4096 output bytes large.
    producer: "host" (the host walk stages the batch's format), "int16" (int16 staging whatever the format: a compact batch packs it on
    the device) or "walk" (mij_batch_add_stream: the GPU Huffman walk writes the planes)."""

    def __init__(self, ica, ctx, oracle, req, fmt, items, producer="host", force_generic=0, stream_bytes=0, spacer_layout=None):
        self.ica, self.oracle, self.req, self.producer = ica, oracle, req, producer
        self.sp = spacer(req) if spacer_layout is None else RC.dense(spacer_layout, SPACER_SIZE, seed=9)
        sp_desc = ica.HostDecoder.probe(self.sp.stream(), req)
        s_out, s_coef = ica.Batch.out_bytes(sp_desc), ica.Batch.coef_bytes(sp_desc)
        descs = [ica.HostDecoder.probe(d, r) for d, r in items]
        first_out = ica.Batch.out_bytes(descs[0])
        # the straddling slot begins `back` bytes in front of the line: a multiple of 2048, so that the trimming picture has whole block rows
        # (its scratch planes on the two-pass path are then exactly as large as its pixels)
        back = align(first_out // 2, 2048)
        assert back < first_out, "the first picture under test has to hold more than 4096 output bytes to straddle"
        self.n_spacers = (LINE - back) // s_out
        gap = LINE - back - self.n_spacers * s_out
        assert gap % 2048 == 0 and gap // 256 <= 65535
        self.trim = trim_case(gap // 256) if gap else None
        t_desc = ica.HostDecoder.probe(self.trim.stream(), 1) if gap else None
        assert not gap or ica.Batch.out_bytes(t_desc) == gap
        out_cap = LINE - back + sum(ica.Batch.out_bytes(d) for d in descs) + 4096
        coef_cap = self.n_spacers * s_coef + (ica.Batch.coef_bytes(t_desc) if gap else 0) + sum(ica.Batch.coef_bytes(d) for d in descs) + MB
        stage = s_coef + (ica.Batch.coef_bytes(t_desc) if gap else 0) + sum(ica.Batch.coef_bytes(d) for d in descs) + MB
        assert stage < 200 * MB, "pinned host memory stays small: clones share their source's staging"
        assert coef_cap > LINE and out_cap > LINE and coef_cap + out_cap < (24 << 30)
        self.out_cap = out_cap
        # the probed descriptors by slot, for the premises: spacers, the trimming picture, the pictures under test
        self.descs = [sp_desc] * self.n_spacers + ([t_desc] if gap else []) + descs
        try:
            b = ica.Batch(ctx, self.n_spacers + 1 + len(items), stage, coef_cap, out_cap)
        except ica.MijError as e:  # the one reason a far test may skip for: the device cannot hold the arenas themselves
            if "out of memory" in str(e).lower():
                pytest.skip("MIJ_E_NOMEM creating %d + %d arena bytes: %s" % (coef_cap, out_cap, e))
            raise
        self.b = b
        try:
            b.set_coef_format(fmt)
            if producer == "walk":
                b.entropy_reserve(stream_bytes or 16 * MB)
            if force_generic:
                b.force_generic(force_generic)
            src = b.add_jpeg(self.sp.stream(), req)
            assert src == 0
            for _ in range(self.n_spacers - 1):
                b.add_clone(0)
            self.trim_slot = b.add_jpeg(self.trim.stream(), 1) if gap else -1
            self.slots = []
            for d, r in items:
                if producer == "walk":
                    st, sl = b.add_jpeg_stream(d, r)
                    assert st == 1, b.last_reason
                else:
                    sl = b.add_jpeg(d, r, stage="int16" if producer == "int16" else None)
                self.slots.append(sl)
            self.first = self.slots[0]
            assert self.slots == list(range(len(self.descs) - len(items), len(self.descs))), "self.descs is indexed by slot"
            self.premise()
        except BaseException:
            b.close()
            raise

    # ---- the premises
    def coef_offset(self, slot):
        """where the slot's region of the coefficient arena begins: the running sum of mij_image_coef_bytes of the slots in front"""
        return sum(self.ica.Batch.coef_bytes(self.descs[s]) for s in range(slot))

    def premise(self):
        b, ica = self.b, self.ica
        off, nb = b.out_offset(self.first), ica.Batch.out_bytes(self.descs[self.first])
        assert off < LINE < off + nb, ("the first slot under test does not straddle 2^32 of the output arena", off, nb)
        run = self.coef_offset(self.first)
        for sl in self.slots:
            assert sl == self.first or b.out_offset(sl) >= LINE, ("output offset", sl, b.out_offset(sl))
            assert run >= LINE, ("coefficient offset", sl, run)
            run += ica.Batch.coef_bytes(self.descs[sl])
        # the coefficient arena is crossed inside a spacer, which the clone comparison covers
        s_coef = ica.Batch.coef_bytes(self.descs[0])
        k = LINE // s_coef
        assert 0 < k < self.n_spacers and k * s_coef < LINE < (k + 1) * s_coef, ("no spacer straddles 2^32 of the coefficient arena", k)
        self.coef_straddler = k

    def plane_offset(self, slot):
        """two-pass path: where the slot's scratch planes begin, relative to the launch's arena: the sum over the slots in front of
        bw * 8 * bh * 8 per component, each rounded up to 256 (every slot of a batch under force_generic takes the two-pass path)"""
        total = 0
        for s in range(slot):
            d = self.descs[s]
            total += sum(align(d.comp[c].bw * 8 * d.comp[c].bh * 8) for c in range(d.ncomp))
        return total

    # ---- paint, launch, read back: the far region only
    def run(self, seed=41):
        """upload, paint from the straddling slot to the arena's end, launch; -> self (got / pat hold that region)"""
        b = self.b
        if self.producer == "walk":
            handed_back = b.entropy_run()
            assert handed_back == [], ("the GPU walk handed streams back to the host", handed_back)
        b.upload()
        b.wait()
        self.base = b.out_offset(self.first)
        assert b.out_total_bytes() + 4096 == self.out_cap
        n = self.out_cap - self.base
        self.pat = RC.paint(self.ica, b, self.first, n, seed)
        b.launch()
        b.wait()
        self.got = RC.read_back(self.ica, b, self.first, (n,))
        return self

    def picture(self, slot, shape):
        """the slot's bytes as read back, and a check that the bytes behind it, up to its 256-byte rounding, are still paint"""
        off = self.b.out_offset(slot) - self.base
        nb = int(np.prod(shape))
        end = align(nb)
        assert np.array_equal(self.got[off + nb:off + end], self.pat[off + nb:off + end]), ("bytes behind the picture were written", slot)
        return self.got[off:off + nb].reshape(shape)

    def check_tail(self):
        """the arena behind the last slot is still paint"""
        used = self.b.out_total_bytes() - self.base
        assert np.array_equal(self.got[used:], self.pat[used:]), "bytes behind the last slot were written"

    def check_spacers(self):
        """the source spacer and the trimming picture against the CPU decode, every clone against the source"""
        b = self.b
        want = RC.want(self.oracle, self.sp, self.req)
        got = b.fetch(0)
        assert np.array_equal(got.reshape(want.shape), want), ("the source spacer differs from the CPU decode", int((got.reshape(want.shape) != want).sum()))
        if self.trim is not None:
            tw = RC.want(self.oracle, self.trim, 1)
            tg = b.fetch(self.trim_slot)
            assert np.array_equal(tg.reshape(tw.shape), tw), "the trimming picture in front of the line differs from the CPU decode"
        bad = b.diff_slots([(0, k) for k in range(1, self.n_spacers)])
        assert bad == 0, ("spacers differ from their source: a store landed in them", bad)

    def close(self):
        self.b.close()


# ------------------------------------------------------------------ the encoder's pixel and unit arenas

ENC_SPACER = (2048, 2048)  # flat, quality 90 (4:2:0): 16384 MCUs of 768 pixel bytes and 6 * 128 unit bytes, 12 582 912 bytes a slot in both arenas
ENC_TRIM_W = 256           # the trimming picture: 16 MCU columns, so 12288 bytes of either arena per MCU row
ENC_BACK = 4096            # the first slot under test begins this many bytes in front of the line of both arenas
ENC_Q = 90


def _flat(w, h):
    a = np.empty((h, w, 3), np.uint8)
    a[:] = (90, 140, 200)
    return a


_enc_want = {}


def _enc_expected(ica, key, w, h):
    """units and stream of a flat picture from the host writer: once, shared, never changed"""
    if key not in _enc_want:
        plan, du = ica.host_transform(_flat(w, h), ENC_Q)
        du.setflags(write=False)
        _enc_want[key] = (du, ica.emit_jpeg(plan, du))
    return _enc_want[key]


class FarEncoder:
    """enc: an Encoder whose first slots are spacers -- one flat 2048 x 2048 host picture and clones of it (their streams stay at some
    tens of KB, so the emission arena and its pinned mirror stay small), then one flat trimming picture -- that end ENC_BACK bytes in
    front of byte 2^32 of the pixel arena AND of the unit arena: at quality 90 a picture of whole MCUs takes the same number of bytes in
    both.  The slots under test are added through the add_* methods below, which keep the running sums of mij_enc_pixel_bytes and of
    the plan's units (128 bytes each, rounded to 256: what the encoder's add does; slots of given units or coefficient planes take no
    pixels); premise() asserts that the first of them straddles the line of every arena it uses and the others lie behind it.

    A store whose offset lost its upper half lands in the first spacers: check_spacers compares every spacer's stream with the host
    writer's (the stream is a function of all of a slot's units) and the units of five of them, the first two among them."""

    def __init__(self, ica, ctx, max_items, force_generic=False, extra=64 * MB, stream_bytes=64 * MB):
        import ctypes as C
        self.ica = ica
        L = ica.lib()
        L.mij_enc_pixel_bytes.restype = C.c_size_t
        L.mij_enc_pixel_bytes.argtypes = [C.c_int] * 4
        self._pixel_bytes = L.mij_enc_pixel_bytes
        w, h = ENC_SPACER
        s_pix = self.pixel_bytes(w, h, 3, ENC_Q)
        plan, _ = ica.host_transform(np.zeros((16, 16, 3), np.uint8), ENC_Q)
        assert plan.subsample and plan.du_per_mcu == 6
        s_du = align((w // 16) * (h // 16) * 6 * 128)
        assert s_pix == s_du == 12582912
        self.n_spacers = (LINE - ENC_BACK) // s_pix
        gap = LINE - ENC_BACK - self.n_spacers * s_pix
        row = self.pixel_bytes(ENC_TRIM_W, 16, 3, ENC_Q)
        assert row == 12288 and gap % row == 0 and gap > 0
        self.trim_h = gap // row * 16
        assert self.pixel_bytes(ENC_TRIM_W, self.trim_h, 3, ENC_Q) == gap
        stage = s_pix + gap + 16 * MB
        assert stage + stream_bytes < 200 * MB, "pinned host memory stays small: clones share their source's staging"
        self.pix_cap = self.du_cap = LINE + extra
        try:
            enc = ica.Encoder(ctx, self.n_spacers + 1 + max_items, self.pix_cap, self.du_cap, stage_bytes=stage)
        except ica.MijError as e:  # the one reason a far test may skip for: the device cannot hold the arenas themselves
            if "out of memory" in str(e).lower():
                pytest.skip("MIJ_E_NOMEM creating 2 x %d arena bytes: %s" % (self.pix_cap, e))
            raise
        self.enc = enc
        try:
            enc.stream_reserve(stream_bytes)
            if force_generic:
                enc.force_generic(True)
            self.pix_used = self.du_used = 0
            self.pix_off, self.du_off, self.pix_bytes_of, self.du_bytes_of = {}, {}, {}, {}
            assert self._account(enc.add(_flat(w, h), ENC_Q), w, h, 3, ENC_Q, True) == 0
            for _ in range(self.n_spacers - 1):
                self._account(enc.add_clone(0), w, h, 3, ENC_Q, True)
            self.trim_slot = self._account(enc.add(_flat(ENC_TRIM_W, self.trim_h), ENC_Q), ENC_TRIM_W, self.trim_h, 3, ENC_Q, True)
            assert self.pix_used == self.du_used == LINE - ENC_BACK
            self.slots = []
        except BaseException:
            enc.close()
            raise

    def pixel_bytes(self, w, h, comp, q):
        n = self._pixel_bytes(w, h, comp, q)
        assert n > 0
        return n

    def _account(self, slot, w, h, comp, q, has_pixels):
        """the running sums of the encoder's add: mij_enc_pixel_bytes for a slot that has pixels, 128 bytes per unit of the slot's plan"""
        p = self.enc.plan(slot)
        nb = self.pixel_bytes(w, h, comp, q) if has_pixels else 0
        nd = align(p.du_elems() * 2)
        self.pix_off[slot], self.du_off[slot], self.pix_bytes_of[slot], self.du_bytes_of[slot] = self.pix_used, self.du_used, nb, nd
        self.pix_used += nb
        self.du_used += nd
        assert self.pix_used <= self.pix_cap and self.du_used <= self.du_cap
        return slot

    def _under_test(self, slot, w, h, comp, q, has_pixels):
        self.slots.append(self._account(slot, w, h, comp, q, has_pixels))
        return slot

    # ---- the slots under test
    def add(self, img, q):
        return self._under_test(self.enc.add(img, q), img.shape[1], img.shape[0], img.shape[2], q, True)

    def add_device(self, t, w, h, comp, q):
        return self._under_test(self.enc.add_device(t, q), w, h, comp, q, True)

    def add_device_float(self, t, cv, w, h, comp, q):
        return self._under_test(self.enc.add_device_float(t, cv, q), w, h, comp, q, True)

    def add_units(self, w, h, comp, q, du):
        return self._under_test(self.enc.add_units(w, h, comp, q, du), w, h, comp, q, False)

    def add_coef(self, batch, slot, orientation=1, trim=False, tables=None, coarsen_only=True):
        s = self.enc.add_coef(batch, slot, orientation, trim, tables, coarsen_only)
        p = self.enc.plan(s)
        return self._under_test(s, p.width, p.height, p.comp, 0, False)

    def premise(self):
        """the first slot under test straddles 2^32 of the unit arena, and of the pixel arena if it has pixels; every later slot begins
        at or behind the line of the arenas it uses"""
        assert self.slots
        first = self.slots[0]
        assert self.du_off[first] < LINE < self.du_off[first] + self.du_bytes_of[first], ("unit arena", self.du_off[first], self.du_bytes_of[first])
        if self.pix_bytes_of[first]:
            assert self.pix_off[first] < LINE < self.pix_off[first] + self.pix_bytes_of[first], ("pixel arena", self.pix_off[first], self.pix_bytes_of[first])
        for sl in self.slots[1:]:
            assert self.du_off[sl] >= LINE, ("unit offset", sl, self.du_off[sl])
            assert not self.pix_bytes_of[sl] or self.pix_off[sl] >= LINE, ("pixel offset", sl, self.pix_off[sl])

    def check_spacers(self):
        """after fetch_streams: every spacer's and the trimming picture's stream against the host writer's, and the units of five slots"""
        enc, ica = self.enc, self.ica
        du, jpg = _enc_expected(ica, "spacer", *ENC_SPACER)
        assert 10000 < len(jpg) < 200000
        bad = [k for k in range(self.n_spacers) if enc.stream(k)[0] != jpg]
        assert bad == [], ("spacers whose streams differ from the host writer's: a store landed in them", bad[:16], len(bad))
        for k in (0, 1, self.n_spacers // 2, self.n_spacers - 2, self.n_spacers - 1):
            assert np.array_equal(enc.fetch(k), du), ("units of spacer", k)
        tdu, tjpg = _enc_expected(ica, "trim", ENC_TRIM_W, self.trim_h)
        assert enc.stream(self.trim_slot)[0] == tjpg and np.array_equal(enc.fetch(self.trim_slot), tdu), "the trimming picture in front of the line"

    def close(self):
        self.enc.close()
