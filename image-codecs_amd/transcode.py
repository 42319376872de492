"""Lossless JPEG transcode on the GPU: jpegtran -optimize for a batch.  The decode front end (Huffman walk on the GPU where it applies,
host walk otherwise) leaves every picture's quantised coefficients in device memory; a conversion kernel re-orders them into the writer's
data units (mij_enc_add_coef) and the emission kernels write the new streams, with Huffman tables built on the GPU from each picture's own
statistics.  The same coefficients, to the bit, in a smaller file: no IDCT, no pixels, no generation loss, and only finished streams
cross PCIe on the way back.  No pixel kernel is launched.

This module needs no torch."""
from .binding import Batch, Context, Encoder, HostDecoder, MijError, _qtable_pair, copy_markers as _copy_markers, emit_transcoded, \
    exif_orientation, exif_set_orientation, quality_tables, restart_interval, transcode_plan, transcode_plan_cropped, transcode_plan_grey, \
    transcode_plan_oriented

# one launch takes at most this many pictures / bytes of coefficient arena; larger calls are cut into chunks
MAX_SLOTS = 4096
MAX_COEF_BYTES = 2 << 30


def _align(v, a):
    return (v + a - 1) // a * a


def _orientations(v, datas):
    """transcode's orientation= as one value 1..8 per source, the files' own tags read where "exif" is asked"""
    n = len(datas)
    what = "orientation must be None, 'exif', 1..8 or one of those per source (got %r)"
    if v is None or isinstance(v, str) or (isinstance(v, int) and not isinstance(v, bool)):
        vals = [v] * n
    else:
        try:
            vals = list(v)
        except TypeError:
            raise ValueError(what % (v,)) from None
        if len(vals) != n:
            raise ValueError("orientation has %d values for %d sources" % (len(vals), n))
    for o in vals:
        if not (o is None or o == "exif" or (isinstance(o, int) and not isinstance(o, bool) and 1 <= o <= 8)):
            raise ValueError(what % (o,))
    return [1 if o is None else exif_orientation(d) if o == "exif" else o for o, d in zip(vals, datas)]


def _targets(quality, qtables, n):
    """transcode's quality= / qtables= as one (luma, chroma) pair of 64-byte tables, or None, per source"""
    if quality is not None and qtables is not None:
        raise ValueError("quality and qtables are two ways to say the same thing: give one")
    if qtables is not None:
        return [_qtable_pair(qtables)] * n
    what = "quality must be None, an int 1..100 or one of those per source (got %r)"
    if quality is None or (isinstance(quality, int) and not isinstance(quality, bool)):
        vals = [quality] * n
    else:
        if isinstance(quality, (str, bytes)):
            raise ValueError(what % (quality,))
        try:
            vals = list(quality)
        except TypeError:
            raise ValueError(what % (quality,)) from None
        if len(vals) != n:
            raise ValueError("quality has %d values for %d sources" % (len(vals), n))
    for q in vals:
        if not (q is None or (isinstance(q, int) and not isinstance(q, bool) and 1 <= q <= 100)):
            raise ValueError(what % (q,))
    made = {}
    for q in vals:
        if q is not None and q not in made:
            made[q] = tuple(t.tobytes() for t in quality_tables(q))
    return [None if q is None else made[q] for q in vals]


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _window(v):
    """one crop window as a tuple of four ints, ValueError for anything else or a size below 1"""
    what = "a crop window is (x0, y0, w, h), four ints with w >= 1 and h >= 1 (got %r)"
    if isinstance(v, (str, bytes)):
        raise ValueError(what % (v,))
    try:
        win = tuple(v)
    except TypeError:
        raise ValueError(what % (v,)) from None
    if len(win) != 4 or not all(_is_int(x) for x in win) or win[2] < 1 or win[3] < 1:
        raise ValueError(what % (v,))
    return win


def _crops(v, n):
    """transcode's crop= as one window or None per source"""
    if v is None:
        return [None] * n
    if isinstance(v, (str, bytes)):
        raise ValueError("crop must be None, one (x0, y0, w, h) or one of those per source (got %r)" % (v,))
    try:
        vals = list(v)
    except TypeError:
        raise ValueError("crop must be None, one (x0, y0, w, h) or one of those per source (got %r)" % (v,)) from None
    if vals and all(_is_int(x) or isinstance(x, (bool, float)) for x in vals):  # numbers: one window for all
        return [_window(vals)] * n
    if len(vals) != n:
        raise ValueError("crop has %d windows for %d sources" % (len(vals), n))
    return [None if w is None else _window(w) for w in vals]


def _greys(v, n):
    """transcode's grey= as one bool per source"""
    if isinstance(v, bool):
        return [v] * n
    if isinstance(v, (str, bytes)):
        raise ValueError("grey must be a bool or one per source (got %r)" % (v,))
    try:
        vals = list(v)
    except TypeError:
        raise ValueError("grey must be a bool or one per source (got %r)" % (v,)) from None
    if len(vals) != n:
        raise ValueError("grey has %d values for %d sources" % (len(vals), n))
    if not all(isinstance(g, bool) for g in vals):
        raise ValueError("grey must be a bool or one per source (got %r)" % (v,))
    return vals


def _progressives(v, n):
    """transcode's progressive= as one bool per source"""
    vals = [v] * n if isinstance(v, bool) else None
    if vals is None:
        if isinstance(v, (str, bytes)):
            raise ValueError("progressive must be a bool or one per source (got %r)" % (v,))
        try:
            vals = list(v)
        except TypeError:
            raise ValueError("progressive must be a bool or one per source (got %r)" % (v,)) from None
        if len(vals) != n:
            raise ValueError("progressive has %d values for %d sources" % (len(vals), n))
    if not all(isinstance(p, bool) for p in vals):
        raise ValueError("progressive must be a bool or one per source (got %r)" % (v,))
    return vals


def _intervals(v, n, name):
    """transcode's restart_rows= / restart_mcus= as one int >= 0 per source (None is 0: none)"""
    what = name + " must be None, an int >= 0 or one of those per source (got %r)"
    if v is None or _is_int(v):
        vals = [v] * n
    else:
        if isinstance(v, (str, bytes)):
            raise ValueError(what % (v,))
        try:
            vals = list(v)
        except TypeError:
            raise ValueError(what % (v,)) from None
        if len(vals) != n:
            raise ValueError("%s has %d values for %d sources" % (name, len(vals), n))
    for x in vals:
        if not (x is None or (_is_int(x) and x >= 0)):
            raise ValueError(what % (x,))
    return [0 if x is None else x for x in vals]


def _destination(desc, o, trim, crop, grey):
    """-> (data-unit elements, pixels) of the picture a source becomes, from its header alone; None where a step refuses (mij_enc_add_coef
    says why later) and the source's own size has to do"""
    t = transcode_plan(desc)[0]
    if t is not None and grey:
        t = transcode_plan_grey(t)
    if t is not None:
        t = transcode_plan_oriented(t, o, trim)[0]
    if t is not None and crop is not None:
        t = transcode_plan_cropped(t, crop)[0]
    return None if t is None else (t.du_elems(), t.plan.width * t.plan.height)


class Transcoder:
    """transcode(datas) -> one new JPEG stream per source, or None where the source cannot be transcoded (last_reasons says why).

    Owns a Context, a Batch and an Encoder with its emission arena, grown as needed and reused across calls.  Synchronous.  Sources that
    are transcodable: grey, and YCbCr (JFIF or Adobe transform 1) as 4:4:4, 4:2:2, 4:4:0 or 4:2:0, baseline or progressive, with or without
    restart intervals, whose quantisation tables hold 8-bit entries and are the same for Cb and Cr.  The output is a baseline stream
    without restart intervals unless they are asked for, or a progressive stream with progressive=True (include/mij_host.h, mjw_tplan
    and PROGRESSIVE STREAMS, has the whole contract).  Slots whose streams do not fit the arena are finished on the host from their units
    and the arena grows for the next call; so are progressive slots in which libjpeg would flush an end-of-band run early
    (last_host_emitted counts both)."""

    def __init__(self, device=None):
        if device is not None and (isinstance(device, bool) or not isinstance(device, int) or device < 0):
            raise ValueError("device must be None (the current device) or a device index, got %r" % (device,))
        self._device = -1 if device is None else device
        self._ctx = None
        self._batch = None
        self._enc = None
        self._bcap = (0, 0, 0, 0)
        self._ecap = (0, 0)
        self._arena = 0
        self._fmt = "compact"
        self.last_reasons = []
        self.last_host_emitted = 0
        self.last_requantized = []
        self.last_crops = []
        self.last_greyed = []
        self.last_restarts = []
        self.last_progressive = []
        self.last_timing = {}

    @property
    def arena_bytes(self):
        return self._arena

    def close(self):
        for name in ("_enc", "_batch", "_ctx"):
            h = getattr(self, name)
            if h is not None:
                h.close()
                setattr(self, name, None)
        self._bcap, self._ecap, self._arena = (0, 0, 0, 0), (0, 0), 0

    def reserve_arena(self, nbytes):
        """Sets the emission arena's size for the next call (tests and measurements; transcode() sizes it by itself)."""
        self._arena = max(0, int(nbytes))
        if self._enc is not None:
            self._enc.stream_reserve(self._arena)

    def set_coef_format(self, fmt):
        """'compact' (default) or 'int16': the format the coefficient planes get in device memory (tests)."""
        if fmt not in ("compact", "int16"):
            raise ValueError("coefficient format must be 'compact' or 'int16'")
        self._fmt = fmt
        if self._batch is not None:
            self._batch.set_coef_format(fmt)

    def _batch_for(self, n, coef, out, stream):
        need = (max(1, n), max(coef, 256), max(out, 256), stream)
        if self._batch is None or any(a > b for a, b in zip(need, self._bcap)):
            if self._batch is not None:
                self._batch.close()
                self._batch = None
            if self._ctx is None:
                self._ctx = Context(self._device)
            cap = tuple(max(a, b) for a, b in zip(need, self._bcap))
            self._batch = Batch(self._ctx, cap[0], cap[1], cap[1], cap[2])
            self._batch.set_coef_format(self._fmt)
            if cap[3]:
                self._batch.entropy_reserve(cap[3])
            self._bcap = cap
        else:
            self._batch.reset()
        return self._batch

    def _encoder_for(self, n, du):
        need = (max(1, n), max(du, 256))
        if self._enc is None or any(a > b for a, b in zip(need, self._ecap)):
            if self._enc is not None:
                self._enc.close()
                self._enc = None
            cap = tuple(max(a, b) for a, b in zip(need, self._ecap))
            self._enc = Encoder(self._ctx, cap[0], 0, cap[1], stage_bytes=0)
            self._ecap = cap
            if self._arena:
                self._enc.stream_reserve(self._arena)
        else:
            self._enc.reset()
        return self._enc

    def transcode(self, datas, *, optimize=True, copy_markers="all", only_if_smaller=False, gpu_entropy=None, threads=16, orientation=None,
                  edge="perfect", quality=None, qtables=None, coarsen_only=True, crop=None, grey=False, restart_rows=None, restart_mcus=None,
                  progressive=False):
        """datas: a sequence of JPEG files as bytes.  -> a list with, per source, the new stream (bytes) or None; last_reasons[i] is None
        or the reason source i was refused or could not be decoded.
        optimize: Huffman tables built from each picture's own statistics (mjw_temit_optimized's stream); False: the Annex-K tables.
        copy_markers: "all" puts the source's APPn and COM segments (those before its first SOS, in source order) directly behind SOI,
        the writer's own JFIF APP0 being dropped when the source carries a JFIF APP0 or an Adobe APP14; "none" leaves the stream as
        emitted.  Offsets inside copied segments (MPF and the like) are not fixed up.
        only_if_smaller: the source's own bytes are returned where the result is not shorter.
        gpu_entropy: the front end, as Batch.decode_jpegs takes it (None: the default; True / False: GPU walk where it applies / host).
        orientation: None (the coefficients as stored), "exif" (each file's own Orientation tag), an int 1..8, or a sequence of those per
        source, as TensorDecoder.decode takes it: the picture is rotated / flipped / transposed in the coefficients, exactly (jpegtran's
        set; include/mij_host.h, mjw_tplan_oriented).  Where that changed the picture the transformed stream is returned whatever
        only_if_smaller says, and copy_markers="all" resets the copied EXIF Orientation tag to 1 (other EXIF fields -- pixel dimensions,
        the thumbnail -- are left as they are).
        edge: a mirrored axis that is no multiple of the MCU size cannot be mirrored exactly: "perfect" refuses that picture (its reason
        names the axis), "trim" drops the partial MCU column / row of the mirrored axes (jpegtran -trim).
        quality: None, an int 1..100 or one of those per source: the coefficients are requantised, on the GPU and without pixels, to the
        tables this writer uses at that quality (one rounding each: include/mij_host.h, mjw_tplan_requant), after the orientation.  The
        sampling, the geometry and the markers stay the source's.  qtables: instead, one (luma, chroma) pair of 64 ints 1..255 in zigzag
        order for all sources.  coarsen_only (default): each entry becomes the larger of the source's and the target's, since a finer
        step restores nothing and only grows the file; False takes the target as it is.  last_requantized[i] says whether source i's
        tables changed; where they did not, the stream is the lossless one.  only_if_smaller keeps its meaning.
        grey: a bool, or one per source: Cb and Cr are dropped and the luma coefficients kept to the bit (jpegtran -grayscale), before the
        orientation -- a grey picture's MCU is 8 x 8, so edge="perfect" mirrors a 4:2:0 picture whose size is a multiple of 8 but not
        of 16 once it is grey.  last_greyed[i] says whether chroma was dropped (not for a grey source).
        crop: None, one window (x0, y0, w, h) for all sources, or a sequence with one window or None per source, in the displayed frame
        (after the orientation), as TensorDecoder's crops are: the window is cut out of the coefficients (jpegtran -crop).  Its origin
        moves down to the MCU grid (8 * h_luma x 8 * v_luma, 8 x 8 once grey) and the size grows by what it moved; last_crops[i] is the
        kept (x0', y0', W', H'), None where no crop was asked.  A window that does not lie inside its picture is refused for that picture
        alone, with its reason in last_reasons[i].  The steps run as grey -> orient -> crop -> requantise (include/mij_host.h,
        mjw_tplan_cropped); where crop or grey changed the picture the result is returned whatever only_if_smaller says.  EXIF pixel
        dimensions and thumbnails of copied markers are not fixed up.
        restart_rows, restart_mcus: None, an int >= 0 or one of those per source: restart markers after every so many MCU rows, or MCUs,
        of the destination -- its geometry after grey -> orient -> crop (jpegtran -restart N / -restart NB; include/mij_host.h, RESTART
        INTERVALS).  None or 0 means none; giving both for the same source is a ValueError.  An interval that resolves above 65535 MCUs
        refuses that picture alone, with its reason in last_reasons[i].  last_restarts[i] is the interval used, in MCUs.  A source's own
        DRI is never copied (copy_markers copies APPn and COM only), and only_if_smaller compares the finished stream as it is.
        progressive: a bool, or one per source: the stream is written as a progressive one (jpegtran -progressive; include/mij_host.h,
        PROGRESSIVE STREAMS): the same coefficients in libjpeg's ten scans (six for grey), each under the optimal tables of its own
        symbols, whatever optimize says.  It composes with every step above; last_progressive[i] says which outputs are progressive
        (False where only_if_smaller kept the source).  Together with a restart interval for the same source it is a ValueError.
        ValueError, before a device is touched, for arguments that are not of these kinds."""
        if not isinstance(optimize, bool) or not isinstance(only_if_smaller, bool):
            raise ValueError("optimize and only_if_smaller must be bools")
        if copy_markers not in ("all", "none"):
            raise ValueError("copy_markers must be 'all' or 'none', got %r" % (copy_markers,))
        if gpu_entropy not in (None, True, False):
            raise ValueError("gpu_entropy must be None, True or False")
        if isinstance(threads, bool) or not isinstance(threads, int) or threads < 1:
            raise ValueError("threads must be a positive int")
        if edge not in ("perfect", "trim"):
            raise ValueError("edge must be 'perfect' or 'trim', got %r" % (edge,))
        if not isinstance(coarsen_only, bool):
            raise ValueError("coarsen_only must be a bool")
        if isinstance(datas, (bytes, bytearray, memoryview, str)):
            raise ValueError("datas is a sequence of JPEG files, not one file")
        datas = list(datas)
        for i, d in enumerate(datas):
            if not isinstance(d, (bytes, bytearray, memoryview)):
                raise ValueError("source %d is not bytes" % i)
        datas = [bytes(d) for d in datas]
        orients = _orientations(orientation, datas)
        targets = _targets(quality, qtables, len(datas))
        crops = _crops(crop, len(datas))
        greys = _greys(grey, len(datas))
        rrows, rmcus = _intervals(restart_rows, len(datas), "restart_rows"), _intervals(restart_mcus, len(datas), "restart_mcus")
        for i, (r, m) in enumerate(zip(rrows, rmcus)):
            if r and m:
                raise ValueError("source %d: restart_rows and restart_mcus are two ways to say the same thing: give one" % i)
        progs = _progressives(progressive, len(datas))
        for i, p in enumerate(progs):
            if p and (rrows[i] or rmcus[i]):
                raise ValueError("source %d: restart intervals are not combined with progressive output" % i)
        self.last_progressive = written = [False] * len(datas)
        self.last_restarts = restarts = [0] * len(datas)
        self.last_requantized = requantized = [False] * len(datas)
        self.last_crops = kept = [None] * len(datas)
        self.last_greyed = greyed = [False] * len(datas)
        windowed = [False] * len(datas)
        out = [None] * len(datas)
        reasons = [None] * len(datas)
        self.last_host_emitted = 0
        self.last_timing = {"convert_ms": 0.0, "emit_ms": 0.0}
        # headers first: sizes for the arenas, and the pictures no front end would take
        todo = []
        for i, d in enumerate(datas):
            try:
                desc = HostDecoder.probe(d, 0)
            except MijError as e:
                reasons[i] = str(e)
                continue
            # what the frame header settles -- component count and sampling -- is refused here; colour and tables may still change behind
            # it, so those are judged on the walked picture's descriptor (mij_enc_add_coef)
            c0 = desc.comp[0]
            if desc.ncomp not in (1, 3) or not (1 <= c0.h <= 2 and 1 <= c0.v <= 2) or (desc.ncomp == 1 and (c0.h, c0.v) != (1, 1)) or \
                    any((desc.comp[c].h, desc.comp[c].v) != (1, 1) for c in range(1, desc.ncomp)):
                reasons[i] = "not transcodable: " + (transcode_plan(desc)[1] or "refused")
                continue
            du, px = sum(desc.comp[c].bw * desc.comp[c].bh for c in range(desc.ncomp)) * 128, desc.width * desc.height
            if crops[i] is not None or greys[i]:  # the arenas hold the destination: a window of a large picture needs little
                dst = _destination(desc, orients[i], edge == "trim", crops[i], greys[i])
                if dst is not None:
                    du, px = dst[0] * 2, dst[1]
            todo.append((i, Batch.coef_bytes(desc), Batch.out_bytes(desc), _align(du, 256), px))
        k = 0
        while k < len(todo):
            j, coef = k, 0
            while j < len(todo) and j - k < MAX_SLOTS and (j == k or coef + todo[j][1] <= MAX_COEF_BYTES):
                coef += todo[j][1]
                j += 1
            self._chunk(datas, todo[k:j], out, reasons, optimize, gpu_entropy, threads, orients, edge == "trim", targets, coarsen_only,
                        requantized, crops, greys, kept, greyed, windowed, rrows, rmcus, restarts, progs)
            k = j
        for i, d in enumerate(datas):
            if out[i] is None:
                continue
            if copy_markers == "all":
                out[i], why = _copy_markers(d, out[i])
                if out[i] is None:
                    reasons[i] = "markers: " + why
                    continue
                if orients[i] != 1:  # the picture is upright now: the copied tag must not turn it again
                    out[i], _ = exif_set_orientation(out[i], 1)
            written[i] = progs[i]
            if only_if_smaller and orients[i] == 1 and not windowed[i] and len(out[i]) >= len(d):
                out[i] = d
                written[i] = False
        self.last_reasons = reasons
        return out

    def _chunk(self, datas, items, out, reasons, optimize, gpu_entropy, threads, orients, trim, targets, coarsen_only, requantized, crops,
               greys, kept, greyed, windowed, rrows, rmcus, restarts, progs):
        n = len(items)
        srcs = [datas[it[0]] for it in items]
        stream = 0
        if gpu_entropy:  # mjh_decode_batch_gpu wants its arena reserved; the default front end makes its own
            stream = _align(sum(len(s) + 4096 for s in srcs), 1 << 20)
        b = self._batch_for(n, sum(it[1] for it in items), sum(it[2] for it in items), stream)
        _, slots, why = b.decode_jpegs(srcs, 0, threads=threads, gpu_entropy=gpu_entropy)
        if not any(sl >= 0 for sl in slots):
            for it, r in zip(items, why):
                reasons[it[0]] = r or "decode failed"
            return
        b.upload()  # the coefficient planes into device memory (pack where needed); no pixel kernel runs
        if not self._arena:  # a first guess, about half a byte per pixel; misses grow it
            self._arena = _align(sum(1024 + it[4] // 2 for it in items), 1 << 20)
        enc = self._encoder_for(n, sum(it[3] for it in items))
        es = {}
        for it, sl, r in zip(items, slots, why):
            if sl < 0:
                reasons[it[0]] = r or "decode failed"
                continue
            try:
                es[it[0]] = enc.add_coef(b, sl, orients[it[0]], trim, targets[it[0]], coarsen_only, crops[it[0]], greys[it[0]])
            except MijError as e:
                reasons[it[0]] = str(e).split(": ", 1)[-1]
                continue
            if crops[it[0]] is not None:
                kept[it[0]] = enc.slot_rect(es[it[0]])
            greyed[it[0]] = enc.slot_greyed(es[it[0]])
            windowed[it[0]] = enc.slot_windowed(es[it[0]])
            requantized[it[0]] = enc.slot_requantized(es[it[0]])
            if progs[it[0]]:  # implies the optimal tables, per scan
                enc.set_progressive(es[it[0]])
            elif optimize:
                enc.set_optimize(es[it[0]])
            if rrows[it[0]] or rmcus[it[0]]:  # resolved on the destination's plan; a refused one costs its slot, which is never fetched
                ri, bad = restart_interval(enc.tplan(es[it[0]]), rrows[it[0]], rmcus[it[0]])
                if ri is None:
                    reasons[it[0]] = "restart interval: " + bad
                    del es[it[0]]
                    continue
                enc.set_restart(es[it[0]], ri)
                restarts[it[0]] = ri
        if not es:
            b.wait()
            return
        enc.upload()
        enc.timer_begin()
        enc.launch()
        enc.timer_end()
        enc.fetch_streams()
        self.last_timing["convert_ms"] += enc.coef_ms() or 0.0
        self.last_timing["emit_ms"] += enc.timer_ms()
        need, host, grow = 0, 0, 0
        for i, slot in es.items():
            data, ln = enc.stream(slot)
            if data is None:
                status = enc.slot_status(slot)
                if status == "uncodable":
                    reasons[i] = "not codable: an AC coefficient outside -1023..1023 or a DC difference outside -2047..2047"
                    continue
                # its units are on the device: the host finishes it, at the same interval or as the same progressive stream
                data = emit_transcoded(enc.tplan(slot), enc.fetch(slot), optimize, restart_mcus=restarts[i], progressive=progs[i])
                host += 1
                if status == "host flush":  # a forced flush, not a lack of room: the device reported no length
                    ln = len(data)
                else:
                    grow += 1
            need += ln
            out[i] = data
        self.last_host_emitted += host
        if grow:
            self._arena = _align(need + need // 8, 1 << 20)
            enc.stream_reserve(self._arena)
