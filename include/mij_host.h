/*
 * mij_host.h -- the host half of the JPEG decode path, as plain C entry points.
 *
 * This is the part of the reference that stays on the CPU -- marker parsing, Huffman tables and
 * the sequential entropy-coded-segment walk (codec/jpeg.c:88-558, :1119-1756) -- restated so
 * that every decoded block lands, still quantised, in the tile-layout staging planes of mij.h
 * instead of being de-quantised and inverse-transformed on the spot
 * (codec/jpeg.c:1178,:1217,:1342).  stbi_load* (image_api.h) is built from exactly these calls.
 */
#ifndef MIJ_HOST_H
#define MIJ_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "mij.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Type test + header + describe (stbi__jpeg_test, then codec/jpeg.c:1670-1699, :2241-2249):
 * fills *desc so the caller can size the coefficient planes.  Returns 1, or 0 with *reason = the
 * reference's short failure string ("unknown image type", "bad req_comp", "only 8-bit", ...).
 */
int mjh_probe_memory(const uint8_t *buf, int len, int req_comp, mij_image_desc *desc, const char **reason);

/*
 * The same plus the scans (codec/jpeg.c:1713-1755) into `arena`: the component planes in tile
 * layout, back to back in component order -- exactly the layout of the staging a mij batch hands
 * out (mij_batch_coef(b, slot, 0)).  The callee zero-fills what it uses.  desc->flags gets
 * MIJ_FLAG_WIDE_IDCT when the fast IDCT's range guarantee does not hold.  Returns 1 / 0 + reason.
 */
int mjh_decode_memory(const uint8_t *buf, int len, int req_comp, mij_image_desc *desc, int16_t *arena, size_t arena_elems, const char **reason);

/*
 * The same into an image's whole staging region (mij_batch_stage_region: mij_image_coef_bytes(desc) bytes), in the format the GPU
 * reads where the file allows it: want_compact != 0 and a baseline file -> COMPACT planes written by the walk itself (mij.h,
 * mij_compact_offsets: low bytes + DC array, escape bytes only for blocks that need them), desc->flags gets
 * MIJ_FLAG_STAGED_COMPACT (and MIJ_FLAG_HAS_ESCAPES): no pack pass on the device and 1.6 instead of 3 bytes per pixel over PCIe.
 * Progressive files (their scans read-modify-write int16 planes, codec/jpeg.c:372-558) and want_compact == 0: int16 tile layout
 * as mjh_decode_memory.  The reference's block decoder being restated either way: codec/jpeg.c:308-370.
 */
int mjh_decode_memory_fmt(const uint8_t *buf, int len, int req_comp, mij_image_desc *desc, uint8_t *region, size_t region_bytes, int want_compact, const char **reason);
/*
 * The same, and the picture's row-extent table (mij.h, "row-extent table") into row_classes: one byte per block row, component
 * after component, row_classes_bytes >= the sum of desc->comp[c].bh (MJH_ROW_CLASSES_MAX always suffices).  A baseline file walked into
 * compact planes gets the classes the walk saw -- folded into its block loop from the positions it writes -- unless the stream needs
 * MIJ_FLAG_WIDE_IDCT; everything else (progressive files, int16 staging) gets 3 throughout.  row_classes may be NULL.
 */
#define MJH_ROW_CLASSES_MAX (4 * 8200)
int mjh_decode_memory_rows(const uint8_t *buf, int len, int req_comp, mij_image_desc *desc, uint8_t *region, size_t region_bytes, int want_compact, uint8_t *row_classes,
									size_t row_classes_bytes, const char **reason);

/* Header parse + extraction of the entropy segment for the GPU entropy stage (mij.h: mjg_scan,
 * mij_batch_add_stream).  Returns 1: *scan filled, the segment without its 0xFF00 stuffing written to stream
 * (stream_cap must leave 32 spare bytes); 2: a valid header but not a layout the GPU walk takes (use
 * mjh_decode_memory); 0: rejected like mjh_probe_memory, *reason set. */
int mjh_extract_scan(const uint8_t *buf, int len, int req_comp, mjg_scan *scan, uint8_t *stream, size_t stream_cap, size_t *stream_len, const char **reason);

/*
 * Batch front end: n JPEGs into a mij batch.  Images are added to the batch in input order
 * (slots[i] = the slot of image i, or -1 with reasons[i] set when its header is rejected);
 * an image whose entropy data is rejected keeps its slot but is flagged MIJ_FLAG_SKIP (reasons[i]
 * set, slot reported as -1 - slot).  reasons[i] is the parser's string, or "decode failed" for the few
 * failures that set none (a DQT or DHT segment with bytes left over, a scan naming a component the frame lacks).  Follow with mij_batch_submit().  Returns the number of
 * images decoded successfully, or a negative MIJ_E_* code when the batch arenas are too small.
 *
 * mjh_decode_batch       the DEFAULT: the Huffman walk itself runs on the GPU wherever it applies (single-scan baseline
 *                        files; mjh_decode_batch_gpu below), the host walk is the fallback for every other layout and for
 *                        any stream the GPU walk reports back.  The batch gets its entropy arena on first use (sized for
 *                        that call; a later, larger call takes the host walk).  Environment MIJ_ENTROPY=host selects the
 *                        host-only front end instead (mjh_gpu_walk_default() says which is in force).  Pictures below
 *                        2200 pixels per host thread (MIJ_GPU_WALK_BATCH_MIN_PIXELS overrides) take the host walk in the same
 *                        call: their few subsequences leave the GPU walk's workgroups mostly idle.
 * mjh_decode_batch_host  the host stage of every image on `threads` host threads (one image per task), straight into the
 *                        batch's pinned staging -- what north_star describes ("the C host keeps the Huffman walk"); its
 *                        end-to-end rate is bounded by the walk (about 0.25-0.5 Gpix/s per host core) and by PCIe.
 */
int mjh_decode_batch(mij_batch *b, const uint8_t *const *bufs, const int *lens, int n, int req_comp, int threads, int *slots, const char **reasons);
int mjh_decode_batch_host(mij_batch *b, const uint8_t *const *bufs, const int *lens, int n, int req_comp, int threads, int *slots, const char **reasons);
int mjh_gpu_walk_default(void);

/*
 * One logical batch over several devices (BASELINE config 3; north_star: "sharded across the 8 GPUs of one node on
 * separate HIP streams ... no RCCL"): batches[k] belongs to device k's context (any contexts will do -- two on one
 * device is what the single-GPU test uses), image i goes to owner[i] = the k-th of n_batches contiguous slices (sizes
 * differing by at most one), slots[i] / reasons[i] as above, relative to that batch.  The host threads are one
 * shared pool; the thread that walks the last image of a slice SUBMITS that batch (upload + kernels, asynchronous on
 * its own stream), so device k works while slice k+1 is still being walked.  Follow with mij_batch_wait() on every
 * batch.  Returns the number of images decoded, or a negative MIJ_E_* code.  No collective, no peer traffic: decoder
 * state is per image (codec/jpeg.c:2445).
 */
int mjh_decode_batch_multi(mij_batch *const *batches, int n_batches, const uint8_t *const *bufs, const int *lens, int n, int req_comp, int threads,
									int *owner, int *slots, const char **reasons);

/* The same contract with the Huffman walk on the GPU where it applies (mij_batch_entropy_reserve must have
 * been called, otherwise this is mjh_decode_batch): the host threads only parse headers and remove byte
 * stuffing, mij_batch_entropy_run walks the streams, and whatever it does not take or refuses is walked on
 * the host as above.  Waits for the GPU walk; follow with mij_batch_submit(). */
int mjh_decode_batch_gpu(mij_batch *b, const uint8_t *const *bufs, const int *lens, int n, int req_comp, int threads, int *slots, const char **reasons);

/* The same in two halves, so that the host can prepare the next batch while the GPU walks this one: begin parses,
 * unstuffs, adds the slots and queues the GPU walk (returns NULL with *rc set on failure; MIJ_E_STATE = no entropy
 * arena reserved); end waits for the walk, host-walks what it handed back and returns the count like above.
 * bufs, lens, slots and reasons must stay valid until end. */
typedef struct mjh_gpu_job mjh_gpu_job;
mjh_gpu_job *mjh_decode_batch_gpu_begin(mij_batch *b, const uint8_t *const *bufs, const int *lens, int n, int req_comp, int threads, int *slots,
													 const char **reasons, int *rc);
int mjh_decode_batch_gpu_end(mjh_gpu_job *job);

/*
 * JPEG writer in three steps (stbi_write_jpg_to_func = plan + transform + emit); step 2 also exists
 * on the GPU (mij_enc_* in mij.h) and must produce the same data units bit for bit.
 *   mjw_plan_init       quality mapping and tables                       codec/jpeg_write.c:220-243
 *   mjw_transform_host  colour transform, edge replication, 2x2 chroma mean, float AAN fDCT, quantiser
 *                       for every data unit                              codec/jpeg_write.c:24-74,96-118,283-352
 *   mjw_emit            headers, Huffman emission, padding, EOI          codec/jpeg_write.c:245-268,120-169,358-363
 * Data units: int16[64] each, zigzag order, MCU after MCU (4:2:0: Y00 Y01 Y10 Y11 U V; 4:4:4: Y U V).
 */
typedef void mjw_write_func(void *context, void *data, int size); /* == stbi_write_func */
typedef struct {
	int width, height, comp; /* comp 1..4 as passed to stbi_write_jpg */
	int subsample;           /* 1: 4:2:0 (quality <= 90), 0: 4:4:4 */
	int mcu_x, mcu_y, du_per_mcu;
	unsigned char ytab[64], ctab[64]; /* quantisation tables, zigzag order (as written to DQT) */
	float fdtbl_y[64], fdtbl_c[64];   /* 1 / (q * aan scale), natural order */
} mjw_plan;

int mjw_plan_init(mjw_plan *p, int width, int height, int comp, int quality); /* 0 on bad arguments */
size_t mjw_plan_du_count(const mjw_plan *p);
void mjw_transform_host(const mjw_plan *p, const void *pixels, int flip_vertically, int16_t *du);
int mjw_emit(const mjw_plan *p, const int16_t *du, mjw_write_func *func, void *context);
int mjw_flip_on_write(void); /* the flag set by stbi_flip_vertically_on_write */
/* The pieces of mjw_emit that GPU emission (mij_enc_stream_reserve, mij.h) reuses: the headers in front of the entropy-coded
 * segment (always MJW_HEADER_BYTES; returns that count), and the writer's four Huffman code tables indexed by symbol, in the order
 * luma DC, chroma DC, luma AC, chroma AC (codes right-aligned, len 0 for a symbol the table lacks). */
#define MJW_HEADER_BYTES 607
size_t mjw_header(const mjw_plan *p, unsigned char *out);
void mjw_huff_tables(uint16_t code[4][256], uint8_t len[4][256]);

/* the plan (tables, geometry) the GPU encoder built for a slot, for mjw_emit */
int mij_enc_plan(const mij_encoder *e, int slot, mjw_plan *out);

/*
 * stbi_write_jpg_to_func with step 2 on the GPU: same arguments, same byte stream (the data units
 * are bit-identical), 0 on bad arguments or when no gfx950 device is present (no CPU fallback: use
 * stbi_write_jpg_to_func for the host-only writer).
 */
int mij_write_jpg_to_func(mjw_write_func *func, void *context, int x, int y, int comp, const void *data, int quality);

/* A batch of pictures in host memory -> their JPEG byte streams (each what stbi_write_jpg_to_func delivers for that picture,
 * codec/jpeg_write.c:283-366): staging copies on `threads` host threads, ONE GPU launch for every picture's transform, one copy
 * back, Huffman emission on the host threads.  out[i] is a malloc'ed stream of out_len[i] bytes (the caller frees it) or NULL for a
 * picture whose arguments were bad (NULL pixels, sizes or comp mjw_plan_init refuses) -- such pictures, even a whole call of them,
 * are not an error.  Returns the number of streams written, or a negative MIJ_E_* (device or memory failure); on a negative
 * return every out[i] is NULL again and nothing is left for the caller to free. */
int mij_write_jpg_batch(const void *const *pixels, const int *x, const int *y, const int *comp, int n, int quality, int threads,
                        unsigned char **out, size_t *out_len);
/* A capacity that holds the stream of `units` data units whatever they contain, with or without restart intervals.  Per unit: a DC symbol of at
 * most 11 + 11 bits and 63 AC symbols of at most 16 + 10, 1660 bits.  The worst interval is one grey unit (Ri = 1, one unit per MCU): its 1660
 * bits and the 7 fill bits are 1667, so 208 whole bytes (the 3 bits left over are dropped); every one of them may be a 0xFF that takes a stuffed
 * zero, 416 bytes, and two marker bytes follow: 418 <= 64 * 7 = 448.  Longer intervals and the unbroken scan pay the fill byte and the marker
 * less often, so 448 bytes per unit bound them too; SOI .. SOS with a DRI segment (MJW_HEADER_RESTART_BYTES) and EOI fit the 2048.  (Two bytes
 * per coefficient are NOT enough: a codable unit can take 1667 bits before stuffing.) */
#define MJW_STREAM_CAP(units) ((size_t)2048 + (size_t)(units) * 64 * 7)
/* mjw_emit into memory: bytes written, 0 when `cap` is too small or an argument is bad (MJW_STREAM_CAP(mjw_plan_du_count(p)) always fits) */
size_t mjw_emit_to_memory(const mjw_plan *p, const int16_t *du, unsigned char *out, size_t cap);

/*
 * Optimised Huffman tables: the same stream as mjw_emit but for the DHT segment and the codes, which come from the picture's own
 * symbol statistics (what libjpeg calls `optimize`).  Tables are indexed luma DC, chroma DC, luma AC, chroma AC throughout.
 *   mjw_histogram        the symbols mjw_emit emits for these units, counted per table: one DC category per unit, one 0xF0 per 16 zeros
 *                        of a run, one run/size symbol per non-zero AC, one 0x00 per unit whose coefficient 63 is zero.  0 when the
 *                        unit count times 64 does not fit 32 bits.
 *   mjw_optimal_table    ITU-T T.81 K.2 as libjpeg's jpeg_gen_optimal_table runs it: a pseudo-symbol 256 of count 1, the two smallest
 *                        non-zero counts merged until one is left (among equal counts the largest index is taken), lengths above 16
 *                        shortened pairwise (K.3), the pseudo-symbol's code removed, HUFFVAL by unlimited length then value.  bits[l-1]
 *                        is the number of codes of length l.  Returns 0, with nothing usable written, when a length before the
 *                        shortening exceeds 32.
 *   mjw_header_optimized mjw_header with these four tables in its one DHT segment (same order and identifiers); returns the length,
 *                        at most MJW_HEADER_BYTES.
 *   mjw_emit_optimized   histogram + four tables + emission; when a table cannot be built (the over-32 case, or a histogram that is
 *                        refused) the stream is mjw_emit's.  mjw_optimized_tables is its table step alone: 0 in those cases.
 */
int mjw_histogram(const mjw_plan *p, const int16_t *du, uint32_t freq[4][256]);
int mjw_optimal_table(const uint32_t freq[256], uint8_t bits[16], uint8_t vals[256], int *nvals);
size_t mjw_header_optimized(const mjw_plan *p, const uint8_t bits[4][16], const uint8_t vals[4][256], unsigned char *out);
int mjw_optimized_tables(const mjw_plan *p, const int16_t *du, uint8_t bits[4][16], uint8_t vals[4][256]);
int mjw_emit_optimized(const mjw_plan *p, const int16_t *du, mjw_write_func *func, void *context);
size_t mjw_emit_optimized_to_memory(const mjw_plan *p, const int16_t *du, unsigned char *out, size_t cap);
/* mij_write_jpg_to_func / mij_write_jpg_batch with flags: MJW_OPTIMIZE_HUFFMAN finishes every stream with mjw_emit_optimized; flags 0 is
 * the plain call. */
#define MJW_OPTIMIZE_HUFFMAN 1u
int mij_write_jpg_to_func_ex(mjw_write_func *func, void *context, int x, int y, int comp, const void *data, int quality, unsigned flags);
int mij_write_jpg_batch_ex(const void *const *pixels, const int *x, const int *y, const int *comp, int n, int quality, int threads,
                           unsigned char **out, size_t *out_len, unsigned flags);

/*
 * Lossless transcode: a decoded picture's QUANTISED coefficients written out again as a new baseline stream -- the same coefficients to
 * the bit, no IDCT, no pixels, no generation loss (jpegtran -optimize).  On the GPU: mij_enc_add_coef (mij.h); these calls are the written
 * contract, the fallback for slots that do not fit the emission arena, and what the CPU tests pin.
 *
 * A source is TRANSCODABLE when its descriptor says: one component at 1x1, or three-component YCbCr (MIJ_COLOR_YCBCR: JFIF, or Adobe
 * transform 1) with chroma at 1x1 and luma (h, v) one of (1,1) (2,1) (1,2) (2,2); every dequant entry of the tables in use <= 255; Cb and
 * Cr tables of equal contents.  Its units are CODABLE when every AC value lies in -1023..1023 and every DC difference (against the previous
 * unit of the same component in MCU order, from 0) in -2047..2047: mij_enc_add_units' ranges.
 *
 * Units: int16[64] each in zigzag order, MCU after MCU in raster MCU order; inside an MCU the luma blocks in raster order (h across, v down),
 * then Cb, then Cr -- 4:2:2 is Y0 Y1 Cb Cr, 4:4:0 is Ytop Ybottom Cb Cr, grey is one unit per MCU.  The block of component c at MCU (mx, my),
 * sub-block (sx, sy) is plane block L = (mx*h_c + sx) + (my*v_c + sy)*bw_c, and unit coefficient k is plane position mij_zigzag_pos[k].
 * Blocks a non-interleaved scan never coded are what the planes hold (zeros) and are emitted like any other.
 *
 * Stream: SOI, the writer's JFIF APP0, DQT with the SOURCE's tables in zigzag order (luma as id 0, chroma as id 1), SOF0 with the source's
 * size and sampling, DHT, SOS and the entropy-coded segment exactly as mjw_emit / mjw_emit_optimized code units; no DRI unless asked (RESTART INTERVALS, below).  For 4:4:4 and 4:2:0
 * the header is mjw_header's (mjw_header_optimized's) byte for byte given those tables, for 4:2:2 and 4:4:0 only the luma sampling byte
 * differs; a grey stream has a one-component SOF0 and SOS, one DQT table and only the luma DC and AC tables in its DHT.  At most
 * MJW_HEADER_BYTES.
 *
 *   mjw_tplan_from_desc    the plan of a descriptor, or 0 with *reason (a static string) when the source is not transcodable.  plan.ytab /
 *                          plan.ctab are the source's tables, plan.du_per_mcu the units per MCU (1, 3, 4 or 6), plan.comp = ncomp,
 *                          plan.subsample 1 for 4:2:0 only; the reciprocal tables are zero (nothing is transformed).
 *   mjw_units_from_region  the units of an image's coefficient region (mjh_decode_memory_fmt, mij_batch_stage_region) in format
 *                          MIJ_COEF_INT16 or MIJ_COEF_COMPACT; 0 when the descriptor is not transcodable.
 *   mjw_tunits_codable     1, or 0 with *reason (may be NULL)
 *   mjw_temit[_optimized]  the stream of the units; 0 also for units that are not codable
 *   mjw_temit_to_memory    flags 0 or MJW_OPTIMIZE_HUFFMAN; bytes written, 0 when cap is too small (MJW_STREAM_CAP(mjw_tplan_du_count(t)) always fits)
 *   mjw_copy_markers       `stream` (as emitted) with the APPn and COM segments the source carries before its first SOS, in source order,
 *                          directly behind SOI; the writer's own APP0 is dropped when the source carries a JFIF APP0 or an Adobe APP14 and
 *                          kept first otherwise.  *out is malloc'ed (the caller frees it).  0 with *reason for a truncated or malformed
 *                          segment length or a source without SOS.  Offsets inside copied segments (MPF and the like) are NOT fixed up.
 *   mjh_transcode_memory   the whole thing on the host: host walk, units, emit; flags MJW_OPTIMIZE_HUFFMAN and / or MJW_COPY_MARKERS.
 *                          *out is malloc'ed (the caller frees it); 0 with *reason for a picture that is undecodable, not transcodable
 *                          or not codable.
 *   mij_enc_tplan          the plan the GPU encoder holds for a slot made by mij_enc_add_coef, or for a pixel slot made with mij_enc_opts
 *                          (SAMPLED ENCODING, below); MIJ_E_ARG for any other slot
 */
typedef struct {
	mjw_plan plan;
	int ncomp, lh, lv; /* 1 or 3 components; luma sampling factors */
} mjw_tplan;
#define MJW_COPY_MARKERS 2u
int mjw_tplan_from_desc(mjw_tplan *t, const mij_image_desc *d, const char **reason);
size_t mjw_tplan_du_count(const mjw_tplan *t);
size_t mjw_theader(const mjw_tplan *t, unsigned char *out);
size_t mjw_theader_optimized(const mjw_tplan *t, const uint8_t bits[4][16], const uint8_t vals[4][256], unsigned char *out);
int mjw_units_from_region(const mij_image_desc *d, const uint8_t *region, int format, int16_t *du);
int mjw_tunits_codable(const mjw_tplan *t, const int16_t *du, const char **reason);
int mjw_temit(const mjw_tplan *t, const int16_t *du, mjw_write_func *func, void *context);
int mjw_temit_optimized(const mjw_tplan *t, const int16_t *du, mjw_write_func *func, void *context);
size_t mjw_temit_to_memory(const mjw_tplan *t, const int16_t *du, unsigned flags, unsigned char *out, size_t cap);
int mjw_copy_markers(const uint8_t *src, int src_len, const unsigned char *stream, size_t stream_len, unsigned char **out, size_t *out_len,
                     const char **reason);
int mjh_transcode_memory(const uint8_t *src, int len, unsigned flags, unsigned char **out, size_t *out_len, const char **reason);
int mij_enc_tplan(const mij_encoder *e, int slot, mjw_tplan *out);

/*
 * Lossless reorientation in the transcode (jpegtran -rotate / -flip / -transpose, exiftran -a): the eight EXIF orientations applied to the
 * coefficients, exactly, without decoding.  On the GPU: mij_enc_add_coef_oriented (mij.h); these calls are the written contract.
 *
 * NUMBERING.  Orientation o is 1..8 with the meaning mij.h gives it for mij_batch_set_out_tensor_oriented: the displayed picture D, in
 * numpy on the stored picture S, is  1: S   2: S[:, ::-1]   3: S[::-1, ::-1]   4: S[::-1]   5: S.T   6: S[::-1].T   7: S[::-1, ::-1].T
 * 8: S[:, ::-1].T -- mirrors of SOURCE axes first (x for o = 2, 3, 7, 8; y for o = 3, 4, 6, 7), then a transpose for o >= 5.
 *
 * BLOCK RULES, per component, u the horizontal and v the vertical frequency (in the planes' position order P = 8 * u + mij_rowslot[v],
 * i.e. unit coefficient k sits at u = mij_zigzag_pos[k] >> 3, mij_rowslot[v] = mij_zigzag_pos[k] & 7):
 *   mirror of source x   block column bx -> BW - 1 - bx, BW the component's block columns after the trim; the coefficient at (u, v) is
 *                        negated where u is odd
 *   mirror of source y   the same with rows, BH and v
 *   transpose            block (bx, by) -> (by, bx); coefficient (u, v) -> (v, u); luma factors (h, v) -> (v, h), so 4:2:2 and 4:4:0 swap
 *                        while 4:4:4, 4:2:0 and grey keep their kind; mcu_x and mcu_y swap; width and height swap; both quantisation
 *                        tables are transposed (Cb and Cr keep sharing theirs)
 * The destination's units are in the writer's unit order OF THE DESTINATION picture (above, with the destination's geometry); DC
 * differences, and so codability, are judged in that order.  AC codability does not depend on o.
 *
 * PARTIAL MCUS.  A mirrored source axis whose size is no multiple of the source's MCU size on that axis (8 * lh wide, 8 * lv high; 8 for
 * grey) cannot be mirrored exactly: its partial MCU would have to become the first.  trim = 0 (perfect) refuses such a picture with a
 * reason that names the axis, its size and the MCU size; trim = 1 drops the partial MCU column / row of the MIRRORED axes only
 * (jpegtran -trim): the size on that axis becomes the largest multiple of the MCU size, and a picture with nothing left is refused.  Axes
 * that are not mirrored keep their partial MCU, padding blocks included, exactly as the planes hold them.
 *
 *   mjw_tplan_oriented        the destination's plan from a source's; 0 with *reason (a static or per-thread string, valid until the
 *                             thread's next call) for o outside 1..8 and the refusals above.  o = 1 copies the plan.
 *   mjw_units_orient          the destination's units from the source's (mjw_units_from_region's order, of the src plan); du_dst holds
 *                             mjw_tplan_du_count(destination) units.  0 where mjw_tplan_oriented refuses.  mjw_temit* run unchanged on
 *                             the destination plan and units.
 *   mjw_transcode_memory_at   mjh_transcode_memory with o in 1..8 and an edge mode, the part that needs no EXIF code; copied markers are
 *                             the source's, untouched.  mjh_transcode_memory is this with (1, 0).
 *   mjh_transcode_memory_oriented   the whole thing: o = 0 means the file's own tag (mjh_exif_orientation).  When markers are copied and
 *                             o != 1, the Orientation entry mjh_exif_orientation reads is rewritten to 1 in the copied APP1
 *                             (mjh_exif_set_orientation): the coefficients are upright now, and a viewer would turn them again.  NOT fixed:
 *                             every other EXIF field (PixelXDimension / PixelYDimension, the thumbnail of IFD1 and its own tag) and offsets
 *                             inside other segments stay as the source has them.
 */
int mjw_tplan_oriented(mjw_tplan *dst, const mjw_tplan *src, int o, int trim, const char **reason);
int mjw_units_orient(const mjw_tplan *src, const int16_t *du_src, int o, int trim, int16_t *du_dst);
int mjw_transcode_memory_at(const uint8_t *src, int len, unsigned flags, int o, int trim, unsigned char **out, size_t *out_len,
                            const char **reason);
int mjh_transcode_memory_oriented(const uint8_t *src, int len, unsigned flags, int o, int trim, unsigned char **out, size_t *out_len,
                                  const char **reason);

/*
 * Requantisation in the transcode: new quantisation tables applied to the coefficients, without pixels -- one rounding per coefficient,
 * the sampling, geometry and markers untouched.  On the GPU: mij_enc_add_coef_requant (mij.h); these calls are the written contract.
 *
 * TABLES, all in zigzag order as mjw_plan.ytab / ctab are.  s_l, s_c: the tables of the plan that is requantised -- the ORIENTED plan
 * (mjw_tplan_oriented) when an orientation is applied too: the result is requant(orient(source)).  t_l, t_c: the target, every entry
 * 1..255.  The destination's tables are d = max(s, t) entry by entry when coarsen_only is set (a finer step restores nothing and only
 * grows the file), d = t otherwise.  Cb and Cr share d_c; grey uses d_l only (its plan keeps ctab = ytab).  A plan whose d equals s
 * everywhere is a plain lossless transcode: same units, same bytes.  What makes a source transcodable is judged on the source, as before.
 *
 * COEFFICIENTS.  Unit coefficient k of a component with source entry a = s[k] and destination entry b = d[k], source value c (int16, the
 * DC included, taken after the orientation's sign):
 *   x = c * a                               |x| <= 32768 * 255 < 2^23
 *   y = sgn(x) * ((|x| + (b >> 1)) / b)     integer division: round to nearest, halves away from zero
 *   y = clamp(y, -32767, 32767)             only so that a unit is an int16; such a unit is uncodable anyway
 * Codability (mjw_tunits_codable) is judged on y in the destination's unit order: an AC of 1500 at a = 1 is codable at b = 2, and with
 * coarsen_only off and b < a a codable source can become uncodable.
 *
 * STREAM: mjw_temit / mjw_temit_optimized of the destination plan -- the (oriented) plan with ytab / ctab replaced by d -- and units.
 *
 *   mjw_quality_tables      the pair mjw_plan_init makes at quality 1..100 (stbi_write_jpg's tables); 0 outside that range
 *   mjw_tplan_requant       dst = src with its tables replaced by d.  0 with *reason for a zero entry in any of the four tables; 1 when d
 *                           equals s everywhere; 2 when an entry changed
 *   mjw_units_requant       the rule above over every unit of src (the plan whose tables are s) into du_dst (the plan whose tables are d;
 *                           the two plans differ in their tables only), with plain `/`: the reference for the kernel.  0 on bad arguments
 *   mjw_requant_magic       the constants of the exact division the conversion kernel runs in place of `/`: returns m and sets *inc so
 *                           that n / b == (uint32_t)(((uint64_t)(n + inc) * m) >> 32) for every n < 2^24.  For b in 2..255
 *                           m = floor(2^32 / b) + 1 and inc = 0: the error n * (m * b - 2^32) <= 2^24 * 255 stays below 2^32.  For b = 1,
 *                           where that m would not fit 32 bits, m = 2^32 - 1 and inc = 1: (n + 1) * (2^32 - 1) >> 32 is n.  0 for b
 *                           outside 1..255.  The kernel's tables are filled by this function (inc is added with the rounding's b >> 1).
 *   mjw_transcode_memory_requant_at   mjw_transcode_memory_at, then the tables (luma and chroma both NULL: none), then the emission
 *   mjh_transcode_memory_requant      the whole thing on the host: orient (o = 0: the file's tag, as mjh_transcode_memory_oriented), then
 *                           requantise, then emit.  mjh_transcode_memory_oriented is this with no tables.
 */
int mjw_quality_tables(int quality, unsigned char luma[64], unsigned char chroma[64]);
int mjw_tplan_requant(mjw_tplan *dst, const mjw_tplan *src, const unsigned char luma[64], const unsigned char chroma[64], int coarsen_only,
                      const char **reason);
int mjw_units_requant(const mjw_tplan *src, const mjw_tplan *dst, const int16_t *du_src, int16_t *du_dst);
uint32_t mjw_requant_magic(int b, uint32_t *inc);
int mjw_transcode_memory_requant_at(const uint8_t *src, int len, unsigned flags, int o, int trim, const unsigned char *luma,
                                    const unsigned char *chroma, int coarsen_only, unsigned char **out, size_t *out_len, const char **reason);
int mjh_transcode_memory_requant(const uint8_t *src, int len, unsigned flags, int o, int trim, const unsigned char *luma,
                                 const unsigned char *chroma, int coarsen_only, unsigned char **out, size_t *out_len, const char **reason);

/*
 * Greyscale and crop in the transcode (jpegtran -grayscale, jpegtran -crop WxH+X+Y): which blocks go where; no coefficient value changes
 * and no pixel is made.  On the GPU: mij_enc_add_coef_window (mij.h); these calls are the written contract.  The steps run in a fixed
 * order, each plan-to-plan and units-to-units:   grey -> orient (edge mode) -> crop -> requantise -> emit
 *
 * GREY.  A three-component plan becomes a one-component plan of the same width and height: lh = lv = 1, mcu_x = ceil(W / 8),
 * mcu_y = ceil(H / 8), du_per_mcu = 1, ytab kept and ctab = ytab (the grey plan's convention).  Unit (bx, by) of the destination is luma
 * plane block (bx, by) of the source; the luma blocks beyond ceil(W / 8) x ceil(H / 8) -- the source's MCU padding -- are dropped.  A grey
 * source is copied.  Every later step sees a grey picture: the edge mode's MCU size and the crop's grid are 8 x 8, so a 4:2:0 picture
 * whose height is a multiple of 8 but not of 16 is mirrored exactly once it is grey.
 *
 * CROP.  In the frame of the plan it is given -- the displayed frame, after the orientation -- of size W x H and MCU size mw = 8 * lh,
 * mh = 8 * lv.  A window (x0, y0, w, h) is refused, with a reason that names the window and the picture's size, unless w >= 1, h >= 1,
 * x0 >= 0, y0 >= 0, x0 + w <= W and y0 + h <= H.  The kept rectangle is jpegtran's: the origin moves down to the MCU grid and the size
 * grows by what the origin moved, so the right and bottom edges stay where they were asked:  x0' = x0 - x0 % mw, W' = w + x0 % mw, the
 * same for y.  The destination has size W' x H', the same sampling and tables, mcu_x = ceil(W' / mw), mcu_y = ceil(H' / mh); its block
 * (bx, by) of component c is the source's block (bx + (x0' / mw) * h_c, by + (y0' / mh) * v_c): the window is shifted by whole MCUs, each
 * component by that many MCUs times its own factor.  A partial last MCU column or row takes the blocks the source planes hold there, as
 * jpegtran does.  A window that is the whole picture copies the plan and the units.
 *
 * Codability (mjw_tunits_codable) is judged on the final units in the destination's unit order: a DC's predecessor is the previous unit
 * of its component INSIDE the window, the first one's is 0 -- so a cut can make a codable source uncodable and the reverse.
 *
 * MARKERS with MJW_COPY_MARKERS are copied as before and the Orientation tag is reset when o != 1.  An Adobe APP14 on a now one-component
 * frame is left alone (a one-component frame takes no colour transform).  NOT fixed, as before: EXIF pixel dimensions and thumbnails.
 *
 *   mjw_tplan_grey      dst = the grey plan of src; 0 for a bad plan
 *   mjw_units_grey      the grey plan's units from src's; 0 on bad arguments
 *   mjw_tplan_cropped   dst = the plan of the kept rectangle, rect (may be NULL) = (x0', y0', W', H'); 0 with *reason (a per-thread string,
 *                       valid until the thread's next call) for a refused window
 *   mjw_units_crop      the units of the kept rectangle `rect` (as mjw_tplan_cropped returned it: origin on the MCU grid) from src's
 *   mjw_transcode_memory_window_at   the whole chain with o in 1..8; crop = (x0, y0, w, h) or NULL, grey 0 or 1; rect_out (may be NULL)
 *                       gets the kept rectangle, (0, 0, W, H) of the oriented picture without a crop.  mjw_transcode_memory_requant_at is
 *                       this with no crop and grey = 0.
 *   mjh_transcode_memory_window      the same with o = 0 meaning the file's own tag; mjh_transcode_memory_requant is this with no crop and
 *                       grey = 0, byte for byte what it was.
 */
int mjw_tplan_grey(mjw_tplan *dst, const mjw_tplan *src);
int mjw_units_grey(const mjw_tplan *src, const int16_t *du_src, int16_t *du_dst);
int mjw_tplan_cropped(mjw_tplan *dst, const mjw_tplan *src, int x0, int y0, int w, int h, int rect[4], const char **reason);
int mjw_units_crop(const mjw_tplan *src, const int16_t *du_src, const int rect[4], int16_t *du_dst);
int mjw_transcode_memory_window_at(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                   const unsigned char *chroma, int coarsen_only, unsigned char **out, size_t *out_len, int *rect_out,
                                   const char **reason);
int mjh_transcode_memory_window(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                const unsigned char *chroma, int coarsen_only, unsigned char **out, size_t *out_len, int *rect_out,
                                const char **reason);

/*
 * RESTART INTERVALS (jpegtran -restart N / -restart NB): every stream above is one unbroken entropy-coded segment unless an interval Ri is
 * asked for, 0..65535 MCUs; Ri = 0 means none and gives the calls above, byte for byte.
 *
 * DRI.  For Ri > 0 the segment FF DD 00 04 Ri_hi Ri_lo stands directly in front of SOS, behind DHT (where libjpeg puts it); nothing else of the
 * header changes, so a header is at most MJW_HEADER_RESTART_BYTES.
 * INTERVAL END.  After every Ri MCUs that are not the last MCUs of the scan the interval is filled exactly as the scan's end is: seven 1-bits
 * are appended and what remains below a byte is dropped; a completed 0xFF byte -- the filled one included -- is followed by a stuffed 0x00; then
 * comes the marker FF D0+(k mod 8), unstuffed, for interval k = 0, 1, ...  No marker follows the final interval, also when the MCU count is a
 * multiple of Ri.  Ri >= the MCU count gives the entropy bytes of Ri = 0 behind a header with a DRI segment.
 * PREDICTORS.  The DC prediction of every component restarts from 0 at each interval's first MCU, and what follows the predictors follows:
 * the histogram of the optimised tables counts the DC categories that are coded, and codability judges a DC difference against the restarted
 * predictor -- DC +1500 then -1500 in one component is uncodable in one segment and codable at Ri = 1; a unit run that is codable unbroken
 * can be uncodable with restarts (a DC beyond +-2047 reached in small steps, then predicted from 0).
 *
 *   mjw_restart_interval   Ri of a plan from an interval in MCU rows (rows x plan.mcu_x) or in MCUs; 0 with *reason (a static string) for
 *                          both given, a negative value, or a result above 65535.  (0, 0) is Ri = 0.
 *   mjw_[t]header[_optimized]_restart   the headers with the DRI segment; 0 for ri outside 0..65535
 *   mjw_[t]histogram_restart            mjw_histogram's counts with the restarted predictors, of a plan's or a transcode plan's units
 *   mjw_units_codable_restart, mjw_tunits_codable_restart   mjw_tunits_codable's ranges with the restarted predictors
 *   mjw_[t]emit_restart[_to_memory]     the stream; flags 0 or MJW_OPTIMIZE_HUFFMAN.  mjw_temit_restart returns 0 for units that are not
 *                          codable at this ri; MJW_STREAM_CAP holds any of these streams.
 *   mjw_transcode_memory_restart_at     mjw_transcode_memory_window_at with an interval in destination MCU rows or MCUs, resolved on the
 *                          destination plan (after grey, orientation and crop); *ri_out (may be NULL) gets the Ri used
 *   mjh_transcode_memory_restart        mjh_transcode_memory_window's arguments plus Ri in MCUs; _by: rows or MCUs, and *ri_out.  A source's
 *                          own DRI is never copied: MJW_COPY_MARKERS copies APPn and COM only.
 */
#define MJW_HEADER_RESTART_BYTES (MJW_HEADER_BYTES + 6)
int mjw_restart_interval(const mjw_tplan *t, int rows, int mcus, int *ri, const char **reason);
size_t mjw_header_restart(const mjw_plan *p, int ri, unsigned char *out);
size_t mjw_header_optimized_restart(const mjw_plan *p, const uint8_t bits[4][16], const uint8_t vals[4][256], int ri, unsigned char *out);
size_t mjw_theader_restart(const mjw_tplan *t, int ri, unsigned char *out);
size_t mjw_theader_optimized_restart(const mjw_tplan *t, const uint8_t bits[4][16], const uint8_t vals[4][256], int ri, unsigned char *out);
int mjw_histogram_restart(const mjw_plan *p, const int16_t *du, int ri, uint32_t freq[4][256]);
int mjw_thistogram_restart(const mjw_tplan *t, const int16_t *du, int ri, uint32_t freq[4][256]);
int mjw_units_codable_restart(const mjw_plan *p, const int16_t *du, int ri, const char **reason);
int mjw_tunits_codable_restart(const mjw_tplan *t, const int16_t *du, int ri, const char **reason);
int mjw_emit_restart(const mjw_plan *p, const int16_t *du, unsigned flags, int ri, mjw_write_func *func, void *context);
int mjw_temit_restart(const mjw_tplan *t, const int16_t *du, unsigned flags, int ri, mjw_write_func *func, void *context);
size_t mjw_emit_restart_to_memory(const mjw_plan *p, const int16_t *du, unsigned flags, int ri, unsigned char *out, size_t cap);
size_t mjw_temit_restart_to_memory(const mjw_tplan *t, const int16_t *du, unsigned flags, int ri, unsigned char *out, size_t cap);
int mjw_transcode_memory_restart_at(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                    const unsigned char *chroma, int coarsen_only, int restart_rows, int restart_mcus, unsigned char **out,
                                    size_t *out_len, int *rect_out, int *ri_out, const char **reason);
int mjh_transcode_memory_restart(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                 const unsigned char *chroma, int coarsen_only, unsigned char **out, size_t *out_len, int *rect_out, int ri,
                                 const char **reason);
int mjh_transcode_memory_restart_by(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                    const unsigned char *chroma, int coarsen_only, int restart_rows, int restart_mcus, unsigned char **out,
                                    size_t *out_len, int *rect_out, int *ri_out, const char **reason);

/*
 * PROGRESSIVE STREAMS (jpegtran -progressive): the same units, so the same coefficients to the bit, written as a multi-scan SOF2 stream whose
 * bytes are libjpeg's for those coefficients.  Restart intervals are not combined with it (libjpeg re-emits DRI per scan with a per-scan
 * interval): these calls take none.  Arbitrary scan scripts are not taken either.
 *
 * STREAM.  SOI, APP0 and DQT exactly as the plan's baseline stream has them; the frame header of that stream under marker FF C2; then the
 * scans of libjpeg's jpeg_simple_progression; EOI.  Every scan is: one DHT segment (FF C4, one table) per table the scan uses, SOS, its
 * entropy-coded segment, filled at its end as the baseline scan is (seven 1-bits, what remains below a byte dropped, 0xFF stuffed).
 * Notation `components: Ss-Se Ah Al`; components are 1 luma, 2 Cb, 3 Cr:
 *   three components, MJW_PROGRESSIVE_SCANS_COLOUR = 10 scans
 *      1,2,3: 0-0 0 1   interleaved, DC tables 0, 1, 1 (two DHT segments: id 0, then id 1)
 *      1: 1-5 0 2       3: 1-63 0 1      2: 1-63 0 1      1: 6-63 0 2      1: 1-63 2 1
 *      1,2,3: 0-0 1 0   no table
 *      3: 1-63 1 0      2: 1-63 1 0      1: 1-63 1 0      (Cr before Cb in both chroma pairs)
 *   grey, MJW_PROGRESSIVE_SCANS_GREY = 6 scans:   0-0 0 1,  1-5 0 2,  6-63 0 2,  1-63 2 1,  0-0 1 0,  1-63 1 0
 * Every AC scan carries one DHT segment of class 1: id 0 for luma, id 1 for chroma.  In SOS a component's table byte names its DC table only
 * in the first DC scan and its AC table only in AC scans; the rest is 0.
 * TABLES.  Each table is mjw_optimal_table of the counts of the symbols that scan codes with it (Cb and Cr add into DC table 1), the pending
 * run's EOBn at the scan's end included.  There is no plain-table fallback: no Annex-K table has EOBn codes, so where mjw_optimal_table
 * refuses (a code longer than 32 bits before limiting) the call returns 0.
 *
 * SEMANTICS, libjpeg's jcphuff.c.  Unit coefficient k is zigzag k, so a band Ss..Se is unit[Ss..Se].
 *   DC, first scan      v = unit[0] >> Al, the ARITHMETIC shift (-1 >> 1 = -1); the difference against the previous v of the component in MCU
 *                       order (from 0) is coded as the baseline DC is: category symbol, then the category's bits.
 *   DC, refinement      one bit per unit: bit Al of unit[0] (of its two's complement), no symbol.
 *   DC scans            are interleaved: every unit of every MCU, padding units included, in the writer's unit order.
 *   AC scans            take one component and visit its ceil(w_i / 8) x ceil(h_i / 8) blocks in raster order -- w_i, h_i the component's own
 *                       size: the picture's for luma, ceil(W / lh) x ceil(H / lv) for chroma.  MCU padding blocks are not coded there.
 *   AC, first scan      a = |c| >> Al, shifted TOWARDS ZERO.  a == 0 counts into the zero run r.  Otherwise: the pending EOB run is flushed,
 *                       one 0xF0 per sixteen of r, then symbol (r << 4) + category(a) and category(a) bits: a, or ~a for c < 0.  A block whose
 *                       band ends in zeros (r > 0) adds one to EOBRUN.
 *   EOB RUNS            EOBRUN is folded across the blocks of the scan.  A flush writes symbol n << 4, n = floor(log2(EOBRUN)), then the low n
 *                       bits of EOBRUN, then the correction bits buffered behind the run.  It is flushed in front of the next coded symbol,
 *                       at the scan's end, and at once when it reaches 0x7FFF.
 *   AC, refinement      a = |c| >> Al.  a == 0: r grows.  a > 1 (already non-zero): its correction bit a & 1 is BUFFERED.  a == 1 (newly
 *                       non-zero): EOB run flushed, symbol (r << 4) + 1, one sign bit (1 for c > 0), then the buffered correction bits, r = 0.
 *                       While r > 15 and a newly non-zero coefficient still follows in the band: EOB run flushed, 0xF0, the buffered
 *                       correction bits, r -= 16 -- so correction bits stand behind the symbol that covers them: behind the first ZRL of a
 *                       run, otherwise behind symbol and sign.  A block that ends with r > 0 or with correction bits buffered adds one to
 *                       EOBRUN, and its trailing correction bits join the run's buffer.  The run is flushed at once when it reaches 0x7FFF
 *                       or when more than MJW_PROGRESSIVE_MAX_CORR_BITS - 64 + 1 = 937 correction bits are pending.
 *
 * CAPACITY.  MJW_PROGRESSIVE_STREAM_CAP(units) holds any such stream.  Per unit, every code at most 16 bits: the DC scans take at most
 * 16 + 11 and 1 bits.  A first AC scan takes at most 16 + 10 bits per coefficient position (a ZRL's 16 bits cover sixteen positions) and an
 * EOBn of at most 16 + 14; a refinement scan at most 16 + 1 per position and the same EOBn.  A luma unit lies in two first scans that share its
 * 63 positions and in two refinement scans: 28 + 63 * 26 + 2 * 30 + 2 * (63 * 17 + 30) = 3928 bits; a chroma unit in one of each: fewer.
 * 3928 bits are 491 bytes, every one of which may be a 0xFF that takes a stuffed zero: 982 <= 1024.  Outside the units: SOI .. SOF2 at most
 * 173 bytes, EOI 2, and per scan at most two DHT segments of 5 + 16 + 256 bytes, an SOS of 14 and a fill byte that may be stuffed:
 * 10 * (2 * 277 + 14 + 2) = 5700.  So 6144 + 1024 per unit.
 *
 *   mjw_[t]emit_progressive[_to_memory]   the stream of a plan's (transcode plan's) units; 0 on bad arguments, for units outside
 *                          mjw_tunits_codable's ranges (judged as for the baseline stream; the shifted DC differences are no larger), where
 *                          a table cannot be built, or when cap is too small
 *   mjw_tprogressive_stats what the writer met on the way, without writing: how often a run was flushed for its length or for its pending bits,
 *                          the longest run and the most correction bits a flush carried.  GPU emission (mij_enc_set_progressive, mij.h) hands
 *                          slots with a forced flush to this writer; the tests hold their inputs against these counters.
 *   mjw_transcode_memory_progressive_at   mjw_transcode_memory_window_at with the request: progressive 0 is that call byte for byte, 1 emits
 *                          the destination's units (after grey, orientation, crop and requantisation) with mjw_temit_progressive;
 *                          MJW_OPTIMIZE_HUFFMAN is implied, MJW_COPY_MARKERS works as before.  Any other value is refused.
 *   mjh_transcode_memory_progressive      the same with o = 0 meaning the file's own tag
 */
#define MJW_PROGRESSIVE_SCANS_COLOUR 10
#define MJW_PROGRESSIVE_SCANS_GREY 6
#define MJW_PROGRESSIVE_MAX_CORR_BITS 1000
#define MJW_PROGRESSIVE_STREAM_CAP(units) ((size_t)6144 + (size_t)(units) * 1024)
typedef struct {
	uint32_t forced_run_flushes; /* runs flushed because they reached 0x7FFF blocks */
	uint32_t forced_bit_flushes; /* runs flushed because more than 937 correction bits were pending */
	uint32_t longest_run;        /* blocks */
	uint32_t most_pending_bits;  /* correction bits one flush carried */
} mjw_progressive_stats;
int mjw_emit_progressive(const mjw_plan *p, const int16_t *du, mjw_write_func *func, void *context);
int mjw_temit_progressive(const mjw_tplan *t, const int16_t *du, mjw_write_func *func, void *context);
size_t mjw_emit_progressive_to_memory(const mjw_plan *p, const int16_t *du, unsigned char *out, size_t cap);
size_t mjw_temit_progressive_to_memory(const mjw_tplan *t, const int16_t *du, unsigned char *out, size_t cap);
int mjw_tprogressive_stats(const mjw_tplan *t, const int16_t *du, mjw_progressive_stats *st);
size_t mjw_tframe_progressive(const mjw_tplan *t, unsigned char *out); /* SOI .. SOF2 of the stream, at most 173 bytes; 0 for a bad plan */
int mjw_transcode_memory_progressive_at(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                        const unsigned char *chroma, int coarsen_only, int progressive, unsigned char **out, size_t *out_len,
                                        int *rect_out, const char **reason);
int mjh_transcode_memory_progressive(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                     const unsigned char *chroma, int coarsen_only, int progressive, unsigned char **out, size_t *out_len,
                                     int *rect_out, const char **reason);

/*
 * SAMPLED ENCODING: the pixel encoder with a chosen chroma subsampling, grey output and given quantisation tables (Pillow's, torchvision's
 * and nvJPEG's subsampling= / qtables=).  On the GPU: mij_enc_add_ex and its kin (mij.h); these calls are the written contract, and the GPU
 * gives the same data units bit for bit.
 *
 * SAMPLING: (ncomp, lh, lv), one of "444" (3,1,1), "422" (3,2,1), "440" (3,1,2), "420" (3,2,2), "grey" (1,1,1).  Chroma is always 1x1, the
 * MCU is 8*lh x 8*lv pixels, and the picture is extended to whole MCUs by repeating its last column and last row (the reference's edge rule,
 * codec/jpeg_write.c:294-296).  Unit order is mjw_tplan's (LOSSLESS TRANSCODE, above): the luma blocks of an MCU in raster order, then Cb, then
 * Cr -- 4:2:2 is Y0 Y1 Cb Cr, 4:4:0 is Ytop Ybottom Cb Cr, grey is one unit per MCU.
 *
 * ARITHMETIC: the channel rule (comp 1 and 2: r = g = b = grey; comp 4: alpha dropped), the colour expressions, the AAN fDCT and the quantiser
 * are mjw_transform_host's, the same float expressions in the same order, no fused multiply-add.  The chroma sample of one subsampled
 * position, from the converted floats of its pixels:
 *   4:2:0  (a + b + c + e) * 0.25f   top-left, top-right, bottom-left, bottom-right (codec/jpeg_write.c:317-318)
 *   4:2:2  (a + b) * 0.5f            left, right
 *   4:4:0  (t + b) * 0.5f            top, bottom
 * Grey computes Y only, from the staged r, g, b (equal for comp 1 and 2); it is allowed for every comp.
 *
 * TABLES: the pair `quality` gives (mjw_plan_init's), or a given (luma, chroma) pair of 64 entries 1..255 in zigzag order, mjw_quality_tables'
 * convention; the reciprocal tables are derived from them by mjw_plan_init's expression.  A grey stream carries the luma table only.
 *
 * STREAMS: mjw_temit*, mjw_temit_restart* and mjw_temit_progressive* of the plan and its units.  With no sampling and no tables given the
 * stream is stbi_write_jpg_to_func's byte for byte, and so is one whose sampling is the writer's own choice named explicitly ("420" up to
 * quality 90, "444" above).
 *
 *   mjw_splan_init      the plan: quality as mjw_plan_init takes it (0: 90); ncomp 0: the writer's own sampling for that quality (lh, lv
 *                       ignored); luma and chroma both NULL: the tables of the quality.  0 on bad arguments: mjw_plan_init's, a sampling
 *                       that is none of the five, one table without the other, a zero entry.  plan.subsample is 1 for (3,2,2) only,
 *                       plan.du_per_mcu 1, 3, 4 or 6, plan.comp the pixels' comp.
 *   mjw_stransform_host the units of the pixels (comp = t->plan.comp bytes each), mjw_tplan_du_count(t) of them
 *   mjh_write_jpg_sampled_to_memory   plan + transform + emit on the host: flags 0 or MJW_OPTIMIZE_HUFFMAN, restart_mcus 0 (none) .. 65535,
 *                       progressive 0 or 1 (not with an interval).  *out is malloc'ed (the caller frees it).  0 on bad arguments.
 */
int mjw_splan_init(mjw_tplan *t, int width, int height, int comp, int quality, int ncomp, int lh, int lv, const unsigned char *luma,
                   const unsigned char *chroma);
void mjw_stransform_host(const mjw_tplan *t, const void *pixels, int flip_vertically, int16_t *du);
int mjh_write_jpg_sampled_to_memory(const void *pixels, int width, int height, int comp, int quality, int ncomp, int lh, int lv,
                                    const unsigned char *luma, const unsigned char *chroma, int flip_vertically, unsigned flags, int restart_mcus,
                                    int progressive, unsigned char **out, size_t *out_len);

/*
 * PLANE ENCODING: the writer fed with Y, Cb and Cr samples as a producer holds them (I420, NV12 / NV21, 4:2:2, 4:4:4, packed YCbCr, grey) --
 * nvJPEG's nvjpegEncodeYUV, Pillow's "YCbCr" mode.  A JPEG's components are Y, Cb and Cr at their sampling factors, so this is SAMPLED
 * ENCODING with its first stage left out: no colour expression and no chroma mean; whatever subsampling the producer did is kept to the
 * sample.  On the GPU: mij_enc_add_planes and mij_enc_add_device_planes (mij.h); these calls are the written contract, and the GPU gives the
 * same data units bit for bit.
 *
 * PLAN: mjw_splan_init's plan for (ncomp, lh, lv), one of the five of SAMPLED ENCODING.  The sampling is REQUIRED: it is never derived from
 * the quality and never guessed from plane shapes (a picture one pixel wide makes "444" and "422" indistinguishable).  plan.comp is 3, or 1
 * for grey.  Tables as SAMPLED ENCODING has them.
 *
 * PLANES: Y is height x width; Cb and Cr are ceil(height / lv) x ceil(width / lh) each; grey has no Cb or Cr (their src must be NULL).
 * Sample (y, x) of a plane is the byte at src + y * row_pitch + x * x_pitch (mij_plane, mij.h; pitches in bytes), so NV12 (x_pitch 2 on one
 * interleaved plane: Cb at base, Cr at base + 1), NV21 (the same, swapped) and packed HWC YCbCr (x_pitch 3) are views, not formats.
 *
 * EDGE RULE: each plane is extended ON ITS OWN to whole blocks of its component -- 8 * mcu_x * lh luma columns and 8 * mcu_x chroma
 * columns, 8 * mcu_y * lv luma rows and 8 * mcu_y chroma rows -- by repeating that plane's last column and last row.  flip_vertically
 * reverses the rows of every plane.
 *
 * ARITHMETIC: the value that enters the fDCT for sample s is (float)s - 128.0f, which is exact; from there on mjw_transform_host's AAN
 * fDCT and quantiser, the same functions.  Unit order is mjw_tplan's.
 *
 * VIDEO RANGE (optional per call): with a conversion cv (mij_in_convert, mij.h; dtype MIJ_DT_U8; entry 0 for Y, 1 for Cb, 2 for Cr) a
 * sample first becomes u by mij_in_convert's contract applied to x = (float)s:
 *     t = fl32( fl32(x * scale[c]) + bias[c] )        two roundings, no fused multiply-add
 *     u = (uint8) rintf( fminf( fmaxf(t, 0.0f), 255.0f ) )
 * and u is what is level-shifted.  mjw_video_range fills cv for studio-range frames (Y 16..235, chroma 16..240) into JFIF's full range:
 * scale_y = float32(255/219), bias_y = float32(-16*255/219), scale_c = float32(255/224), bias_c = float32(128 - 128*255/224), each computed
 * in double and rounded once: 16 -> 0, 235 -> 255, chroma 128 -> 128, chroma 240 -> 255, values outside clamp.  Only the range is
 * converted: the colour MATRIX (BT.601 against BT.709) is not touched -- a decoder of the stream applies JFIF's BT.601 matrix.
 *
 *   mjw_pplan_init       mjw_splan_init with comp = ncomp and the sampling required: 0 also for ncomp 0
 *   mjw_ptransform_host  the units of the planes, mjw_tplan_du_count(t) of them; cv may be NULL.  0 on bad arguments: a plan that is not
 *                        mjw_pplan_init's, a missing plane, a chroma plane given for grey, a zero x_pitch, a scale or bias that is not finite
 *   mjh_write_jpg_planes_to_memory   plan + transform + mjw_temit* on the host; flags, restart_mcus and progressive as
 *                        mjh_write_jpg_sampled_to_memory takes them.  *out is malloc'ed (the caller frees it).  0 on bad arguments.
 * Out of scope: decoding to planes, 4:1:1 and other factors, samples wider than 8 bits, conversion between colour matrices.
 */
void mjw_video_range(mij_in_convert *cv);
int mjw_pplan_init(mjw_tplan *t, int width, int height, int quality, int ncomp, int lh, int lv, const unsigned char *luma,
                   const unsigned char *chroma);
int mjw_ptransform_host(const mjw_tplan *t, const mij_plane *planes, const mij_in_convert *cv, int flip_vertically, int16_t *du);
int mjh_write_jpg_planes_to_memory(const mij_plane *planes, int width, int height, int quality, int ncomp, int lh, int lv,
                                   const unsigned char *luma, const unsigned char *chroma, const mij_in_convert *cv, int flip_vertically,
                                   unsigned flags, int restart_mcus, int progressive, unsigned char **out, size_t *out_len);

/*
 * LIBJPEG ENCODING: the pixel and plane encoders with libjpeg's default compression arithmetic and libjpeg's framing of the header, so that
 * the file is what PIL.Image.save, torchvision.io.encode_jpeg and cv2.imencode (libjpeg-turbo) write, byte for byte.  On the GPU:
 * mij_enc_set_arith(e, slot, MIJ_ARITH_LIBJPEG) (mij.h); these calls are the written contract, tests/libjpeg_enc_model.py restates it in
 * numpy, and Pillow's files (tests/golden/libjpeg_pillow_enc.npz) are the judge: where a formula here and Pillow disagree, Pillow wins and
 * this text is corrected.  All arithmetic is integer (nothing leaves 32 bits) and every shift is arithmetic.  Only the pixel side and the
 * header differ from SAMPLED ENCODING: the emission behind the data units (plain, optimised, restart intervals, progressive) is the same.
 *
 * SERVED: uint8 pictures of 3 components (RGB) as "444" (3,1,1), "422" (3,2,1) or "420" (3,2,2), and pictures of 1 or 3 components as
 * "grey" (1,1,1).  REFUSED, never approximated: "440" (Pillow cannot write it: nothing judges it) and comp 2 and 4.  With no sampling given
 * (ncomp 0) the sampling is "420", libjpeg's default, whatever the quality.
 *
 * COLOUR (jccolor, 16 fraction bits; comp 1: r = g = b, which gives Y = the sample):
 *   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *   Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 *
 * EDGES.  The MCU is 8 lh x 8 lv pixels.  Columns: every component plane of pixels is extended by its last column to whole MCUs before
 * any chroma filter.  Luma rows: extended by the last pixel row.  Chroma rows -- NOT the rule of SAMPLED ENCODING -- : the pixel rows are
 * extended by the last row to a multiple of lv, filtered, and then the last SAMPLE row is repeated down to 8 mcu_y rows.  An 8 x 8 or
 * 160 x 120 4:2:0 picture therefore has below the picture a chroma row equal to the mean of its last two pixel rows, not the last row alone.
 *
 * CHROMA FILTER (jcsample), x the OUTPUT column:
 *   4:2:2  (a + b + (x & 1)) >> 1                left, right
 *   4:2:0  (a + b + c + d + 1 + (x & 1)) >> 2    the bias alternates 1, 2, 1, 2 along a row and starts at 1 in every row
 *
 * FORWARD DCT (jfdctint, ISLOW) on sample - 128, rows first, then columns; D(x, n) = (x + (1 << (n - 1))) >> n:
 *   t0=d0+d7 t7=d0-d7 t1=d1+d6 t6=d1-d6 t2=d2+d5 t5=d2-d5 t3=d3+d4 t4=d3-d4
 *   t10=t0+t3 t13=t0-t3 t11=t1+t2 t12=t1-t2
 *   rows:    o0=(t10+t11)<<2   o4=(t10-t11)<<2   n=11
 *   columns: o0=D(t10+t11,2)   o4=D(t10-t11,2)   n=15
 *   z1=(t12+t13)*4433   o2=D(z1+t13*6270,n)   o6=D(z1-t12*15137,n)
 *   z1=t4+t7 z2=t5+t6 z3=t4+t6 z4=t5+t7 z5=(z3+z4)*9633
 *   t4*=2446 t5*=16819 t6*=25172 t7*=12299 z1*=-7373 z2*=-20995 z3=z3*-16069+z5 z4=z4*-3196+z5
 *   o7=D(t4+z1+z3,n) o5=D(t5+z2+z4,n) o3=D(t6+z2+z3,n) o1=D(t7+z1+z4,n)
 * The result is the DCT scaled by 8; |o| <= 32768.
 *
 * QUANTISER, q the table entry: y = sign(x) * ((|x| + 4q) div 8q).  The division is one multiply-high: with m = floor(2^32 / 8q) + 1
 * (mjw_lj_quant_magic), (a * m) >> 32 == a div 8q for every a = |x| + 4q with |x| <= 32768 and q = 1..255 -- walked exhaustively by
 * tests/test_encode_libjpeg_host.py.
 *
 * DUMMY BLOCKS.  A luma block of an MCU that lies wholly outside the ceil(W/8) x ceil(H/8) blocks of the picture is not transformed: its AC
 * terms are 0 and its DC is the QUANTISED DC of the block before it -- in a real block row the block to its left; in a block row below the
 * picture, for every block of that row, the last block of the MCU's previous block row (which may itself be a right-edge dummy).  Chroma,
 * "444" and grey have no dummy blocks.
 *
 * TABLES: as SAMPLED ENCODING (the quality mapping is libjpeg's own, forced to 1..255), or a given pair.
 *
 * STREAM: SOI; APP0 JFIF 1.01, units 0, density 1 x 1, no thumbnail; one DQT segment PER TABLE (table 0 always, table 1 for three
 * components); SOF0 or SOF2 with component ids 1, 2, 3 and tables 0, 1, 1; one DHT segment PER TABLE in the order DC0, AC0, DC1, AC1
 * (grey: DC0, AC0); DRI, if any, directly before SOS; SOS, data, EOI.  That is mjw_theader*'s header with its DQT and its DHT segment split
 * (mjw_lj_reframe): 4 bytes more per table after the first, at most MJW_LJ_HEADER_BYTES.  A progressive stream's scans already carry one
 * DHT segment per table; only the DQT segment in front of SOF2 changes.
 *
 * PLANES (mjw_lj_ptransform_host): PLANE ENCODING's staging -- each plane extended on its own by its last column and row, no filter -- then
 * the forward DCT, quantiser and dummy blocks above.
 *
 *   mjw_lj_plan_init       mjw_splan_init under the rules of SERVED; 0 for what is refused
 *   mjw_lj_stage_host      pass 1: the pixels as planes of whole MCUs -- Y (8 lh mcu_x x 8 lv mcu_y), then Cb, then Cr (8 mcu_x x 8 mcu_y
 *                          each), mjw_lj_staged_bytes(t) bytes: colour, edges and the chroma filter
 *   mjw_lj_units_from_staged   pass 2: those planes -> the units in mjw_tplan order, dummy blocks included
 *   mjw_lj_transform_host  both; 0 on bad arguments or when memory runs out
 *   mjw_lj_theader_restart, mjw_lj_theader_optimized_restart, mjw_lj_tframe_progressive   the siblings of mjw_theader_restart,
 *                          mjw_theader_optimized_restart and mjw_tframe_progressive in libjpeg's framing
 *   mjh_write_jpg_libjpeg_to_memory   plan + transform + mjw_temit* + framing on the host; arguments as mjh_write_jpg_sampled_to_memory.
 *                          *out is malloc'ed (the caller frees it).  0 on bad arguments and for what is refused.
 * Out of scope: 4:4:0 and 4:1:1, alpha inputs, dpi / ICC / EXIF segments, input smoothing, the fast and float DCTs, trellis or mozjpeg
 * tables, arithmetic coding.
 */
#define MJW_LJ_HEADER_EXTRA 16 /* three more DHT segments and one more DQT segment */
#define MJW_LJ_HEADER_BYTES (MJW_HEADER_RESTART_BYTES + MJW_LJ_HEADER_EXTRA)
int mjw_lj_plan_init(mjw_tplan *t, int width, int height, int comp, int quality, int ncomp, int lh, int lv, const unsigned char *luma,
                     const unsigned char *chroma);
uint32_t mjw_lj_quant_magic(int q);
int mjw_lj_quantise(int x, int q);
void mjw_lj_quantise_all(int q, int32_t *out); /* out[x + 32768] = mjw_lj_quantise(x, q) for x = -32768 .. 32768 */
void mjw_lj_ycc(int r, int g, int b, unsigned char ycc[3]);
size_t mjw_lj_staged_bytes(const mjw_tplan *t);
int mjw_lj_stage_host(const mjw_tplan *t, const void *pixels, int flip_vertically, unsigned char *staged);
int mjw_lj_units_from_staged(const mjw_tplan *t, const unsigned char *staged, int16_t *du);
int mjw_lj_transform_host(const mjw_tplan *t, const void *pixels, int flip_vertically, int16_t *du);
int mjw_lj_ptransform_host(const mjw_tplan *t, const mij_plane *planes, const mij_in_convert *cv, int flip_vertically, int16_t *du);
size_t mjw_lj_reframe(const unsigned char *in, size_t len, unsigned char *out);
size_t mjw_lj_theader_restart(const mjw_tplan *t, int ri, unsigned char *out);
size_t mjw_lj_theader_optimized_restart(const mjw_tplan *t, const uint8_t bits[4][16], const uint8_t vals[4][256], int ri, unsigned char *out);
size_t mjw_lj_tframe_progressive(const mjw_tplan *t, unsigned char *out);
int mjh_write_jpg_libjpeg_to_memory(const void *pixels, int width, int height, int comp, int quality, int ncomp, int lh, int lv,
                                    const unsigned char *luma, const unsigned char *chroma, int flip_vertically, unsigned flags, int restart_mcus,
                                    int progressive, unsigned char **out, size_t *out_len);

/* The tables of stbi__ldr_to_hdr(common.c:391-424) for mij_batch_set_out_f32: lut[256*k + v] for channel k < n_out.  Colour
 * channels (all of them for odd n_out, all but the last for even n_out) get (float)(pow(v / 255.0f, gamma) * scale), the
 * alpha channel of n_out 2 and 4 gets v / 255.0f -- the reference's expressions, evaluated with libm's pow. */
void mjh_ldr_to_hdr_lut(int n_out, float gamma, float scale, float *lut);

/* One axis of the resized tensor output's contract (include/mij.h, mij_batch_set_out_tensor_resized): `in` samples to `out` with
 * filter MIJ_FILTER_*.  Returns ksize, the taps per output row of k, or MIJ_E_ARG (in or out outside 1..2^24, unknown filter).
 * When lo_n and k are non-NULL and cap >= out * ksize, also writes lo_n[2*o] = lo and lo_n[2*o+1] = n of output o and its fixed-point
 * taps at k[o*ksize .. o*ksize + n) (the rest of the row is zero); with a smaller cap nothing is written. */
int mjh_resize_coeffs(int in, int out, int filter, int32_t *lo_n, int32_t *k, size_t cap);

/* The EXIF Orientation (tag 0x0112) of a JPEG file in memory, 1..8 (include/mij.h, mij_batch_set_out_tensor_oriented); never fails:
 * whatever it cannot read gives 1.  Walks the marker segments from SOI by their lengths (0xFF fill bytes allowed before a marker),
 * stopping at SOS, EOI, a bad length or the end of the buffer.  Only the first APP1 whose payload starts with "Exif\0\0" counts: its
 * TIFF header (II*\0 or MM\0*) gives the byte order, and only IFD0 is read (IFD1, the thumbnail's, is not), for an entry of tag
 * 0x0112, type SHORT and count 1.  Every offset is checked against that segment, and a directory that does not fit it gives 1, as
 * does a value outside 1..8.  stbi_* and the rest of the library ignore the tag, as the reference does. */
int mjh_exif_orientation(const uint8_t *buf, int len);
/* Sets that entry: the same walk with the same bounds checks, then the entry's two value bytes are overwritten in place with `value`
 * (1..8) in the TIFF block's byte order.  1 when an entry was patched; 0, and the buffer untouched, where the walk finds no Orientation
 * entry of one SHORT (mjh_exif_orientation's "cannot read" cases) or value is outside 1..8.  Nothing else of the file changes. */
int mjh_exif_set_orientation(uint8_t *buf, int len, int value);

#ifdef __cplusplus
}
#endif

#endif /* MIJ_HOST_H */
