/*
 * mij.h -- C-ABI of the MI355X (gfx950) JPEG back end: "MI JPEG".
 *
 * This is the drop-in boundary for the reference's per-block / per-row kernel seam
 *     stbi__jpeg::idct_block_kernel        (codec/jpeg.c:83, called :1178 :1217 :1342)
 *     stbi__jpeg::resample_row_hv_2_kernel (codec/jpeg.c:85, called :2287/:2308)
 *     stbi__jpeg::YCbCr_to_RGB_kernel      (codec/jpeg.c:84, called :2338 :2357 :2369)
 * coarsened from "one block / one row per call" to "one batch of images per submit":
 * the host entropy decoder (the part of codec/jpeg.c:1155-1317 that stays on the CPU) writes
 * the *quantised* coefficients of every block straight into pinned staging memory owned by a
 * batch; one submit then runs, on the GPU, for every image of the batch
 *     de-quantisation   codec/jpeg.c:325,345,365 (baseline) / :1319-1324 (progressive)
 *     8x8 integer IDCT  codec/jpeg.c:615-679
 *     chroma upsample   codec/jpeg.c:1765-1840,1962-1971 chosen as :2280-2289, rows as :2301-2319
 *     colour + output   codec/jpeg.c:1976-2018 and the branches of :2320-2431
 * and leaves n_out*width*height interleaved bytes per image in device memory (fetch = D2H).
 *
 * Plain C: no HIP, C++ or torch types cross this boundary.  All functions return 0 on
 * success or a negative MIJ_E_* code; mij_last_error() gives a thread-local message.
 * A batch is owned by one host thread at a time; different batches may be driven from
 * different threads concurrently (each batch has its own HIP stream).
 */
#ifndef MIJ_H
#define MIJ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIJ_ABI_VERSION 1

enum {
	MIJ_OK = 0,
	MIJ_E_NODEVICE = -1, /* no usable HIP device / HIP runtime error at init */
	MIJ_E_ARG = -2,      /* bad argument or descriptor */
	MIJ_E_NOMEM = -3,    /* batch arenas exhausted or allocation failed */
	MIJ_E_HIP = -4,      /* HIP runtime error (message has the HIP string) */
	MIJ_E_STATE = -5     /* call out of order (e.g. fetch before submit) */
};

/* how the decoded components map to output pixels: the branches of codec/jpeg.c:2320-2431 */
enum {
	MIJ_COLOR_GREY = 0,  /* 1 component (or luma-only decode of YCbCr when n_out < 3, :2246) */
	MIJ_COLOR_YCBCR = 1, /* 3 components, stbi__YCbCr_to_RGB_row (:2338) */
	MIJ_COLOR_RGB = 2,   /* 3 components tagged RGB: copy (:2325-2335), luma via stbi__compute_y for n_out<3 (:2382-2395) */
	MIJ_COLOR_CMYK = 3,  /* 4 components, Adobe transform 0 (:2343-2354, :2396-2408) */
	MIJ_COLOR_YCCK = 4,  /* 4 components, Adobe transform 2 (:2355-2366, :2409-2417) */
	MIJ_COLOR_YCBCRA = 5 /* 4 components, other transform: YCbCr, 4th ignored (:2367-2370); n_out<3: luma (:2418-2430) */
};

/* descriptor flags */
#define MIJ_FLAG_WIDE_IDCT 1u /* host could not prove that every first-pass IDCT output fits int16:
                                 run the exact 32-bit second pass (see MIJ_BLOCK_L1_LIMIT) */
#define MIJ_FLAG_SKIP 2u      /* the host stage rejected this image after its slot was taken: upload and
                                 launch ignore the slot (its output is undefined) */
#define MIJ_FLAG_STAGED_COMPACT 4u /* the host stage wrote the slot's staging as COMPACT planes itself (mij_compact_offsets; the
                                      baseline Huffman walk does: mjh_decode_memory_fmt): upload copies them as they are, no pack */
#define MIJ_FLAG_HAS_ESCAPES 8u    /* ... and at least one block holds a coefficient beyond a byte: the escape region goes up too */
#define MIJ_FLAG_L1_ON_DEVICE 16u  /* a progressive file whose per-block L1 bound (MIJ_BLOCK_L1_LIMIT) the host did NOT compute: the pack
                                      kernel, which reads every coefficient of the int16 staging anyway, takes the maximum and
                                      mij_batch_upload raises MIJ_FLAG_WIDE_IDCT from it (one small copy back and a wait inside upload) */

/* per component geometry, exactly the reference's img_comp[] fields (codec/jpeg.c:48-62, :1624-1655) */
typedef struct {
	int32_t h, v;   /* sampling factors 1..4 */
	int32_t tq;     /* quantisation table index 0..3 */
	int32_t x, y;   /* effective size in samples (:1627-1628) */
	int32_t bw, bh; /* padded size in 8x8 blocks: w2/8, h2/8 (:1636-1637, = coeff_w, coeff_h :1649-1650) */
} mij_comp_desc;

typedef struct {
	int32_t width, height; /* img_x, img_y */
	int32_t ncomp;         /* components decoded by the entropy stage: 1, 3 or 4 */
	int32_t n_out;         /* output bytes per pixel, 1..4 (:2241) */
	int32_t color;         /* MIJ_COLOR_* */
	uint32_t flags;        /* MIJ_FLAG_* */
	int32_t h_max, v_max;  /* img_h_max, img_v_max (:1616-1617) */
	int32_t mcu_x, mcu_y;  /* img_mcu_x, img_mcu_y (:1621-1622) */
	mij_comp_desc comp[4];
	uint16_t dequant[4][64]; /* natural (de-zigzagged) order, as stored at codec/jpeg.c:1376 */
} mij_image_desc;

/*
 * Coefficient staging layout ("tile layout").  Per component the blocks are numbered
 * L = bx + by*bw (the reference's coefficient indexing, codec/jpeg.c:1252,:1296,:1340); 64
 * consecutive blocks form one 8 KiB tile, and inside a tile the 16-byte chunk c (0..7) of
 * block lane l (= L & 63) sits at byte (c*64 + l)*16, so a 64-lane wavefront that owns one
 * block per lane reads each chunk as one fully coalesced 1 KiB access.  Chunk c holds
 * column c of the block as the four int16 pairs (r0,r4) (r2,r6) (r1,r3) (r5,r7) -- the
 * operand pairs of the first (column) IDCT pass -- so coefficient (row,col) has in-block
 * position P = 8*col + mij_rowslot[row].
 *
 * mij_coef_index(L, P) is the int16 index of that coefficient inside its component plane;
 * mij_zigzag_pos[k] is P for the k-th coefficient in zigzag (bitstream) order.
 */
static const uint8_t mij_rowslot[8] = {0, 4, 2, 5, 1, 6, 3, 7};

static const uint8_t mij_zigzag_pos[64] = {
	/* P of natural index dezigzag[k]; natural = 8*row+col -> 8*col + rowslot[row] */
	0, 8, 4, 2, 12, 16, 24, 20,
	10, 5, 1, 13, 18, 28, 32, 40,
	36, 26, 21, 9, 6, 3, 14, 17,
	29, 34, 44, 48, 56, 52, 42, 37,
	25, 22, 11, 7, 15, 19, 30, 33,
	45, 50, 60, 58, 53, 41, 38, 27,
	23, 31, 35, 46, 49, 61, 57, 54,
	43, 39, 47, 51, 62, 59, 55, 63};

/*
 * Compact coefficient planes: the DEFAULT format of the coefficients in HBM (the staging above stays int16: the
 * host walk and the progressive scans read-modify-write it, and mij_batch_upload packs it on the device).  Per
 * component and 64-block tile: 4 KiB of low bytes in the same chunk order (chunk c of block lane l at byte
 * (c*64 + l)*8, eight bytes = column c in mij_rowslot order), then behind all tiles an int16 DC array (one entry
 * per block; the byte at in-block position 0 holds the block's flags instead) and 64 "escape" bytes per block in
 * position order P.  coefficient == sext8(low byte) + 256 * (int8)escape byte  (mod 2^16 -- all that
 * (short)(coef * dequant), codec/jpeg.c:325-365, depends on); the escape bytes of a block are only defined (and
 * only read) when bit 0 of its flags byte is set, i.e. when one of its coefficients lies outside -128..127.  The
 * reference's coefficients have up to 15 magnitude bits (codec/jpeg.c:250-265), so this is exact for every stream;
 * a typical q=90 photograph reads 4.1 KiB per tile instead of 8.
 */
#define MIJ_TILE_COMPACT_BYTES (4096 + 128 + 4096)
enum { MIJ_COEF_INT16 = 0, MIJ_COEF_COMPACT = 1 };

static inline size_t mij_coef_index(uint32_t L, uint32_t P)
{
	return ((size_t)(L >> 6) << 12) + ((size_t)(P >> 3) << 9) + ((size_t)(L & 63u) << 3) + (P & 7u);
}
/* int16 elements in the plane of a component with nblocks blocks (whole tiles) */
static inline size_t mij_plane_elems(uint32_t nblocks) { return ((size_t)(nblocks + 63u) >> 6) << 12; }

/* Where the compact planes of component `comp` lie inside an image's coefficient region (the same in pinned staging and in HBM),
 * in bytes from the region's start: first, for every component in turn, its low-byte tiles followed by its int16 DC array -- the
 * MAIN part, mij_compact_main_bytes() in all, which is all that has to cross PCIe for an image without escaped blocks -- then the
 * escape bytes of every component (64 per block, position order P).  n_tiles = whole 64-block tiles of the component. */
static inline size_t mij_comp_tiles(const mij_comp_desc *c) { return ((size_t)(c->bw * c->bh) + 63u) >> 6; }
static inline size_t mij_compact_main_bytes(const mij_image_desc *d)
{
	size_t t = 0;
	int c;
	for (c = 0; c < d->ncomp; ++c)
		t += mij_comp_tiles(&d->comp[c]) * (4096 + 128);
	return t;
}
/* bytes of an image's coefficient region: room for either format (= mij_image_coef_bytes) */
static inline size_t mij_image_region_bytes(const mij_image_desc *d)
{
	size_t t = 0;
	int c;
	for (c = 0; c < d->ncomp; ++c)
		t += mij_comp_tiles(&d->comp[c]) * MIJ_TILE_COMPACT_BYTES;
	return t;
}
static inline void mij_compact_offsets(const mij_image_desc *d, int comp, size_t *lo, size_t *dc, size_t *hi)
{
	size_t main = 0, esc = mij_compact_main_bytes(d);
	int c;
	for (c = 0; c < comp; ++c) {
		main += mij_comp_tiles(&d->comp[c]) * (4096 + 128);
		esc += mij_comp_tiles(&d->comp[c]) * 4096;
	}
	*lo = main;
	*dc = main + mij_comp_tiles(&d->comp[comp]) * 4096;
	*hi = esc;
}

/*
 * Fast/exact IDCT contract.  The second IDCT pass runs on packed int16 first-pass outputs
 * (v_dot2_i32_i16) when the host guarantees they fit; a sufficient condition is that for every
 * block the sum of |de-quantised coefficient| is <= MIJ_BLOCK_L1_LIMIT (max |weight| of the
 * first pass is 5683, so |sum| + 512 < 2^25 and (..)>>10 fits int16).  Otherwise the host sets
 * MIJ_FLAG_WIDE_IDCT and the kernel computes the second pass in full 32-bit (wrapping)
 * arithmetic, like the reference's int math on such streams.
 */
#define MIJ_BLOCK_L1_LIMIT 5903

typedef struct mij_ctx mij_ctx;     /* one per (process, device) */
typedef struct mij_batch mij_batch; /* staging + device arenas + one HIP stream */

const char *mij_last_error(void);
int mij_abi_version(void);
int mij_device_count(void);

/* device < 0: use the HIP current device.  Fails with MIJ_E_NODEVICE when no GPU is present. */
int mij_ctx_create(int device, mij_ctx **out);
void mij_ctx_destroy(mij_ctx *ctx);
int mij_ctx_device(const mij_ctx *ctx);
/* "gfx950", CU count, bytes of device memory -- for logs and the bench header */
int mij_ctx_info(const mij_ctx *ctx, char *arch, size_t arch_len, int *cu_count, size_t *total_mem);

/*
 * A batch holds up to max_images images.  stage_bytes = pinned host staging for coefficients
 * (0: none, images can then only be added as clones or filled on the device), coef_bytes /
 * out_bytes = device arenas.  mij_image_coef_bytes / mij_image_out_bytes give an image's needs.
 */
int mij_batch_create(mij_ctx *ctx, int max_images, size_t stage_bytes, size_t coef_bytes, size_t out_bytes, mij_batch **out);
void mij_batch_destroy(mij_batch *b);
int mij_batch_reset(mij_batch *b); /* forget all images; arenas are reused */

size_t mij_image_coef_bytes(const mij_image_desc *d); /* sum over components of whole tiles, MIJ_TILE_COMPACT_BYTES each: room for either format */
size_t mij_image_out_bytes(const mij_image_desc *d);  /* n_out*width*height, rounded up to 256 */

/* Adds an image; returns its slot (>= 0) or a negative error.  Its staging planes are zeroed. */
int mij_batch_add(mij_batch *b, const mij_image_desc *d);
/* The same without the clearing, for a caller that writes every element of the planes itself (mjh_decode_memory
 * clears them on its own thread: the batch front ends add all images up front, in order, on one thread). */
int mij_batch_add_uncleared(mij_batch *b, const mij_image_desc *d);
/* Adds an image that shares descriptor and coefficients with slot src but gets its own device
 * coefficient and output buffers (filled device-to-device at upload).  For benchmarks that need
 * many resident images from a few distinct inputs. */
int mij_batch_add_clone(mij_batch *b, int src_slot);
/* Pinned host plane of component c of a slot (tile layout, int16, zero-filled). */
int16_t *mij_batch_coef(mij_batch *b, int slot, int comp);
/* The slot's whole staging region (mij_image_coef_bytes of pinned host memory) for a host stage that writes COMPACT planes itself
 * (mij_compact_offsets) and then raises MIJ_FLAG_STAGED_COMPACT with mij_batch_set_flags; NULL for clones and slots without staging. */
uint8_t *mij_batch_stage_region(mij_batch *b, int slot, size_t *bytes);
/* MIJ_COEF_COMPACT / MIJ_COEF_INT16: the format host-staged planes get in HBM (a host stage asked for int16 planes stages int16) */
int mij_batch_coef_format(const mij_batch *b);
/* MIJ_FLAG_* of a slot as they stand (after mij_batch_upload: with MIJ_FLAG_WIDE_IDCT where the device found it, MIJ_FLAG_L1_ON_DEVICE cleared) */
uint32_t mij_batch_slot_flags(const mij_batch *b, int slot);
/* May be called after the entropy stage to raise flags it only knows late (e.g. WIDE_IDCT). */
int mij_batch_set_flags(mij_batch *b, int slot, uint32_t flags);

/* May be called after the entropy stage when a marker behind SOF changed the colour branch (the reference decides
 * is_rgb / CMYK / YCCK after the last marker, codec/jpeg.c:2244); the new mode must fit the slot's component count. */
int mij_batch_set_color(mij_batch *b, int slot, int color);

/* May be called after the entropy stage when DQT segments behind SOF changed the quantisation tables (the reference de-quantises a
 * baseline block with the table current at its scan and a progressive file with the last definition): takes comp[].tq and dequant
 * of *from, which must describe the slot's picture otherwise; clones already made of the slot take them too.  A caller that pairs
 * mij_batch_add with mjh_decode_memory compares the descriptor the walk returns with the one it added, as for flags and colour. */
int mij_batch_set_dequant(mij_batch *b, int slot, const mij_image_desc *from);

/* submit = upload + launch.  All asynchronous on the batch's stream; wait blocks. */
int mij_batch_upload(mij_batch *b); /* H2D of staged coefficients (+ D2D for clones) + descriptors */
int mij_batch_launch(mij_batch *b); /* the decode kernels over every image of the batch */
int mij_batch_submit(mij_batch *b);
int mij_batch_wait(mij_batch *b);

/* D2H of one image's pixels into dst (dst_bytes >= n_out*width*height); waits for the batch. */
int mij_batch_fetch(mij_batch *b, int slot, uint8_t *dst, size_t dst_bytes);
/* The whole output arena in one asynchronous D2H on the batch's stream (image `slot` starts at byte
 * mij_batch_out_offset(b, slot) of dst; mij_batch_out_bytes(b) in total); mij_batch_wait() completes it.
 * Full PCIe rate needs a pinned destination: mij_host_alloc / mij_host_free. */
int mij_batch_fetch_all_async(mij_batch *b, uint8_t *dst, size_t dst_bytes);
size_t mij_batch_out_offset(const mij_batch *b, int slot);
size_t mij_batch_out_bytes(const mij_batch *b);
void *mij_host_alloc(size_t bytes);
void mij_host_free(void *p);
/* Device address of an image's pixels (valid until reset/destroy) for device-resident consumers. */
void *mij_batch_device_out(mij_batch *b, int slot);
int mij_batch_image_count(const mij_batch *b);

/*
 * Measurement hooks (used by bench.py): HIP events recorded on the batch's own stream.
 * begin/end bracket whatever was enqueued between them; elapsed waits for the end event.
 */
int mij_batch_timer_begin(mij_batch *b);
int mij_batch_timer_end(mij_batch *b);
int mij_batch_timer_elapsed_ms(mij_batch *b, float *ms);
/* FNV-1a 64 of an image's output computed on the device copy (D2H + hash on host); for parity checks of big batches */
int mij_batch_hash_out(mij_batch *b, int slot, uint64_t *hash);

/* Parity of big batches without bringing the pixels to the host: *ndiff = number of 16-byte words in which the
 * device images of the slot pairs (sa[i], sb[i]) differ (same sizes required); e.g. every clone against its source. */
int mij_batch_diff_slots(mij_batch *b, const int *sa, const int *sb, int n, uint64_t *ndiff);

/* which kernel family the last upload chose for a slot: 0 none (skipped), 1 fused 4:2:0, 2 generic two-pass,
 * 3 fused 4:4:4, 4 fused 4:2:2, 5 fused grey, 6 fused 4:4:0, 7 fused 1x1 RGB-tagged / CMYK / YCCK, 8 reduced-size decode, 9 plane output,
 * 10 libjpeg arithmetic (mij_batch_set_arith) */
int mij_batch_slot_path(const mij_batch *b, int slot);
/* parity tests compare the kernel families: on = 1 sends every image of the batch down the two-pass path (IDCT to sample
 * planes, then resampling + colour; its pass 2 compiled per resampler where the layout allows), on = 2 also insists on
 * the run-time-general pass 2 (k_resample_color), on = 0 is the default choice */
int mij_batch_force_generic(mij_batch *b, int on);

/*
 * Reduced-size decode: a slot may ask, before upload, for its picture at 1/denom size (denom 1, 2, 4 or 8; 1 takes the request
 * back).  With N = 8 / denom every component is transformed by an N * h_max / h point row and an N * v_max / v point column inverse
 * DCT on the low coefficients of each block -- libjpeg's scale_denom, Pillow's draft mode -- so all components come out at one
 * resolution and nothing is upsampled; pixel (X, Y) takes sample (Y mod NV, X mod NH) of block (Y div NV, X div NH) of each
 * component.  Per block, exactly (32-bit wrapping arithmetic, arithmetic shifts; tests/scaled_model.py restates it in numpy):
 *     d[u][v] = (short)(coef * q)                                         u < NV, v < NH; nothing outside is read
 *     t[y][v] = (sum_u K_NV[y][u] * d[u][v] + 512) >> 10
 *     p[y][x] = clamp255((sum_v K_NH[x][v] * t[y][v] + 65536 + (128 << 17)) >> 17)
 * K_8 is the reference's STBI__IDCT_1D, K_n[x][u] = rint(4096 * sqrt(2) * a(u) * cos((2x + 1) u pi / 2n)) below it (a(0) = 1 / sqrt(2),
 * else 1): K_1 = [4096], K_2 = [[4096, 4096], [4096, -4096]], K_4 has rows [4096, 5352, 4096, 2217], [4096, 2217, -4096, -5352],
 * [4096, -2217, -4096, 5352], [4096, -5352, 4096, -2217].  Colour and channel replication are the full-size path's.
 *
 * The stored picture of the slot is then mij_scaled_dim(width, denom) x mij_scaled_dim(height, denom), at the start of the output
 * region the slot got when it was added, with pitch n_out * that width; mij_batch_fetch, mij_batch_device_out, mij_batch_hash_out,
 * mij_batch_diff_slots and the three tensor requests (their windows and orientations included) all see that picture.  Set the scale
 * before the slot's tensor request: changing it under a request is MIJ_E_STATE.  Supported layouts: one component, and three-component
 * YCbCr whose luma has the picture's resolution with 4:4:4, 4:2:0 or 4:2:2 chroma (n_out 1 / 2: the luma alone).  MIJ_E_ARG for
 * another denominator, for any other layout with denom > 1 (4:4:0, 4:1:1, RGB-tagged, CMYK / YCCK: refused, not approximated) and for
 * a slot with a float request (mij_batch_set_out_f32 refuses a reduced slot in turn); MIJ_E_STATE after upload.  Asking again
 * replaces the request, mij_batch_reset forgets it, clones start at 1.  mij_batch_slot_path reports 8 for such a slot; a batch
 * without one launches exactly what it launches without this section.
 */
static inline int mij_scaled_dim(int v, int denom) { return (v + denom - 1) / denom; }
int mij_batch_set_scale(mij_batch *b, int slot, int denom);
/* the stored picture's size: the descriptor's, or the reduced one */
int mij_batch_slot_out_size(const mij_batch *b, int slot, int *w, int *h);

/*
 * LIBJPEG ARITHMETIC: a slot may ask, before upload, to be decoded with the arithmetic of libjpeg's default decode (libjpeg-turbo as
 * Pillow, torchvision and OpenCV use it: ISLOW inverse DCT, fancy upsampling, the jdcolor tables) instead of the reference's, so that its
 * pixels are those libraries' pixels byte for byte.  Nothing changes without the request: the stbi_* names and every other path keep the
 * reference's bytes, and a batch without a request plans and launches exactly what it does without this section.
 * THE CONTRACT (tests/libjpeg_model.py restates it in numpy).  Input: the slot's quantised coefficients c[u][v] and tables q[u][v] in
 * natural order.  All arithmetic is 32-bit two's-complement and wrapping; shifts are arithmetic.
 *   De-quantise: d = c * q, the 32-bit product (not the reference's (short)).
 *   Inverse DCT (jidctint.c: CONST_BITS 13, PASS1_BITS 2): the 1-D transform below on the eight columns with descale (x + 1024) >> 11
 *   into a 32-bit workspace, then on the eight workspace rows with descale (x + 131072) >> 18; sample = clamp(result + 128, 0, 255).
 *       z1 = (s2 + s6) * 4433;  t2 = z1 - s6 * 15137;  t3 = z1 + s2 * 6270
 *       t0 = (s0 + s4) << 13;   t1 = (s0 - s4) << 13
 *       e0 = t0 + t3; e3 = t0 - t3; e1 = t1 + t2; e2 = t1 - t2
 *       a = s7; b = s5; c = s3; d = s1
 *       z1 = a + d; z2 = b + c; z3 = a + c; z4 = b + d; z5 = (z3 + z4) * 9633
 *       a *= 2446; b *= 16819; c *= 25172; d *= 12299
 *       z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5
 *       a += z1 + z3; b += z2 + z4; c += z2 + z3; d += z1 + z4
 *       out = (e0 + d, e1 + c, e2 + b, e3 + a, e3 - a, e2 - b, e1 - c, e0 - d)
 *   libjpeg's zero-column and zero-row shortcuts give the same values.  The clamp is libjpeg-turbo's SIMD behaviour; libjpeg's C code
 *   wraps through a 1024-entry table beyond +-512 instead.  The two agree on every stream an encoder wrote.
 *   Planes: component c is ph_c x pw_c = ceil(H * v_c / v_max) x ceil(W * h_c / h_max) samples (mij_comp_desc.y / .x); samples of the
 *   padding blocks beyond that are never used as neighbours.
 *   Upsampling (jdsample.c, fancy); p is a chroma plane, row and column indices are clamped to [0, ph_c - 1] and [0, pw_c - 1]:
 *       4:2:2 (h2v1), per row:     out[2i] = (3 p[i] + p[i-1] + 1) >> 2,  out[2i+1] = (3 p[i] + p[i+1] + 2) >> 2
 *                                  (so out[0] = p[0] and out[2 pw_c - 1] = p[pw_c - 1])
 *       4:4:0 (h1v2), per column:  out[2j] = (3 p[j] + p[j-1] + 1) >> 2,  out[2j+1] = (3 p[j] + p[j+1] + 2) >> 2
 *       4:2:0 (h2v2):              s[2j] = 3 p[j] + p[j-1], s[2j+1] = 3 p[j] + p[j+1] down the columns, unshifted; then per row
 *                                  out[2i] = (3 s[i] + s[i-1] + 8) >> 4,  out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4
 *                                  (so out[0] = (4 s[0] + 8) >> 4 and out[2 pw_c - 1] = (4 s[pw_c - 1] + 7) >> 4)
 *   libjpeg's small-width rule: when pw_c <= 2, 4:2:2 and 4:2:0 are not filtered at all: every chroma sample is replicated 2 x 1 or
 *   2 x 2.  4:4:0 has no such rule.  The result is cut to W x H.
 *   Colour (jdcolor.c, SCALEBITS 16), with cb -= 128 and cr -= 128:
 *       R = clamp(Y + ((91881 cr + 32768) >> 16))
 *       G = clamp(Y + ((-22554 cb - 46802 cr + 32768) >> 16))
 *       B = clamp(Y + ((116130 cb + 32768) >> 16))
 *   Output channels: n_out 3: R, G, B; 4: R, G, B, 255; 1: Y alone (libjpeg's JCS_GRAYSCALE, Pillow's draft("L")); 2: Y, 255; a
 *   one-component file: its samples, replicated for n_out >= 3.
 * Served: one component, and three-component YCbCr (MIJ_COLOR_YCBCR; n_out < 3: its luma) whose luma has the picture's resolution with
 * 4:4:4, 4:2:2, 4:4:0 or 4:2:0 chroma; baseline or progressive; either coefficient-plane format; either front end.  Refused, not
 * approximated (MIJ_E_ARG): 4:1:1 and other sampling factors, RGB-tagged, CMYK and YCCK files, and a slot with mij_batch_set_scale above 1,
 * in either order of the two calls (libjpeg's reduced transforms are another contract).  Not promised: parity for truncated progressive
 * files, where libjpeg smooths blocks whose scans are missing.
 * mij_batch_set_arith: before mij_batch_upload (else MIJ_E_STATE); MIJ_E_STATE for a skipped slot; asking again replaces the request,
 * mij_batch_reset forgets it, clones start at MIJ_ARITH_STB.  A slot with a plane request refuses it, and such a slot refuses a plane
 * request (MIJ_E_STATE): plane output has the reference's samples.  mij_batch_slot_path reports 10; mij_batch_slot_work_items and
 * mij_batch_slot_kernel answer as for a two-pass slot (pass 2's items; *kind the family of k_lj_color by chroma subsampling, *variant
 * n_out - 1).  The stored picture lies where the slot's picture always lies, with the same pitch: mij_batch_fetch, mij_batch_device_out,
 * mij_batch_hash_out, mij_batch_diff_slots, the float request and the three tensor requests (windows, resize, orientations) see it
 * unchanged.  A region (mij_batch_set_roi) is accepted and the picture is decoded whole, as for two-pass layouts.  The kernels are
 * k_lj_idct and k_lj_color (mij_libjpeg_kernels.h); the sample planes between them live in the scratch arena of the two-pass path.
 */
enum { MIJ_ARITH_STB = 0, MIJ_ARITH_LIBJPEG = 1 };
int mij_batch_set_arith(mij_batch *b, int slot, int arith);

/*
 * Region of interest: a slot may carry, before upload, a rectangle (x0, y0, w, h) in pixels of its STORED picture -- the reduced one when
 * mij_batch_set_scale is in force, and before any orientation -- outside of which nothing needs to be decoded.  The Huffman walk and the
 * coefficient planes are the whole picture's; the saving is in everything behind them (transform, upsampling, colour, pixel stores).
 *   - Every pixel inside the rectangle is byte for byte what the slot holds without a region.
 *   - The decode writes only inside a DECODED RECTANGLE, which mij_batch_slot_roi_rect reports after upload (the whole picture for a slot
 *     without a region).  It contains the region.  Bytes of the slot's output region outside it are NOT WRITTEN AT ALL: they are
 *     unspecified -- whatever the arena held -- for mij_batch_fetch, mij_batch_fetch_all_async and mij_batch_device_out, which return
 *     the slot's region as it is.  mij_batch_hash_out and mij_batch_diff_slots refuse such a slot (MIJ_E_STATE).
 *   - The slot keeps its full output region and pitch: nothing moves, and tensor requests address pixels as before.
 *   - By kernel family (mij_batch_slot_path): 4:2:0, 4:4:0, grey, 4:4:4, RGB-tagged / CMYK / YCCK at 1x1 and the reduced-size decode skip
 *     rows and columns -- the decoded rectangle is the region rounded out to MCU boundaries (8 x 8 blocks for the 1x1 families) and
 *     clipped to the picture; the contract allows one MCU more on each side.  4:2:2 skips rows only: the decoded rectangle has the
 *     picture's width.  Two-pass layouts accept the region and decode the picture whole.  A region that needs every MCU is dropped:
 *     such a slot, and a batch without regions, launch exactly what they launch without this section.
 * mij_batch_set_roi: w == 0 && h == 0 takes the region back; a later call replaces it; mij_batch_reset forgets it; clones start without.
 * MIJ_E_ARG for an empty rectangle or one that leaves the stored picture and for a slot with a float request (mij_batch_set_out_f32
 * refuses a slot with a region in turn); MIJ_E_STATE after upload.
 * mij_batch_set_roi_auto(on): at upload the region becomes the slot's tensor request window mapped to the stored frame (orientations
 * folded in; for a resized request the window is its crop, which the filter taps never leave).  An explicit region wins over it.
 * Upload checks again, since region, scale and request may be set in any order: MIJ_E_ARG for a region outside the stored picture as
 * the scale in force makes it, and for a tensor request whose stored-frame window leaves an explicit region; MIJ_E_STATE for an
 * automatic region on a slot without a tensor request.
 */
int mij_batch_set_roi(mij_batch *b, int slot, int x0, int y0, int w, int h);
int mij_batch_set_roi_auto(mij_batch *b, int slot, int on);
/* the decoded rectangle (x0, y0, w, h in stored pixels) the last upload planned for the slot; MIJ_E_STATE before upload */
int mij_batch_slot_roi_rect(const mij_batch *b, int slot, int rect[4]);

/* ---- GPU entropy stage (experimental): the baseline Huffman walk itself on the GPU, for single-scan interleaved
 * baseline files, restart intervals included.  The host only parses headers and removes
 * the 0xFF00 byte stuffing (mjh_extract_scan, mij_host.h); coefficients never cross PCIe.  Any stream the GPU
 * walk does not like (invalid code, run past coefficient 63, early end, no convergence) is reported back and
 * must be re-done with the host walk, whose behaviour on malformed input is the reference's. ---- */
typedef struct { /* stbi__huffman without code[] (codec/jpeg.c:21-32) */
	uint8_t fast[512];
	uint8_t size[256];
	uint8_t values[256];
	uint32_t maxcode[18];
	int32_t delta[18];
} mjg_huff;

typedef struct {
	mij_image_desc desc;
	uint32_t nblocks, blocks_per_mcu;
	uint8_t blk_comp[12], blk_dx[12], blk_dy[12]; /* block inside the MCU -> component, block offset inside the MCU */
	uint8_t dc_tab[4], ac_tab[4];                 /* component -> index into huff[] (0..3 DC tables, 4..7 AC tables) */
	mjg_huff huff[8];
	uint16_t qz[4][64];                           /* per component, zigzag order */
	/* Restart intervals (DRI): every interval is walked on its own (DC prediction starts at 0 in each, codec/jpeg.c
	 * :1142-1153).  n_seg intervals of restart_mcus MCUs (the last one shorter); their unstuffed bytes lie at
	 * seg[k].off .. + seg[k].len of the stream buffer, 4-byte aligned and 32 zero bytes apart, where seg = the
	 * table of n_seg {uint32 off, uint32 len} pairs at byte seg_table_off of the same buffer.  n_seg == 0: no
	 * restart interval, the whole stream is one segment at offset 0. */
	uint32_t n_seg, restart_mcus, seg_table_off, reserved;
} mjg_scan;

/* pinned + device arenas for stream_bytes of unstuffed entropy data; once per batch.  Device memory: about 9 bytes per stream byte (the write
 * pass's record arena takes 8.1 of them; streams beyond about 1 GiB per batch fall back to a form that needs 64 bytes per block instead). */
int mij_batch_entropy_reserve(mij_batch *b, size_t stream_bytes);
/* pinned region where the caller writes streams (capacity as reserved; reset by mij_batch_reset) */
uint8_t *mij_batch_entropy_stage(mij_batch *b, size_t *capacity);
/* new slot whose coefficients the GPU walk will produce; stream = what mjh_extract_scan wrote (segments, each
 * followed by 32 zero bytes, and the segment table), 4-byte aligned inside the pinned region.  Returns the slot
 * or a negative code (MIJ_E_NOMEM also when the image has more restart intervals than the arena has room for). */
int mij_batch_add_stream(mij_batch *b, const mjg_scan *scan, uint8_t *stream, size_t stream_len); /* stream_len: everything mjh_extract_scan wrote, segment table included */
/* H2D of the streams, the five kernels, D2H of the verdicts; waits.  fallback[0..*n_fallback) = slots the host
 * walk must redo (mij_batch_fallback_prepare, then decode into mij_batch_coef as usual). */
int mij_batch_entropy_run(mij_batch *b, int *fallback, int cap, int *n_fallback);
/* The same in two halves: launch queues everything on the batch's stream and returns at once (the host can
 * parse the next batch's headers meanwhile), finish waits and reports. */
int mij_batch_entropy_launch(mij_batch *b);
int mij_batch_entropy_finish(mij_batch *b, int *fallback, int cap, int *n_fallback);
int mij_batch_fallback_prepare(mij_batch *b, int slot);
/* tests: the coefficient planes of a slot as they sit in HBM, after entropy_run or upload, always returned in the
 * int16 tile layout (compact planes are expanded on the host); dst_elems >= sum of mij_plane_elems */
int mij_batch_fetch_coef(mij_batch *b, int slot, int16_t *dst, size_t dst_elems);
/* tests: why the GPU walk handed a slot back -- the OR of the anomaly words of the slot's scans (one per restart interval) after
 * mij_batch_entropy_run / _finish.  0: kept.  1: a run past coefficient 63 or a bad code; 2: inconsistent chain (with 8); 4: the stream ends before the last
 * block; 8: no convergence; 16: data ran out inside a block; 32: a 0xff data byte behind the final bit position of the last segment;
 * 64: a restart interval ends a byte or more before its marker, or past it (k_es_dc).  Negative code for a slot the walk never had. */
int mij_batch_entropy_anomaly(mij_batch *b, int slot);
/* tests: how many work items the last upload put on the slot's own family list -- bands x column segments of the band kernels, one per 256
 * lane units of a windowed or reduced-size slot, one per 256 blocks of an unwindowed 1x1 slot, pass 2's row groups of a two-pass slot (its
 * pass-1 blocks and the pack kernel's tiles are not counted).  0 for a skipped slot; MIJ_E_STATE before upload, MIJ_E_ARG for a bad slot. */
int mij_batch_slot_work_items(const mij_batch *b, int slot);
/* tests: the kernel the last upload chose for a slot -- *kind the index of its family in the launch plan (the MK_* order of mij_runtime.hip:
 * which form of a band kernel, which pass 2 of the two-pass path), *variant the family's variant bits (4: four channels, 2: wide IDCT --
 * pass 2: YCbCr colour --, 1: compact planes), *segments the column segments per band (1 unless the row of MCUs is cut).  Any pointer may
 * be NULL.  *kind is -1 for a skipped slot; MIJ_E_STATE before upload, MIJ_E_ARG for a bad slot. */
int mij_batch_slot_kernel(const mij_batch *b, int slot, int *kind, int *variant, int *segments);
/* tests: 1 when the launch that decodes the slot runs the pipelined twin of its kernel (k_fused420p: compact planes without the wide IDCT, in a
 * list whose LDS leaves a CU three workgroups at most), 0 when the plain kernel; kind, variant and segments do not tell the two apart */
int mij_batch_slot_pipelined(const mij_batch *b, int slot);
/* tests: 1 when that launch runs k_fused420m, the pipelined twin whose phase B marches down its lanes' own strips: a pipelined list of which every
 * picture has rows of whole dwords (four channels, or a width that is a multiple of four) of at most 2048 pixels; 0 otherwise */
int mij_batch_slot_marched(const mij_batch *b, int slot);
/*
 * Row-extent table: library-internal state of a slot, beside its coefficient planes and not part of their format.  One byte per block
 * row, component after component (comp[c].bh bytes each): the largest extent class over the row's blocks -- 0 DC only, 1 non-zero
 * coefficients inside the top-left 2 x 2, 2 inside the 4 x 4, 3 anything, an escaped block, a stream that needs MIJ_FLAG_WIDE_IDCT, or
 * simply unknown.  Every slot starts as all 3, handing out its staging (mij_batch_stage_region, mij_batch_coef) makes it all 3 again,
 * and only a producer inside the library that saw every block of the slot's rows lowers entries, after it has written the staging
 * (csrc/mij_internal.h; not part of this interface): the host walk of the batch front ends (mjh_decode_batch*) does for baseline files.
 * mij_batch_upload sends the table with the slot and gives a clone its source's; the 4:2:0 / 4:4:0 band kernels fetch only the
 * coefficient chunks a row of that class can hold anything in (mij_kernels.h, "Row classes").  A table that claims less than the
 * planes hold changes pixels: staging written from outside keeps all 3.
 * tests: mij_batch_slot_row_classes copies the table the next upload sends (a clone's: its source's) into dst when cap allows and
 * returns its length.
 */
int mij_batch_slot_row_classes(const mij_batch *b, int slot, uint8_t *dst, size_t cap);
/* tests: the table as the last upload put it on the device for the band kernels, copied back from there: one byte per MCU row, bits 2c and
 * 2c+1 the largest class of component c's block rows in that MCU row (bits of components the picture does not have read 3); returns
 * mcu_y.  MIJ_E_STATE before upload. */
int mij_batch_fetch_row_classes_packed(mij_batch *b, int slot, uint8_t *dst, size_t cap);
/* The format new coefficient planes of this batch get in HBM: MIJ_COEF_COMPACT (default; environment
 * MIJ_COEF_FORMAT=int16 flips the default) or MIJ_COEF_INT16.  Applies to slots added or uploaded afterwards. */
int mij_batch_set_coef_format(mij_batch *b, int fmt);
/* 1 if the slot's coefficients sit in HBM as compact planes (after upload or the GPU walk) */
int mij_batch_slot_coef_bytes(const mij_batch *b, int slot);
/* number of escaped blocks of a slot (blocks holding a coefficient outside -128..127), read back from HBM; tests */
int mij_batch_slot_escapes(mij_batch *b, int slot);

/* Measurement only: the decode kernels transform a wavefront's 64 blocks with the cheapest IDCT that covers all of them
 * (class 0: DC only -- the reference's own shortcut, codec/jpeg.c:625-633, taken per block instead of per column; 1: non-zeros
 * inside the top-left 2x2; 2: inside the 4x4; 3: the full transform).  mij_batch_count_idct_classes(b, 1) after mij_batch_upload
 * clears the device counters and makes the batch's launches count wavefronts per class; mij_batch_idct_class_counts reads them
 * (out[class]); (b, 0) switches the counting off again.  Counting costs an atomic per wavefront: never on in timed launches. */
/* Measurement: milliseconds k_pack_c8 (int16 staging -> compact planes) took in the last mij_batch_upload, -1 when nothing was packed */
int mij_batch_pack_ms(mij_batch *b, float *ms);
int mij_batch_count_idct_classes(mij_batch *b, int on);
int mij_batch_idct_class_counts(mij_batch *b, uint64_t out[4]);
/* tests / tuning: synchronisation rounds the last entropy_run needed for its slowest image */
int mij_batch_entropy_rounds(const mij_batch *b);

/*
 * Float output (stbi_loadf*, codec-free consumers that want float pixels in HBM).  A slot may ask, before upload, for its
 * n_out*W*H bytes to be turned into as many floats by one 256-entry table per channel (byte i uses table i % n_out): a pass of
 * its own (k_out_f32) behind every decode kernel of the launch writes them into a separate device arena.  mjh_ldr_to_hdr_lut
 * (mij_host.h) builds the reference's stbi__ldr_to_hdr tables.  The slot's uint8 output stays valid and fetchable; a batch
 * without float requests launches exactly what it launches without this section.  mij_batch_reset forgets every request.
 */
size_t mij_image_out_f32_bytes(const mij_image_desc *d); /* 4*n_out*width*height, rounded up to 256 */
/* The float arena: bytes of device memory (grows only; MIJ_E_STATE while slots hold requests).  On MIJ_E_NOMEM the old arena is kept
 * when there was room to try beside it, else the batch is left with none (set_out_f32 then gives MIJ_E_ARG until a reserve succeeds). */
int mij_batch_out_f32_reserve(mij_batch *b, size_t bytes);
/* lut = n_out*256 floats, table of channel k at lut[256*k], copied.  Before mij_batch_upload (else MIJ_E_STATE); MIJ_E_STATE for a
 * skipped slot, MIJ_E_ARG when the arena has no room for mij_image_out_f32_bytes more.  Asking again replaces the tables. */
int mij_batch_set_out_f32(mij_batch *b, int slot, const float *lut);
/* D2H of a float slot's n_out*W*H floats (MIJ_E_STATE for a slot without float output or before launch); waits for the batch. */
int mij_batch_fetch_f32(mij_batch *b, int slot, float *dst, size_t dst_elems);
/* Device address of a float slot's floats (NULL for a slot without float output); valid until reset/destroy. */
void *mij_batch_device_out_f32(mij_batch *b, int slot);

/*
 * Tensor output (a PyTorch input pipeline, any consumer that wants the pixels in device memory it owns).  A slot may ask, before
 * upload, for a crop window [x0, x0+w) x [y0, y0+h) of its decoded picture to be written to `dst`, optionally flipped (flip_x
 * reverses columns, flip_y rows, inside the window; channel order is kept), each value v of channel c as table[c][v] in the output
 * element type.  C = n_out of the slot; pitches are in elements:
 *     MIJ_LAYOUT_HWC  element (y, x, c) at dst + y*row_pitch + x*C + c        (plane_pitch ignored)
 *     MIJ_LAYOUT_CHW  element (c, y, x) at dst + c*plane_pitch + y*row_pitch + x
 * A pass of its own (k_out_tensor) behind every decode kernel of the launch -- and behind the float pass -- writes exactly those
 * elements: row padding and whatever lies around them stay untouched.  The slot's uint8 output (and a float request of the same
 * slot) stays valid and fetchable; a batch without tensor requests launches exactly what it launches without this section.
 *
 * ORDERING: dst is written on the batch's stream during mij_batch_launch (mij_batch_submit).  Nothing orders that write against the
 * caller's other streams: make dst idle before the submit (e.g. synchronise the stream that last used it) and mij_batch_wait before
 * reading it.
 */
enum { MIJ_DT_U8 = 0, MIJ_DT_F16 = 1, MIJ_DT_BF16 = 2, MIJ_DT_F32 = 3 };
enum { MIJ_LAYOUT_HWC = 0, MIJ_LAYOUT_CHW = 1 };
typedef struct {
	void *dst;                      /* device memory on the batch's device, owned by the caller (e.g. a torch tensor's data_ptr()) */
	int32_t dtype, layout;          /* MIJ_DT_*, MIJ_LAYOUT_* */
	int32_t x0, y0, w, h;           /* crop window in the decoded picture */
	int32_t flip_x, flip_y;
	int64_t row_pitch, plane_pitch; /* elements; plane_pitch ignored for HWC */
} mij_out_tensor;
/* table = n_out*256 elements of dtype (the table of channel k at element 256*k), copied; NULL only for MIJ_DT_U8 (identity).
 * Before mij_batch_upload (else MIJ_E_STATE); MIJ_E_STATE for a skipped slot; asking again replaces the request; mij_batch_reset
 * forgets every request.  MIJ_E_ARG, checked on the host, when the window leaves the picture or w or h < 1, when a pitch lets rows
 * or planes overlap (HWC: row_pitch < w*C; CHW: row_pitch < w or plane_pitch < (h-1)*row_pitch + w; a pitch only counts where there
 * is more than one row or plane), when dst is not aligned to the element size, when dst is not device memory of the batch's device,
 * or when the written extent [dst, last element] is not inside the one allocation hipMemGetAddressRange reports for dst (a range that
 * cannot be determined is refused too).  A refused request leaves any earlier request of the slot in place. */
int mij_batch_set_out_tensor(mij_batch *b, int slot, const mij_out_tensor *t, const void *table);

/*
 * Resized tensor output: the crop window (t->x0, t->y0, t->w, t->h) resized to out_w x out_h, then flipped, looked up in the tables and
 * stored as mij_batch_set_out_tensor does.  The contract, exact and integer (Pillow's resampling of one 8-bit channel, crop first):
 * every channel is resized on its own with filter F -- box, bilinear, hamming, bicubic (a = -0.5) or lanczos (a = 3), supports
 * 0.5 / 1 / 1 / 2 / 3.  One axis with `in` samples and `out` outputs:
 *     scale = in / out (double);  fs = max(scale, 1);  support = F.support * fs;  ksize = 2 * ceil(support) + 1
 *     for o in 0..out-1:
 *         center = (o + 0.5) * scale
 *         lo = max((int)(center - support + 0.5), 0);  n = min((int)(center + support + 0.5), in) - lo
 *         w[t] = F((t + lo - center + 0.5) / fs) for t < n;  ww = sum of w[t] in order;  w[t] /= ww when ww != 0
 *         k[t] = (int)(w[t] * 2^22 + (w[t] < 0 ? -0.5 : 0.5))
 *         y[o] = clamp((2^21 + sum_t x[lo + t] * k[t]) >> 22, 0, 255)
 * The horizontal pass runs first over every row of the window (skipped when out_w == w) and gives a uint8 h x out_w image; the
 * vertical pass runs on that (skipped when out_h == h).  Taps never read outside the window.  flip_x / flip_y then reverse the
 * output's columns / rows.  Unlike Pillow, RGBA and grey+alpha pictures are not premultiplied: alpha is one more channel.
 * A resized request with out_w == w and out_h == h gives the plain request's bytes.
 */
enum { MIJ_FILTER_BOX = 0, MIJ_FILTER_BILINEAR = 1, MIJ_FILTER_HAMMING = 2, MIJ_FILTER_BICUBIC = 3, MIJ_FILTER_LANCZOS = 4 };
typedef struct {
	int32_t out_w, out_h; /* 1..16384 */
	int32_t filter;       /* MIJ_FILTER_* */
	int32_t reserved;     /* 0 */
} mij_out_resize;
/* t->w, t->h: the source window (inside the picture); pitches, alignment and the one-allocation check apply to the out_w x out_h
 * extent.  Otherwise the rules of mij_batch_set_out_tensor: before upload, not for a skipped slot, forgotten by reset, a refused
 * request keeps the earlier one.  A slot holds one tensor request: a plain and a resized request replace each other.  MIJ_E_ARG also
 * for an unknown filter, out_w or out_h outside 1..16384, a non-zero reserved, and for coefficients whose 32-bit sums could
 * overflow (255 * sum |k| + 2^21 >= 2^31; no such case is known). */
int mij_batch_set_out_tensor_resized(mij_batch *b, int slot, const mij_out_tensor *t, const mij_out_resize *r, const void *table);

/*
 * Oriented tensor output: the request above applied to the displayed picture D instead of the stored picture S (the decoded
 * H x W x C pixels of the slot).  Orientation o is 1..8, the EXIF / TIFF Orientation tag (mjh_exif_orientation reads it from a
 * file); in numpy on S:
 *     o   D                                   D's size (w x h)
 *     1   S                                   W x H
 *     2   S[:, ::-1]                          W x H
 *     3   S[::-1, ::-1]                       W x H
 *     4   S[::-1]                             W x H
 *     5   S.transpose(1, 0, 2)                H x W
 *     6   S[::-1].transpose(1, 0, 2)          H x W      (the usual portrait shot: rotate 90 degrees clockwise to display)
 *     7   S[::-1, ::-1].transpose(1, 0, 2)    H x W
 *     8   S[:, ::-1].transpose(1, 0, 2)       H x W
 * (PIL.ImageOps.exif_transpose for every o).  The request writes exactly what mij_batch_set_out_tensor (r NULL) or
 * mij_batch_set_out_tensor_resized (r given) writes when applied to D: the window (t->x0, t->y0, t->w, t->h) is in D's coordinates and
 * must lie inside D; the resize is the contract above run on D's window, horizontal pass first in D's frame; flip_x / flip_y, the
 * tables, the layout and the pitches are unchanged, the flips still reversing the final output.  The order is orient, crop, resize,
 * flip, table, store.  Two consequences: for o = 5..8 the first pass of a resize runs along S's columns, and for a mirroring o the
 * mirror comes before the resize (the coefficients are not mirror-symmetric, so resize(mirror(x)) may differ from mirror(resize(x))).
 * o = 1 is byte for byte the request of the existing setters.  Every rule of the two setters above holds (one tensor request per slot,
 * replaced when asked again, forgotten by reset, a refused request keeps the earlier one; pitches, alignment and the one-allocation
 * check apply to the output extent); MIJ_E_ARG also for o outside 1..8 and for a window outside D, one that fits S but not D included.
 * Orientations 2..4 run k_out_tensor / k_out_resize with the mirror folded into the window, the flips and the coefficients;
 * 5..8 run passes of their own (k_out_tensor_t, k_out_resize_t), launched only when such a request exists.
 */
int mij_batch_set_out_tensor_oriented(mij_batch *b, int slot, const mij_out_tensor *t, const mij_out_resize *r, int32_t orientation, const void *table);

/*
 * PLANE OUTPUT (the mirror image of mij_enc_add_device_planes): a slot may ask, before upload, for the samples of its stored
 * COMPONENTS -- the Y, Cb and Cr planes of a YCbCr file as they are coded, at their own resolutions -- in device memory the caller owns.
 * THE CONTRACT, for a picture of W x H whose component c has sampling factors (h_c, v_c) under (h_max, v_max):
 *   - plane c is pw_c x ph_c samples, pw_c = ceil(W * h_c / h_max), ph_c = ceil(H * v_c / v_max): mij_comp_desc.x / .y, the reference's
 *     img_comp[c].x / .y (4:2:0: ceil(W / 2) x ceil(H / 2) chroma, the shapes mij_enc_add_device_planes takes);
 *   - sample (x, y) of plane c is byte (x & 7, y & 7) of the reference's IDCT (codec/jpeg.c:615-679, the clamp included) of the
 *     de-quantised block (x >> 3, y >> 3) of that component;
 *   - nothing else is applied: no upsampling, no colour conversion, no CMYK inversion; the planes of an RGB-tagged, CMYK or YCCK file
 *     are its stored components, in the frame header's order.  Every file the decoder accepts is eligible, whatever its factors
 *     (4:1:1 included), baseline or progressive;
 *   - samples of padding blocks, and of columns or rows beyond pw_c x ph_c, do not exist and are never written.
 * Addressing: sample (y, x) of a component's window goes to dst + y * row_pitch + x * x_pitch (bytes; the convention of mij_plane).
 * NV12 is planes[1] = {p, pitch, 2}, planes[2] = {p + 1, pitch, 2}; NV21 swaps the two; packed YCbCr has x_pitch 3.  dst NULL: the
 * component is not wanted, and none of its blocks is transformed (luma only: a third of the blocks of a 4:4:4 file).
 * Window (x0, y0, w, h) in picture coordinates, all 0 for the whole picture: x0 * h_c must be a multiple of h_max and y0 * v_c of v_max
 * for every wanted component (x0 a multiple of h_max / h_c: 2 for 4:2:0 chroma); component c then receives
 *     [x0 * h_c / h_max, ceil((x0 + w) * h_c / h_max)) x [y0 * v_c / v_max, ceil((y0 + h) * v_c / v_max))
 * of its plane, which mij_batch_slot_plane_rect reports (x0, y0, w, h in the component's own samples; any time after the request).
 *
 * Rules, checked on the host: before mij_batch_upload (else MIJ_E_STATE); MIJ_E_STATE for a skipped slot; asking again replaces the
 * request, mij_batch_reset forgets it, a refused request keeps the earlier one.  MIJ_E_ARG for: a window that is empty, leaves the
 * picture or is off the grid above; no wanted component; a plane given for a component the file lacks; a pitch below 1; rows of one
 * plane that overlap (row_pitch < (w_c - 1) * x_pitch + 1 where the window has more than one row); dst that is not device memory of the
 * batch's device; a written extent [dst, last sample] not inside the one allocation hipMemGetAddressRange reports for dst; a non-zero
 * reserved.  Planes may interleave with each other (that is NV12); the library does not look for planes that overwrite each other.
 * A slot holds either a plane request or a float / tensor request: the second kind asked for is refused with MIJ_E_STATE.  With a
 * plane request mij_batch_set_scale above 1, mij_batch_set_roi (other than taking a region back) and mij_batch_set_roi_auto are refused
 * with MIJ_E_STATE, and a slot that has a scale or a region refuses the plane request likewise.
 *
 * A slot with a plane request launches no pixel kernel: k_planes_out (mij_planes_out_kernels.h; mij_batch_slot_path 9) writes the
 * planes and nothing else.  Its share of the output arena is not written; mij_batch_fetch, mij_batch_fetch_f32, mij_batch_hash_out and
 * mij_batch_diff_slots on it return MIJ_E_STATE; mij_batch_fetch_coef works; mij_batch_slot_work_items counts one item per 256 blocks
 * of each wanted component's window (components 1 and 2 of an NV12 / NV21 request count once: one lane transforms both).  A batch
 * without plane requests plans, uploads and launches exactly what it does without this section.  ORDERING as for tensor output.
 */
typedef struct {
	void *dst;                  /* NULL: this component is not wanted */
	int64_t row_pitch, x_pitch; /* bytes */
} mij_out_plane;
typedef struct {
	mij_out_plane planes[4]; /* in the frame header's component order */
	int32_t x0, y0, w, h;    /* window in picture coordinates; all 0: the whole picture */
	int32_t reserved[2];     /* 0 */
} mij_out_planes;
int mij_batch_set_out_planes(mij_batch *b, int slot, const mij_out_planes *p);
int mij_batch_slot_plane_rect(const mij_batch *b, int slot, int comp, int rect[4]);

/*
 * Encoder half (BASELINE config 5): the JPEG writer's colour transform, edge replication, 2x2
 * chroma mean, float AAN forward DCT and quantiser (codec/jpeg_write.c:24-74, :96-118, :283-352)
 * for a batch of images on the GPU.  Input: interleaved 8-bit pixels, comp 1..4 as passed to
 * stbi_write_jpg; output: int16[64] data units in zigzag order, MCU after MCU (4:2:0: Y00 Y01 Y10
 * Y11 U V; 4:4:4: Y U V), bit-identical to mjw_transform_host (mij_host.h), for the host's
 * Huffman stage (mjw_emit).  Algorithmic bytes per 1080p image: 6 220 800 read + 6 266 880 written.
 */
typedef struct mij_encoder mij_encoder;

int mij_enc_create(mij_ctx *ctx, int max_images, size_t pixel_bytes, size_t du_bytes, mij_encoder **out);
/* the same with pinned staging of its own size (mij_enc_create: stage_bytes = pixel_bytes); an encoder fed only by mij_enc_add_device
 * and mij_enc_add_units needs none (0) */
int mij_enc_create_ex(mij_ctx *ctx, int max_images, size_t stage_bytes, size_t pixel_bytes, size_t du_bytes, mij_encoder **out);
void mij_enc_destroy(mij_encoder *e);
int mij_enc_reset(mij_encoder *e);
/* copies the pixels into pinned staging; quality and 4:2:0/4:4:4 choice as stbi_write_jpg; returns the slot */
int mij_enc_add(mij_encoder *e, const void *pixels, int width, int height, int comp, int quality, int flip_vertically);
int mij_enc_add_clone(mij_encoder *e, int src_slot); /* own device buffers, same pixels (benchmarks) */
/* the same slot bookkeeping without the copy: the caller stages the pixels with mij_enc_stage_pixels(slot) before
 * mij_enc_upload (batch front ends fill the slots from several host threads at once, mij_write_jpg_batch) */
int mij_enc_add_uncopied(mij_encoder *e, int width, int height, int comp, int quality, int flip_vertically);
void *mij_enc_staging(mij_encoder *e, int slot);
/* Bytes one picture takes in the pixel arenas (pix_cap of mij_enc_create).  Every picture is staged as packed RGB with rows of whole MCU
 * columns (width rounded up to 16, or to 8 above quality 90): the last pixel of a row repeated -- codec/jpeg_write.c:294-296 -- and the
 * channels picked as the reference picks them (:276-279: grey and grey + alpha pictures become r = g = b = grey, RGBA loses its alpha), both
 * applied on the way in, so that the strip kernels take every width and every comp; rounded up to 256. */
size_t mij_enc_pixel_bytes(int width, int height, int comp, int quality);
/* Copies a picture (comp bytes per pixel, as passed to stbi_write_jpg) into the staging of a slot made by mij_enc_add_uncopied in that layout
 * (callable from several threads for different slots).  mij_enc_staging() returns the same memory: packed RGB, row pitch = padded width x 3. */
int mij_enc_stage_pixels(mij_encoder *e, int slot, const void *pixels);
/* every slot's data units into the encoder's pinned mirror with one device-to-host copy (waits for it); mij_enc_units(slot)
 * points into that mirror until the next mij_enc_fetch_all / mij_enc_destroy */
int mij_enc_fetch_all(mij_encoder *e);
int mij_enc_fetch_all_async(mij_encoder *e); /* queued behind the launch, no wait: mij_enc_wait before reading mij_enc_units */
const int16_t *mij_enc_units(const mij_encoder *e, int slot);
int mij_enc_upload(mij_encoder *e);
int mij_enc_launch(mij_encoder *e);
int mij_enc_wait(mij_encoder *e);
int mij_enc_force_generic(mij_encoder *e, int on); /* tests: per-unit kernels even where the fused 4:2:0 kernel applies; before upload.  Default
                                                     * slots only: a slot made with mij_enc_opts stays on its strip kernel */
/* D2H of a slot's data units (mcu_x*mcu_y*du_per_mcu*64 int16) */
int mij_enc_fetch(mij_encoder *e, int slot, int16_t *dst, size_t dst_elems);
int mij_enc_timer_begin(mij_encoder *e);
int mij_enc_timer_end(mij_encoder *e);
int mij_enc_timer_elapsed_ms(mij_encoder *e, float *ms);

/*
 * Huffman emission on the GPU.  With an emission arena reserved, mij_enc_launch also queues, behind the transform, the kernels
 * that turn every slot's data units into its complete stream -- exactly the bytes mjw_emit (mij_host.h) writes for those units:
 * headers, entropy-coded segment with 0xFF 0x00 stuffing, fill bits, EOI.  Only the streams come back to the host.
 *
 * The arena holds the streams, placed in slot order: slot i starts where slot i-1 ends.  A slot fits when its stream ends inside
 * the arena; the first slot that does not fit and every slot after it are not written at all (the kernels write nothing outside
 * the arena), but their lengths are still computed.  The data-unit arena is only read: mij_enc_fetch / mij_enc_fetch_all still
 * return every slot's units, so host mjw_emit can always finish a slot that did not fit.
 *
 * mij_enc_stream_reserve: before mij_enc_upload; bytes of device arena and of its pinned mirror (0 releases both).  Without an
 * arena the encoder queues exactly the launches and copies it queues without this section.
 * mij_enc_fetch_streams: waits for the launch, brings back the lengths and the used part of the arena (two copies) and returns
 * the number of slots that fit; MIJ_E_STATE without an arena or before mij_enc_launch.
 * mij_enc_stream: the slot's stream in the pinned mirror, valid until the next mij_enc_fetch_streams, mij_enc_reset or
 * mij_enc_destroy; *len (when len is not NULL) is the stream's length.  For a slot that did not fit: NULL, *len the length it needs,
 * and mij_last_error says so.
 */
int mij_enc_stream_reserve(mij_encoder *e, size_t bytes);
int mij_enc_fetch_streams(mij_encoder *e);
const unsigned char *mij_enc_stream(const mij_encoder *e, int slot, size_t *len);

/*
 * Encoder slots whose pixels are caller-owned device memory (the mirror image of tensor output).  uint8 elements; C = comp (1..4,
 * the meaning stbi_write_jpg gives comp); pitches in elements, addressed as mij_out_tensor addresses them:
 *     MIJ_LAYOUT_HWC  element (y, x, c) at src + y*row_pitch + x*comp + c        (plane_pitch ignored)
 *     MIJ_LAYOUT_CHW  element (c, y, x) at src + c*plane_pitch + y*row_pitch + x
 * The slot's stream (GPU emission, or mjw_emit of its units) equals stbi_write_jpg_to_func(width, height, comp, picture, quality)
 * for the picture those elements describe; with flip_vertically, what that call writes under stbi_flip_vertically_on_write(1).
 * At mij_enc_upload a gather kernel stages the pixels on the device in place of the host-to-device copy; the slot takes no pinned
 * staging, and mij_enc_add_clone of it works.  MIJ_E_ARG, checked on the host, for: an unknown layout; width, height, comp or
 * quality that mjw_plan_init refuses; pitches that let rows or planes overlap (HWC: row_pitch < width*comp; CHW: row_pitch <
 * width or plane_pitch < (height-1)*row_pitch + width; a pitch only counts where there is more than one row or plane); src not
 * device memory of the encoder's device; the read extent [src, last element] not inside the one allocation hipMemGetAddressRange
 * reports for src.
 *
 * ORDERING: src is read on the encoder's stream from mij_enc_upload until mij_enc_wait (or a fetch that waits).  Make it idle
 * before the upload (e.g. synchronise the stream that last wrote it) and leave it unchanged until the wait.
 */
typedef struct {
	const void *src;                /* device memory on the encoder's device, owned by the caller */
	int32_t layout;                 /* MIJ_LAYOUT_* */
	int32_t width, height, comp;
	int64_t row_pitch, plane_pitch; /* elements; plane_pitch ignored for HWC */
} mij_in_tensor;
int mij_enc_add_device(mij_encoder *e, const mij_in_tensor *t, int quality, int flip_vertically);

/*
 * Device-pixel slots whose elements are float16, bfloat16 or float32: the backward direction of tensor output.  The gather kernel
 * de-normalises every element on its way into the pixel arena.  THE CONTRACT, for element x of channel c, with the caller's
 * float32 scale[c] and bias[c]:
 *
 *     t = fl32( fl32(x) * scale[c] )      // x widened exactly: f16 and bf16 -> f32 lose nothing
 *     t = fl32( t + bias[c] )             // two roundings: NO fused multiply-add
 *     u = (uint8) rintf( fminf( fmaxf(t, 0.0f), 255.0f ) )   // round half to even; NaN -> 0, -Inf -> 0, +Inf -> 255
 *
 * The picture that is encoded is the uint8 picture of those u.  From there on the slot is an ordinary device-pixel slot: the comp
 * channel rule (grey and grey + alpha take channel 0 for r, g and b; alpha is never read as a colour), edge replication, flip,
 * mij_enc_add_clone, mij_enc_set_optimize, mij_enc_stream_reserve and mij_enc_fetch work on it unchanged, and its stream equals
 * stbi_write_jpg_to_func(width, height, comp, the picture of u, quality).  The kernels (k_enc_gather_float, one per dtype)
 * multiply and add with __fmul_rn and __fadd_rn, which the compiler cannot contract.  Subnormal float32 inputs and products may or
 * may not be flushed to zero; with |scale| < 2^100 that never changes u (such a product stays below 2^-26).  For tensors made by mij_batch_set_out_tensor's tables ((v/255 - mean)/std):
 * scale = 255*std and bias = 255*mean invert them exactly, for all three dtypes (tests/test_tensor_encode_float_host.py).
 *
 * t's pitches count elements of cv->dtype.  Every check of mij_enc_add_device applies, the read extent taken in bytes of the
 * element size.  MIJ_E_ARG also for: MIJ_DT_U8 (mij_enc_add_device's job) or an unknown dtype; src not aligned to its element
 * size; a scale or bias among the first comp entries that is not finite.  uint8 slots and float slots of one upload each get
 * their own gather launch (float slots one per dtype); an upload without a float slot queues exactly what it queued before.
 * ORDERING as for mij_enc_add_device.
 */
typedef struct {
	int32_t dtype; /* MIJ_DT_F16 | MIJ_DT_BF16 | MIJ_DT_F32 */
	float scale[4], bias[4];
} mij_in_convert;
int mij_enc_add_device_float(mij_encoder *e, const mij_in_tensor *t, const mij_in_convert *cv, int quality, int flip_vertically);

/*
 * Pixel slots with a chroma subsampling, grey output or quantisation tables of their own (mij_host.h, SAMPLED ENCODING, is the contract;
 * the units equal mjw_stransform_host's bit for bit).  (ncomp, lh, lv) is one of (3,1,1) 4:4:4, (3,2,1) 4:2:2, (3,1,2) 4:4:0, (3,2,2)
 * 4:2:0, (1,1,1) grey; ncomp 0 leaves the sampling to the quality as stbi_write_jpg does.  luma and chroma are 64 entries 1..255 each in
 * zigzag order (read during the call only), both NULL for the tables of the quality.  opts NULL or all zero: the call without _ex,
 * exactly.  MIJ_E_ARG for any other sampling, one table without the other and a zero entry.
 * A slot made with options keeps its plan as an mjw_tplan: mij_enc_tplan (mij_host.h) answers for it, its header is mjw_theader's
 * (one component and the luma tables only for grey), its rows are staged as whole MCU columns of ITS sampling (width rounded up to
 * 8 * lh: mij_enc_pixel_bytes_ex), its data-unit share is mjw_tplan_du_count, and a restart interval counts MCUs of its own MCU size.
 * mij_enc_set_optimize, mij_enc_set_restart, mij_enc_set_progressive, mij_enc_add_clone, emission and the fetches work on it unchanged.
 * 4:2:2, 4:4:0 and grey slots run k_encode422, k_encode440 and k_encode_grey; a 4:2:0 or 4:4:4 slot runs the kernel instance a default
 * slot of that shape runs, and with the writer's own sampling and no tables its stream is the default slot's byte for byte.
 * mij_enc_force_generic keeps its meaning for default slots; slots made with options stay on their strip kernels.
 */
typedef struct {
	int ncomp, lh, lv;                  /* 0, 0, 0: as the quality decides */
	const unsigned char *luma, *chroma; /* NULL, NULL: as the quality decides */
} mij_enc_opts;
int mij_enc_add_ex(mij_encoder *e, const void *pixels, int width, int height, int comp, int quality, int flip_vertically, const mij_enc_opts *opts);
int mij_enc_add_uncopied_ex(mij_encoder *e, int width, int height, int comp, int quality, int flip_vertically, const mij_enc_opts *opts);
int mij_enc_add_device_ex(mij_encoder *e, const mij_in_tensor *t, int quality, int flip_vertically, const mij_enc_opts *opts);
int mij_enc_add_device_float_ex(mij_encoder *e, const mij_in_tensor *t, const mij_in_convert *cv, int quality, int flip_vertically,
                                const mij_enc_opts *opts);
size_t mij_enc_pixel_bytes_ex(int width, int height, int comp, int quality, const mij_enc_opts *opts);

/*
 * Slots whose input is Y, Cb and Cr PLANES (mij_host.h, PLANE ENCODING, is the contract; the units equal mjw_ptransform_host's bit for
 * bit): frames of a video decoder (NV12, I420), 4:2:2 camera frames, the planes a model works in.  No colour conversion and no chroma
 * filter runs: the samples reach the stream as they lie.  Sample (y, x) of plane c is the byte at planes[c].src + y * row_pitch +
 * x * x_pitch; planes[0] is Y (height x width), planes[1] and [2] are Cb and Cr (ceil(height / lv) x ceil(width / lh)), both with
 * src NULL for grey.  opts.ncomp, lh, lv are REQUIRED (one of the five samplings of mij_enc_opts; never 0), its tables optional.
 * convert NULL: full-range samples; else dtype MIJ_DT_U8 and scale / bias [0] for Y, [1] for Cb, [2] for Cr (mjw_video_range fills it
 * for studio-range frames).
 * mij_enc_add_planes: host pointers, read during the call and staged in pinned memory.  mij_enc_add_device_planes: caller-owned device
 * memory; every check of mij_enc_add_device applies to each plane (device memory of this device, the read extent inside one
 * allocation, rows that do not overlap: row_pitch >= (w - 1) * x_pitch + 1 where the plane has more than one row), and its ORDERING rule.
 * At mij_enc_upload k_enc_gather_planes brings the planes of device slots into the slot's share of the pixel arena as planar rows padded
 * to whole MCUs of each component (mij_enc_plane_bytes), edge rule, flip, de-interleaving and range conversion applied; host slots are
 * staged in that layout by the call.  k_encode_planes<LH, LV> then makes the units; mij_enc_force_generic does not apply.  MIJ_E_ARG for:
 * a missing sampling, a chroma plane given for grey or missing otherwise, a zero or negative pitch, sizes mjw_plan_init refuses, a scale
 * or bias that is not finite.  Everything behind the units works unchanged: mij_enc_set_optimize, mij_enc_set_restart (in the slot's own
 * MCUs), mij_enc_set_progressive, mij_enc_add_clone, emission, the fetches, mij_enc_tplan.  Plane slots and pixel slots may share an
 * upload; an upload without a plane slot queues exactly what it queued before.
 */
typedef struct {
	const void *src;
	int64_t row_pitch, x_pitch; /* bytes */
} mij_plane;
typedef struct {
	mij_plane planes[3]; /* Y, Cb, Cr */
	int32_t width, height;
	mij_enc_opts opts;             /* sampling required */
	const mij_in_convert *convert; /* NULL: none */
	int32_t flip_vertically;
} mij_in_planes;
int mij_enc_add_planes(mij_encoder *e, const mij_in_planes *p, int quality);
int mij_enc_add_device_planes(mij_encoder *e, const mij_in_planes *p, int quality);
/* bytes a plane slot takes in the pixel arenas: (lh * lv + 2) * 64 * mcu_x * mcu_y (64 * mcu_x * mcu_y for grey), rounded up to 256 */
size_t mij_enc_plane_bytes(int width, int height, const mij_enc_opts *opts);

/* A slot whose quantised data units are given: mjw_plan_du_count * 64 int16 in zigzag order, MCU after MCU (copied).  No transform
 * runs for it; its units are uploaded and emitted.  MIJ_E_ARG when a DC difference (per component, in MCU order, from 0) leaves
 * -2047..2047 or an AC value leaves -1023..1023: those fall outside the writer's tables.  mij_enc_add_clone refuses such a slot. */
int mij_enc_add_units(mij_encoder *e, int width, int height, int comp, int quality, const int16_t *du);

/*
 * Optimised Huffman tables: a slot's stream with tables built from its own symbol statistics in place of the four Annex-K tables --
 * the bytes mjw_emit_optimized (mij_host.h) writes for the slot's units.  Only the DHT segment and the codes of the entropy-coded
 * segment differ from the plain stream; coefficients, MCU order, stuffing, fill bits and every other segment are the same.  With an
 * emission arena the counts (k_emit_hist) and the tables (k_emit_build, ITU-T T.81 K.2) are made on the GPU in front of the emission
 * kernels, for the optimised slots only; a launch without such a slot queues what it queued before.  Without an arena nothing new is
 * queued: finish such a slot with mjw_emit_optimized on its fetched units.
 *
 * mij_enc_set_optimize: for a slot of any kind (host pixels, device pixels, given units, clone), after it is added and before
 * mij_enc_upload; MIJ_E_STATE after the upload, MIJ_E_ARG for a bad slot or one whose unit count times 64 does not fit 32 bits (the
 * counts are uint32).  A clone inherits the request of the slot it is made from; mij_enc_reset forgets all requests.
 * mij_enc_slot_optimized: after mij_enc_fetch_streams (MIJ_E_STATE before): 1 when the slot's stream carries its own tables, 0 when
 * optimisation was not asked for it or the slot fell back to the plain tables (a code of more than 32 bits before K.2's shortening;
 * its stream is then mjw_emit's).  A slot that does not fit the arena still reports its exact length under its tables.
 */
int mij_enc_set_optimize(mij_encoder *e, int slot, int on);
int mij_enc_slot_optimized(const mij_encoder *e, int slot);

/*
 * Restart intervals: a slot's stream with a DRI segment and an RSTk marker after every restart_mcus MCUs (0..65535; 0: none, the
 * default) -- the bytes mjw_emit_restart / mjw_temit_restart (mij_host.h, RESTART INTERVALS) write for the slot's units at that
 * interval, plain or optimised.  With an emission arena the same launches write it: the slot's tile list is cut at the interval ends
 * (mij_emit_kernels.h), so a small interval means many small tiles.  A slot whose stream is finished on the host (no arena, or no room
 * in it) is finished with those host calls at mij_enc_slot_restart's interval: the same bytes.
 *
 * mij_enc_set_restart: for a slot of any kind, after it is added and before mij_enc_upload; MIJ_E_STATE after the upload, MIJ_E_ARG for
 * a bad slot, an interval outside 0..65535 and, for a slot of given units (mij_enc_add_units, which judged them unbroken), units whose DC
 * differences against the restarted predictors leave -2047..2047.  A coefficient slot's codability is judged against the restarted
 * predictors by the conversion kernel.  A clone inherits the interval of the slot it is made from; mij_enc_reset forgets all requests.
 * mij_enc_slot_restart: the slot's interval, or a negative code for a bad slot.
 */
int mij_enc_set_restart(mij_encoder *e, int slot, int restart_mcus);
int mij_enc_slot_restart(const mij_encoder *e, int slot);

/*
 * Progressive output (jpegtran -progressive): a slot's stream written as the multi-scan SOF2 stream of include/mij_host.h, PROGRESSIVE
 * STREAMS -- libjpeg's jpeg_simple_progression script, every scan under the optimal tables of its own symbols, libjpeg's bytes for the
 * slot's units.  With an emission arena the GPU writes it (mij_progressive_kernels.h): four launches in front of the emission's six over the
 * progressive tiles only, their number independent of the slots and the scans, and none without a progressive slot; a slot without the
 * request runs the code it ran before and gives the same bytes.  The request implies optimised tables (mij_enc_set_optimize adds nothing to
 * it, and mij_enc_slot_optimized reports 0: the tables are per scan).
 *
 * FORCED FLUSHES.  libjpeg flushes an end-of-band run early when it reaches 32767 blocks or when more than 937 correction bits are
 * pending.  Both are sequential decisions and do not run on the GPU: a slot in which one occurs, and a slot with a scan whose table K.2
 * cannot build (there are no plain tables with EOBn codes to fall back to), is reported as MIJ_ENC_SLOT_HOST_FLUSH by mij_enc_slot_status
 * (mij_enc_stream: NULL, length 0): finish it on the host from its units with mjw_emit_progressive / mjw_temit_progressive, which also
 * finish a progressive slot that had no room or no arena.  The bytes are the contract's either way.
 *
 * mij_enc_set_progressive: for a slot of any kind, after it is added and before mij_enc_upload; MIJ_E_STATE after the upload; MIJ_E_ARG
 * for a bad slot, for a slot with a restart interval (mij_enc_set_restart in turn refuses an interval on a progressive slot: libjpeg
 * re-emits DRI per scan, which is out of scope) and for one whose unit count times 64 does not fit 32 bits.  A clone inherits the request;
 * mij_enc_reset forgets all requests.
 * mij_enc_slot_progressive: 1 or 0, or a negative code for a bad slot.
 */
int mij_enc_set_progressive(mij_encoder *e, int slot, int on);
int mij_enc_slot_progressive(const mij_encoder *e, int slot);

/*
 * libjpeg's arithmetic for a slot: mij_batch_set_arith's counterpart on the writing side.  With MIJ_ARITH_LIBJPEG the slot's data units and
 * header are those of the section LIBJPEG ENCODING of mij_host.h -- jccolor's constants, jcsample's chroma filter with its edge rules, the
 * ISLOW forward DCT, libjpeg's quantiser and dummy-block DCs, a DQT and a DHT segment per table -- so that its stream is what Pillow,
 * torchvision and OpenCV (libjpeg-turbo) write for those pixels, byte for byte.  MIJ_ARITH_STB (the default) is the reference's writer.
 *
 * For pixel slots (host, device, device-float) and plane slots.  A pixel slot runs two kernels (mij_libjpeg_enc_kernels.h):
 * k_lj_enc_color<LH, LV, NC> turns its staged rows into whole-MCU planes of Y, Cb and Cr in a plane scratch the encoder owns and grows at
 * upload; k_lj_encode_planes<LH, LV, NC> makes the units.  A plane slot runs the second alone on its staged planes.  The slot keeps the
 * sampling it was added with -- a slot added without options has the writer's own choice for its quality, not libjpeg's "420" default;
 * name the sampling to be sure.  Optimised tables, restart intervals, progressive output, clones (which inherit the request), emission and
 * the fetches work unchanged; mij_enc_force_generic does not apply.  An encoder without a request queues exactly what it queued before.
 *
 * mij_enc_set_arith: after the slot is added and before mij_enc_upload: MIJ_E_STATE after the upload.  MIJ_E_ARG for a bad slot or
 * value and, with MIJ_ARITH_LIBJPEG, for a slot of given units or coefficient planes (nothing is transformed), a "440" slot (nothing
 * judges it) and pictures of 2 or 4 channels.  Asking again replaces the request; mij_enc_reset forgets all requests.
 * mij_enc_slot_arith: the slot's arithmetic, or a negative code for a bad slot.
 */
int mij_enc_set_arith(mij_encoder *e, int slot, int arith);
int mij_enc_slot_arith(const mij_encoder *e, int slot);
/* Measurement and tests: the work items the last mij_enc_upload queued for transform kernel `group` of the encoder's kernel table, in
 * launch order: 0..3 the per-unit pairs (4:4:4 luma, chroma; 4:2:0 luma, chroma), 4..8 the strip kernels of pixel slots (420, 444, 422,
 * 440, grey), 9..13 those of plane slots (444, 422, 440, 420, grey), 14..17 k_lj_enc_color (444, 422, 420, grey) and 18..21
 * k_lj_encode_planes (the same).  A group without items is not launched.  MIJ_E_ARG beyond MIJ_ENC_GROUPS, MIJ_E_STATE before upload. */
#define MIJ_ENC_GROUPS 22
int mij_enc_group_work(const mij_encoder *e, int group);

/*
 * Lossless transcode: an encoder slot whose data units are the QUANTISED coefficients of a decode batch's slot, taken from the batch's
 * coefficient planes in device memory -- a new slot kind beside given units.  The contract (which sources are transcodable, the unit
 * order, the stream) is written in mij_host.h (mjw_tplan); the slot's stream is what mjw_temit / mjw_temit_optimized write for
 * mjw_units_from_region of the slot's planes.
 *
 * mij_enc_add_coef: takes the batch slot's descriptor as it stands and makes the transcode plan.  MIJ_E_ARG, with the reason in
 * mij_last_error ("not transcodable: ..."), for a picture that is not transcodable, a slot flagged MIJ_FLAG_SKIP, a batch of another
 * context, and a batch that has not been uploaded since the slot was added (its planes are not in HBM yet: mij_batch_upload, which
 * launches no pixel kernel).  Reserves room in the unit arena (MIJ_E_NOMEM).  At mij_enc_upload a conversion kernel (k_coef_units: planes
 * to units, either plane format) is queued on the encoder's stream in place of a copy of units, behind an event recorded on the batch's
 * stream; the same pass decides whether the units are codable (AC in -1023..1023, DC differences in -2047..2047).  A slot that is not
 * is reported like one that does not fit the arena (mij_enc_stream: NULL, length 0) and is never packed by the emission kernels.
 * mij_enc_set_optimize, mij_enc_stream_reserve, mij_enc_fetch_streams, mij_enc_stream and mij_enc_fetch work on such a slot unchanged;
 * mij_enc_add_clone refuses it; mij_enc_plan gives its geometry only (use mij_enc_tplan, mij_host.h, and mjw_temit for its units).
 *
 * ORDERING: the batch's planes are read on the encoder's stream from mij_enc_upload until mij_enc_wait (or a fetch that waits).  The batch
 * must not be reset, uploaded again, walked again or destroyed until then.
 *
 * mij_enc_slot_status: after mij_enc_fetch_streams (MIJ_E_STATE before), for a slot of any kind: MIJ_ENC_SLOT_OK, MIJ_ENC_SLOT_NO_ROOM
 * (it did not fit the arena: finish it on the host from its units), MIJ_ENC_SLOT_UNCODABLE (never for slots that are not coefficient
 * slots) or MIJ_ENC_SLOT_HOST_FLUSH (a progressive slot the host finishes: mij_enc_set_progressive); mij_last_error says the same in words.
 * mij_enc_coef_ms: measurement: milliseconds the conversion kernels of the last mij_enc_upload took, -1 when there were none.
 *
 * mij_enc_add_coef_oriented: the same slot with one of the eight EXIF orientations applied to the coefficients on the way (lossless
 * rotate / flip / transpose; the numbering is mij_batch_set_out_tensor_oriented's, the rules and the two edge modes are written in
 * mij_host.h, mjw_tplan_oriented).  The conversion kernel permutes the blocks, transposes them and changes the signs; the slot's plan
 * (mij_enc_tplan), units (mij_enc_fetch) and stream are the DESTINATION picture's, and codability is judged in its unit order.  MIJ_E_ARG
 * with the host's reason ("not transformable: ...") for an orientation outside 1..8, for a picture with a partial MCU on a mirrored axis
 * when trim is 0, and for one with nothing left after the trim.  mij_enc_add_coef is this with (1, 0).
 *
 * mij_enc_add_coef_requant: the same slot with new quantisation tables as well: luma and chroma are the 64-entry target tables in zigzag
 * order, entries 1..255 (both NULL: none, which is mij_enc_add_coef_oriented exactly); coarsen_only takes the entry-wise maximum with the
 * source's.  The rule, the rounding and the order -- requant(orient(source)) -- are written in mij_host.h (mjw_tplan_requant,
 * mjw_units_requant).  The conversion kernel's requantising instances divide exactly by multiply-high constants from a per-slot table
 * (mjw_requant_magic) and judge codability on the RESULT; a slot whose tables do not change is a plain slot and takes the plain
 * instance.  mij_enc_tplan reports the destination plan, tables included, and mij_enc_fetch the requantised units, so a slot that
 * misses the arena is finished on the host as before.  MIJ_E_ARG ("not requantisable: ...") for a zero table entry.  One upload may
 * hold plain, oriented and requantising slots.  mij_enc_slot_requantized: 1 for a coefficient slot whose tables changed, 0 for a plain
 * one, MIJ_E_ARG for any other slot.
 *
 * mij_enc_add_coef_window: the same slot with jpegtran's -grayscale and -crop as well, in the order grey -> orient -> crop -> requantise
 * (the contract is mij_host.h's, mjw_tplan_grey and mjw_tplan_cropped).  grey != 0 drops Cb and Cr of a colour source: the destination
 * is a one-component picture whose MCU is 8 x 8, which the edge mode and the crop then see.  crop = (x0, y0, w, h) in the displayed
 * frame (after the orientation), or NULL; the kept rectangle -- the origin moved down to the MCU grid -- is written to rect_out (may be
 * NULL; (0, 0, W, H) of the destination without a crop) and mij_enc_slot_rect returns it later.  MIJ_E_ARG ("not croppable: ...") for a
 * window that does not lie inside the picture.  A slot with no crop (or the whole picture) and no grey (or a grey source) is a plain slot
 * and is converted by the instance that converted it before; every other one is a windowed slot: the conversion kernel's WIN instances
 * read, per component, only the 64-block plane tiles that hold a block of the kept rectangle, and no chroma tile for a grey
 * destination.  mij_enc_add_coef_requant is this with no crop and grey = 0.
 * mij_enc_slot_greyed: 1 for a coefficient slot whose chroma was dropped; mij_enc_slot_windowed: 1 for a windowed slot (crop or grey
 * changed the picture), 0 for a plain one; MIJ_E_ARG for any other slot.
 * mij_enc_coef_tiles: the number of plane tiles the last mij_enc_upload queued for conversion, over all its coefficient slots.
 */
enum { MIJ_ENC_SLOT_OK = 0, MIJ_ENC_SLOT_NO_ROOM = 1, MIJ_ENC_SLOT_UNCODABLE = 2, MIJ_ENC_SLOT_HOST_FLUSH = 3 };
int mij_enc_add_coef(mij_encoder *e, mij_batch *b, int slot);
int mij_enc_add_coef_oriented(mij_encoder *e, mij_batch *b, int slot, int orientation, int trim);
int mij_enc_add_coef_requant(mij_encoder *e, mij_batch *b, int slot, int orientation, int trim, const unsigned char *luma,
                             const unsigned char *chroma, int coarsen_only);
int mij_enc_add_coef_window(mij_encoder *e, mij_batch *b, int slot, int orientation, int trim, const int *crop, int grey, const unsigned char *luma,
                            const unsigned char *chroma, int coarsen_only, int *rect_out);
int mij_enc_slot_rect(const mij_encoder *e, int slot, int rect[4]);
int mij_enc_slot_greyed(const mij_encoder *e, int slot);
int mij_enc_slot_windowed(const mij_encoder *e, int slot);
int mij_enc_coef_tiles(const mij_encoder *e, uint32_t *tiles);
int mij_enc_slot_requantized(const mij_encoder *e, int slot);
int mij_enc_slot_status(const mij_encoder *e, int slot);
int mij_enc_coef_ms(mij_encoder *e, float *ms);

#ifdef __cplusplus
}
#endif

#endif /* MIJ_H */
