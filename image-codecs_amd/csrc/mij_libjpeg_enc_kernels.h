/*
 * mij_libjpeg_enc_kernels.h -- the two kernels of an encoder slot that asked for libjpeg's arithmetic (mij_enc_set_arith,
 * MIJ_ARITH_LIBJPEG; the contract is the section LIBJPEG ENCODING of include/mij_host.h, restated in numpy in
 * tests/libjpeg_enc_model.py):
 *     pass 1  k_lj_enc_color      staged packed-RGB rows -> colour (jccolor) -> chroma filter (jcsample) and both edge rules -> u8 planes
 *     pass 2  k_lj_encode_planes  planes -> ISLOW forward DCT (jfdctint) -> quantiser -> dummy-block DCs -> data units
 * The planes have the layout of a plane slot's staging (k_encode_planes): Y of 8 lh mcu_x x 8 lv mcu_y samples, then Cb, then Cr of
 * 8 mcu_x x 8 mcu_y each.  A pixel slot's lie in the encoder's plane scratch at LjEncSlot.off; a plane slot runs pass 2 alone, on the
 * planes its staging or gather left in the pixel arena.  All arithmetic is 32-bit integer and every offset into an arena is 64-bit.
 */
#ifndef MIJ_LIBJPEG_ENC_KERNELS_H
#define MIJ_LIBJPEG_ENC_KERNELS_H

#include "mij_kernels.h"

namespace mij {

/* one per slot of an encoder that has a libjpeg slot, indexed like EncImage; only libjpeg slots' entries are read */
struct LjEncSlot {
	uint64_t off;        /* the slot's planes in the plane scratch (pixel slots) */
	uint32_t from_pix;   /* a plane slot: pass 2 reads the pixel arena at EncImage.pix_off instead */
	uint32_t rw, rh;     /* ceil(width / 8), ceil(height / 8): the luma blocks that are not dummies */
	uint32_t srows;      /* ceil(height / lv): the chroma sample rows that come from pixel rows */
	uint32_t m[2][64];   /* the exact division by 8 q (mjw_lj_quant_magic), luma and chroma, natural order */
	uint32_t h[2][64];   /* 4 q: what the magnitude takes before the multiply-high */
};

/* ------------------------------------------------------------------ pass 1: colour, chroma filter, edges */

/* jccolor's three rows, 16 fraction bits.  Every product is below 2^24 in magnitude (a byte times a constant below 2^16), so the sums stay
 * far inside 32 bits. */
__device__ __forceinline__ uint32_t lj_y(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }
__device__ __forceinline__ uint32_t lj_cb(uint32_t r, uint32_t g, uint32_t b)
{
	return (uint32_t)((int)(32768u * b - 11059u * r - 21709u * g + (128u << 16) + 32767u) >> 16);
}
__device__ __forceinline__ uint32_t lj_cr(uint32_t r, uint32_t g, uint32_t b)
{
	return (uint32_t)((int)(32768u * r - 27439u * g - 5329u * b + (128u << 16) + 32767u) >> 16);
}

/* byte i of a run of dwords */
template <int N>
__device__ __forceinline__ uint32_t lj_byte(const uint32_t (&w)[N], int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

/* A work item is one row of cells of one slot; a lane owns a cell: 4 LH pixels across and LV rows down -- LV x LH dwords of Y and, NC == 3,
 * one dword each of Cb and Cr, all loaded and stored as aligned dwords (staged rows are whole MCU columns of packed RGB: 24 lh bytes a
 * MCU, so a cell's 12 LH bytes start on a dword).  Columns need no rule here: the staging repeated the last pixel into the padding, which
 * is the contract's "every plane extended by its last column before any filter".  Rows: cell row cy holds chroma sample row cy and luma
 * rows LV cy .. LV cy + LV - 1.  Below the last sample row (cy >= srows) the chroma is that of sample row srows - 1 again -- the repeated
 * SAMPLE row -- and the luma is the last pixel row, which is the last row that sample read. */
template <int LH, int LV, int NC>
__global__ __launch_bounds__(256) void k_lj_enc_color(const EncImage *__restrict__ imgs, const WorkIdct *__restrict__ work, const uint8_t *__restrict__ pix,
                                                      int16_t *__restrict__, const LjEncSlot *__restrict__ lj, uint8_t *__restrict__ scratch)
{
	constexpr int ND = 3 * LH; /* dwords of a cell's row: 4 LH pixels */
	const WorkIdct wk = work[blockIdx.x];
	const EncImage &im = imgs[wk.img];
	const LjEncSlot &L = lj[wk.img];
	const uint32_t cy = wk.first, srows = L.srows, height = (uint32_t)im.height;
	const uint32_t ccy = min(cy, srows - 1u); /* the sample row this cell row shows */
	const size_t in_pitch = (size_t)im.width * 3u;
	const size_t ypitch = (size_t)im.mcu_x * (8 * LH), cpitch = (size_t)im.mcu_x * 8;
	const size_t ybytes = ypitch * (size_t)im.mcu_y * (8 * LV), cbytes = cpitch * (size_t)im.mcu_y * 8;
	const uint32_t ncell = (uint32_t)im.mcu_x * 2u; /* cells across: 8 lh mcu_x / (4 lh) */
	const uint8_t *src = pix + im.pix_off;
	uint8_t *dst = scratch + L.off;
	size_t row_off[LV];
#pragma unroll
	for (int k = 0; k < LV; ++k) {
		const uint32_t r = min((uint32_t)LV * ccy + (uint32_t)k, height - 1u);
		row_off[k] = (size_t)(im.flip ? height - 1u - r : r) * in_pitch;
	}
	for (uint32_t cx = threadIdx.x; cx < ncell; cx += 256u) {
		uint32_t w[LV][ND];
#pragma unroll
		for (int k = 0; k < LV; ++k) {
			const uint32_t *p = reinterpret_cast<const uint32_t *>(src + row_off[k] + (size_t)cx * (12u * LH));
#pragma unroll
			for (int i = 0; i < ND; ++i)
				w[k][i] = p[i];
		}
		uint32_t yy[LV][LH] = {}, cb[LV][4 * LH], cr[LV][4 * LH];
#pragma unroll
		for (int k = 0; k < LV; ++k)
#pragma unroll
			for (int x = 0; x < 4 * LH; ++x) {
				const uint32_t r = lj_byte(w[k], 3 * x), g = lj_byte(w[k], 3 * x + 1), b = lj_byte(w[k], 3 * x + 2);
				yy[k][x >> 2] |= lj_y(r, g, b) << (8 * (x & 3));
				if (NC == 3) {
					cb[k][x] = lj_cb(r, g, b);
					cr[k][x] = lj_cr(r, g, b);
				}
			}
		/* luma row k of the cell row: its own pixel row, or below the last sample row the last pixel row, which row LV - 1 here is */
#pragma unroll
		for (int k = 0; k < LV; ++k) {
			uint32_t *o = reinterpret_cast<uint32_t *>(dst + ((size_t)cy * LV + (size_t)k) * ypitch + (size_t)cx * (4u * LH));
#pragma unroll
			for (int i = 0; i < LH; ++i)
				o[i] = cy < srows ? yy[k][i] : yy[LV - 1][i];
		}
		if (NC == 3) {
			uint32_t ob = 0, orr = 0;
#pragma unroll
			for (int x = 0; x < 4; ++x) { /* output column 4 cx + x: its bias bit is x & 1 */
				uint32_t sb, sr;
				if (LH == 1) {
					sb = cb[0][x], sr = cr[0][x];
				} else if (LV == 1) {
					sb = (cb[0][2 * x] + cb[0][2 * x + 1] + (uint32_t)(x & 1)) >> 1;
					sr = (cr[0][2 * x] + cr[0][2 * x + 1] + (uint32_t)(x & 1)) >> 1;
				} else {
					sb = (cb[0][2 * x] + cb[0][2 * x + 1] + cb[LV - 1][2 * x] + cb[LV - 1][2 * x + 1] + 1u + (uint32_t)(x & 1)) >> 2;
					sr = (cr[0][2 * x] + cr[0][2 * x + 1] + cr[LV - 1][2 * x] + cr[LV - 1][2 * x + 1] + 1u + (uint32_t)(x & 1)) >> 2;
				}
				ob |= sb << (8 * x);
				orr |= sr << (8 * x);
			}
			uint8_t *c0 = dst + ybytes + (size_t)cy * cpitch + (size_t)cx * 4u;
			*reinterpret_cast<uint32_t *>(c0) = ob;
			*reinterpret_cast<uint32_t *>(c0 + cbytes) = orr;
		}
	}
}

/* ------------------------------------------------------------------ pass 2: forward DCT, quantiser, dummy blocks */

__device__ __forceinline__ int lj_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

/* jfdctint.c's pass over eight values in place; FIRST (rows) scales up by 4, the second (columns) descales.  Inputs stay below 2^16 in
 * magnitude and constants below 2^15 (include/mij_host.h): plain 32-bit products, which cannot wrap. */
template <bool FIRST>
__device__ __forceinline__ void lj_fdct8(int &d0, int &d1, int &d2, int &d3, int &d4, int &d5, int &d6, int &d7)
{
	constexpr int n = FIRST ? 11 : 15;
	int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
	const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
	d0 = FIRST ? (t10 + t11) * 4 : lj_descale(t10 + t11, 2);
	d4 = FIRST ? (t10 - t11) * 4 : lj_descale(t10 - t11, 2);
	int z1 = (t12 + t13) * 4433;
	d2 = lj_descale(z1 + t13 * 6270, n);
	d6 = lj_descale(z1 - t12 * 15137, n);
	z1 = t4 + t7;
	int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
	const int z5 = (z3 + z4) * 9633;
	t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
	z1 *= -7373, z2 *= -20995;
	z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
	d7 = lj_descale(t4 + z1 + z3, n);
	d5 = lj_descale(t5 + z2 + z4, n);
	d3 = lj_descale(t6 + z2 + z3, n);
	d1 = lj_descale(t7 + z1 + z4, n);
}

/* sign(x) * ((|x| + 4q) div 8q): one multiply-high, no divide and no branch (h = 4q, m = mjw_lj_quant_magic(q)) */
__device__ __forceinline__ int lj_quantise(int x, uint32_t h, uint32_t m)
{
	const int s = x >> 31;
	const int y = (int)__umulhi((uint32_t)((x ^ s) - s) + h, m);
	return (y ^ s) - s;
}

/* k_encode_planes' strip: STRIP consecutive MCUs per workgroup, one lane per data unit, lanes ordered so that a wavefront reads whole
 * rows and is all luma or all chroma (the table sits behind one wave-uniform pointer), units staged in LDS in mjw_tplan order and stored
 * by enc_strip_store.  Between the two: the dummy luma units of the strip -- blocks wholly right of or below the picture's own blocks --
 * are rewritten in LDS, one lane per MCU walking its luma units in order, row by row: no AC, the DC of the unit before it in a real block
 * row, of the last unit of the MCU's previous block row in a row below the picture.  The rule is per MCU, so a strip that runs over the end
 * of an MCU row needs nothing more. */
template <int LH, int LV, int NC>
__global__ __launch_bounds__(MIJ_ENCP_NT(LH, LV, NC)) void k_lj_encode_planes(const EncImage *__restrict__ imgs, const WorkIdct *__restrict__ work,
                                                                             const uint8_t *__restrict__ pix, int16_t *__restrict__ du,
                                                                             const LjEncSlot *__restrict__ lj, uint8_t *__restrict__ scratch)
{
	constexpr int STRIP = MIJ_ENCP_STRIP(LH, LV, NC), DPM = MIJ_ENCP_DPM(LH, LV, NC), NT = MIJ_ENCP_NT(LH, LV, NC);
	constexpr int NL = STRIP * LH * LV; /* luma lanes */
	static_assert(NL % 64 == 0 && NT <= 256, "a wavefront is all luma or all chroma");
	constexpr int zz[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
									10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
	extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
	uint8_t *const sdu = lds; /* the staged data units */
	const WorkIdct wk = work[blockIdx.x];
	const EncImage &im = imgs[wk.img];
	const LjEncSlot &L = lj[wk.img];
	const int tid = threadIdx.x;
	const uint32_t nmcu = (uint32_t)(im.mcu_x * im.mcu_y);
	const uint32_t m0 = wk.first;
	const uint32_t cnt = min((uint32_t)STRIP, nmcu - m0);
	const bool chroma = NC == 3 && __builtin_amdgcn_readfirstlane(tid >> 6) >= NL / 64;

	const size_t ybytes = (size_t)im.mcu_x * (8 * LH) * (size_t)im.mcu_y * (8 * LV), cbytes = (size_t)im.mcu_x * 8 * (size_t)im.mcu_y * 8;
	uint32_t j, usub;
	size_t off, pitch;
	if (!chroma) {
		const uint32_t sy = (uint32_t)tid / (uint32_t)(STRIP * LH), i = (uint32_t)tid % (uint32_t)(STRIP * LH), bx = i % (uint32_t)LH;
		j = i / (uint32_t)LH;
		usub = sy * LH + bx;
		const uint32_t m = min(m0 + j, nmcu - 1u); /* MCUs past the last one read valid samples; their units are dropped */
		const uint32_t my = m / (uint32_t)im.mcu_x, mx = m - my * (uint32_t)im.mcu_x;
		pitch = (size_t)im.mcu_x * (8 * LH);
		off = ((size_t)my * (8 * LV) + sy * 8u) * pitch + ((size_t)mx * LH + bx) * 8u;
	} else {
		const uint32_t c = (uint32_t)(tid - NL) / (uint32_t)STRIP;
		j = (uint32_t)(tid - NL) % (uint32_t)STRIP;
		usub = LH * LV + c;
		const uint32_t m = min(m0 + j, nmcu - 1u);
		const uint32_t my = m / (uint32_t)im.mcu_x, mx = m - my * (uint32_t)im.mcu_x;
		pitch = (size_t)im.mcu_x * 8;
		off = ybytes + c * cbytes + (size_t)my * 8u * pitch + (size_t)mx * 8u;
	}
	const uint8_t *src = (L.from_pix ? pix + im.pix_off : scratch + L.off) + off;
	uint2 r[8];
#pragma unroll
	for (int y = 0; y < 8; ++y)
		r[y] = *reinterpret_cast<const uint2 *>(src + (size_t)y * pitch);
	int d[8][8];
#pragma unroll
	for (int y = 0; y < 8; ++y) {
#pragma unroll
		for (int x = 0; x < 8; ++x)
			d[y][x] = (int)(((x < 4 ? r[y].x : r[y].y) >> (8 * (x & 3))) & 0xffu) - 128;
		lj_fdct8<true>(d[y][0], d[y][1], d[y][2], d[y][3], d[y][4], d[y][5], d[y][6], d[y][7]);
	}
#pragma unroll
	for (int x = 0; x < 8; ++x)
		lj_fdct8<false>(d[0][x], d[1][x], d[2][x], d[3][x], d[4][x], d[5][x], d[6][x], d[7][x]);
	{
		const uint32_t *__restrict__ qm = L.m[chroma ? 1 : 0], *__restrict__ qh = L.h[chroma ? 1 : 0];
		int q[64]; /* zigzag order */
#pragma unroll
		for (int n = 0; n < 64; ++n)
			q[zz[n]] = lj_quantise(d[n >> 3][n & 7], qh[n], qm[n]);
		const int u = (int)(j * DPM + usub);
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			uint4 w;
			w.x = ((uint32_t)q[8 * k + 0] & 0xffffu) | (uint32_t)q[8 * k + 1] << 16;
			w.y = ((uint32_t)q[8 * k + 2] & 0xffffu) | (uint32_t)q[8 * k + 3] << 16;
			w.z = ((uint32_t)q[8 * k + 4] & 0xffffu) | (uint32_t)q[8 * k + 5] << 16;
			w.w = ((uint32_t)q[8 * k + 6] & 0xffffu) | (uint32_t)q[8 * k + 7] << 16;
			*reinterpret_cast<uint4 *>(sdu + enc_du_chunk(u, k)) = w;
		}
	}
	__syncthreads();
	if (LH * LV > 1) {
		if ((uint32_t)tid < cnt) { /* lane = MCU tid of the strip */
			const uint32_t m = m0 + (uint32_t)tid;
			const uint32_t my = m / (uint32_t)im.mcu_x, mx = m - my * (uint32_t)im.mcu_x;
#pragma unroll
			for (int sy = 0; sy < LV; ++sy)
#pragma unroll
				for (int sx = 0; sx < LH; ++sx) {
					const bool real_row = my * LV + (uint32_t)sy < L.rh;
					if (real_row && mx * LH + (uint32_t)sx < L.rw)
						continue;
					/* sx >= 1 in a real block row and sy >= 1 below the picture: an MCU's first block column and row are never dummies */
					const int u = tid * DPM + sy * LH + sx, from = real_row ? max(u - 1, 0) : tid * DPM + max(sy - 1, 0) * LH + LH - 1;
					const uint32_t dc = *reinterpret_cast<const uint16_t *>(sdu + enc_du_chunk(from, 0));
#pragma unroll
					for (int k = 0; k < 8; ++k)
						*reinterpret_cast<uint4 *>(sdu + enc_du_chunk(u, k)) = uint4{k == 0 ? dc : 0u, 0u, 0u, 0u};
				}
		}
		__syncthreads();
	}
	enc_strip_store<DPM, NT>(im, m0, cnt, sdu, du, tid);
}

} /* namespace mij */

#endif /* MIJ_LIBJPEG_ENC_KERNELS_H */
