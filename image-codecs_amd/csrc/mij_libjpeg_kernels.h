/*
 * mij_libjpeg_kernels.h -- the two kernels of a slot that asked for libjpeg's arithmetic (mij_batch_set_arith, MIJ_ARITH_LIBJPEG;
 * the contract is the section LIBJPEG ARITHMETIC of include/mij.h, restated in numpy in tests/libjpeg_model.py):
 *     pass 1  k_lj_idct   quantised coefficients -> 32-bit de-quantisation -> ISLOW inverse DCT (jidctint.c) -> u8 sample planes
 *     pass 2  k_lj_color  sample planes -> fancy upsampling (jdsample.c) -> colour (jdcolor.c) -> the slot's picture
 * Both have the shape of the two-pass path (k_idct_planes, k_resample_fast): the planes lie in the batch's scratch arena at
 * DevComp.plane_off, rows of bw * 8 samples.  All arithmetic is 32-bit and wrapping -- written on uint32_t, read as int where a shift
 * has to be arithmetic -- and every offset into an arena is 64-bit.
 */
#ifndef MIJ_LIBJPEG_KERNELS_H
#define MIJ_LIBJPEG_KERNELS_H

#include "mij_kernels.h"

namespace mij {

/* ------------------------------------------------------------------ pass 1: ISLOW inverse DCT */

/* jidctint.c's 1-D transform (CONST_BITS 13), outputs not yet descaled */
__device__ __forceinline__ void lj_idct1d(const uint32_t (&s)[8], uint32_t (&o)[8])
{
	uint32_t z1 = (s[2] + s[6]) * 4433u;
	const uint32_t t2 = z1 - s[6] * 15137u, t3 = z1 + s[2] * 6270u;
	const uint32_t t0 = (s[0] + s[4]) << 13, t1 = (s[0] - s[4]) << 13;
	const uint32_t e0 = t0 + t3, e3 = t0 - t3, e1 = t1 + t2, e2 = t1 - t2;
	uint32_t a = s[7], b = s[5], c = s[3], d = s[1];
	z1 = a + d;
	uint32_t z2 = b + c, z3 = a + c, z4 = b + d;
	const uint32_t z5 = (z3 + z4) * 9633u;
	a *= 2446u, b *= 16819u, c *= 25172u, d *= 12299u;
	z1 *= (uint32_t)-7373, z2 *= (uint32_t)-20995;
	z3 = z3 * (uint32_t)-16069 + z5, z4 = z4 * (uint32_t)-3196 + z5;
	a += z1 + z3, b += z2 + z4, c += z2 + z3, d += z1 + z4;
	o[0] = e0 + d, o[1] = e1 + c, o[2] = e2 + b, o[3] = e3 + a;
	o[4] = e3 - a, o[5] = e2 - b, o[6] = e1 - c, o[7] = e0 - d;
}
__device__ __forceinline__ uint32_t lj_descale1(uint32_t x) { return (uint32_t)((int)(x + 1024u) >> 11); }                  /* PASS1_BITS 2 */
__device__ __forceinline__ uint32_t lj_sample(uint32_t x) { return (uint32_t)clamp255(((int)(x + 131072u) >> 18) + 128); } /* the range limit */

/* 8 bytes of a column in the planes' row order (r0, r4, r2, r6, r1, r3, r5, r7) -> the transform's inputs s0..s7, times the quantisers
 * (dq: the component's table as u16 pairs in the same order, wave-uniform).  v[i]: the quantised coefficient of slot i. */
__device__ __forceinline__ void lj_dequant_col(const int (&v)[8], const uint32_t *__restrict__ dq, uint32_t (&s)[8])
{
	const uint32_t q0 = dq[0], q1 = dq[1], q2 = dq[2], q3 = dq[3];
	s[0] = (uint32_t)v[0] * (q0 & 0xffffu), s[4] = (uint32_t)v[1] * (q0 >> 16);
	s[2] = (uint32_t)v[2] * (q1 & 0xffffu), s[6] = (uint32_t)v[3] * (q1 >> 16);
	s[1] = (uint32_t)v[4] * (q2 & 0xffffu), s[3] = (uint32_t)v[5] * (q2 >> 16);
	s[5] = (uint32_t)v[6] * (q3 & 0xffffu), s[7] = (uint32_t)v[7] * (q3 >> 16);
}

/* One block per lane, 256 consecutive blocks of one component per workgroup (k_idct_planes' work items).  B8: compact planes, escapes
 * included; otherwise the int16 tile layout.  A wavefront whose 64 blocks hold a DC term only takes the transform of that term alone:
 * the same formulas on the one non-zero input, so the same values. */
template <bool B8>
__global__ __launch_bounds__(256) void k_lj_idct(const DevImage *__restrict__ imgs, const WorkIdct *__restrict__ work, const uint8_t *__restrict__ coef,
																 uint8_t *__restrict__ planes)
{
	const WorkIdct wk = work[blockIdx.x];
	const DevImage &im = imgs[wk.img];
	const DevComp &cp = im.comp[wk.comp];
	const uint32_t nblk = (uint32_t)(cp.bw * cp.bh);
	const uint32_t L = wk.first + threadIdx.x;
	if (L >= nblk)
		return;
	const uint32_t *__restrict__ dq = im.dq[wk.comp];
	const CoefView cv = coef_view(coef, cp);
	int v[8][8]; /* [column][slot]: the quantised coefficients */
	if constexpr (B8) {
		RawB8 raw;
		load_raw_b8(cv, L, raw);
		const bool esc = (raw.h[0].x & 1u) != 0;
#pragma unroll
		for (int k = 0; k < 8; ++k) {
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				v[k][i] = (int)(int8_t)(raw.h[k].x >> (8 * i));
				v[k][4 + i] = (int)(int8_t)(raw.h[k].y >> (8 * i));
			}
		}
		if (esc) { /* coefficient == sext8(low) + 256 * escape (mod 2^16) */
			const uint4 *hp = reinterpret_cast<const uint4 *>(cv.hi + ((size_t)L << 6));
#pragma unroll
			for (int k = 0; k < 8; ++k) {
				const uint4 e = hp[k >> 1];
				const uint32_t ex = (k & 1) ? e.z : e.x, ey = (k & 1) ? e.w : e.y;
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					v[k][i] = (int)(int16_t)(v[k][i] + 256 * (int)(int8_t)(ex >> (8 * i)));
					v[k][4 + i] = (int)(int16_t)(v[k][4 + i] + 256 * (int)(int8_t)(ey >> (8 * i)));
				}
			}
		}
		v[0][0] = (int)(int16_t)raw.dc; /* the byte in its place holds the block's flags */
	} else {
		uint4 c[8];
		load_block(cv.plane, L, c);
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			const uint32_t p[4] = {c[k].x, c[k].y, c[k].z, c[k].w};
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				v[k][2 * i] = (int)(int16_t)(p[i] & 0xffffu);
				v[k][2 * i + 1] = (int)(int16_t)(p[i] >> 16);
			}
		}
	}
	uint32_t ac = 0;
#pragma unroll
	for (int k = 0; k < 8; ++k)
#pragma unroll
		for (int i = 0; i < 8; ++i)
			if (k | i)
				ac |= (uint32_t)v[k][i];
	uint2 rows[8];
	if (__builtin_amdgcn_ballot_w64(ac != 0u) == 0ull) { /* wave-uniform: DC only */
		const uint32_t d = (uint32_t)v[0][0] * (dq[0] & 0xffffu);
		const uint32_t px = lj_sample(lj_descale1(d << 13) << 13) * 0x01010101u;
#pragma unroll
		for (int i = 0; i < 8; ++i)
			rows[i] = make_uint2(px, px);
	} else {
		uint32_t ws[8][8]; /* [row][column] */
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			uint32_t s[8], o[8];
			lj_dequant_col(v[k], dq + 4 * k, s);
			lj_idct1d(s, o);
#pragma unroll
			for (int r = 0; r < 8; ++r)
				ws[r][k] = lj_descale1(o[r]);
		}
#pragma unroll
		for (int r = 0; r < 8; ++r) {
			uint32_t o[8];
			lj_idct1d(ws[r], o);
			rows[r] = make_uint2(lj_sample(o[0]) | lj_sample(o[1]) << 8 | lj_sample(o[2]) << 16 | lj_sample(o[3]) << 24,
										lj_sample(o[4]) | lj_sample(o[5]) << 8 | lj_sample(o[6]) << 16 | lj_sample(o[7]) << 24);
		}
	}
	const uint32_t by = L / (uint32_t)cp.bw, bx = L - by * (uint32_t)cp.bw;
	const size_t w2 = (size_t)cp.bw * 8;
	uint8_t *dst = planes + cp.plane_off + (size_t)by * 8 * w2 + (size_t)bx * 8;
#pragma unroll
	for (int i = 0; i < 8; ++i)
		*reinterpret_cast<uint2 *>(dst + (size_t)i * w2) = rows[i];
}

/* ------------------------------------------------------------------ pass 2: fancy upsampling, colour, pixel stores */

/* One work item: MIJ_LJ_ITEM_W x MIJ_LJ_ITEM_H pixels -- 32 x 8 lanes, each with a run of eight pixels of two rows (2j, 2j + 1), which
 * share chroma row j of a vertically subsampled file.  WorkIdct.comp = item column, .first = item row. */
#define MIJ_LJ_ITEM_W 256
#define MIJ_LJ_ITEM_H 16

/* eight samples of a row from column x0 (a multiple of 8: two aligned dwords inside the padded row) */
__device__ __forceinline__ void lj_load8(const uint8_t *__restrict__ row, int x0, int (&v)[8])
{
	const uint2 d = *reinterpret_cast<const uint2 *>(row + x0);
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		v[i] = (int)((d.x >> (8 * i)) & 255u);
		v[4 + i] = (int)((d.y >> (8 * i)) & 255u);
	}
}
/* samples i0 - 1 .. i0 + 4 of a row, the indices clamped to [0, last] (i0 a multiple of 4, i0 <= last): no sample of a padding column
 * is ever a neighbour */
__device__ __forceinline__ void lj_load6(const uint8_t *__restrict__ row, int i0, int last, int (&v)[6])
{
	const uint32_t d = *reinterpret_cast<const uint32_t *>(row + i0);
	const int edge = (int)row[i0 + 4 < last ? i0 + 4 : last];
	v[0] = (int)row[i0 > 0 ? i0 - 1 : 0];
#pragma unroll
	for (int i = 0; i < 4; ++i)
		v[1 + i] = i0 + i > last ? edge : (int)((d >> (8 * i)) & 255u);
	v[5] = edge;
}

/* The chroma samples under the lane's eight pixels of rows ya (even) and ya + 1.  LH, LV: the component's subsampling.  cp.x, cp.y: the
 * plane's real size; rows are clamped into it, so the second row of a lane at the picture's last row reads a valid address. */
template <int LH, int LV>
__device__ __forceinline__ void lj_chroma(const uint8_t *__restrict__ planes, const DevComp &cp, int ya, int x0, int (&c)[2][8])
{
	const size_t pitch = (size_t)cp.bw * 8;
	const uint8_t *__restrict__ base = planes + cp.plane_off;
	const int lastx = cp.x - 1, lasty = cp.y - 1;
	const bool plain = LH == 2 && cp.x <= 2; /* libjpeg's small-width rule: h2v1 and h2v2 replicate, unfiltered */
	if constexpr (LV == 1) {
#pragma unroll
		for (int r = 0; r < 2; ++r) {
			const int y = ya + r < lasty ? ya + r : lasty;
			const uint8_t *__restrict__ row = base + (size_t)y * pitch;
			if constexpr (LH == 1) {
				lj_load8(row, x0, c[r]);
			} else {
				int v[6];
				lj_load6(row, x0 >> 1, lastx, v);
#pragma unroll
				for (int k = 0; k < 4; ++k) {
					c[r][2 * k] = plain ? v[k + 1] : (3 * v[k + 1] + v[k] + 1) >> 2;
					c[r][2 * k + 1] = plain ? v[k + 1] : (3 * v[k + 1] + v[k + 2] + 2) >> 2;
				}
			}
		}
	} else {
		const int j = ya >> 1, up = plain ? j : (j > 0 ? j - 1 : 0), dn = plain ? j : (j < lasty ? j + 1 : lasty);
		const uint8_t *__restrict__ rm = base + (size_t)j * pitch, *__restrict__ ru = base + (size_t)up * pitch, *__restrict__ rd = base + (size_t)dn * pitch;
		if constexpr (LH == 1) {
			int a[8], m[8], b[8];
			lj_load8(ru, x0, a);
			lj_load8(rm, x0, m);
			lj_load8(rd, x0, b);
#pragma unroll
			for (int k = 0; k < 8; ++k) {
				c[0][k] = (3 * m[k] + a[k] + 1) >> 2;
				c[1][k] = (3 * m[k] + b[k] + 2) >> 2;
			}
		} else {
			int a[6], m[6], b[6];
			lj_load6(ru, x0 >> 1, lastx, a);
			lj_load6(rm, x0 >> 1, lastx, m);
			lj_load6(rd, x0 >> 1, lastx, b);
			int s[2][6]; /* the vertical sums, computed once for both neighbours of every sample */
#pragma unroll
			for (int k = 0; k < 6; ++k) {
				s[0][k] = 3 * m[k] + a[k];
				s[1][k] = 3 * m[k] + b[k];
			}
#pragma unroll
			for (int r = 0; r < 2; ++r)
#pragma unroll
				for (int k = 0; k < 4; ++k) {
					c[r][2 * k] = plain ? m[k + 1] : (3 * s[r][k + 1] + s[r][k] + 8) >> 4;
					c[r][2 * k + 1] = plain ? m[k + 1] : (3 * s[r][k + 1] + s[r][k + 2] + 7) >> 4;
				}
		}
	}
}

/* A lane's run of nb bytes (the dwords w[], eight pixels at most) to p.  The misalignment of p is the same for every lane of a row
 * (a run is 8 * N bytes), so a lane whose left neighbour works in the same workgroup (left) starts at the aligned dword below p with
 * that neighbour's last bytes (prev: the neighbour's last dword) in front of its own, and a lane whose right neighbour does (right)
 * leaves the bytes behind its last whole dword to it.  Where there is no such neighbour -- the two ends of a row, the seams between
 * work items -- the bytes up to the next aligned address and behind the last one are stored one by one.  No store is misaligned and
 * none leaves [p, p + nb) but for the neighbour's bytes, which belong to the same row. */
template <int NW>
__device__ __forceinline__ void lj_store_run(uint8_t *__restrict__ p, const uint32_t (&w)[NW], uint32_t prev, int nb, bool left, bool right)
{
	const int m = (int)(reinterpret_cast<uintptr_t>(p) & 3u);
	int so; /* offset of the first dword in the lane's own bytes */
	if (left) {
		so = -m;
	} else {
		so = m ? 4 - m : 0;
		so = so < nb ? so : nb;
#pragma unroll
		for (int i = 0; i < 3; ++i)
			if (i < so)
				p[i] = (uint8_t)(w[0] >> (8 * i));
	}
	uint32_t E[NW + 3]; /* prev, then the lane's dwords */
	E[0] = prev;
#pragma unroll
	for (int k = 0; k < NW; ++k)
		E[k + 1] = w[k];
	E[NW + 1] = E[NW + 2] = 0u;
	const int at = 4 + so, hi = at >> 2, sh = 8 * (at & 3);
	const int nd = (nb - so) >> 2, tail = nb - so - 4 * nd;
	uint8_t *__restrict__ q = p + so;
#pragma unroll
	for (int k = 0; k <= NW; ++k) {
		const uint32_t lo = hi ? E[k + 1] : E[k], up = hi ? E[k + 2] : E[k + 1];
		const uint32_t x = (uint32_t)((((uint64_t)up << 32) | lo) >> sh);
		if (k < nd) {
			*reinterpret_cast<uint32_t *>(q + 4 * k) = x;
		} else if (k == nd && !right) {
#pragma unroll
			for (int i = 0; i < 3; ++i)
				if (i < tail)
					q[4 * k + i] = (uint8_t)(x >> (8 * i));
		}
	}
}

/* LH, LV: chroma subsampling (1, 1), (2, 1), (1, 2) or (2, 2); N = n_out.  The (1, 1) form also serves a one-component file and the
 * luma-only outputs (N < 3: Y alone, libjpeg's JCS_GRAYSCALE), which read no chroma plane at all. */
template <int LH, int LV, int N>
__global__ __launch_bounds__(256) void k_lj_color(const DevImage *__restrict__ imgs, const WorkIdct *__restrict__ work, const uint8_t *__restrict__ planes,
																  uint8_t *__restrict__ out)
{
	const WorkIdct wk = work[blockIdx.x];
	const DevImage &im = imgs[wk.img];
	const int W = im.width, H = im.height;
	const int lx = (int)(threadIdx.x & 31u);
	const int x0 = ((int)wk.comp * 32 + lx) * 8;
	const int ya = ((int)wk.first * 8 + (int)(threadIdx.x >> 5)) * 2;
	if (x0 >= W || ya >= H)
		return;
	const bool grey = N < 3 || im.ncomp == 1;
	const DevComp &cy = im.comp[0];
	const size_t py = (size_t)cy.bw * 8;
	const uint8_t *__restrict__ Y = planes + cy.plane_off;
	const int npx = W - x0 < 8 ? W - x0 : 8;
	const bool left = lx > 0, right = lx < 31 && x0 + 8 < W;
	int cb[2][8], cr[2][8];
	if (!grey) {
		lj_chroma<LH, LV>(planes, im.comp[1], ya, x0, cb);
		lj_chroma<LH, LV>(planes, im.comp[2], ya, x0, cr);
	}
#pragma unroll
	for (int r = 0; r < 2; ++r) {
		const int y = ya + r;
		if (y >= H)
			break;
		int yy[8];
		lj_load8(Y + (size_t)y * py, x0, yy);
		uint8_t px[8 * N];
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			int R = yy[k], G = yy[k], B = yy[k];
			if (!grey) {
				const int u = cb[r][k] - 128, v = cr[r][k] - 128;
				R = clamp255(yy[k] + ((91881 * v + 32768) >> 16));
				G = clamp255(yy[k] + ((-22554 * u - 46802 * v + 32768) >> 16));
				B = clamp255(yy[k] + ((116130 * u + 32768) >> 16));
			}
			px[N * k] = (uint8_t)R;
			if constexpr (N == 2)
				px[N * k + 1] = 255;
			if constexpr (N >= 3) {
				px[N * k + 1] = (uint8_t)G;
				px[N * k + 2] = (uint8_t)B;
			}
			if constexpr (N == 4)
				px[N * k + 3] = 255;
		}
		uint32_t w[2 * N];
#pragma unroll
		for (int i = 0; i < 2 * N; ++i)
			w[i] = (uint32_t)px[4 * i] | (uint32_t)px[4 * i + 1] << 8 | (uint32_t)px[4 * i + 2] << 16 | (uint32_t)px[4 * i + 3] << 24;
		const uint32_t prev = (uint32_t)__shfl_up((int)w[2 * N - 1], 1);
		lj_store_run<2 * N>(out + im.out_off + ((size_t)y * (size_t)W + (size_t)x0) * N, w, prev, npx * N, left, right);
	}
}

} // namespace mij

#endif
