/*
 * mij_planes_out_kernels.h -- plane output (include/mij.h, PLANE OUTPUT): coefficients in, the stored components' own samples out, into
 * memory the caller owns.  No upsampling and no colour stage: the kernel ends where phase A of the band kernels ends.
 *
 * One block per lane through load_idct_block (both plane formats, the wide IDCT, the sparse classes).  A work item is 256 lanes of one
 * (slot, component); its lanes count in raster order through the rectangle of blocks that the component's window touches (DevPlane.blk,
 * as roi_unit counts), so a component that is not wanted queues nothing and padding blocks are never transformed.
 *
 * The stores come in three forms, chosen per (request, component) on the host and therefore wave-uniform:
 *   general  every sample of the block that lies inside the window as one byte store at dst + y * row_pitch + x * x_pitch.  This form is
 *            the contract; a block whose COLUMNS the window's edge cuts takes it in the other two forms as well (per lane).
 *   fast     x_pitch == 1 and every block's first sample of every row 8-byte aligned: one 8-byte store per row.  Consecutive lanes hold
 *            consecutive blocks of a block row, so one store instruction writes 512 contiguous bytes.  A block cut by the window's top
 *            or bottom edge alone (the last chroma block row of a 1080p 4:2:0 picture holds four sample rows) keeps the row stores
 *            and leaves out the rows that do not exist.
 *   paired   components 1 and 2 with one rectangle, x_pitch == 2 and destinations one byte apart (NV12, NV21): the lane transforms both
 *            blocks, interleaves each row with two v_perm per eight bytes and stores its 16 bytes with the widest store that the
 *            alignment of the pair's base and pitch allows (16, 8, 4 or 2 bytes; never a misaligned one).
 * All address arithmetic towards dst is 64-bit.
 */
#ifndef MIJ_PLANES_OUT_KERNELS_H
#define MIJ_PLANES_OUT_KERNELS_H

#include "mij_kernels.h"

namespace mij {

enum { PLN_GENERAL = 0, PLN_FAST = 1, PLN_PAIRED = 2 };

/* The destinations arrive as integers in the request table, so the compiler cannot know their address space and would store through flat
 * instructions; they are the caller's device memory (checked on the host), hence global.  G(T): T in the global address space. */
#define MIJ_G(T) __attribute__((address_space(1))) T
typedef MIJ_G(uint8_t) *gbytes;
typedef uint32_t u2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st_global(gbytes q, uint2 v) { *reinterpret_cast<MIJ_G(u2v) *>(q) = u2v{v.x, v.y}; }
__device__ __forceinline__ void st_global(gbytes q, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { *reinterpret_cast<MIJ_G(u4v) *>(q) = u4v{a, b, c, d}; }

/* one component of a plane request.  Samples [sx0, sx1) x [sy0, sy1) of the component go to dst + (y - sy0) * row_pitch + (x - sx0) *
 * x_pitch; blk is the rectangle of blocks they lie in.  PLN_PAIRED: dst is the lower of the two destinations, `first` the component (1 or
 * 2) whose samples take the even bytes, and align the store width in bytes. */
struct DevPlane {
	uint64_t dst;
	int64_t row_pitch, x_pitch;
	DevRoi blk;
	uint32_t sx0, sy0, sx1, sy1;
	uint32_t form, first, align, pad;
};
struct DevPlanes {
	DevPlane c[4];
};

/* the samples of one block that lie inside the window, byte by byte */
__device__ __forceinline__ void planes_store_general(const DevPlane &p, gbytes dst, int64_t xp, uint32_t bx, uint32_t by, const uint2 (&rows)[8])
{
#pragma unroll
	for (uint32_t i = 0; i < 8; ++i) {
		const uint32_t y = 8u * by + i;
		if (y < p.sy0 || y >= p.sy1)
			continue;
		gbytes row = dst + (int64_t)(y - p.sy0) * p.row_pitch;
#pragma unroll
		for (uint32_t j = 0; j < 8; ++j) {
			const uint32_t x = 8u * bx + j;
			if (x >= p.sx0 && x < p.sx1)
				row[(int64_t)(x - p.sx0) * xp] = (uint8_t)(((j < 4 ? rows[i].x : rows[i].y) >> (8u * (j & 3u))) & 255u);
		}
	}
}

/* the 16 interleaved bytes of one row of a pair, with stores of A bytes */
template <int A>
__device__ __forceinline__ void planes_store_pair_row(gbytes q, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
	if constexpr (A == 16) {
		st_global(q, w0, w1, w2, w3);
	} else if constexpr (A == 8) {
		st_global(q, make_uint2(w0, w1));
		st_global(q + 8, make_uint2(w2, w3));
	} else if constexpr (A == 4) {
		MIJ_G(uint32_t) *d = reinterpret_cast<MIJ_G(uint32_t) *>(q);
		d[0] = w0, d[1] = w1, d[2] = w2, d[3] = w3;
	} else {
		MIJ_G(uint16_t) *d = reinterpret_cast<MIJ_G(uint16_t) *>(q);
		d[0] = (uint16_t)w0, d[1] = (uint16_t)(w0 >> 16), d[2] = (uint16_t)w1, d[3] = (uint16_t)(w1 >> 16);
		d[4] = (uint16_t)w2, d[5] = (uint16_t)(w2 >> 16), d[6] = (uint16_t)w3, d[7] = (uint16_t)(w3 >> 16);
	}
}

/* rows [r0, r1) of the block */
template <int A>
__device__ __forceinline__ void planes_store_pair(gbytes q, int64_t rp, const uint2 (&a)[8], const uint2 (&b)[8], uint32_t r0, uint32_t r1)
{
#pragma unroll
	for (uint32_t i = 0; i < 8; ++i) {
		if (i < r0 || i >= r1)
			continue;
		/* v_perm: selector bytes 0-3 take the second operand's bytes, 4-7 the first's: (a0 b0 a1 b1) (a2 b2 a3 b3) */
		planes_store_pair_row<A>(q + (int64_t)i * rp, __builtin_amdgcn_perm(b[i].x, a[i].x, 0x05010400u), __builtin_amdgcn_perm(b[i].x, a[i].x, 0x07030602u),
										 __builtin_amdgcn_perm(b[i].y, a[i].y, 0x05010400u), __builtin_amdgcn_perm(b[i].y, a[i].y, 0x07030602u));
	}
}

/* PAIR: the instance for slots whose request has a paired form (it serves their other components as well: one launch per batch); the
 * instance without carries no second block, which leaves it the registers of k_idct_planes */
template <bool WIDE, bool B8 = false, bool PAIR = false>
__global__ __launch_bounds__(256) void k_planes_out(const DevImage *__restrict__ imgs, const WorkIdct *__restrict__ work, const uint8_t *__restrict__ coef,
																	 uint8_t *__restrict__ /* the output arena: not written */, const DevPlanes *__restrict__ reqs)
{
	const WorkIdct wk = work[blockIdx.x];
	const DevImage &im = imgs[wk.img];
	const DevPlane &p = reqs[wk.img].c[wk.comp];
	/* a pair's item names component 1; the lane transforms the component of the even bytes first (NV21: component 2), then the other */
	const bool pair = PAIR && p.form == PLN_PAIRED;
	const uint32_t comp = pair ? p.first : wk.comp;
	const DevComp &cp = im.comp[comp];
	const uint32_t Lr = wk.first + threadIdx.x;
	if (Lr >= p.blk.w * p.blk.h)
		return;
	const uint32_t wy = Lr / p.blk.w, by = p.blk.y0 + wy, bx = p.blk.x0 + (Lr - wy * p.blk.w); /* roi_unit, keeping the coordinates */
	const uint32_t L = by * (uint32_t)cp.bw + bx;
	IdctK K;
	K.init();
	const int count = im.flags & MIJ_DEV_COUNT_CLASSES;
	uint2 rows[8];
	load_idct_block<WIDE, B8>(K, coef_view(coef, cp), L, im.dq[comp], rows, count);
	/* all eight columns inside the window: whole rows are stored, the rows [r0, r1) of the block that the window holds */
	const bool inside = 8u * bx >= p.sx0 && 8u * bx + 8u <= p.sx1;
	const uint32_t r0 = p.sy0 > 8u * by ? p.sy0 - 8u * by : 0u, r1 = min(8u, p.sy1 - 8u * by);
	const gbytes dst = (gbytes)p.dst;
	if (pair) {
		const uint32_t other = 3u - comp; /* components 1 and 2 share geometry and rectangle */
		uint2 rows2[8];
		load_idct_block<WIDE, B8>(K, coef_view(coef, im.comp[other]), L, im.dq[other], rows2, count);
		if (!inside) {
			planes_store_general(p, dst, 2, bx, by, rows);
			planes_store_general(p, dst + 1, 2, bx, by, rows2);
			return;
		}
		gbytes q = dst + ((int64_t)8 * by - (int64_t)p.sy0) * p.row_pitch + ((int64_t)8 * bx - (int64_t)p.sx0) * 2;
		if (p.align >= 16u)
			planes_store_pair<16>(q, p.row_pitch, rows, rows2, r0, r1);
		else if (p.align == 8u)
			planes_store_pair<8>(q, p.row_pitch, rows, rows2, r0, r1);
		else if (p.align == 4u)
			planes_store_pair<4>(q, p.row_pitch, rows, rows2, r0, r1);
		else
			planes_store_pair<2>(q, p.row_pitch, rows, rows2, r0, r1);
		return;
	} else if (p.form == PLN_FAST && inside) {
		gbytes q = dst + ((int64_t)8 * by - (int64_t)p.sy0) * p.row_pitch + ((int64_t)8 * bx - (int64_t)p.sx0);
#pragma unroll
		for (uint32_t i = 0; i < 8; ++i)
			if (i >= r0 && i < r1)
				st_global(q + (int64_t)i * p.row_pitch, rows[i]);
		return;
	} else {
		planes_store_general(p, dst, p.x_pitch, bx, by, rows);
	}
}

#undef MIJ_G

} /* namespace mij */

#endif /* MIJ_PLANES_OUT_KERNELS_H */
